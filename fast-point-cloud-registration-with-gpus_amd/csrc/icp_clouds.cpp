// icp_clouds.cpp -- the resident clouds: upload and layout, the non-finite check, the device-side set-up decisions (spatial
// order, exact duplicates, the sparse kernels' model tables), the work buffers of the plan, and the downloads of the
// moving cloud and of the matches
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <new>

#include "icp_ctx.h"

namespace {

static int check_nonfinite(icp_ctx* c, int count)
{
    // Non-finite coordinates are refused (include/icp_mi355x.h, "non-finite input": a deliberate deviation).  The reference
    // does not look at its input: the match of such a point is whatever cblas_idamin (src/ICP_CPU.c:232) answers for a vector
    // that holds NaN -- MKL documents nothing -- and the centroid sums (:342-366) then turn the whole transform into NaN:
    // nothing a caller could use, and the pruned search has no bound to go by.
    if (const unsigned int bad = *(volatile unsigned int*)c->h_nonfinite) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%u of the %d points have a NaN or infinite coordinate: non-finite input is refused", bad, count);
        return fail(ICP_ERR_INVALID, msg);
    }
    return ICP_OK;
}

// upload a host AoS cloud and convert it to the padded SoA layout
// deferred: no synchronisation here -- the caller synchronises once, at the end of its set-up, and asks check_nonfinite then
// (soa2: a second copy of the converted cloud; enc: the bounding cube's six words, see launch_aos_to_soa)
int upload_cloud(icp_ctx* c, const void* aos, int count, int pad, int precision, DevBuf& dst, bool deferred = false, void* soa2 = nullptr, unsigned int* enc = nullptr)
{
    const size_t es = icp::elem_size(precision);
    HIP_TRY(dst.ensure(3 * (size_t)pad * es));
    if (count <= 0) return ICP_OK;
    const size_t bytes = 3 * (size_t)count * es;
    const void* src = nullptr;
    if (deferred && bytes <= (4u << 20)) {
        // a small cloud whose set-up ends with a wait anyway: copied by this thread into pinned, mapped memory and laid out straight
        // from there by the layout kernel (one pass over PCIe) -- no copy command, no runtime staging of a pageable source
        if (bytes > c->h_stage_cap) {
            if (c->h_stage) { (void)hipHostFree(c->h_stage); c->h_stage = nullptr; c->h_stage_cap = 0; }
            const size_t want = std::max(bytes, (size_t)1 << 20);
            HIP_TRY(hipHostMalloc(&c->h_stage, want, hipHostMallocMapped | hipHostMallocCoherent));
            c->h_stage_cap = want;
        }
        std::memcpy(c->h_stage, aos, bytes);
        src = c->h_stage;
    } else {
        HIP_TRY(c->stage.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(c->stage.p, aos, bytes, hipMemcpyHostToDevice, c->stream));
        src = c->stage.p;
    }
    *(volatile unsigned int*)c->h_nonfinite = 0u;
    HIP_TRY(icp::launch_aos_to_soa(precision, src, count, pad, dst.p, c->stream, c->h_nonfinite, soa2, enc));
    if (deferred) return ICP_OK;
    // the staging buffer is reused by the next upload: order them on the stream, and make sure the
    // pageable host source has been consumed before returning
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_nonfinite(c, count);
}

// ---- spatial order and duplicate flags, on the device ---------------------------------------------------------------
// The sparse matching kernel prunes by bounding boxes of 8 consecutive model points and of 128 consecutive moving
// points: it needs clouds whose index order has spatial locality.  A LiDAR scan has it; a mesh's vertex list
// (Bunny) does not.  Where Morton order makes the groups clearly tighter than the given order, the kernel works
// on a Morton-ordered view (a permutation: the clouds at the ABI and every index it returns stay in user order).
// Sorting and the extent test run on the device (rocPRIM radix sorts, fixed-order reductions): a few dozen
// microseconds per cloud instead of milliseconds of std::sort on the host.
// the set-up's scratch as the launchers take it (sized for `count` points by prep_buffers)
static void prep_views(const icp_ctx* c, int count, icp::PrepBuffers& b)
{
    b.keys[0] = (unsigned int*)c->prep_keys[0].p; b.keys[1] = (unsigned int*)c->prep_keys[1].p;
    b.vals[0] = (int32_t*)c->prep_vals[0].p; b.vals[1] = (int32_t*)c->prep_vals[1].p;
    b.temp = c->prep_tmp.p; b.temp_bytes = icp::prep_sort_temp_bytes(count);
    b.box = (float*)c->prep_small.p; b.ext = (double*)c->prep_ext.p;
}

static int prep_buffers(icp_ctx* c, int count, icp::PrepBuffers& b)
{
    const size_t tb = icp::prep_sort_temp_bytes(count);
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c->prep_keys[k].ensure((size_t)count * sizeof(unsigned int)));
        HIP_TRY(c->prep_vals[k].ensure((size_t)count * sizeof(int32_t)));
    }
    HIP_TRY(c->prep_tmp.ensure(tb));
    HIP_TRY(c->prep_small.ensure(sizeof(icp_ctx::PrepSmall)));
    HIP_TRY(c->prep_ext.ensure((size_t)((count + 7) / 8) * sizeof(double)));
    HIP_TRY(c->prep_voided.ensure((size_t)icp::round_up(count, 16) + 16));
    HIP_TRY(c->prep_perm.ensure((size_t)count * sizeof(int32_t)));
    prep_views(c, count, b);
    HIP_TRY(hipMemsetAsync(c->prep_small.p, 0, sizeof(icp_ctx::PrepSmall), c->stream));
    return ICP_OK;
}

// reads the extent totals back and decides: true when Morton order makes the groups at least 3x tighter.  A scan that
// already has locality must keep its order even if Morton cells are tighter: the hall scan's model chunks are 2.1x
// tighter in Morton order, yet matching gets 20 % slower -- its 8-point half columns line up with the moving groups
// (8 columns), compact Morton cells do not; the Bunny vertex list is 10x / 5.8x looser than Morton order.
static int morton_decision(icp_ctx* c, int count, int group, int group2, bool* use_sorted, int* voided_out)
{
    icp_ctx::PrepSmall h{};
    HIP_TRY(hipMemcpyAsync(&h, c->prep_small.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (voided_out) *voided_out = h.voided;
    const int force = c->tune.sort;   // ICP_SORT=0 never, =1 always (A/B runs, tests)
    if (force == 0) *use_sorted = false;
    else if (count <= group) *use_sorted = false;
    else if (force == 1) *use_sorted = true;
    else {
        *use_sorted = 3.0 * h.totals[1] < h.totals[0];
        // a model searched through the box hierarchy: the order also has to serve the level above the chunks (a
        // row-major grid has tight 8-point chunks but 512-point boxes one row thin and a fifth of the cloud long)
        if (group2 > 0 && 3.0 * h.totals[3] < h.totals[2] && h.totals[1] <= h.totals[0]) *use_sorted = true;
    }
    if (c->trace) {
        std::fprintf(stderr, "[icp trace] %d points, groups of %d: extent %.4g in the given order, %.4g in Morton order", count, group, h.totals[0], h.totals[1]);
        if (group2 > 0) std::fprintf(stderr, "; groups of %d: %.4g, %.4g", group2, h.totals[2], h.totals[3]);
        std::fprintf(stderr, " -> %s; %d exact duplicates voided\n", *use_sorted ? "Morton view" : "own order", h.voided);
    }
    return ICP_OK;
}

// The order decision of a small cloud (<= kPrepSmallMax points) with ONE synchronisation: summed group extents of the given order
// and -- unless the remembered decision says it is not needed -- of the Hilbert-curve order, in fixed point relative to the bounding
// cube the layout kernel left in PrepSmall::enc.  Ends the deferred upload: the non-finite count is checked here.
static int decide_order_small(icp_ctx* c, const icp::PrepBuffers& pb, const void* X_soa, int count, int pad, int group, icp_ctx::OrderMemo& memo, bool* use_sorted,
                              int* voided_out, const char* what)
{
    icp_ctx::PrepSmall* small = (icp_ctx::PrepSmall*)c->prep_small.p;
    const int force = c->tune.sort;
    const bool trivial = count <= group || force == 0;                       // never sorted: nothing to measure
    const bool fast = !trivial && force < 0 && memo.valid && memo.count == count && memo.group == group && !memo.sorted;
    bool have_sorted = false;
    unsigned int seq = 0;
    auto sorted_extents = [&](int which) -> int {
        HIP_TRY(icp::launch_curve_order_small(pb, (const float*)X_soa, count, pad, small->enc, (int32_t*)c->prep_perm.p, c->stream));
        seq = ++c->prep_seq ? c->prep_seq : ++c->prep_seq;
        HIP_TRY(icp::launch_extents_fixed((const float*)X_soa, count, pad, (const int32_t*)c->prep_perm.p, group, small->enc, small->fixed, which, c->stream,
                                          &small->ticket, &small->voided, c->h_prep, seq));
        have_sorted = true;
        return ICP_OK;
    };
    // the launch's last block leaves the sums in pinned memory: the host spins on the sequence word (a copy back and a stream
    // synchronisation cost 15-20 us more); should the word never come, the runtime says why
    struct Report { unsigned long long fixed[4]; int voided; };
    auto wait_report = [&](Report& h) -> int {
        if (seq != 0) {
            const auto t0 = std::chrono::steady_clock::now();
            const volatile unsigned int* w = &c->h_prep->seq;
            bool there = false;
            for (unsigned spins = 1; !(there = *w == seq); ++spins)
                if ((spins & 0x3ff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) break;
            if (there) {
                std::atomic_thread_fence(std::memory_order_acquire);
                for (int k = 0; k < 4; ++k) h.fixed[k] = c->h_prep->fixed[k];
                h.voided = c->h_prep->voided;
                return ICP_OK;
            }
        }
        icp_ctx::PrepSmall full{};
        HIP_TRY(hipMemcpyAsync(&full, c->prep_small.p, sizeof full, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 4; ++k) h.fixed[k] = full.fixed[k];
        h.voided = full.voided;
        return ICP_OK;
    };
    if (!trivial) {
        if (fast) {
            seq = ++c->prep_seq ? c->prep_seq : ++c->prep_seq;
            HIP_TRY(icp::launch_extents_fixed((const float*)X_soa, count, pad, nullptr, group, small->enc, small->fixed, 0, c->stream, &small->ticket, &small->voided, c->h_prep, seq));
        } else if (int rc = sorted_extents(0)) return rc;
    }
    Report h{};
    if (int rc = wait_report(h)) return rc;
    if (int rc = check_nonfinite(c, count)) return rc;
    constexpr double kFix = 1.0 / 68719476736.0;   // 2^-36
    double given = (double)h.fixed[0] * kFix, sorted = (double)h.fixed[1] * kFix;
    if (fast && !(given <= 1.25 * memo.given_rel)) {
        // the cloud is not what the one before was: measure the curve order after all (a second short round trip, once)
        if (int rc = sorted_extents(1)) return rc;
        if (int rc = wait_report(h)) return rc;
        given = (double)h.fixed[2] * kFix;
        sorted = (double)h.fixed[3] * kFix;
    }
    if (voided_out) *voided_out = h.voided;
    if (trivial) *use_sorted = false;
    else if (force == 1) *use_sorted = true;
    else if (!have_sorted) *use_sorted = false;                              // (remembered: own order, and the cloud still looks the same)
    else *use_sorted = 3.0 * sorted < given;
    if (c->trace) {
        std::fprintf(stderr, "[icp trace] %s: %d points, groups of %d: extent %.4g of the bounding cube's edge in the given order", what, count, group, given);
        if (have_sorted) std::fprintf(stderr, ", %.4g along the Hilbert curve", sorted); else std::fprintf(stderr, " (curve order not measured: %s)", trivial ? "not applicable" : "as the cloud before");
        std::fprintf(stderr, " -> %s; %d exact duplicates voided\n", *use_sorted ? "sorted view" : "own order", h.voided);
    }
    if (!trivial && force < 0) { memo.valid = true; memo.count = count; memo.group = group; memo.sorted = *use_sorted; if (have_sorted || !memo.given_rel) memo.given_rel = given; }
    return ICP_OK;
}

int check_precision(int precision)
{
    if (precision != ICP_F32 && precision != ICP_F64) return fail(ICP_ERR_INVALID, "unknown precision");
    return ICP_OK;
}

// Morton order or the given one for the moving cloud's slots ("spatial order"): decided on groups of `grp`
int decide_moving_order(icp_ctx* c, const void* P_soa, int grp, bool have_enc = false)
{
    const int n = c->n, n_pad = icp::pad_moving(n);
    icp::PrepBuffers pb{};
    if (have_enc) {
        // (the upload has prepared the buffers and left the bounding cube: the short form, which also ends the deferred upload)
        prep_views(c, n, pb);
        if (int rc = decide_order_small(c, pb, P_soa, n, n_pad, grp, c->memo_moving, &c->moving_sorted, nullptr, "moving cloud")) return rc;
    } else {
    if (int rc = prep_buffers(c, n, pb)) return rc;
    icp_ctx::PrepSmall* small = (icp_ctx::PrepSmall*)c->prep_small.p;
    HIP_TRY(icp::launch_morton_order(pb, (const float*)P_soa, n, n_pad, grp, 0, (int32_t*)c->prep_perm.p, small->totals, c->stream));
    if (int rc = morton_decision(c, n, grp, 0, &c->moving_sorted, nullptr)) return rc;
    }
    if (c->moving_sorted) {
        HIP_TRY(c->Pperm.ensure((size_t)n_pad * sizeof(int32_t)));
        HIP_TRY(icp::launch_slot_map((const int32_t*)c->prep_perm.p, n, n_pad, (int32_t*)c->Pperm.p, c->stream));
    }
    c->moving_group = grp;
    return ICP_OK;
}

}  // namespace

int ensure_work_buffers(icp_ctx* c)
{
    const icp::NNPlan before = c->plan;
    c->plan = icp::nn_plan(c->n, c->m, c->prec, c->num_cus, c->tune);
    const icp::NNPlan& pl = c->plan;
    // the moving cloud's order was judged when it was uploaded, possibly before the model was known: now that the plan is
    // fixed, judge it again if the kernel works on groups of another size than the one assumed then
    if (c->prec == ICP_F32 && c->have_moving && c->n > 128 && icp::nn_is_sparse(pl) && c->moving_group != 0 && c->moving_group != icp::nn_moving_group(pl) && c->P0.p)
        if (int rc = decide_moving_order(c, c->P0.p, icp::nn_moving_group(pl))) return rc;
    if (before.n_pad != pl.n_pad || before.m_pad != pl.m_pad) c->resident_refused = false;  // another geometry: ask again
    if (before.n_pad != pl.n_pad || before.blocks_x != pl.blocks_x) c->rows_format = -1;     // (rows that were not in use keep old tags: wiped before the next launch)
    const size_t es = icp::elem_size(c->prec);
    const size_t S = pl.splits > 0 ? (size_t)pl.splits : 1;
    HIP_TRY(c->part_d.ensure(S * (size_t)pl.n_pad * es));
    HIP_TRY(c->part_idx.ensure(S * (size_t)pl.n_pad * sizeof(int32_t)));
    HIP_TRY(c->idx[0].ensure((size_t)pl.n_pad * sizeof(int32_t)));
    HIP_TRY(c->idx[1].ensure((size_t)pl.n_pad * sizeof(int32_t)));
    const bool fresh = c->mom_partials.cap == 0;
    size_t rows = (size_t)icp::MOM_MAX_BLOCKS;
    if ((size_t)pl.blocks_x > rows) rows = (size_t)pl.blocks_x;
    // (and one error row per matching block row -- fused transform -- or per transform block)
    if (rows > c->rows_cap) {
        if (c->h_mom_partials) { (void)hipHostFree(c->h_mom_partials); c->h_mom_partials = nullptr; }
        if (c->h_err_partials) { (void)hipHostFree(c->h_err_partials); c->h_err_partials = nullptr; }
        c->rows_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&c->h_mom_partials, rows * ICP_NMOM * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc((void**)&c->h_err_partials, rows * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(c->h_mom_partials, 0, rows * ICP_NMOM * sizeof(double));
        std::memset(c->h_err_partials, 0, rows * sizeof(double));
        delete[] c->rows_seen;
        c->rows_seen = new (std::nothrow) unsigned char[rows];
        if (!c->rows_seen) return fail(ICP_ERR_NOMEM, "row flags allocation failed");
        c->rows_cap = rows;
        c->rows_format = -1;
    }
    HIP_TRY(c->mom_partials.ensure(rows * ICP_NMOM * sizeof(double)));
    HIP_TRY(c->err_partials.ensure(rows * sizeof(double)));
    if (icp::nn_can_fuse_tail(pl)) {
        const size_t kb = (size_t)pl.n_pad * sizeof(unsigned long long), tb = (size_t)pl.blocks_x * sizeof(unsigned int);
        if (kb > c->keys.cap) {
            HIP_TRY(c->keys.ensure(kb));
            HIP_TRY(hipMemsetAsync(c->keys.p, 0xFF, c->keys.cap, c->stream));   // "no candidate yet"
        }
        if (tb > c->tickets.cap) {
            HIP_TRY(c->tickets.ensure(tb));
            HIP_TRY(hipMemsetAsync(c->tickets.p, 0, c->tickets.cap, c->stream));
        }
    }
    if (pl.share_blocks > 0) {
        const size_t sb = 5 * (size_t)pl.blocks_x * sizeof(unsigned int);
        if (sb > c->share_counts.cap || before.blocks_x != pl.blocks_x || before.share_blocks != pl.share_blocks) {
            HIP_TRY(c->share_counts.ensure(sb));
            HIP_TRY(hipMemsetAsync(c->share_counts.p, 0, c->share_counts.cap, c->stream));   // "nothing known": every row is one block
            c->share_seq = 0;
            c->share_cold_seq = 0;
        }
        HIP_TRY(c->seed_pub.ensure((size_t)pl.blocks_x * 384 * sizeof(float)));
    }
    if (c->sums_in_launch(pl)) {   // (whether or not the tail is fused now: ICP_FUSED_TAIL is looked at per launch)
        if (c->fin_tickets.cap == 0) {
            HIP_TRY(c->fin_tickets.ensure((icp::NN_FIN_GROUPS + 1) * sizeof(unsigned int)));
            HIP_TRY(hipMemsetAsync(c->fin_tickets.p, 0, c->fin_tickets.cap, c->stream));
        }
        HIP_TRY(c->fin_scratch.ensure((size_t)icp::NN_FIN_GROUPS * ICP_NMOM * sizeof(double)));
    }
    c->row_order = nullptr;
    if (pl.order) {
        const size_t rb = (size_t)pl.blocks_x * sizeof(unsigned int);
        if (rb > c->row_hits.cap || before.blocks_x != pl.blocks_x) {
            HIP_TRY(c->row_hits.ensure(rb));
            HIP_TRY(hipMemsetAsync(c->row_hits.p, 0, c->row_hits.cap, c->stream));   // "nothing known": index order
            c->order_regs = 0;
            c->order_launches = 0;
        }
        for (int k = 0; k < 2; ++k) { HIP_TRY(c->order_keys[k].ensure(rb)); HIP_TRY(c->order_vals[k].ensure(rb)); }
        HIP_TRY(c->order_roles.ensure(((size_t)pl.blocks_x + icp::NN_ORDER_EXTRA) * sizeof(int32_t)));
        if (c->order_totals.cap == 0) {
            HIP_TRY(c->order_totals.ensure(2 * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(c->order_totals.p, 0, c->order_totals.cap, c->stream));
            c->order_seq = 0;
        }
        HIP_TRY(c->order_tmp.ensure(icp::row_order_temp_bytes(pl.blocks_x)));
    }
    if (icp::nn_can_fuse_transform(pl)) HIP_TRY(c->P2.ensure(3 * (size_t)pl.n_pad * es));
    HIP_TRY(c->mom_own.ensure(ICP_NMOM * sizeof(double)));
    if (fresh) {
        HIP_TRY(hipMemsetAsync(c->mom_partials.p, 0, c->mom_partials.cap, c->stream));
        HIP_TRY(hipMemsetAsync(c->err_partials.p, 0, c->err_partials.cap, c->stream));
        HIP_TRY(hipMemsetAsync(c->mom_own.p, 0, c->mom_own.cap, c->stream));
    }
    if (!c->mom_dev) c->mom_dev = (double*)c->mom_own.p;
    return ICP_OK;
}

// icp_reset_moving is lazy: whoever needs the moving cloud in c->P asks for it here (the resident kernel does not --
// it reads the pristine copy directly and writes c->P itself, which saves a device-to-device copy and a dependent
// dispatch per registration)
int materialize_moving(icp_ctx* c)
{
    if (c->moving_is_pristine && c->n > 0) {
        const size_t bytes = 3 * (size_t)icp::pad_moving(c->n) * icp::elem_size(c->prec);
        HIP_TRY(hipMemcpyAsync(c->P.p, c->P0.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    c->moving_is_pristine = false;
    return ICP_OK;
}

int download_idx(icp_ctx* c, int which, int32_t* out)
{
    if (c->n == 0) return ICP_OK;
    if (!out) return fail(ICP_ERR_INVALID, "idx_out == NULL");
    if (!c->idx[which].p) return fail(ICP_ERR_STATE, "no matching pass has run");
    HIP_TRY(hipMemcpyAsync(out, c->idx[which].p, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ICP_OK;
}

int require_clouds(icp_ctx* c)
{
    if (!c->have_model || !c->have_moving) return fail(ICP_ERR_STATE, "model and moving clouds must be resident");
    if (c->n > 0 && c->m == 0) return fail(ICP_ERR_EMPTY, "empty model cloud");
    return ICP_OK;
}

#pragma GCC visibility push(default)   // (the C ABI: exported although its icp_ctx is a hidden type)
extern "C" {

int icp_set_model(icp_ctx* c, const void* xyz, int m, int precision)
{
    if (int rc = use(c)) return rc;
    if (int rc = check_precision(precision)) return rc;
    if (m < 0 || (m > 0 && !xyz)) return fail(ICP_ERR_INVALID, "bad model cloud");
    if (c->have_moving && c->prec != precision) { c->have_moving = false; c->n = 0; }
    c->prec = precision;
    c->m = m;
    c->have_normals = false;
    c->loop.active = false;
    c->idx_valid = false;
    c->have_model = false;     // (until the upload has been accepted)
    c->have_scan_copy = false;
    c->have_records = false;
    // (the model's size decides the search form -- together with the CLOUD's: a model of 2^16 .. 2^17 points is searched through the
    // hierarchy by a cloud of more rows than shared 8-wave blocks serve, flat by a smaller one, and the model is set before the cloud is
    // known: it gets the upper levels and the records whenever SOME cloud would ask for them.  Round 3 built them by the plan of a
    // one-row cloud; a 65 536-point grid against itself then failed with "invalid argument" at its first pass.)
    const int group2 = icp::nn_model_may_be_hier(m, precision, c->tune) ? 512 : 0;
    const bool short_setup = precision == ICP_F32 && m > 0 && m <= icp_ctx::kPrepSmallMax && group2 == 0;
    const int m_pad = icp::pad_model(m);
    icp::PrepBuffers pb{};
    if (short_setup) {
        // (round 4: upload, layout and bounding cube without a synchronisation of their own; see decide_order_small)
        if (int rc = prep_buffers(c, m, pb)) return rc;
        icp_ctx::PrepSmall* small0 = (icp_ctx::PrepSmall*)c->prep_small.p;
        if (int rc = upload_cloud(c, xyz, m, m_pad, precision, c->Q, true, nullptr, small0->enc)) return rc;
    } else if (int rc = upload_cloud(c, xyz, m, m_pad, precision, c->Q)) return rc;
    if (precision == ICP_F32 && m > 0) {
        // scan copy for the early-out matching kernels: exact duplicates of a lower-index point (and the padding)
        // voided to +inf -- they can never be the lowest-index minimum (see NNCullInputs).  Flags, Morton order and
        // the extent test are computed on the device from the uploaded cloud.
        if (!short_setup) if (int rc = prep_buffers(c, m, pb)) return rc;
        icp_ctx::PrepSmall* small = (icp_ctx::PrepSmall*)c->prep_small.p;
        HIP_TRY(c->Qs.ensure(3 * (size_t)m_pad * sizeof(float)));
        if (m <= (1 << 21)) {
            // exact duplicates by hashing: two launches instead of three radix sorts (icp_k_setup.hip)
            unsigned int entries = 1024u;
            while (entries < 2u * (unsigned int)m) entries <<= 1;
            if ((size_t)entries * sizeof(unsigned int) > c->dup_table.cap) {
                HIP_TRY(c->dup_table.ensure((size_t)entries * sizeof(unsigned int)));
                HIP_TRY(hipMemsetAsync(c->dup_table.p, 0, c->dup_table.cap, c->stream));
                c->dup_gen = 0;
            }
            if (++c->dup_gen > 255u) {   // (generation 0 is "never written")
                HIP_TRY(hipMemsetAsync(c->dup_table.p, 0, c->dup_table.cap, c->stream));
                c->dup_gen = 1;
            }
            HIP_TRY(icp::launch_duplicates_hashed((const float*)c->Q.p, m, m_pad, (unsigned int*)c->dup_table.p, entries, c->dup_gen, (unsigned char*)c->prep_voided.p,
                                                  &small->voided, (float*)c->Qs.p, c->stream));
        } else {
            HIP_TRY(icp::launch_duplicates_and_scan_copy(pb, (const float*)c->Q.p, m, m_pad, (unsigned char*)c->prep_voided.p, &small->voided,
                                                         (float*)c->Qs.p, c->stream));
        }
        if (short_setup) {
            if (int rc = decide_order_small(c, pb, c->Q.p, m, m_pad, 8, c->memo_model, &c->model_sorted, &c->voided, "model")) return rc;
        } else {
            HIP_TRY(icp::launch_morton_order(pb, (const float*)c->Q.p, m, m_pad, 8, group2, (int32_t*)c->prep_perm.p, small->totals, c->stream));
            if (int rc = morton_decision(c, m, 8, group2, &c->model_sorted, &c->voided)) return rc;
        }
        // the sparse kernel's view: the same voided copy, in Morton order if the model's own order has no locality
        const void* view = c->Qs.p;
        if (c->model_sorted) {
            HIP_TRY(c->Qss.ensure(3 * (size_t)m_pad * sizeof(float)));
            HIP_TRY(c->Qperm.ensure((size_t)m_pad * sizeof(int32_t)));
            HIP_TRY(icp::launch_gather_sorted((const float*)c->Qs.p, m, m_pad, (const int32_t*)c->prep_perm.p, (float*)c->Qss.p,
                                              (int32_t*)c->Qperm.p, c->stream));
            view = c->Qss.p;
        }
        // bounding boxes of its 8-point chunks (the first, cheapest level of the early-out) and one point per chunk
        HIP_TRY(c->Qbox.ensure(icp::model_boxes_bytes(m_pad)));
        HIP_TRY(c->Qsamp.ensure(icp::model_samples_bytes(m_pad)));
        if (group2 == 0) {   // (searched flat: the upper box levels are never read -- one launch for boxes and samples)
            HIP_TRY(icp::launch_model_boxes_samples(view, m_pad, (float*)c->Qbox.p, (float*)c->Qsamp.p, c->stream));
        } else {
            HIP_TRY(icp::launch_model_boxes(view, m_pad, (float*)c->Qbox.p, c->stream));
            HIP_TRY(icp::launch_model_samples(view, m_pad, (float*)c->Qsamp.p, c->stream));
        }
        c->have_records = false;
        if (group2 > 0) {   // a model searched through the box hierarchy: the hits are fetched from per-chunk records
            HIP_TRY(c->Qrec.ensure(icp::model_records_bytes(m_pad)));
            HIP_TRY(icp::launch_model_records(view, (const float*)c->Qbox.p, c->model_sorted ? (const int32_t*)c->Qperm.p : nullptr, m_pad, (float*)c->Qrec.p, c->stream));
            c->have_records = true;
        }
        c->have_scan_copy = true;
    }
    if (precision == ICP_F64 && m > 0) {
        // fp64 on the sparse structure: the scan copy (exact duplicates of a lower-index point and the padding voided to
        // +inf -- the hall scan's 4361 coincident points would otherwise put 545 chunks on every origin point's hit list),
        // its chunk boxes and the cold-start samples, all in double.  No Morton view is built: the CPU path's clouds are
        // grids and scans, which have locality.
        if (int rc = prep_buffers(c, m, pb)) return rc;
        icp_ctx::PrepSmall* small = (icp_ctx::PrepSmall*)c->prep_small.p;
        HIP_TRY(c->Qs.ensure(3 * (size_t)m_pad * sizeof(double)));
        HIP_TRY(icp::launch_duplicates_and_scan_copy_f64(pb, (const double*)c->Q.p, m, m_pad, (unsigned char*)c->prep_voided.p, &small->voided,
                                                         (double*)c->Qs.p, c->stream));
        HIP_TRY(c->Qbox.ensure(icp::model_boxes_f64_bytes(m_pad)));
        HIP_TRY(c->Qsamp.ensure(icp::model_samples_f64_bytes(m_pad)));
        HIP_TRY(icp::launch_model_tables_f64(c->Qs.p, m_pad, c->Qbox.p, c->Qsamp.p, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->model_sorted = false;
        c->have_scan_copy = true;
    }
    c->have_model = true;
    return ICP_OK;
}

int icp_set_moving(icp_ctx* c, const void* xyz, int n, int precision)
{
    if (int rc = use(c)) return rc;
    if (int rc = check_precision(precision)) return rc;
    if (n < 0 || (n > 0 && !xyz)) return fail(ICP_ERR_INVALID, "bad moving cloud");
    if (c->have_model && c->prec != precision)
        return fail(ICP_ERR_INVALID, "moving cloud precision differs from the resident model");
    c->prec = precision;
    c->n = n;
    c->loop.active = false;
    c->idx_valid = false;
    c->have_moving = false;    // (until the upload has been accepted)
    const bool judged = precision == ICP_F32 && n > 128;
    const bool short_setup = judged && n <= icp_ctx::kPrepSmallMax;
    if (n > 0) HIP_TRY(c->P0.ensure(3 * (size_t)icp::pad_moving(n) * icp::elem_size(precision)));
    if (short_setup) {
        // (round 4: one layout launch writes the cloud, its pristine copy and the bounding cube; no synchronisation until the order is decided)
        icp::PrepBuffers pb{};
        if (int rc = prep_buffers(c, n, pb)) return rc;
        if (int rc = upload_cloud(c, xyz, n, icp::pad_moving(n), precision, c->P, true, c->P0.p, ((icp_ctx::PrepSmall*)c->prep_small.p)->enc)) return rc;
    } else if (int rc = upload_cloud(c, xyz, n, icp::pad_moving(n), precision, c->P, false, n > 0 ? c->P0.p : nullptr)) return rc;
    c->moving_sorted = false;
    c->moving_group = 0;
    if (judged) {
        // judged on the groups the matching kernel will work on (rows of 64 or of 128 points: nn_plan's rule, overrides
        // included); with no model resident yet the plan assumes one of the moving cloud's size -- ensure_work_buffers looks again
        const icp::NNPlan guess = icp::nn_plan(n, c->have_model && c->m > 0 ? c->m : n, precision, c->num_cus, c->tune);
        if (int rc = decide_moving_order(c, c->P.p, icp::nn_moving_group(guess), short_setup)) return rc;
    }
    c->have_moving = true;
    c->moving_is_pristine = false;
    c->moving_untouched = true;
    return ICP_OK;
}

int icp_reset_moving(icp_ctx* c)
{
    if (int rc = use(c)) return rc;
    if (!c->have_moving) return fail(ICP_ERR_STATE, "no moving cloud resident");
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    c->moving_is_pristine = true;
    c->moving_untouched = true;
    c->loop.active = false;
    c->idx_valid = false;
    return ICP_OK;
}

int icp_set_model_normals(icp_ctx* c, const void* nxyz, int m)
{
    if (int rc = use(c)) return rc;
    if (!c->have_model) return fail(ICP_ERR_STATE, "set the model before its normals");
    if (m != c->m || (m > 0 && !nxyz)) return fail(ICP_ERR_INVALID, "normal count must equal the model size");
    c->have_normals = false;
    if (int rc = upload_cloud(c, nxyz, m, icp::pad_model(m), c->prec, c->Nrm)) return rc;
    c->have_normals = true;
    return ICP_OK;
}

int icp_get_moving(icp_ctx* c, void* out)
{
    if (int rc = use(c)) return rc;
    if (int rc = materialize_moving(c)) return rc;
    if (!c->have_moving) return fail(ICP_ERR_STATE, "no moving cloud resident");
    if (c->n == 0) return ICP_OK;
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    const size_t bytes = 3 * (size_t)c->n * icp::elem_size(c->prec);
    HIP_TRY(c->stage.ensure(bytes));
    HIP_TRY(icp::launch_soa_to_aos(c->prec, c->P.p, c->n, icp::pad_moving(c->n), c->stage.p, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->stage.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ICP_OK;
}

int icp_get_indices(icp_ctx* c, int32_t* out)
{
    if (int rc = use(c)) return rc;
    return download_idx(c, c->cur, out);
}

}  // extern "C"
#pragma GCC visibility pop
