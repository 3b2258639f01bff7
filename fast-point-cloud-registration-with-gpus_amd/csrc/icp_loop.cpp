// icp_loop.cpp -- the ICP driver loops (icp_loop_*, icp_point_to_*) that replace the reference's main() while-loops
//   src/ICP_CPU.c:217-271, src/ICP_point_to_point.cu:295-423, src/ICP_point_to_plane.cu:517-631.
//
// Loop shape (one host round trip per iteration, no H2D traffic at all):
//
//   enqueue k:  [transform_error(R_{k-1}, t_{k-1})]  ->  nn_match  ->  moments  ->  finalize
//               (R, t travel as kernel arguments)        P_k vs Q      fused       32 doubles
//   <optional all-reduce of the 32-double vector across ranks, in place, on the same stream>
//   complete k: D2H 256 B, E[k] and the stop rule on the host, 3x3 SVD / 6x6 Cholesky -> R_k, t_k
//
// The error of transform k-1 rides in slot 0 of the vector produced by enqueue k, so matching pass k
// is issued speculatively before the stop rule for E[k] is known; when the rule fires that one
// pass is discarded (it never touched P).  Correspondences ping-pong between two buffers so the
// indices of the last CONTRIBUTING pass survive the speculative one.
//
// This file holds the loop's decisions: which form runs, what is pending, when to arm, withdraw or redo.  The bytes that travel
// between the host and a running kernel -- mailbox lines, row formats, the row sweep, the adders, the tags -- are icp_wire.h's.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <unistd.h>

#include "../../include/icp_mi355x_diag.h"
#include "icp_comm.h"
#include "icp_ctx.h"

namespace {

// one message to the kernel listening at mb, in the registration's precision (ICP_MAILBOX=plain: written word by word)
inline void post(const icp_ctx* c, icp::NNMailbox* mb, const double* R9, const double* t3, int cmd, double seq)
{
    if (c->prec == ICP_F64) icp::post_message64(mb, R9, t3, cmd, seq, c->mail_wide);
    else icp::post_message(mb, R9, t3, cmd, seq, c->mail_wide);
}

// Time budgets of a kernel that waits for the host, ordered so that a late host and a waiting kernel can never disagree:
//   * a waiting block gives up (and reads that as EXIT) only after ICP_MAILBOX_BUDGET_S of WALL-CLOCK time (icp_kernels.h);
//   * the host posts a message only while at most kMailLeaseS have passed since it last knew the kernel to be waiting (the
//     rows of the previous pass complete / the launch); when it is later than that -- descheduled, or held up in the
//     inter-rank exchange, whose own limit is longer -- it sends EXIT instead (an EXIT is consistent at any time: a block
//     that has already given up did exactly that) and relaunches.  kMailLeaseS < budget / 2;
//   * the host's wait for a pass's rows (kRowPollS) is shorter than the budget too: when it gives up it withdraws the
//     kernel and lets the runtime report what happened.
constexpr double kMailLeaseS = 1.5;
constexpr double kRowPollS = 2.0;
static_assert(kMailLeaseS * 2.0 < (double)ICP_MAILBOX_BUDGET_S && kRowPollS < (double)ICP_MAILBOX_BUDGET_S, "host budgets must stay inside the kernel's");

// Rows added up inside the matching launch (NNTail::fin_*, icp_device.h): the sparse kernels with rows of 128 points, a fused tail,
// and more rows than the host takes (host_rows_max).  to_host: the vector lands in pinned memory with the pass's tag (the host
// polls it) -- else in the device vector a collective, or the caller, goes on from.
bool fin_in_launch(const icp_ctx* c, const icp::NNPlan& pl)
{
    return c->fused_tail && c->sums_in_launch(pl) && c->fin_tickets.p != nullptr && c->fin_scratch.p != nullptr && c->h_final != nullptr;
}
bool fin_to_host(const icp_ctx* c) { return !c->comm && c->mom_dev == (double*)c->mom_own.p; }
// rows the host itself adds up (single GPU, or ranks meeting in host memory) leave the sparse point-to-point kernels in
// the compact two-cache-line form (icp_kernels.h, NNTailArgs)
bool use_compact_rows(const icp_ctx* c, const icp::NNPlan& pl, int metric, const double* rows)
{
    // (fp32 only: the compact row spends mantissa bits on its tag, and the fp64 path is held to 1e-12 against src/ICP_CPU.c's arithmetic)
    return c->prec == ICP_F32 && icp::nn_is_sparse(pl) && metric == ICP_POINT_TO_POINT && rows == c->h_mom_partials;
}

// The two row formats keep their completion tags in different places of the same pinned buffer: when the format changes
// (another metric, a communicator attached or removed -- never inside a loop) the buffer is wiped, so that no sum left by
// the other format can ever be mistaken for a tag.
void prepare_rows_format(icp_ctx* c, bool compact)
{
    const int want = compact ? 1 : 0;
    if (c->rows_format == want || !c->h_mom_partials) { c->rows_format = want; return; }
    std::memset(c->h_mom_partials, 0, c->rows_cap * ICP_NMOM * sizeof(double));
    icp::bar_fence();
    c->rows_format = want;
}

// ordered rows: sort the rows by the hits of the launch before (and zero the counters) -- enqueued right before a pass of the loop
int prepare_row_order(icp_ctx* c)
{
    if (!c->plan.order || c->row_hits.p == nullptr) { c->row_order = nullptr; return ICP_OK; }
    icp::RowOrderBuffers b{};
    for (int k = 0; k < 2; ++k) { b.keys[k] = (unsigned int*)c->order_keys[k].p; b.vals[k] = (int32_t*)c->order_vals[k].p; }
    b.temp = c->order_tmp.p;
    b.temp_bytes = c->order_tmp.cap;
    b.roles = (int32_t*)c->order_roles.p;
    b.totals = (unsigned long long*)c->order_totals.p;
    b.seq = c->order_seq++;
    c->order_launches++;
    // (8192 hits for a 16-wave block, and in proportion for smaller ones; the target itself: a quarter of a block slot's mean load)
    const int nw = c->plan.nw > 0 ? c->plan.nw : 16;
    b.min_part = c->split_min >= 0 ? c->split_min : 512 * nw;
    b.total_div = 4 * c->num_cus * (16 / nw);
    HIP_TRY(icp::launch_row_order(b, (unsigned int*)c->row_hits.p, c->plan.blocks_x, &c->row_order, c->stream));
    return ICP_OK;
}

}  // namespace

icp::NNCullInputs make_cull(const icp_ctx* c, const int32_t* seed)
{
    icp::NNCullInputs o{c->have_scan_copy ? c->Qs.p : nullptr, seed, c->use_boxes ? c->Qbox.p : nullptr, c->use_boxes ? c->Qsamp.p : nullptr};
    o.tune = &c->tune;
    if (c->count_work) o.work = (unsigned long long*)c->work.p;
    if (c->prec == ICP_F64) return o;   // (fp64: no sorted views)
    if (c->have_scan_copy && c->model_sorted) { o.Q_scan_sorted = c->Qss.p; o.q_perm = (const int32_t*)c->Qperm.p; }
    o.waves64 = c->exclusive ? 16 : 0;
    if (c->moving_sorted) o.p_perm = (const int32_t*)c->Pperm.p;
    if (c->plan.order && c->row_order != nullptr) { o.row_order = c->row_order; o.row_hits = (unsigned int*)c->row_hits.p; o.order_history = c->order_regs > 0; }
    if (c->have_records && c->use_boxes && c->plan.hier) o.records = (const float*)c->Qrec.p;
    if (c->plan.share_blocks > 0 && c->share_counts.p != nullptr) { o.share_counts = (unsigned int*)c->share_counts.p; o.share_seq = &c->share_seq; o.share_cold_seq = &c->share_cold_seq; o.seed_pub = (float*)c->seed_pub.p; }
    return o;
}

namespace {

// The fused tail of a matching pass (icp_kernels.h, NNTailArgs), the same for the plain, armed and resident forms -- one of
// the decisions that keep their results bit-identical.  host_reduce: the rows go to pinned memory and the host adds them up;
// else they stay on the device and, where the plan allows, the launch adds them up itself (fin_tickets set).
icp::NNTailArgs tail_args(const icp_ctx* c, const icp::NNPlan& pl, int32_t* idx_out, double tag, bool host_reduce)
{
    icp::NNTailArgs ta{};
    ta.metric = c->loop.H.prm.metric;
    ta.keys = (unsigned long long*)c->keys.p;
    ta.tickets = (unsigned int*)c->tickets.p;
    ta.err_tile = (double*)c->err_partials.p;
    ta.idx_out = idx_out;
    ta.Nrm_soa = c->Nrm.p;
    ta.rows = host_reduce ? c->h_mom_partials : (double*)c->mom_partials.p;
    ta.tag = tag;
    ta.compact = use_compact_rows(c, pl, ta.metric, ta.rows) ? 1 : 0;
    ta.rows_on_device = host_reduce ? 0 : 1;
    if (!host_reduce && fin_in_launch(c, pl)) {
        ta.fin_tickets = (unsigned int*)c->fin_tickets.p;
        ta.fin_scratch = (double*)c->fin_scratch.p;
        ta.fin_host = fin_to_host(c) ? 1 : 0;
        ta.fin_out = ta.fin_host ? c->h_final : c->mom_dev;
    }
    return ta;
}

// The pass just issued -- enqueued, released from its mailbox, or sent to the resident kernel -- is the one the next complete
// waits for: how many rows, in which format, who adds them up, and under which tag.  slot_written: it leaves its points and
// matches in slot order, in the other plane of the slot-order points (the next such launch starts from them).
void set_pending(LoopState& L, int mom_blocks, int err_blocks, bool compact, bool host_reduce, bool final_poll, bool timed, double tag,
                 bool slot_written, int route)
{
    L.route = route | (host_reduce ? ICP_ROUTE_HOST_ROWS : 0) | (compact ? ICP_ROUTE_COMPACT : 0);
    L.mom_blocks = mom_blocks;
    L.err_blocks = err_blocks;
    L.rows_compact = compact;
    L.host_reduce = host_reduce;
    L.final_poll = final_poll;
    L.timed_nn = timed;
    L.wait_tag = tag;
    L.pending = true;
    L.slot_written = slot_written;
    if (slot_written) L.slot_flip = !L.slot_flip;
}

// icp_set_profiling: a launch bracketed by the events ev0 / ev1 has ended -- its time joins the loop's and the context's totals
int add_timed_launch(icp_ctx* c, long long passes)
{
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->loop.seconds_nn += 1e-3 * ms;
    c->prof_seconds_nn += 1e-3 * ms;
    c->prof_nn_launches += 1;
    c->prof_nn_passes += passes;
    return ICP_OK;
}

// A pass of icp_loop_run failed.  If it completed on the device and the MINIMISATION refused its sums, the cloud is in the state
// the last applied transform left and the loop's counters and error series stay readable.  Otherwise blocks may have applied its
// transform to their part of the cloud and others not: nothing of that state is offered to the caller -- the loop is over, the
// moving cloud goes back to what icp_set_moving uploaded (materialised from the pristine copy on its next use), the matches are
// void.  Returns true when the loop was abandoned.
bool abandon_loop(icp_ctx* c)
{
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    if (c->loop.numeric_failure) return false;
    c->moving_is_pristine = true;
    c->idx_valid = false;
    c->loop.active = false;
    c->loop.pending = false;
    return true;
}

// test hook (ICP_DEBUG=stall=pass:seconds): the host sleeps once, right before it would publish the message of that pass
void debug_stall(icp_ctx* c)
{
    if (c->debug_stall_pass < 0 || c->loop.H.applied != c->debug_stall_pass) return;
    c->debug_stall_pass = -1;
    usleep((useconds_t)(c->debug_stall_s * 1e6));
}

// ---- the three waits of a complete -------------------------------------------------------------------------------
const icp::RowFormat& pending_format(const LoopState& L) { return L.rows_compact ? icp::kCompactRows : icp::kFullRows; }

// The kernels wrote their partial rows into mapped pinned memory.  Instead of a stream synchronisation the host polls the
// per-row completion tags (icp_wire.h, sweep_rows); the matching kernel's error rows were complete before the moments
// kernel started.  sum_host_rows adds the rows up in block order once all are there.
int wait_host_rows(icp_ctx* c, bool tracing)
{
    LoopState& L = c->loop;
    const icp::RowFormat& fmt = pending_format(L);
    const int rows = L.mom_blocks;
    if (rows > 0 && !L.timed_nn && L.err_blocks == 0) {
        // (the poll's start: what the 2 s time-out counts from; the host got here right after posting the message, whose
        // time the resident loop has just read -- an armed or plain pass reads the clock itself)
        const auto t0 = L.live_mailbox != nullptr && !tracing ? c->posted_at : std::chrono::steady_clock::now();
        const int left = icp::sweep_rows(c->h_mom_partials, rows, fmt, L.wait_tag, c->rows_seen, t0, kRowPollS, c->trace_passes ? &c->tr_first_row : nullptr);
        c->rows_done_at = std::chrono::steady_clock::now();
        if (c->trace_passes) { c->tr_last_row = std::chrono::duration<double>(c->rows_done_at - t0).count(); c->tr_rows_done = c->rows_done_at; }
        if (left == 0) return ICP_OK;
        if (c->trace) {
            std::fprintf(stderr, "[icp trace]   poll gave up with %d of %d rows in; rows still missing:", rows - left, rows);
            int shown = 0;
            for (int r = 0; r < rows && shown < 40; ++r)
                if (!c->rows_seen[r]) { std::fprintf(stderr, " %d", r); ++shown; }
            std::fprintf(stderr, "\n");
        }
    }
    // not polled (a timed pass, error rows of their own) or the poll gave up: a resident kernel would go on waiting for its
    // next message -- withdraw it (under the tag it will wait for) -- and let the stream say what happened
    if (L.live_mailbox) post(c, L.live_mailbox, nullptr, nullptr, icp::ICP_CMD_EXIT, L.wait_tag + 1.0);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double want = fmt.shows(L.wait_tag);
    for (int b = 0; b < rows; ++b)
        if (icp::row_tag(c->h_mom_partials, b, fmt) != want) {
            L.pending = false;
            char msg[240];
            int have = 0;
            for (int r = 0; r < rows; ++r) have += icp::row_tag(c->h_mom_partials, r, fmt) == want ? 1 : 0;
            std::snprintf(msg, sizeof msg, "a matching pass ended without producing its rows: row %d of %d carries tag %.0f, expected %.0f; %d rows arrived (armed / resident launch timed out?)",
                          b, rows, icp::row_tag(c->h_mom_partials, b, fmt), want, have);
            c->rows_timed_out = true;
            return fail(ICP_ERR_HIP, msg);
        }
    return ICP_OK;
}

// The pending pass's rows (and error rows) added up into c->h_mom, rows in block order: every slot is the same sum whichever
// adder runs (ICP_MAILBOX=plain keeps the scalar loop: the same bits, for the A/B).
// Returns ICP_ROUTE_AVX when a wide adder ran, else 0.
int sum_host_rows(icp_ctx* c)
{
    const LoopState& L = c->loop;
    double* mom = c->h_mom;
    for (int k = 0; k < ICP_NMOM; ++k) mom[k] = 0.0;
    for (int b = 0; b < L.err_blocks; ++b) mom[ICP_MOM_ERR] += c->h_err_partials[b];
    // (a compact row does not carry its point count: a row of the sparse kernels holds the real points of its slots)
    if (L.rows_compact) mom[ICP_MOM_CNT] = (double)c->n;
    if (L.mom_blocks == 0) return 0;
    return icp::sum_rows(c->h_mom_partials, L.mom_blocks, pending_format(L), c->mail_wide, mom) ? ICP_ROUTE_AVX : 0;
}

// the launch itself added its rows up and leaves the vector in pinned memory, the pass's tag in its last slot
int wait_final_vector(icp_ctx* c)
{
    LoopState& L = c->loop;
    const volatile double* fin = c->h_final;
    bool there = false;
    if (!L.timed_nn) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 1; !(there = fin[ICP_NMOM - 1] == L.wait_tag); ++spins)
            if ((spins & 0x3ff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kRowPollS) break;
        c->rows_done_at = std::chrono::steady_clock::now();
    }
    if (!there) {
        // (a timed pass is completed with a synchronisation; so is one whose tag never came: the runtime says what happened)
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (fin[ICP_NMOM - 1] != L.wait_tag) {
            L.pending = false;
            char msg[200];
            std::snprintf(msg, sizeof msg, "a matching pass ended without leaving its sums: the vector carries tag %.0f, expected %.0f (armed launch timed out?)",
                          fin[ICP_NMOM - 1], L.wait_tag);
            c->rows_timed_out = true;
            return fail(ICP_ERR_HIP, msg);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int k = 0; k < ICP_NMOM - 1; ++k) c->h_mom[k] = fin[k];
    c->h_mom[ICP_NMOM - 1] = 0.0;
    return ICP_OK;
}

// the vector was finalised on the device (and all-reduced across ranks there): 256 bytes come back
int copy_back(icp_ctx* c)
{
    HIP_TRY(hipMemcpyAsync(c->h_mom, c->mom_dev, ICP_NMOM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ICP_OK;
}

// ---- one step: enqueue + complete ---------------------------------------------------------------------------------
int loop_enqueue_body(icp_ctx* c)
{
    LoopState& L = c->loop;
    if (!L.active || L.H.done || L.pending) return fail(ICP_ERR_STATE, "enqueue: loop not ready");
    if (int rc = materialize_moving(c)) return rc;
    const auto tr0 = std::chrono::steady_clock::now();
    const icp::NNPlan& pl = c->plan;
    int mom_blocks = 0, err_blocks = 0;
    const bool host_reduce = c->host_reduce();
    double* err_rows = (double*)c->err_partials.p;  // device: the moments kernel folds them into its rows
    const bool apply = L.H.have_rt;
    const bool final_only = L.H.next_is_final();  // the loop ends after this error whatever it is
    // the transform of the previous pass rides in the front of the matching kernel when that kernel
    // supports it; otherwise (fp64, or nothing left to match) it is its own launch
    const bool fused = apply && !final_only && icp::nn_can_fuse_transform(pl);
    if (apply) {
        if (!fused)  // with nothing left to match, the last pass's rows go straight to the host
            HIP_TRY(icp::launch_transform_error(c->prec, c->P.p, c->n, pl.n_pad, L.H.R, L.H.t, c->Q.p, pl.m_pad,
                                                (const int32_t*)c->idx[c->cur].p,
                                                (final_only && host_reduce) ? c->h_err_partials : err_rows,
                                                &err_blocks, c->stream));
        L.applied_idx = c->cur;
        L.H.note_applied();
    }
    // fused tail: the matching kernel itself merges the segments (atomic keys), stores idx and produces the
    // moment rows -- no partial arrays, no second launch.  ICP_FUSED_TAIL=0 keeps the two-kernel form.
    const bool tail = !final_only && c->fused_tail && icp::nn_can_fuse_tail(pl);
    icp::NNTailArgs ta{};
    bool timed = false, slots = false;
    if (!final_only) {
        // the previous pass's matches seed the early-out bound (any valid index would do)
        if (tail) { if (int rc = prepare_row_order(c)) return rc; } else c->row_order = nullptr;
        const icp::NNCullInputs cull = make_cull(c, L.matched ? (const int32_t*)c->idx[c->cur].p : nullptr);
        c->cur ^= 1;
        L.matched = true;
        c->idx_valid = true;
        const bool time_this = c->profile_stride > 0 && (c->nn_launch_count++ % (uint64_t)c->profile_stride) == 0;
        if (time_this) { HIP_TRY(hipEventRecord(c->ev0, c->stream)); }
        if (tail) ta = tail_args(c, pl, (int32_t*)c->idx[c->cur].p, (double)icp::take_tags(c->tag_seq, 1), host_reduce);
        if (host_reduce) prepare_rows_format(c, ta.compact != 0);   // (also the two-kernel form: launch_moments writes full rows)
        icp::NNFusedTransform ft{L.H.R, L.H.t, (const int32_t*)c->idx[L.applied_idx].p, c->P2.p, err_rows};
        // every fused pass of the sparse kernels leaves its points and matches in slot order; the next one starts from them
        // (one level of coalesced loads instead of slot -> point -> seed -> model point), as the armed launches do
        if (fused && tail && icp::nn_keeps_slot_order(pl) && c->slot_state.ensure(9 * (size_t)pl.n_pad * sizeof(float)) == hipSuccess) {
            ft.slot_state = c->slot_state.p;
            ft.slot_valid = L.slot_written;
            ft.slot_flip = L.slot_flip;
            slots = true;
        }
        HIP_TRY(icp::launch_nn(pl, c->P.p, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, fused ? &ft : nullptr, &cull, tail ? &ta : nullptr, c->stream));
        if (fused) {
            std::swap(c->P, c->P2);  // the moved cloud is the current one from here on
            err_blocks = pl.blocks_x;
        }
        if (time_this) { HIP_TRY(hipEventRecord(c->ev1, c->stream)); timed = true; }
        if (tail) {
            mom_blocks = pl.blocks_x;   // one row per row of matching blocks, error share in slot 0
            err_blocks = 0;
        } else {
            HIP_TRY(icp::launch_moments(pl, L.H.prm.metric, c->P.p, c->Q.p, c->Nrm.p, c->part_d.p,
                                        (const int32_t*)c->part_idx.p, (int32_t*)c->idx[c->cur].p, host_reduce ? c->h_mom_partials : (double*)c->mom_partials.p,
                                        &mom_blocks, (double)icp::take_tags(c->tag_seq, 1), err_rows, err_blocks, c->stream));
            if (host_reduce) err_blocks = 0;  // already inside the moment rows
        }
    }
    const bool fin = ta.fin_tickets != nullptr;   // this pass's rows are added up inside its launch
    int route = final_only ? ICP_ROUTE_ERROR_ONLY : tail ? ICP_ROUTE_FUSED_TAIL : ICP_ROUTE_MOMENTS_KERNEL;
    if (fin) route |= ICP_ROUTE_FIN_LAUNCH | (fin_to_host(c) ? ICP_ROUTE_FIN_PINNED : 0);
    if (!host_reduce) {
        if (!fin) {
            route |= ICP_ROUTE_FIN_KERNEL | (mom_blocks > 2048 ? ICP_ROUTE_FIN_TWO_STAGE : 0);
            if (mom_blocks > 2048) HIP_TRY(c->fin_scratch.ensure(256 * ICP_NMOM * sizeof(double)));
            HIP_TRY(icp::launch_finalize(c->mom_dev, (const double*)c->mom_partials.p, mom_blocks,
                                         (const double*)c->err_partials.p, err_blocks, tail ? 1 : 0, c->stream, (double*)c->fin_scratch.p));
        }
        if (c->comm) {  // the iteration's one collective: 32 doubles, in place, on the loop's stream
            std::string err;
            if (int rc = icp::comm_allreduce_sum_f64(c->comm, c->mom_dev, ICP_NMOM, c->stream, err)) return fail(rc, err);
        }
    }
    set_pending(L, mom_blocks, err_blocks, ta.compact != 0, host_reduce, fin && fin_to_host(c), timed, (double)c->tag_seq, slots, route);
    if (c->trace) c->tr_enqueue += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
    return ICP_OK;
}

// (icp_loop_run's forms call this once per pass: the device was selected and the thread placed when the call came in --
// a hipSetDevice and a sched_getcpu per pass are a measurable part of a 9 us iteration)
int loop_complete_body(icp_ctx* c, int* done)
{
    LoopState& L = c->loop;
    if (!L.active || !L.pending) return fail(ICP_ERR_STATE, "complete without enqueue");
    // (clock reads cost ~25 ns apiece and there were seven per pass: the ones that only feed ICP_TRACE are taken when it is on)
    const bool tracing = c->trace || c->trace_passes;
    const auto tr0 = tracing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point{};
    if (int rc = L.host_reduce ? wait_host_rows(c, tracing) : L.final_poll ? wait_final_vector(c) : copy_back(c)) return rc;
    const auto tr1 = tracing ? std::chrono::steady_clock::now() : tr0;
    if (L.host_reduce) L.route |= sum_host_rows(c);
    const auto tr2 = tracing ? std::chrono::steady_clock::now() : tr1;
    L.pending = false;
    if (L.timed_nn)
        if (int rc = add_timed_launch(c, 1)) return rc;
    if (c->lcomm && c->mom_dev == (double*)c->mom_own.p) {  // the node's ranks exchange their sums (rank order: identical on every rank)
        std::string err;
        // (only the entries the metric uses travel: 19 doubles = 3 cache lines per slot instead of 5)
        const int used = L.H.prm.metric == ICP_POINT_TO_PLANE ? ICP_MOM_B + 6 : ICP_MOM_SQQ + 1;
        if (int rc = icp::lcomm_allreduce_sum_f64(c->lcomm, c->h_mom, used, err)) return fail(rc, err);
    }
    // (the host half of a pass is timed only while profiling is on: two clock reads are 0.5 % of a 9 us iteration)
    const bool time_host = c->profile_stride > 0;
    const auto th0 = time_host ? std::chrono::steady_clock::now() : tr2;
    L.mom_valid = true;   // (icp_diag_loop_moments: c->h_mom as the host half receives it)
    const int adv = L.H.advance(c->h_mom);
    if (time_host) L.seconds_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - th0).count();
    if (adv != ICP_OK) {
        if (done) *done = 1;
        L.numeric_failure = true;   // (the loop is over; what its completed passes produced stays readable: icp_loop_state)
        return fail(adv, "minimisation failed (degenerate correspondences)");
    }
    if (c->trace) {
        const auto tr3 = std::chrono::steady_clock::now();
        c->tr_wait += std::chrono::duration<double>(tr1 - tr0).count();
        c->tr_reduce += std::chrono::duration<double>(tr2 - tr1).count();
        c->tr_solve += std::chrono::duration<double>(tr3 - tr2).count();
        c->tr_n += 1;
    }
    L.steps += 1;
    if (done) *done = L.H.done ? 1 : 0;
    return ICP_OK;
}

// what an armed and a resident launch both need: a mailbox the kernel can poll, the fused tail of the sparse kernels over the
// resident scan copy and its boxes, and a loop that goes on
bool mailbox_launch_possible(const icp_ctx* c)
{
    const icp::NNPlan& pl = c->plan;
    return c->h_mail && (c->relay || c->mail_in_bar) && c->fused_tail && icp::nn_is_sparse(pl) && icp::nn_can_fuse_tail(pl) && c->have_scan_copy && c->use_boxes &&
           c->loop.active && !c->loop.H.done;
}

}  // namespace

// (share_wants_resident, can_arm, loop_arm, loop_release_armed, loop_withdraw_armed, can_reside and loop_run_resident have
// always been exported under their C names -- an accident of where they were once defined; kept, so that the library's
// symbol table stays what it was)
#pragma GCC visibility push(default)
extern "C" {

// ---- armed launches ------------------------------------------------------------------------------
// icp_loop_run keeps one matching pass enqueued AHEAD of the (R, t) it will apply: the kernel is launched and
// dispatched while the previous pass still runs and the host still solves, waits on a mailbox in pinned memory
// and starts the moment the solution is published -- the launch + dispatch latency (~8 us of a ~23 us iteration
// on the hall cloud) leaves the critical path.  If the loop stops instead, the pass is withdrawn and exits
// without having touched anything.

// A plan with shared rows (33-57 k moving points) runs armed launches: every launch deals its blocks anew, by the hits of the
// launch before.  A resident kernel can share its rows too -- its blocks keep, for the whole launch, the roles the counts at
// its start give them; whichever block closes a split row publishes the matches for the others -- and is what ICP_RESIDENT=2
// (from the first pass, by the counts of the registration before) and ICP_SHARE_RESIDENT_AFTER=n (after n armed passes) select.
// Measured on Bunny.csv, registrations repeated in one context: 32.9 us per iteration armed, 30.7 resident from the start,
// 33.2 switching after 6 passes; a context's FIRST registration has no counts and runs a resident launch unshared (late passes
// of 42 us instead of 24), which is why armed is the default.
bool share_wants_resident(const icp_ctx* c)
{
    if (!(c->plan.share_blocks > 0 && c->resident == 1 && !c->resident_refused)) return false;
    // Round 3 default: a context's FIRST registration of a geometry has no counts to deal the roles by -- it runs armed launches,
    // which adapt within one pass; from the second registration on the counts of the one before are there, and the whole
    // registration is ONE resident kernel with shared rows (Bunny.csv, registrations repeated in one context: 32.9 -> 30.7 us per
    // iteration, profiles/r2/r2_03_bunny_shared_rows.txt).  ICP_SHARE_AUTO=0: armed throughout, as in round 2.
    if (c->share_auto && c->share_cold_seq >= 1 && c->loop.H.applied == 0 && !c->loop.matched) return true;
    // Round 4: the FIRST registration does not stay armed to its end either -- its cold pass has left counts (share_cold_seq == 1),
    // and from its second pass on it is one resident kernel dealt by them: 33.1 -> 31.7 us per iteration for that one registration
    // (profiles/r4/r4_12_bunny_first_registration_anatomy.txt, ICP_SHARE_RESIDENT_AFTER=2; = 3, 4: the same).
    if (c->share_auto && c->share_resident_after < 0 && c->share_cold_seq == 1 && c->loop.matched && c->loop.H.applied >= 1) return true;
    return c->share_resident_after >= 0 && c->loop.H.applied + 1 >= c->share_resident_after;
}


bool can_arm(icp_ctx* c)
{
    const LoopState& L = c->loop;
    const icp::NNPlan& pl = c->plan;
    return c->arm && !c->shares_device && !share_wants_resident(c) && c->prec == ICP_F32 && mailbox_launch_possible(c) &&
           (c->host_reduce() || (fin_in_launch(c, pl) && fin_to_host(c))) && icp::nn_can_fuse_transform(pl) &&
           L.pending && !L.armed && L.matched && !L.H.have_rt &&
           !L.timed_nn &&  // a timed pass is completed with a stream synchronisation: nothing may wait behind it
           L.H.applied + 1 < L.H.prm.max_iter &&  // the pass after the pending one still matches (it is not the final, error-only one)
           !(c->profile_stride > 0 && (c->nn_launch_count % (uint64_t)c->profile_stride) == 0);  // timed launches stay plain
}

int loop_arm(icp_ctx* c)
{
    LoopState& L = c->loop;
    const icp::NNPlan& pl = c->plan;
    if (int rc = prepare_row_order(c)) return rc;
    const icp::NNCullInputs cull = make_cull(c, (const int32_t*)c->idx[c->cur].p);
    const int prev_cur = c->cur;
    const int slot = (int)(c->mail_seq++ % kMailSlots);
    icp::NNMailbox* mb = mail_slot(c->h_mail, slot);
    const double tag = (double)icp::take_tags(c->tag_seq, 1);
    post(c, mb, nullptr, nullptr, icp::ICP_CMD_EXIT, 0.0);   // cleared: nothing to act on yet
    // (can_arm: the host adds the rows up, or the launch does and the vector comes back in pinned memory)
    const bool host_rows = c->host_reduce();
    const icp::NNTailArgs ta = tail_args(c, pl, (int32_t*)c->idx[prev_cur ^ 1].p, tag, host_rows);
    L.armed_compact = ta.compact != 0;
    if (host_rows) prepare_rows_format(c, L.armed_compact);
    icp::NNFusedTransform ft{nullptr, nullptr, (const int32_t*)c->idx[prev_cur].p, c->P2.p, (double*)c->err_partials.p, mb, c->mail_in_bar ? nullptr : c->relay, tag};
    // every armed pass leaves its points and matches in slot order; the next one starts from them (one level of
    // coalesced loads instead of slot -> point -> seed -> model point) if the pass before it was such a pass
    if (pl.splits == 1 && c->slot_state.ensure(9 * (size_t)pl.n_pad * sizeof(float)) == hipSuccess) {
        ft.slot_state = c->slot_state.p;
        ft.slot_valid = L.slot_written;
        ft.slot_flip = L.slot_flip;
    }
    if (c->profile_stride > 0) c->nn_launch_count++;
    HIP_TRY(icp::launch_nn(pl, c->P.p, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, &ft, &cull, &ta, c->stream));
    std::swap(c->P, c->P2);
    c->cur = prev_cur ^ 1;
    L.armed = true;
    L.armed_at = std::chrono::steady_clock::now();
    L.armed_tag = tag;
    L.armed_slot = slot;
    L.armed_prev_cur = prev_cur;
    return ICP_OK;
}

// the solution is in: publish it to the waiting kernel, which becomes the pending pass
void loop_release_armed(icp_ctx* c)
{
    LoopState& L = c->loop;
    if (c->debug_lose_pass >= 0 && L.H.applied == c->debug_lose_pass) c->debug_lose_pass = -1;   // (test hook: this message is lost)
    else post(c, mail_slot(c->h_mail, L.armed_slot), L.H.R, L.H.t, icp::ICP_CMD_TRANSFORM_MATCH, L.armed_tag);
    L.applied_idx = L.armed_prev_cur;
    L.H.note_applied();
    L.armed = false;
    const bool host_rows = c->host_reduce();
    set_pending(L, c->plan.blocks_x, 0, L.armed_compact, host_rows, !host_rows, false, L.armed_tag, c->plan.splits == 1 && c->slot_state.p != nullptr,
                ICP_ROUTE_ARMED | ICP_ROUTE_FUSED_TAIL | (host_rows ? 0 : ICP_ROUTE_FIN_LAUNCH | ICP_ROUTE_FIN_PINNED));
}

// the loop ended (or failed): the waiting kernel exits without touching anything; undo the bookkeeping
void loop_withdraw_armed(icp_ctx* c)
{
    LoopState& L = c->loop;
    if (!L.armed) return;
    post(c, mail_slot(c->h_mail, L.armed_slot), nullptr, nullptr, icp::ICP_CMD_EXIT, L.armed_tag);
    std::swap(c->P, c->P2);
    c->cur = L.armed_prev_cur;
    L.armed = false;
}

// ---- resident registration ---------------------------------------------------------------------------
// One launch (every block resident) carries the whole loop: the blocks keep their points in registers and their seeds in
// LDS, every pass is one mailbox message (command + R, t) and one set of rows coming back.  No launch, no
// dispatch and no kernel boundary between two passes; what is left of an iteration is the pass itself plus one
// host <-> device round trip (~2 us, tools/mailbox_probe.hip).  The host side is the step-wise loop unchanged:
// the same HostLoop decides, the same rows are reduced in the same order -- the results are bit-identical.
bool can_reside(icp_ctx* c)
{
    const icp::NNPlan& pl = c->plan;
    // (a plan with shared rows starts with armed launches, see share_wants_resident; ICP_RESIDENT=2: resident from the first pass)
    // (ranks of one node communicator that share a DEVICE never reside: each fits the machine alone, the two together need
    // not -- one rank's waiting blocks would hold the CUs the other's rows are waited for on, the circular wait of can_arm)
    // ICP_DEBUG=shared_resident (tests: two hall-sized ranks, 2 x 256 half-CU blocks, known to fit together) lifts it.
    return c->resident && (!c->shares_device || c->debug_shared_resident) && (c->resident > 1 || pl.share_blocks == 0 || share_wants_resident(c)) &&
           (c->prec == ICP_F32 || pl.family == icp::NNFamily::Row64F64) && !c->resident_refused && mailbox_launch_possible(c) && c->host_reduce() && !c->loop.pending;
}

// returns ICP_OK with *fell_back = true when the resident kernel could not be launched (nothing has been done)
int loop_run_resident(icp_ctx* c, int max_steps, int* k_io, int* d_io, bool* fell_back)
{
    LoopState& L = c->loop;
    icp::NNPlan rp = c->plan;   // the resident kernel closes every row inside its block: one segment
    rp.splits = 1;
    rp.seg_len = icp::round_up(rp.m_pad, 8);
    icp::NNMailbox* mb = mail_slot(c->h_mail, (int)(c->mail_seq++ % kMailSlots));
    const int pass_cap = L.H.prm.max_iter + 2;
    const double base = (double)icp::take_tags(c->tag_seq, (uint64_t)pass_cap + 1);
    post(c, mb, nullptr, nullptr, icp::ICP_CMD_EXIT, 0.0);   // cleared
    const int c0 = c->cur;
    const icp::NNCullInputs cull = make_cull(c, L.matched ? (const int32_t*)c->idx[c0].p : nullptr);
    icp::NNTailArgs ta = tail_args(c, rp, (int32_t*)c->idx[c0 ^ 1].p, 0.0, true);   // pass 0, 2, ... (the step-wise loop flips before it writes, too)
    ta.idx_out_odd = (int32_t*)c->idx[c0].p;
    prepare_rows_format(c, ta.compact != 0);
    icp::NNFusedTransform ft{nullptr, nullptr, (const int32_t*)c->idx[c0].p, c->P.p /* in place */, (double*)c->err_partials.p, mb, c->mail_in_bar ? nullptr : c->relay, base, true};
    // icp_set_profiling(n): every n-th resident kernel is bracketed by events (read after it has ended)
    const bool time_this = c->profile_stride > 0 && (c->resident_launch_count++ % (uint64_t)c->profile_stride) == 0;
    if (time_this) HIP_TRY(hipEventRecord(c->ev0, c->stream));
    // after icp_reset_moving the kernel reads the pristine copy and (re)writes c->P itself -- no copy is enqueued
    const void* P_in = c->moving_is_pristine ? c->P0.p : c->P.p;
    ft.store_first = c->moving_is_pristine;
    // shared rows: several blocks read a row's points at kernel entry, one of them stores the moved points in pass 0 -- not into
    // the buffer a block that starts late is still reading: the cloud goes to the second buffer (as an armed launch does)
    const bool two_buffers = rp.share_blocks > 0 && !c->moving_is_pristine && c->P2.p != nullptr;
    if (two_buffers) { ft.P_out = c->P2.p; ft.store_first = true; }
    const hipError_t le = icp::launch_nn(rp, P_in, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, &ft, &cull, &ta, c->stream);
    if (le != hipSuccess) {
        (void)hipGetLastError();
        c->resident_refused = true;   // does not fit the machine
        *fell_back = true;
        return ICP_OK;
    }
    c->moving_is_pristine = false;
    if (two_buffers) std::swap(c->P, c->P2);
    *fell_back = false;
    if (time_this) HIP_TRY(hipEventRecord(c->ev1, c->stream));
    if (c->trace_passes) std::fprintf(stderr, "[icp trace] resident launch: mailbox %p relay %p base %.0f\n", (void*)mb, (void*)c->relay, base);
    int k = *k_io, d = *d_io, sent = 0, matched = 0, rc = ICP_OK;
    bool alive = true;
    c->rows_done_at = std::chrono::steady_clock::now();   // (the launch: the kernel waits from now on at the earliest)
    L.live_mailbox = mb;
    while (!d && k < max_steps && sent < pass_cap) {
        debug_stall(c);
        const auto tr0 = std::chrono::steady_clock::now();
        if (std::chrono::duration<double>(tr0 - c->rows_done_at).count() > kMailLeaseS) {
            // this thread was away for too long (descheduled, or held up in the inter-rank exchange): the kernel may have
            // given up waiting.  EXIT is consistent whatever each block has decided; icp_loop_run launches a new kernel,
            // which resumes from the state the last complete pass left (P in place, idx ping-pong).
            if (c->trace) std::fprintf(stderr, "[icp trace] resident kernel withdrawn: the host was %.2f s late\n",
                                       std::chrono::duration<double>(tr0 - c->rows_done_at).count());
            break;
        }
        const bool apply = L.H.have_rt;
        const bool final_only = L.H.next_is_final();
        const int cmd = !apply ? icp::ICP_CMD_MATCH : (final_only ? icp::ICP_CMD_TRANSFORM_ONLY : icp::ICP_CMD_TRANSFORM_MATCH);
        if (apply) {
            L.applied_idx = c->cur;
            L.H.note_applied();
        }
        if (cmd != icp::ICP_CMD_TRANSFORM_ONLY) {
            c->cur ^= 1;
            L.matched = true;
            c->idx_valid = true;
            ++matched;
        }
        if (c->debug_lose_pass >= 0 && L.H.applied == c->debug_lose_pass + (apply ? 1 : 0)) c->debug_lose_pass = -1;   // (test hook: this message is lost)
        else post(c, mb, L.H.R, L.H.t, cmd, base + (double)sent);   // (R, t: ignored by a plain MATCH)
        if (c->trace_passes && sent > 0)
            std::fprintf(stderr, "[icp trace]   host turnaround (last row seen -> next message out): %.2f us\n",
                         1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - c->tr_rows_done).count());
        // (the kernel works in place: no slot-order points are left behind)
        set_pending(L, rp.blocks_x, 0, ta.compact != 0, true, false, false, base + (double)sent, false,
                    ICP_ROUTE_RESIDENT | (cmd == icp::ICP_CMD_TRANSFORM_ONLY ? ICP_ROUTE_ERROR_ONLY : ICP_ROUTE_FUSED_TAIL));
        ++sent;
        if (c->trace) c->tr_enqueue += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
        c->posted_at = tr0;
        const auto tc0 = c->trace_passes ? std::chrono::steady_clock::now() : tr0;
        rc = loop_complete_body(c, &d);
        if (c->trace_passes)
            std::fprintf(stderr, "[icp trace] resident pass %d cmd %d: %.2f us from message to reduced rows + solve (row 0 after %.2f us, all rows after %.2f us)\n", sent - 1, cmd,
                         1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count(), 1e6 * c->tr_first_row, 1e6 * c->tr_last_row);
        if (rc != ICP_OK) {
            if (c->trace) std::fprintf(stderr, "[icp trace] resident pass %d failed: mailbox %p reads back tags %08x %08x cmd %d (sent tag %08x)\n",
                                       sent - 1, (void*)mb, *(volatile uint32_t*)&mb->w[icp::ICP_MB_TAG0], *(volatile uint32_t*)&mb->w[icp::ICP_MB_TAG1],
                                       (int)*(volatile uint32_t*)&mb->w[icp::ICP_MB_CMD], icp::mailbox_tag(base + (double)(sent - 1)));
            break;
        }
        ++k;
        if (cmd == icp::ICP_CMD_TRANSFORM_ONLY) { alive = false; break; }  // the kernel ends itself after that pass
    }
    if (alive) post(c, mb, L.H.R, L.H.t, icp::ICP_CMD_EXIT, base + (double)sent);
    L.live_mailbox = nullptr;
    if (rc != ICP_OK && abandon_loop(c)) g_last_error += " [the loop was abandoned; the moving cloud is reset to its uploaded state]";
    if (time_this && rc == ICP_OK) {
        // the kernel ends within microseconds of the exit message: spin on the event instead of a blocking wait
        // (whose wake-up alone costs tens of microseconds of the loop being measured)
        const auto tq = std::chrono::steady_clock::now();
        hipError_t qe = hipErrorNotReady;
        while ((qe = hipEventQuery(c->ev1)) == hipErrorNotReady)
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tq).count() > 5.0) break;
        if (qe != hipSuccess) { (void)hipGetLastError(); HIP_TRY(hipEventSynchronize(c->ev1)); }
        if (int trc = add_timed_launch(c, matched)) return trc;
    }
    *k_io = k;
    *d_io = d;
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop

namespace {

int loop_run_inner(icp_ctx* c, int max_steps, int* k_out, int* d_out)
{
    int d = c->loop.active && c->loop.H.done ? 1 : 0, k = 0;
    while (!d && k < max_steps) {
        if (can_reside(c)) {
            bool fell_back = false;
            if (int rc = loop_run_resident(c, max_steps, &k, &d, &fell_back)) return rc;
            if (!fell_back) continue;
        }
        if (!c->loop.pending)
            if (int rc = loop_enqueue_body(c)) return rc;
        if (k + 1 < max_steps && can_arm(c))
            if (int rc = loop_arm(c)) return rc;
        if (int rc = loop_complete_body(c, &d)) {
            loop_withdraw_armed(c);
            abandon_loop(c);
            return rc;
        }
        if (c->loop.armed) {
            // (a host that comes back too late may not publish any more: the waiting kernel may have given up -- it is
            // withdrawn, which is consistent either way, and the pass is launched afresh)
            debug_stall(c);
            const bool late = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->loop.armed_at).count() > kMailLeaseS;
            if (d || late) loop_withdraw_armed(c);
            else loop_release_armed(c);
        }
        ++k;
    }
    *k_out = k;
    *d_out = d;
    return ICP_OK;
}

// A pass that never delivered its rows (a message that no block saw, blocks another process kept off the machine) ends the
// resident / armed conversation -- but not necessarily the registration: when the loop started from the uploaded cloud
// (icp_set_moving / icp_reset_moving) the copy is still there, and the same registration is run again with plain launches,
// one per pass, nothing resident and nothing armed.  Every loop form produces the same bits, so the caller gets what an
// undisturbed run would have returned; only when that fails too (a device that is really gone) does the error surface.
int redo_stepwise(icp_ctx* c, const icp_params& prm, long long target_steps, int* d_out)
{
    if (hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return ICP_ERR_HIP; }
    const int keep_resident = c->resident;
    const bool keep_arm = c->arm;
    c->resident = 0;
    c->arm = false;
    c->moving_is_pristine = true;
    c->moving_untouched = true;
    int d = 0;
    int rc = icp_loop_begin(c, &prm);
    while (rc == ICP_OK && !d && c->loop.steps < target_steps) {
        rc = loop_enqueue_body(c);
        if (rc == ICP_OK) rc = loop_complete_body(c, &d);
    }
    c->resident = keep_resident;
    c->arm = keep_arm;
    *d_out = d;
    return rc;
}

// icp_point_to_point / icp_point_to_plane: the clouds (and, point-to-plane, the model's normals) set up, one whole registration
int run_registration(icp_ctx* c, const void* data, int n, const void* model, int m, const void* normals, const icp_params* prm, int metric,
                     icp_result* out)
{
    if (int rc = use(c)) return rc;
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (n <= 0) return fail(ICP_ERR_INVALID, "empty moving cloud");
    if (m <= 0) return fail(ICP_ERR_EMPTY, "empty model cloud");
    icp_params p = *prm;
    p.metric = metric;
    const auto s0 = std::chrono::steady_clock::now();
    if (int rc = icp_set_model(c, model, m, p.precision)) return rc;
    if (metric == ICP_POINT_TO_PLANE)
        if (int rc = normals ? icp_set_model_normals(c, normals, m) : icp_estimate_normals(c, nullptr, nullptr)) return rc;
    if (int rc = icp_set_moving(c, data, n, p.precision)) return rc;
    const double seconds_setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - s0).count();
    ScopedPin pin(c);
    if (int rc = icp_loop_begin(c, &p)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    int done = 0;
    while (!done)
        if (int rc = icp_loop_run(c, 1 << 20, nullptr, &done)) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    const LoopState& L = c->loop;
    if (out) {
        std::memcpy(out->T, L.H.T, sizeof L.H.T);
        out->iterations = L.H.iterations;
        out->passes = L.H.applied;
        out->seconds_total = std::chrono::duration<double>(t1 - t0).count();
        out->seconds_nn = L.seconds_nn;
        out->seconds_host = L.seconds_host;
        out->seconds_setup = seconds_setup;
        if (out->err)
            for (size_t i = 0; i < L.H.err.size(); ++i) out->err[i] = L.H.err[i];
        if (out->idx)
            if (int rc = icp_loop_indices(c, out->idx)) return rc;
        if (out->moved)
            if (int rc = icp_get_moving(c, out->moved)) return rc;
    }
    return ICP_OK;
}

}  // namespace

#pragma GCC visibility push(default)   // (the C ABI: exported although its icp_ctx is a hidden type)
extern "C" {

int icp_loop_begin(icp_ctx* c, const icp_params* prm)
{
    if (int rc = use(c)) return rc;
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (int rc = require_clouds(c)) return rc;
    if (prm->max_iter < 1) return fail(ICP_ERR_INVALID, "max_iter must be >= 1");
    if (prm->metric != ICP_POINT_TO_POINT && prm->metric != ICP_POINT_TO_PLANE) return fail(ICP_ERR_INVALID, "unknown metric");
    if (prm->precision != c->prec) return fail(ICP_ERR_INVALID, "params precision differs from the resident clouds");
    if (prm->metric == ICP_POINT_TO_PLANE && !c->have_normals) return fail(ICP_ERR_STATE, "point-to-plane needs model normals");
    if (c->n == 0) return fail(ICP_ERR_INVALID, "empty moving cloud");
    if (int rc = ensure_work_buffers(c)) return rc;
    LoopState& L = c->loop;
    L = LoopState();
    if (c->order_launches > 0) { c->order_regs++; c->order_launches = 0; }   // (the loop before left its rows' counters: history for this one's cold pass)
    // (the tickets of the in-launch finalize are zero between launches; a loop that was abandoned in mid-pass may have left some drawn)
    if (c->fin_tickets.p != nullptr && fin_in_launch(c, c->plan)) HIP_TRY(hipMemsetAsync(c->fin_tickets.p, 0, c->fin_tickets.cap, c->stream));
    if (int rc = L.H.begin(*prm)) return fail(rc, "bad loop parameters");
    L.active = true;
    L.from_pristine = c->moving_untouched;
    c->moving_untouched = false;   // (a loop moves the cloud)
    return ICP_OK;
}

int icp_loop_enqueue(icp_ctx* c)
{
    if (int rc = use(c)) return rc;
    return loop_enqueue_body(c);
}

void* icp_loop_moments_dev(icp_ctx* c) { return c ? (void*)c->mom_dev : nullptr; }

int icp_loop_set_moments_dev(icp_ctx* c, void* dev_ptr)
{
    if (int rc = use(c)) return rc;
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    if (!dev_ptr) {
        HIP_TRY(c->mom_own.ensure(ICP_NMOM * sizeof(double)));
        c->mom_dev = (double*)c->mom_own.p;
    } else {
        // (whoever owns the buffer reduces it across ranks; a library-side exchange on top would add the ranks up twice)
        if (c->lcomm) return fail(ICP_ERR_STATE, "a node communicator is attached (icp_comm_init_local): the library exchanges the vector itself");
        if (c->comm) return fail(ICP_ERR_STATE, "a device communicator is attached (icp_comm_init): the library all-reduces its own vector");
        c->mom_dev = (double*)dev_ptr;
    }
    return ICP_OK;
}

int icp_loop_complete(icp_ctx* c, int* done)
{
    if (int rc = use(c)) return rc;
    ScopedPin pin(c);
    return loop_complete_body(c, done);
}

int icp_loop_run(icp_ctx* c, int max_steps, int* steps_done, int* done)
{
    if (max_steps < 0) return fail(ICP_ERR_INVALID, "max_steps < 0");
    if (int rc = use(c)) return rc;
    ScopedPin pin(c);
    const bool can_redo = c->loop.active && c->loop.from_pristine && !c->comm && !c->lcomm;   // (ranks of a communicator must move together)
    const icp_params prm = c->loop.H.prm;
    const long long steps_before = c->loop.steps;
    c->rows_timed_out = false;
    // (should the registration have to be run again, the aborted attempt's share of the profiling and trace totals is taken back)
    const double keep_nn = c->prof_seconds_nn, keep_tr[4] = {c->tr_enqueue, c->tr_wait, c->tr_reduce, c->tr_solve};
    const int keep_launches = c->prof_nn_launches;
    const long long keep_passes = c->prof_nn_passes;
    const uint64_t keep_tr_n = c->tr_n;
    int k = 0, d = 0;
    int rc = loop_run_inner(c, max_steps, &k, &d);
    if (rc == ICP_ERR_HIP && c->rows_timed_out && can_redo) {
        const std::string first = g_last_error;
        c->prof_seconds_nn = keep_nn; c->prof_nn_launches = keep_launches; c->prof_nn_passes = keep_passes;
        c->tr_enqueue = keep_tr[0]; c->tr_wait = keep_tr[1]; c->tr_reduce = keep_tr[2]; c->tr_solve = keep_tr[3]; c->tr_n = keep_tr_n;
        if (c->trace) std::fprintf(stderr, "[icp trace] %s -- running the registration again step-wise\n", first.c_str());
        c->loop.active = false;
        c->loop.pending = false;
        c->idx_valid = false;
        rc = redo_stepwise(c, prm, steps_before + (long long)max_steps, &d);
        if (rc == ICP_OK) {
            c->recoveries += 1;
            k = (int)std::max<long long>(0, c->loop.steps - steps_before);
        } else {
            g_last_error = first + " [the step-wise re-run failed as well: " + g_last_error + "]";
        }
    }
    if (rc != ICP_OK) return rc;
    if (steps_done) *steps_done = k;
    if (done) *done = d;
    return ICP_OK;
}

int icp_recoveries(icp_ctx* c) { return c ? c->recoveries : ICP_ERR_INVALID; }

int icp_loop_state(icp_ctx* c, int* iterations, int* passes, double* err, int err_cap, double* T16)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    const LoopState& L = c->loop;
    if (!L.active) return fail(ICP_ERR_STATE, "no loop");
    if (iterations) *iterations = L.H.iterations;
    if (passes) *passes = L.H.applied;
    if (err) {
        const int cnt = (int)L.H.err.size() < err_cap ? (int)L.H.err.size() : err_cap;
        for (int i = 0; i < cnt; ++i) err[i] = L.H.err[i];
    }
    if (T16) std::memcpy(T16, L.H.T, sizeof L.H.T);
    return ICP_OK;
}

int icp_loop_timing(icp_ctx* c, double* seconds_nn, int* nn_launches)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (seconds_nn) *seconds_nn = c->prof_seconds_nn;
    if (nn_launches) *nn_launches = c->prof_nn_launches;
    return ICP_OK;
}

int icp_loop_phase_seconds(icp_ctx* c, double* seconds_nn, double* seconds_host)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (seconds_nn) *seconds_nn = c->loop.seconds_nn;
    if (seconds_host) *seconds_host = c->loop.seconds_host;
    return ICP_OK;
}

int icp_loop_timing_passes(icp_ctx* c, long long* passes)
{
    if (!c || !passes) return fail(ICP_ERR_INVALID, "null argument");
    *passes = c->prof_nn_passes;
    return ICP_OK;
}

int icp_diag_loop_moments(icp_ctx* c, double* out32, int* route)
{
    if (!c || !out32) return fail(ICP_ERR_INVALID, "null argument");
    const LoopState& L = c->loop;
    if (!L.active || !L.mom_valid || !c->h_mom) return fail(ICP_ERR_STATE, "no completed pass of a loop");
    // (an enqueued pass has set its route already while the vector is still the pass's before it: never hand out the two together)
    if (L.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight (icp_loop_complete first)");
    std::memcpy(out32, c->h_mom, ICP_NMOM * sizeof(double));
    if (route) *route = L.route;
    return ICP_OK;
}

int icp_loop_indices(icp_ctx* c, int32_t* out)
{
    if (int rc = use(c)) return rc;
    if (!c->loop.active) return fail(ICP_ERR_STATE, "no loop");
    return download_idx(c, c->loop.H.applied > 0 ? c->loop.applied_idx : c->cur, out);
}

int icp_point_to_point(icp_ctx* c, const void* data, int n, const void* model, int m, const icp_params* prm,
                       icp_result* out)
{
    return run_registration(c, data, n, model, m, nullptr, prm, ICP_POINT_TO_POINT, out);
}

int icp_point_to_plane(icp_ctx* c, const void* data, int n, const void* model, int m, const void* normals,
                       const icp_params* prm, icp_result* out)
{
    return run_registration(c, data, n, model, m, normals, prm, ICP_POINT_TO_PLANE, out);
}

}  // extern "C"
#pragma GCC visibility pop
