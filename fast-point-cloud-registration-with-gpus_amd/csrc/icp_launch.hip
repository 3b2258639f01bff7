// icp_launch.hip -- the dispatch of the matching kernels (launch_nn): it turns a plan (icp_plan.h) into a launch.  Host code only;
// the kernels themselves live in the family files (icp_k_*.hip), which hand out their instantiations as function pointers.
// Compiled by hipcc because the kernels' argument blocks (RT, NNFuse, NNTail: icp_device.h) are built here.
#include "icp_device.h"

#include <math.h>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace icp {

// the instantiations of the family files
const void* sparse128_kernel_fn(int nw, int tl, bool diag, bool perm, bool hier);
const void* row64_kernel_fn(bool waves16, int tl, bool diag, bool perm);
const void* row64_f64_kernel_fn(int tl, bool waves16, bool diag);
template <typename F> hipError_t launch_nn_t(const NNPlan& pl, const void* P, const void* Q, void* part_d, int32_t* part_idx, hipStream_t st);
hipError_t launch_dense_v2(const NNPlan& pl, const void* P, const void* Qscan, void* part_d, int32_t* part_idx, const RT<float>& rt, const NNFuse& fuse,
                           const NNTail& tail, int tl, bool cull, hipStream_t st);

unsigned int share_rows_plan(const unsigned int* hits, int rows, int blocks, int m_pad, int min_hits, int* parts_out)
{
    // (statement by statement what a block of nn_match_sparse computes; the block's reductions are plain loops here)
    unsigned int total = 0;
    for (int r = 0; r < rows; ++r) total += share_clamp(hits[r]);
    const unsigned int spare = blocks > rows ? (unsigned int)(blocks - rows) : 0u;
    const unsigned int T0 = share_first_target(total, spare), cap = share_cap(m_pad), Tmin = (unsigned int)min_hits;
    unsigned int T = T0 < Tmin ? Tmin : T0;
    if (share_tries_candidates(T0, Tmin, spare)) {
        unsigned int sums[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            for (int r = 0; r < rows; ++r) sums[k] += share_parts(share_clamp(hits[r]), share_candidate(T0, k), cap);
            sums[k] &= 0xffffu;   // (16-bit fields in the kernel; <= 512 x 32 never reaches them)
        }
        T = share_pick(T0, Tmin, sums, (unsigned int)blocks);
    }
    long long all = 0;
    for (int r = 0; r < rows; ++r) { parts_out[r] = (int)share_parts(share_clamp(hits[r]), T, cap); all += parts_out[r]; }
    if (all > blocks)
        for (int r = 0; r < rows; ++r) parts_out[r] = 1;   // (cannot happen with clamped counts and blocks >= rows; the kernel falls back the same way)
    return T;
}

// blocks the machine holds at once of a resident kernel, per (device, kernel): asked once (the occupancy query a cooperative
// launch is built on), remembered under a lock -- contexts of several devices and threads share this table.  <= 0: unknown.
static long long resident_capacity(const void* fn, int threads)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, long long> capacity;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(mu);
    long long& slot = capacity[std::make_pair(dev, fn)];
    if (slot <= 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 0;
        slot = (long long)per_cu * cus;
    }
    return slot;
}

// fp32: rows of 64, rows of 128 and the packed kernel over every pair share the fused front end and the fused tail
static hipError_t launch_nn_f32(const NNPlan& pl, const void* P, const void* Q, void* part_d, int32_t* part_idx,
                               const NNFusedTransform* ft, const NNCullInputs* opt, const NNTailArgs* ta, hipStream_t st)
{
    static const NNTuning defaults{};
    const NNTuning& tune = (opt && opt->tune) ? *opt->tune : defaults;
    const bool sparse = nn_is_sparse(pl);
    dim3 grid(pl.blocks_x, pl.splits);
    RT<float> rt{};
    NNFuse fuse{};
    fuse.n = pl.n;
    fuse.m = pl.m;
    fuse.Q_gather = (const float*)Q;
    fuse.tlog = tune.phase_log;
    fuse.tlog_cap = tune.phase_cap;
    fuse.tlog_pass = tune.phase_pass;
    // (diagnostic: the log cleared ahead of every launch -- launches of different block sizes, spare blocks and the parts of split
    // rows that do not close them would otherwise leave older stamps among the last launch's)
    if (tune.phase_wipe && tune.phase_log != nullptr && hipMemsetAsync(tune.phase_log, 0, (size_t)tune.phase_cap * sizeof(long long), st) != hipSuccess) return hipErrorInvalidValue;
    fuse.work = opt ? opt->work : nullptr;
    const void* Qscan = Q;
    if (pl.cull && opt && opt->Q_scan) {
        Qscan = opt->Q_scan;
        fuse.seed_idx = opt->seed_idx;
        // (the boxes describe the sparse kernel's view of the model: usable here only if that is the model's own order)
        fuse.boxes = (pl.chunk == 8 && !opt->Q_scan_sorted) ? (const float*)opt->boxes : nullptr;
    }
    if (ft) {
        if (ft->mailbox) {
            if (!sparse) return hipErrorInvalidValue;  // only the sparse kernel can be armed
            fuse.mailbox = ft->mailbox;
            fuse.relay = ft->relay;
            fuse.want = ft->want;
            fuse.want_lo = (unsigned int)(unsigned long long)ft->want;
            fuse.slot_state = (nn_keeps_slot_order(pl) && !ft->resident) ? (float*)ft->slot_state : nullptr;
            fuse.slot_valid = (fuse.slot_state && ft->slot_valid) ? 1 : 0;
            fuse.slot_flip = ft->slot_flip ? 1 : 0;
            fuse.resident = ft->resident ? 1 : 0;
            fuse.speculate = (ft->resident && tune.speculate) ? 1 : 0;   // (ICP_NN_SPECULATE=0: A/B runs and tests)
            // the guess: the next displacement <= twice this one + a thousandth of the group box (profiles/r2: 90 % of the lists cover)
            fuse.spec_gain = 2.0f;
            fuse.spec_floor = 1e-3f;
            fuse.store_first = ft->store_first ? 1 : 0;
        } else {
            for (int k = 0; k < 9; ++k) rt.r[k] = (float)ft->R9[k];
            for (int k = 0; k < 3; ++k) rt.t[k] = (float)ft->t3[k];
            // (round 3: a plain launch -- the loop of a cloud whose rows the device adds up -- leaves and finds its points and
            // matches in slot order too, as an armed one does)
            fuse.slot_state = nn_keeps_slot_order(pl) ? (float*)ft->slot_state : nullptr;
            fuse.slot_valid = (fuse.slot_state && ft->slot_valid) ? 1 : 0;
            fuse.slot_flip = ft->slot_flip ? 1 : 0;
        }
        fuse.apply = 1;
        fuse.n = pl.n;
        fuse.idx_prev = ft->idx_prev;
        fuse.P_out = (float*)ft->P_out;
        fuse.err_rows = ft->err_rows;
    }
    NNTail tail{};
    tail.row = -1;
    if (ta) {
        if (!nn_can_fuse_tail(pl)) return hipErrorInvalidValue;
        tail.keys = ta->keys;
        tail.tickets = ta->tickets;
        tail.err_tile = ta->err_tile;
        tail.idx_out = ta->idx_out;
        tail.idx_out_odd = ta->idx_out_odd ? ta->idx_out_odd : ta->idx_out;
        tail.Nrm = (const float*)ta->Nrm_soa;
        tail.rows = ta->rows;
        tail.tag = ta->tag;
        tail.tag_lo = (unsigned int)(unsigned long long)ta->tag;
        tail.compact = (ta->compact && sparse && ta->metric == ICP_POINT_TO_POINT) ? 1 : 0;
        tail.rows_on_device = (ta->rows_on_device && !tail.compact) ? 1 : 0;
        if (tail.rows_on_device && ta->fin_tickets != nullptr && ta->fin_scratch != nullptr && ta->fin_out != nullptr && nn_can_sum_rows_in_launch(pl)) {
            // rows added up inside the launch: ~sqrt(rows) ranges of rows (at most NN_FIN_GROUPS), so that the sum of a range and the
            // sum of the ranges are equally short
            const int rows = pl.blocks_x;
            int groups = (int)ceil(sqrt((double)rows));
            groups = groups < 1 ? 1 : groups > NN_FIN_GROUPS ? NN_FIN_GROUPS : groups;
            const int per = (rows + groups - 1) / groups;
            tail.fin_tickets = ta->fin_tickets;
            tail.fin_scratch = ta->fin_scratch;
            tail.fin_out = ta->fin_out;
            tail.fin_host = ta->fin_host;
            tail.fin_rows = rows;
            tail.fin_per = per;
            tail.fin_groups = (rows + per - 1) / per;
        }
    }
    if (sparse) {
        // the plan's geometry is the sparse kernel's: it needs the scan copy and its chunk boxes
        if (!(opt && opt->Q_scan && opt->boxes)) return hipErrorInvalidValue;
        if (pl.m_pad >= (1 << 28)) return hipErrorInvalidValue;  // the in-block merge key carries 28 index bits
        fuse.seed_idx = opt->seed_idx;
        fuse.boxes = (const float*)opt->boxes;
        fuse.q_perm = opt->Q_scan_sorted ? opt->q_perm : nullptr;
        fuse.p_perm = opt->p_perm;
        const void* Qsp = opt->Q_scan_sorted ? opt->Q_scan_sorted : opt->Q_scan;
        fuse.samples = (const float*)opt->samples;
        // the cold start's full round (its probe round is 8 groups): 64 groups = 512 samples on a small model -- measured
        // (round 2, rows of 64): as good as 2048 on the 128 x 128 grid, Bunny_res and a random cloud, and 4 us less of a cold
        // pass on the hall scan, where a few blocks take the full round without gaining from it; 2048 on large models
        fuse.sample_groups = pl.m_pad <= 32768 ? 64 : 256;
        // (round 3: with the refinement round of the traversal -- local samples, where the row's neighbours are -- the coarse sample
        // round of a SEEDED pass cost more than it added, 5.14 -> 5.10 ms without: removed in round 4)
        // seeded: few hits, long rounds; cold: short rounds so that the exchanged minima start pruning early
        const NNLaunchKind kind{ta != nullptr, fuse.seed_idx == nullptr && fuse.slot_valid == 0, opt->row_order != nullptr && opt->order_history, opt->waves64 == 16};
        const NNLaunchShape shape = nn_launch_shape(pl, kind, tune);
        const int nw = shape.waves;
        int passes = (fuse.seed_idx || fuse.samples) ? shape.max_passes : 1;
        if (pl.family == NNFamily::Row64) {
            // ---- 64-point rows ----
            if (pl.splits != 1 || pl.hier) return hipErrorInvalidValue;
            const bool diag = fuse.tlog != nullptr || fuse.work != nullptr, perm = fuse.q_perm != nullptr;
            const int tl = !ta ? 0 : (ta->metric == ICP_POINT_TO_PLANE ? 2 : 1);
            const void* fn = row64_kernel_fn(nw == 16, tl, diag, perm);
            const float* Pp = (const float*)P;
            const float* Qp = (const float*)Qsp;
            int n_pad = pl.n_pad, m_pad = pl.m_pad;
            float* pd = (float*)part_d;
            void* args[] = {&Pp, &n_pad, &Qp, &m_pad, &passes, &pd, &part_idx, &rt, &fuse, &tail};
            const dim3 g64(pl.blocks_x, 1);
            if (fuse.resident) {
                if (!ta) return hipErrorInvalidValue;
                // every block must be on the machine at once (see below): blocks <= CUs x resident blocks per CU
                const long long cap = resident_capacity(fn, nw * 64);
                if (cap <= 0) return hipErrorCooperativeLaunchTooLarge;
                if ((long long)g64.x > cap) return hipErrorCooperativeLaunchTooLarge;
            }
            return hipLaunchKernel(fn, g64, dim3(nw * 64), args, 0, st);
        }
        {
            // ---- 128-point rows: one table of instantiations (which of them a launch takes: nn_launch_shape) ----
            const bool diag = fuse.tlog != nullptr || fuse.work != nullptr, perm = fuse.q_perm != nullptr, hier = pl.hier != 0;
            const int tl = !ta ? 0 : (ta->metric == ICP_POINT_TO_PLANE ? 2 : 1);
            if (!hier && (pl.m_pad >> 3) > 65536) return hipErrorInvalidValue;   // (the flat search lists 16-bit chunk numbers; nn_plan never asks for it)
            const void* fn = sparse128_kernel_fn(nw, tl, diag, perm, hier);
            if (fn == nullptr) return hipErrorInvalidValue;
            const float* Pp = (const float*)P;
            const float* Qp = (const float*)Qsp;
            int n_pad = pl.n_pad, m_pad = pl.m_pad, seg = pl.seg_len;
            float* pd = (float*)part_d;
            void* args[] = {&Pp, &n_pad, &Qp, &m_pad, &seg, &passes, &pd, &part_idx, &rt, &fuse, &tail};
            // Shared rows: a grid of more blocks than rows, the roles dealt out inside the kernel from the
            // hits each row had in the previous launch (three count arrays in rotation: read, add to, zero for the next)
            dim3 g = grid;
            if (nw == 8 && pl.share_blocks > pl.blocks_x && pl.splits == 1 && opt->share_counts != nullptr && opt->share_seq != nullptr && opt->share_cold_seq != nullptr &&
                (!fuse.resident || (opt->seed_pub != nullptr && tune.share_resident)) &&   // (ICP_NN_SHARE_RESIDENT=0: a resident launch keeps one block per row -- A/B runs)
                pl.blocks_x <= nw * 64) {
                const unsigned long long seq = (*opt->share_seq)++;
                const size_t R = (size_t)pl.blocks_x;
                fuse.share_prev = opt->share_counts + ((seq + 2) % 3) * R;
                fuse.share_cur = opt->share_counts + (seq % 3) * R;
                fuse.share_next = opt->share_counts + ((seq + 1) % 3) * R;
                // The first pass of a registration (no previous match: the launch has no seeds) has no previous pass to go by:
                // it takes the counts of the PREVIOUS registration's first pass (two more arrays, alternating) -- a sensor's
                // consecutive scans are heavy in the same places; a first registration finds zeros there and runs unshared.
                // The array the next first pass adds to is zeroed by every ordinary pass in between.
                unsigned int* cold = opt->share_counts + 3 * R;
                if (fuse.seed_idx == nullptr) {
                    const unsigned long long k = (*opt->share_cold_seq)++;
                    fuse.share_prev = cold + ((k + 1) % 2) * R;
                    fuse.share_cur2 = cold + (k % 2) * R;
                    // The array this launch adds to is zeroed on the stream, ahead of the launch: where every launch is a first pass
                    // (resident kernels, one per registration) no ordinary pass in between would do it, and the counts of all
                    // registrations would pile up.  (Not by a block of the launch itself: nothing orders block 0's stores before
                    // another block's adds, and lost counts would make the roles -- and the timings -- differ from run to run.)
                    if (hipMemsetAsync(fuse.share_cur2, 0, R * sizeof(unsigned int), st) != hipSuccess) return hipErrorInvalidValue;
                    fuse.share_zero2 = nullptr;
                } else {
                    fuse.share_zero2 = cold + (*opt->share_cold_seq % 2) * R;
                }
                fuse.share_rows = pl.blocks_x;
                fuse.share_min = 8 * nw;      // one batch for every wave (32 .. 128 measured: no difference)
                g = dim3(pl.share_blocks, 1);
            }
            fuse.seed_pub = opt->seed_pub;
            fuse.records = hier ? opt->records : nullptr;
            // (a round of the chunk find covers 16 listed super boxes -- the hit list would hold 64: every round starts from the largest
            // bound the rounds before have left, so shorter rounds list less; 10 M x 10 M, rounds of 64 / 32 / 16 / 8: 1.41 / 1.29 / 1.19 /
            // 1.13 G chunks listed per registration, 5.93 / 5.75 / 5.65 / 5.69 ms per iteration.  ICP_NN_ROUND_SUPERS for the A/B)
            // (the refinement round of a pass that lists >= 12 super boxes, over <= 256 of their chunk samples: 10 M x 10 M 5.68 -> 5.14 ms,
            // 1.19 -> 0.99 G chunks listed and 370 -> 327 M evaluated per registration; 24 / 512: 5.26, 12 / 128: 5.15, 8 / 256: 5.17.
            // The switches of those A/B runs are gone with round 4.)
            fuse.refine_min = 12;
            fuse.refine_cnt = 256;
            fuse.round_supers = 16;
            if (hier && fuse.records == nullptr) return hipErrorInvalidValue;   // (the hierarchical search fetches its hits from the records)
            if (pl.order && ta && !fuse.resident && opt->row_order != nullptr && opt->row_hits != nullptr) {
                fuse.row_order = opt->row_order;
                fuse.row_hits = opt->row_hits;
                fuse.xcd_shift = NN_ORDER_XCD_SHIFT;
                g = dim3(pl.blocks_x + NN_ORDER_EXTRA, 1);   // (the roles of the blocks beyond the rows: parts of split rows, or none)
            }
            if (fuse.resident) {
                if (!ta || pl.splits != 1) return hipErrorInvalidValue;
                // Every block must be on the machine at once (they all wait for the same host).  A cooperative launch
                // guarantees that or refuses, but costs ~13 us more per launch here; the same guarantee comes from the
                // occupancy query it is built on: the grid fits iff blocks <= CUs x resident blocks per CU.  Blocks that
                // start late (behind the previous kernel of the stream) only delay the first pass, nothing waits on them
                // that they cannot deliver.
                const long long cap = resident_capacity(fn, nw * 64);
                if (cap <= 0) return hipErrorCooperativeLaunchTooLarge;
                if ((long long)g.x * g.y > cap) return hipErrorCooperativeLaunchTooLarge;
                return hipLaunchKernel(fn, g, dim3(nw * 64), args, 0, st);
            }
            return hipLaunchKernel(fn, g, dim3(nw * 64), args, 0, st);
        }
    }
    // measured (profiles/r1/03_nn_sweep_cull.txt): without a seed the early-out variant loses to the plain
    // packed kernel on every cloud (its bound starts at +inf), with one it wins on every cloud
    const bool cull = pl.cull && Qscan != Q && fuse.seed_idx != nullptr;
    if (!cull) { Qscan = Q; fuse.seed_idx = nullptr; fuse.boxes = nullptr; }
    return launch_dense_v2(pl, P, Qscan, part_d, part_idx, rt, fuse, tail, ta ? (ta->metric == ICP_POINT_TO_PLANE ? 2 : 1) : 0, cull, st);
}

// fp64, rows of 64 points: one launch per pass, no mailbox (NNFusedTransform::mailbox must be NULL)
static hipError_t launch_row64_f64(const NNPlan& pl, const void* P, const void* Q, void* part_d, int32_t* part_idx,
                                   const NNFusedTransform* ft, const NNCullInputs* opt, const NNTailArgs* ta, hipStream_t st)
{
    if (!(opt && opt->Q_scan && opt->boxes)) return hipErrorInvalidValue;
    if (ft && ft->mailbox && !ft->resident) return hipErrorInvalidValue;   // (no armed launches in double)
    RT<double> rt{};
    NNFuse fuse{};
    fuse.n = pl.n;
    fuse.m = pl.m;
    fuse.Q_gather = (const float*)Q;                 // (typed by the kernel: doubles)
    fuse.seed_idx = opt->seed_idx;
    fuse.boxes = (const float*)opt->boxes;
    fuse.samples = (const float*)opt->samples;
    fuse.sample_groups = 256;
    if (ft) {
        if (ft->mailbox) {   // resident launch: (R, t) arrive as messages (NNMailbox64)
            fuse.mailbox = ft->mailbox;
            fuse.relay = ft->relay;
            fuse.want = ft->want;
            fuse.want_lo = (unsigned int)(unsigned long long)ft->want;
            fuse.resident = 1;
            fuse.store_first = ft->store_first ? 1 : 0;
        } else {
            for (int k = 0; k < 9; ++k) rt.r[k] = ft->R9[k];
            for (int k = 0; k < 3; ++k) rt.t[k] = ft->t3[k];
        }
        fuse.apply = 1;
        fuse.idx_prev = ft->idx_prev;
        fuse.P_out = (float*)ft->P_out;
        fuse.err_rows = ft->err_rows;
    }
    NNTail tail{};
    tail.row = -1;
    if (ta) {
        tail.idx_out = ta->idx_out;
        tail.idx_out_odd = ta->idx_out_odd ? ta->idx_out_odd : ta->idx_out;
        tail.Nrm = (const float*)ta->Nrm_soa;
        tail.rows = ta->rows;
        tail.tag = ta->tag;
        tail.tag_lo = (unsigned int)(unsigned long long)ta->tag;
        tail.compact = (ta->compact && ta->metric == ICP_POINT_TO_POINT) ? 1 : 0;
    }
    static const NNTuning defaults{};
    const NNLaunchShape shape = nn_launch_shape(pl, NNLaunchKind{ta != nullptr, fuse.seed_idx == nullptr, false, false}, opt->tune ? *opt->tune : defaults);
    const int nw = shape.waves;
    const int passes = (fuse.seed_idx || fuse.samples) ? shape.max_passes : 1;
    const dim3 grid(pl.blocks_x), block(nw * 64);
    const double* Pp = (const double*)P;
    const double* Qs = (const double*)opt->Q_scan;
    const int tl = !ta ? 0 : (ta->metric == ICP_POINT_TO_PLANE ? 2 : 1);
    // icp_set_work_counting: the instrumented instantiation (point-to-point rows only: what the fp64 loop of src/ICP_CPU.c runs)
    fuse.work = (opt->work != nullptr && tl == 1) ? opt->work : nullptr;
    const void* fn = row64_f64_kernel_fn(tl, nw == 16, fuse.work != nullptr);
    if (fuse.resident) {
        // every block must be on the machine at once: blocks <= CUs x resident blocks per CU (the occupancy query)
        if (!ta) return hipErrorInvalidValue;
        const long long cap = resident_capacity(fn, nw * 64);
        if (cap <= 0 || (long long)pl.blocks_x > cap) return hipErrorCooperativeLaunchTooLarge;
    }
    int n_pad = pl.n_pad, m_pad = pl.m_pad, passes_ = passes;
    double* pd = (double*)part_d;
    void* args[] = {&Pp, &n_pad, &Qs, &m_pad, &passes_, &pd, &part_idx, &rt, &fuse, &tail};
    return hipLaunchKernel(fn, grid, block, args, 0, st);
}

hipError_t launch_nn(const NNPlan& pl, const void* P, const void* Q, void* part_d, int32_t* part_idx,
                     const NNFusedTransform* ft, const NNCullInputs* opt, const NNTailArgs* ta, hipStream_t st)
{
    if (pl.n <= 0 || pl.m <= 0) return hipSuccess;
    switch (pl.family) {
        case NNFamily::DensePacked:
        case NNFamily::Row64:
        case NNFamily::Row128: return launch_nn_f32(pl, P, Q, part_d, part_idx, ft, opt, ta, st);
        case NNFamily::Row64F64: return launch_row64_f64(pl, P, Q, part_d, part_idx, ft, opt, ta, st);
        case NNFamily::Dense: break;
    }
    if (ft || ta) return hipErrorInvalidValue;  // the thread-per-point kernel carries neither the fused front end nor a tail
    return pl.precision == ICP_F64 ? launch_nn_t<double>(pl, P, Q, part_d, part_idx, st)
                                   : launch_nn_t<float>(pl, P, Q, part_d, part_idx, st);
}

}  // namespace icp
