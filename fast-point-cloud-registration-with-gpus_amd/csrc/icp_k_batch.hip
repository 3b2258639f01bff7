// icp_k_batch.hip -- gfx950 kernels of batched ICP (icp_batch.cpp): the pass of every running pair in one launch (nn_match_batch:
// front end, matching, moments), the reverse search of reciprocal pairs (nn_match_batch_rev), trimmed rejection and the deferred
// decision (batch_trim_select, batch_trim_moments), robust kernels (batch_robust_moments), the per-pair reduction
// (batch_finalize_kernel), the evaluation of every pair at its present pose (batch_eval_moments), the start clouds of a batch
// with initial transforms (batch_init_kernel) and voxel-grid downsampling (batch_voxel_keys, batch_voxel_group, batch_voxel_rank,
// batch_voxel_compact) and statistical / radius outlier removal (batch_outlier_scan, batch_outlier_decide, batch_outlier_compact).
// The batched neighbours and
// normals (knn4_batch, normals_batch_kernel) live with the single-pair ones in icp_k_plane.hip.  Reference statements: the loop a
// pair runs is src/ICP_point_to_point.cu:295-423 / src/ICP_point_to_plane.cu:517-631; the kernels restate nn_match_kernel,
// moments_kernel and transform_error_kernel (icp_k_dense.hip) per work item.
#include "icp_device_batch.h"
#include "../../include/icp_mi355x_diag.h"
#include <math.h>
#include <stdlib.h>
#include <cstring>

namespace icp {

// ------------------------------------------------------------------------------------------------
// batched ICP (icp_batch.cpp): the pass of every running pair of a batch in one launch.
//
// grid = one block per work item: BATCH_ITEM moving points of one pair, cut from that pair's first point.  All four waves
// hold the item's points (one per lane); wave w scans the w-th contiguous quarter of the pair's model through its own LDS
// sub-tile (every lane reads the same address), keeping the running minimum and the first chunk that lowered it, as
// nn_match_kernel does; the index is recovered inside that chunk, and the quarters are merged in ascending order with a
// strict <: the lowest index wins ties, as in the reference's ascending scan.
//   front end (pass >= 1): the pair's previous R, t by apply_rt -- every wave moves its copy of the points with the same
//     instructions; wave 0 stores them and adds |p_new - q[idx_prev]|^2 in double (transform_error_kernel's arithmetic);
//   tail: wave 0 stores idx, gathers q[idx] and forms moments_kernel's point-to-point terms in double; block_sum_store
//     writes the item's row partials[item][0 .. ICP_MOM_SQQ] (error in slot ICP_MOM_ERR).
//   METRIC == ICP_POINT_TO_PLANE (its own instantiation: the point-to-point one has no branch on the metric): wave 0 gathers
//     n[idx] too, from the normal planes laid out as the model's, and forms moments_kernel's plane terms statement for
//     statement -- cn = (p x n, n), bi = (p - q) . n, C += cn cn^T, b -= cn bi -- into slots ICP_MOM_CNT, ICP_MOM_C ..
//     ICP_MOM_B + 5.  The front end and the error-only last pass are the same code.
//   GATE (its own instantiations: the ungated ones have no branch on it and never read thr): wave 0 keeps the match only if
//     the merged minimum b -- the dist2<F> the scan already holds, nothing recomputed -- is <= thr[pair], the pair's squared
//     maximum correspondence distance in F (+inf: not gated).  A rejected point leaves every accumulator 0, ICP_MOM_CNT
//     included, and its idx entry carries BATCH_IDX_REJECTED above the nearest neighbour's index; the next pass's front end
//     reads that entry anyway (idx_prev) and adds the point's error only if the bit is clear.  Downloads strip the bit.
// A pair's blocks, their geometry and every sum depend on that pair alone (no atomics): its bits do not depend on the batch.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(RT<float>) == 12 * sizeof(float) && sizeof(RT<double>) == 12 * sizeof(double), "the host writes R, t as 12 values per pair");

// slots of the moment vector a batch pass fills: error, count, sum p, sum q, sum q p^T, |p|^2, |q|^2 -- or error, count, C (21), b (6)
template <int METRIC> struct BatchAcc { static constexpr int N = (METRIC == ICP_POINT_TO_POINT) ? ICP_MOM_SQQ + 1 : ICP_MOM_B + 6; };

// What one moving point (x, y, z), matched to model point j of its pair, adds to the accumulators acc[] of its lane (all zero
// before): nothing if the match was not kept.  ONE definition for the fused tail of nn_match_batch and for batch_trim_moments,
// so that the two cannot drift and a pair that is not trimmed has the same bits on either route.  A macro, not a function: a
// __device__ function, force-inlined, is simplified on its own before it is inlined, and the eight fused instantiations then
// come out with other register numbers and commuted operands than the kernels whose timings DESIGN.md records (tried: by value,
// by reference, into a local array).  As statements they compile to the listings they always had.  To be used inside a template
// with METRIC in scope; Qx_, Qy_, Qz_: the pair's model planes, Nrm_ + q_off_: its normal planes (read for the plane metric only).
#define ICP_BATCH_POINT_TERMS(acc, kept_, x_, y_, z_, j_, Qx_, Qy_, Qz_, Nrm_, q_off_, q_plane_)                              \
    {                                                                                                                        \
        const double px = (double)(x_), py = (double)(y_), pz = (double)(z_);                                                \
        const double qx = (double)(Qx_)[j_], qy = (double)(Qy_)[j_], qz = (double)(Qz_)[j_];                                 \
        if (!(kept_)) {                                                                                                      \
            /* (a rejected point adds nothing: every accumulator stays 0, the count included) */                             \
        } else if constexpr (METRIC == ICP_POINT_TO_POINT) {                                                                 \
            acc[ICP_MOM_CNT] = 1.0;                                                                                          \
            acc[ICP_MOM_SP + 0] = px; acc[ICP_MOM_SP + 1] = py; acc[ICP_MOM_SP + 2] = pz;                                    \
            acc[ICP_MOM_SQ + 0] = qx; acc[ICP_MOM_SQ + 1] = qy; acc[ICP_MOM_SQ + 2] = qz;                                    \
            acc[ICP_MOM_SQP + 0] = qx * px; acc[ICP_MOM_SQP + 1] = qx * py; acc[ICP_MOM_SQP + 2] = qx * pz;                  \
            acc[ICP_MOM_SQP + 3] = qy * px; acc[ICP_MOM_SQP + 4] = qy * py; acc[ICP_MOM_SQP + 5] = qy * pz;                  \
            acc[ICP_MOM_SQP + 6] = qz * px; acc[ICP_MOM_SQP + 7] = qz * py; acc[ICP_MOM_SQP + 8] = qz * pz;                  \
            acc[ICP_MOM_SPP] = px * px + py * py + pz * pz;                                                                  \
            acc[ICP_MOM_SQQ] = qx * qx + qy * qy + qz * qz;                                                                  \
        } else {                                                                                                             \
            acc[ICP_MOM_CNT] = 1.0;                                                                                          \
            const F* Nx = (Nrm_) + (q_off_);                                                                                 \
            const double nx = (double)Nx[j_], ny = (double)Nx[(q_plane_) + j_], nz = (double)Nx[2 * (q_plane_) + j_];        \
            double cn[6];                                                                                                    \
            cn[0] = py * nz - pz * ny;                                                                                       \
            cn[1] = pz * nx - px * nz;                                                                                       \
            cn[2] = px * ny - py * nx;                                                                                       \
            cn[3] = nx; cn[4] = ny; cn[5] = nz;                                                                              \
            const double bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;                                              \
            int o = ICP_MOM_C;                                                                                               \
            _Pragma("unroll") for (int a = 0; a < 6; ++a)                                                                    \
                _Pragma("unroll") for (int c = a; c < 6; ++c) acc[o++] += cn[a] * cn[c];                                     \
            _Pragma("unroll") for (int a = 0; a < 6; ++a) acc[ICP_MOM_B + a] -= cn[a] * bi;                                  \
        }                                                                                                                    \
    }

// DEFER (its own instantiations, <F, METRIC, true, true>, for a batch that trims: see batch_trim_select below): the gated front
// end and the same search, and a tail in which wave 0 only stores idx_cur[gi] = j and dist[gi] = the merged minimum b -- no
// decision, no terms; the row carries ICP_MOM_ERR and zeros.  The fused instantiations never touch dist.
template <typename F, int METRIC, bool GATE, bool DEFER = false>
__global__ __launch_bounds__(NN_BLOCK) void nn_match_batch(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                           const int* __restrict__ mode, const RT<F>* __restrict__ rts,
                                                           F* __restrict__ P, long long p_plane, const F* __restrict__ Q,
                                                           const F* __restrict__ Nrm, long long q_plane,
                                                           const int32_t* __restrict__ idx_prev, int32_t* __restrict__ idx_cur,
                                                           double* __restrict__ partials, const F* __restrict__ thr,
                                                           F* __restrict__ dist)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = BatchCfg<F>::TW, C = NN_CHUNK;
    constexpr int NACC = BatchAcc<METRIC>::N;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM, "one point per lane, four waves per item");
    __shared__ __attribute__((aligned(16))) F sq[4][3][TW];
    __shared__ F md[4][BATCH_ITEM];
    __shared__ int mi[4][BATCH_ITEM];

    const BatchItem it = items[blockIdx.x];
    const int pm = mode[it.pair];
    if (pm == 0) return;   // the pair has ended (or takes no part in this pass): the whole block leaves
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const long long gi = pr.p_off + it.first + (live ? lane : 0);   // (lanes past the item's end work on its first point: nothing of theirs is kept)
    const F* Qx = Q + pr.q_off;
    const F* Qy = Qx + q_plane;
    const F* Qz = Qx + 2 * q_plane;

    F x = P[gi], y = P[p_plane + gi], z = P[2 * p_plane + gi];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    __syncthreads();   // every wave holds its points before wave 0 overwrites them

    if (pm & BATCH_APPLY) {
        apply_rt<F>(rts[it.pair], x, y, z, x, y, z);
        if (w == 0 && live) {
            P[gi] = x;
            P[p_plane + gi] = y;
            P[2 * p_plane + gi] = z;
            const int jr = idx_prev[gi];
            const int j = GATE ? (jr & BATCH_IDX_MASK) : jr;
            const double dx = (double)Qx[j] - (double)x;
            const double dy = (double)Qy[j] - (double)y;
            const double dz = (double)Qz[j] - (double)z;
            if (!GATE || jr >= 0) acc[ICP_MOM_ERR] = dx * dx + dy * dy + dz * dz;   // (only a point kept by that matching pass)
        }
    }

    if (pm & BATCH_MATCH) {
        const int m = pr.m;
        const int wseg = ((m + 3) / 4 + C - 1) / C * C;   // model points per wave, whole chunks
        const int my0 = w * wseg, my1 = min(my0 + wseg, m);  // may be empty (my1 <= my0)
        const int ntile = (wseg + TW - 1) / TW;           // the same for every wave: the barriers pair up
        F best = inf_<F>();
        int cst = -1;   // first model index of the chunk that last lowered `best`
        for (int k = 0; k < ntile; ++k) {
            const int t0 = my0 + k * TW;
            __syncthreads();
            // this wave's sub-tile; places past the quarter's end hold +inf, which never lowers a minimum
            for (int e = lane; e < TW; e += 64) {
                const int j = t0 + e;
                F qx = inf_<F>(), qy = inf_<F>(), qz = inf_<F>();
                if (j < my1) { qx = Qx[j]; qy = Qy[j]; qz = Qz[j]; }
                sq[w][0][e] = qx;
                sq[w][1][e] = qy;
                sq[w][2][e] = qz;
            }
            __syncthreads();
            const int len = min(TW, my1 - t0);   // <= 0: this wave's quarter is exhausted
            for (int c = 0; c < len; c += C) {
                const F bo = best;
#pragma unroll
                for (int kk = 0; kk < C; kk += VN) {
                    const V qx = *reinterpret_cast<const V*>(&sq[w][0][c + kk]);
                    const V qy = *reinterpret_cast<const V*>(&sq[w][1][c + kk]);
                    const V qz = *reinterpret_cast<const V*>(&sq[w][2][c + kk]);
#pragma unroll
                    for (int v = 0; v < VN; ++v) best = fmin_(best, dist2<F>(x, y, z, vget(qx, v), vget(qy, v), vget(qz, v)));
                }
                cst = (best < bo) ? t0 + c : cst;
            }
        }
        // the lowest j of the winning chunk with d_j == min (global memory, L2-resident)
        int bi = 0x7fffffff;
        if (cst >= 0) {
            bi = cst;
            for (int kk = C - 1; kk >= 0; --kk) {
                const int j = cst + kk;
                if (j < my1) {
                    const F d = dist2<F>(x, y, z, Qx[j], Qy[j], Qz[j]);
                    bi = (d == best) ? j : bi;
                }
            }
        }
        md[w][lane] = cst >= 0 ? best : inf_<F>();
        mi[w][lane] = bi;
        __syncthreads();
        if (w == 0 && live) {
            F b = md[0][lane];
            int j = mi[0][lane];
#pragma unroll
            for (int ww = 1; ww < 4; ++ww)
                if (md[ww][lane] < b) { b = md[ww][lane]; j = mi[ww][lane]; }
            j = ((unsigned)j < (unsigned)m) ? j : 0;   // (nothing found only if every distance overflowed: idx stays in range)
            if constexpr (DEFER) {
                // (the deferred route: batch_trim_select ranks the pair's distances, batch_trim_moments decides and forms the terms)
                idx_cur[gi] = j;
                dist[gi] = b;
            } else {
                const bool kept = !GATE || b <= thr[it.pair];
                idx_cur[gi] = kept ? j : (j | BATCH_IDX_REJECTED);
                ICP_BATCH_POINT_TERMS(acc, kept, x, y, z, j, Qx, Qy, Qz, Nrm, pr.q_off, q_plane)
            }
        }
    }
    // (waves 1-3 add zeros: the row is wave 0's 64 lanes, summed in lane order)
    block_sum_store<NACC, NN_BLOCK>(acc, partials + (size_t)blockIdx.x * ICP_NMOM);
}

// ------------------------------------------------------------------------------------------------
// reciprocal matches (icp_batch_set_reciprocal): the reverse search of a step -- rev[j] = the lowest i that minimises
// dist2<F>(p_i, q_j) over the pair's n moving points, for every model point j of every reciprocal pair that matches in this
// step.  nn_match_batch with the two clouds exchanged, and only its search:
//   grid = one block per MODEL work item (q_items: BATCH_ITEM model points of one pair, the items of knn4_batch); all four
//   waves hold the item's model points (one per lane); wave w scans the w-th contiguous quarter of the pair's MOVING cloud,
//   wseg = ceil(ceil(n / 4) / NN_CHUNK) * NN_CHUNK points, through its own LDS sub-tile of BatchCfg<F>::TW points (every lane
//   reads the same address: a broadcast, no bank conflict), keeping the running minimum and the first chunk that lowered it;
//   the lowest index inside that chunk is recovered from global memory, and the quarters are merged in ascending order with a
//   strict <: the lowest i wins ties.
// No front end, no accumulators, no block_sum_store: wave 0 writes rev[q_off + first + lane] for its live lanes and nothing
// else.  P is read as the forward launch of the same step left it (stream order): the cloud this pass matched on.  dist2
// squares its differences, so the distance of (j, i) here is the forward distance of (i, j) bit for bit.  A block leaves at
// once when its pair does not match in this step or is not reciprocal: rev keeps that pair's rows of its last matching pass.
// The scan is restated, not shared with nn_match_batch, whose listings stay as they are (see ICP_BATCH_POINT_TERMS).
// LDS: 4 x 3 x TW x sizeof(F) = 24 KiB of tiles + 2 KiB of merge slots, the forward kernel's footprint (six blocks per CU).
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void nn_match_batch_rev(const BatchItem* __restrict__ q_items, const BatchPair* __restrict__ pairs,
                                                               const int* __restrict__ mode, const uint8_t* __restrict__ recip,
                                                               const F* __restrict__ P, long long p_plane, const F* __restrict__ Q,
                                                               long long q_plane, int32_t* __restrict__ rev)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = BatchCfg<F>::TW, C = NN_CHUNK;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM && TW % C == 0, "one model point per lane, four waves per item, whole chunks per tile");
    __shared__ __attribute__((aligned(16))) F sp[4][3][TW];
    __shared__ F md[4][BATCH_ITEM];
    __shared__ int mi[4][BATCH_ITEM];

    const BatchItem it = q_items[blockIdx.x];
    if (!(mode[it.pair] & BATCH_MATCH) || recip[it.pair] == 0) return;   // (block-uniform: no barrier is left waiting)
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const long long gj = pr.q_off + it.first + (live ? lane : 0);   // (lanes past the item's end work on its first point: nothing of theirs is kept)
    const F* Px = P + pr.p_off;
    const F* Py = Px + p_plane;
    const F* Pz = Px + 2 * p_plane;
    const F x = Q[gj], y = Q[q_plane + gj], z = Q[2 * q_plane + gj];

    const int n = pr.n;
    const int wseg = ((n + 3) / 4 + C - 1) / C * C;   // moving points per wave, whole chunks
    const int my0 = w * wseg, my1 = min(my0 + wseg, n);  // may be empty (my1 <= my0)
    const int ntile = (wseg + TW - 1) / TW;           // the same for every wave: the barriers pair up
    F best = inf_<F>();
    int cst = -1;   // first moving index of the chunk that last lowered `best`
    for (int k = 0; k < ntile; ++k) {
        const int t0 = my0 + k * TW;
        __syncthreads();
        // this wave's sub-tile; places past the quarter's end hold +inf, which never lowers a minimum
        for (int e = lane; e < TW; e += 64) {
            const int i = t0 + e;
            F px = inf_<F>(), py = inf_<F>(), pz = inf_<F>();
            if (i < my1) { px = Px[i]; py = Py[i]; pz = Pz[i]; }
            sp[w][0][e] = px;
            sp[w][1][e] = py;
            sp[w][2][e] = pz;
        }
        __syncthreads();
        const int len = min(TW, my1 - t0);   // <= 0: this wave's quarter is exhausted
        for (int c = 0; c < len; c += C) {
            const F bo = best;
#pragma unroll
            for (int kk = 0; kk < C; kk += VN) {
                const V px = *reinterpret_cast<const V*>(&sp[w][0][c + kk]);
                const V py = *reinterpret_cast<const V*>(&sp[w][1][c + kk]);
                const V pz = *reinterpret_cast<const V*>(&sp[w][2][c + kk]);
#pragma unroll
                for (int v = 0; v < VN; ++v) best = fmin_(best, dist2<F>(vget(px, v), vget(py, v), vget(pz, v), x, y, z));
            }
            cst = (best < bo) ? t0 + c : cst;
        }
    }
    // the lowest i of the winning chunk with d_i == min (global memory, L2-resident)
    int bi = 0x7fffffff;
    if (cst >= 0) {
        bi = cst;
        for (int kk = C - 1; kk >= 0; --kk) {
            const int i = cst + kk;
            if (i < my1) {
                const F d = dist2<F>(Px[i], Py[i], Pz[i], x, y, z);
                bi = (d == best) ? i : bi;
            }
        }
    }
    md[w][lane] = cst >= 0 ? best : inf_<F>();
    mi[w][lane] = bi;
    __syncthreads();
    if (w == 0 && live) {
        F b = md[0][lane];
        int i = mi[0][lane];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww)
            if (md[ww][lane] < b) { b = md[ww][lane]; i = mi[ww][lane]; }
        rev[gj] = ((unsigned)i < (unsigned)n) ? i : 0;   // (nothing found only if every distance overflowed: rev stays in range)
    }
}

// ------------------------------------------------------------------------------------------------
// trimmed rejection (icp_batch_set_trim): a pair keeps the K closest of its n matches (and every match tied with the K-th).  The
// K-th smallest distance of a pair is known only when every one of its points has been matched -- by other blocks, for a
// pair of more than one work item -- so the fused pass cannot decide; a step of a batch that trims runs four launches:
//   nn_match_batch<.., DEFER>   front end + search as the gated pass; wave 0 stores idx and the winning distance, no terms
//   batch_trim_select         one block per pair: tau[pair] = the K-th smallest of the pair's n distances
//   batch_trim_moments        one block per work item: kept = d <= tau[pair] (and d <= thr[pair]); marks idx, forms the terms
//   batch_finalize_kernel     as ever
// A pair's tau, its masks and its sums depend on that pair alone: integer counts, fixed summation order, no floating-point
// atomics.  A pair that is not trimmed (rank 0, tau = +inf, written once by the host) keeps everything, and its rows are the
// fused pass's bit for bit: the same terms (ICP_BATCH_POINT_TERMS) in the same lanes through the same block_sum_store.
// ------------------------------------------------------------------------------------------------
// the values are >= +0 and never NaN (a sum of squares of finite differences, +inf on overflow): their bit patterns, read as
// unsigned integers, sort as the values do
template <typename F> struct TrimKey;
template <> struct TrimKey<float> {
    using U = unsigned int;
    static __device__ __forceinline__ U key(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(U k) { return __uint_as_float(k); }
};
template <> struct TrimKey<double> {
    using U = unsigned long long;
    static __device__ __forceinline__ U key(double v) { return (U)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(U k) { return __longlong_as_double((long long)k); }
};

// one block per pair: tau[pair] = the rank[pair]-th smallest of dist[p_off .. p_off + n), one of those values bit for bit.
// Most-significant-digit radix select, 8 bits per round (4 rounds for fp32, 8 for fp64): every thread adds the values that
// still carry the prefix found so far to a 256-bin LDS histogram of their next digit (integer LDS atomics: the counts do not
// depend on the order of the adds), wave 0 scans the bins for the one that holds the remaining rank, and that digit joins the
// prefix.  Each round re-reads the pair's at most ICP_BATCH_MAX_POINTS values (L2-resident).  rank 0: the pair is not trimmed.
constexpr int TRIM_BLOCK = 256;
template <typename F>
__global__ __launch_bounds__(TRIM_BLOCK) void batch_trim_select(const BatchPair* __restrict__ pairs, const int* __restrict__ mode,
                                                                const int* __restrict__ rank, const F* __restrict__ dist,
                                                                F* __restrict__ tau)
{
    using K = TrimKey<F>;
    using U = typename K::U;
    constexpr int BITS = 8 * (int)sizeof(U);
    __shared__ unsigned int hist[256];
    __shared__ U s_prefix;
    __shared__ unsigned int s_rest;
    const int pair = blockIdx.x;
    if (!(mode[pair] & BATCH_MATCH)) return;
    const int kth = rank[pair];
    const int n = pairs[pair].n;
    if (kth < 1 || kth > n) return;   // not trimmed (a trimmed pair's rank lies in [1, n])
    const F* d = dist + pairs[pair].p_off;
    const int lane = threadIdx.x & 63;
    U prefix = 0;
    unsigned int rest = (unsigned int)(kth - 1);   // values below the wanted one among those that carry the prefix
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0u;
        __syncthreads();
        // (a shift by the type's width is undefined: the first round, where every value carries the empty prefix, has no mask)
        const U high = (shift + 8 < BITS) ? (~U(0) << ((shift + 8) & (BITS - 1))) : U(0);
        for (int i = threadIdx.x; i < n; i += TRIM_BLOCK) {
            const U k = K::key(d[i]);
            if ((k & high) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // lane l holds bins 4l .. 4l + 3; an inclusive scan over the lanes finds the lane, then the bin, that holds `rest`
            const unsigned int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const unsigned int mine = c0 + c1 + c2 + c3;
            unsigned int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const unsigned int excl = incl - mine;
            if (excl <= rest && rest < incl) {   // exactly one lane: the bins hold more than `rest` values between them
                unsigned int r = rest - excl, bin = 4u * lane;
                if (r >= c0) { r -= c0; ++bin; if (r >= c1) { r -= c1; ++bin; if (r >= c2) { r -= c2; ++bin; } } }
                s_prefix = prefix | ((U)bin << shift);
                s_rest = r;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rest = s_rest;
    }
    if (threadIdx.x == 0) tau[pair] = K::value(prefix);
}

// one block per work item, over nn_match_batch's items and in its block shape (wave 0 alone carries data, waves 1-3 add zeros, so
// that block_sum_store adds a row in the fused pass's order): kept = batch_kept's d <= tau[pair] && (no gate || d <= thr[pair]); a rejected
// point's idx entry gets BATCH_IDX_REJECTED; the kept points' terms go to slots 1 .. of the item's row.  Slot ICP_MOM_ERR, which
// nn_match_batch<.., DEFER> wrote, is not touched.
// MUTUAL (its own instantiations, for a batch with a reciprocal pair; the others keep their code and never read rev or recip):
// kept = mutual && d <= tau[pair] && d <= thr[pair], three independent tests, with mutual = rev[idx[i]] == i for a pair whose flag
// recip[pair] is set (rev: nn_match_batch_rev's, of this step) and true for a pair whose flag is 0.  These instantiations take a
// NULL tau -- a reciprocal batch that holds no trim allocates no tau and launches no batch_trim_select -- and read it as +inf.  A
// pair with flag 0 and no trim keeps what the gate keeps: the fused pass's rows bit for bit, as any untrimmed pair on this route.
template <typename F, int METRIC, bool MUTUAL = false>
__global__ __launch_bounds__(NN_BLOCK) void batch_trim_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                               const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                               const F* __restrict__ Q, const F* __restrict__ Nrm, long long q_plane,
                                                               int32_t* __restrict__ idx_cur, const F* __restrict__ dist,
                                                               const F* __restrict__ tau, const F* __restrict__ thr,
                                                               double* __restrict__ partials, const int32_t* __restrict__ rev = nullptr,
                                                               const uint8_t* __restrict__ recip = nullptr)
{
    constexpr int NACC = BatchAcc<METRIC>::N;
    static_assert(ICP_MOM_ERR == 0, "the row's slots behind the error are written as one run");
    const BatchItem it = items[blockIdx.x];
    if (!(mode[it.pair] & BATCH_MATCH)) return;   // nothing was matched for this pair: the row stays the error and zeros
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (w == 0 && lane < it.count) {
        const long long gi = pr.p_off + it.first + lane;
        const F* Qx = Q + pr.q_off;
        const int j = idx_cur[gi];
        const bool kept = batch_kept<F, MUTUAL, !MUTUAL>(dist[gi], it.pair, tau, thr, recip, rev, pr.q_off + j, it.first + lane);
        if (!kept) idx_cur[gi] = j | BATCH_IDX_REJECTED;
        const F* Qy = Qx + q_plane;
        const F* Qz = Qx + 2 * q_plane;
        const F x = P[gi], y = P[p_plane + gi], z = P[2 * p_plane + gi];
        ICP_BATCH_POINT_TERMS(acc, kept, x, y, z, j, Qx, Qy, Qz, Nrm, pr.q_off, q_plane)
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}
#undef ICP_BATCH_POINT_TERMS

// ------------------------------------------------------------------------------------------------
// robust kernels (icp_batch_set_robust): the decision, the residual, the weight and the weighted terms of a step of a batch that
// holds a robust pair -- batch_trim_moments' place on the deferred route, over the same items and in its block shape (wave 0 alone
// carries data, waves 1-3 add zeros, block_sum_store adds a row in the fused pass's order).
//   kept: batch_kept, batch_trim_moments' decision.  A rejected point's idx entry gets BATCH_IDX_REJECTED and its weight entry 0.0.
//   residual, in double from the widened coordinates: point-to-point r2 = dx*dx + dy*dy + dz*dz, d = q - p (the front end's error
//     arithmetic); point-to-plane r2 = bi * bi, the bi of the plane terms.
//   weight w, in double, from kind[pair], k[pair], k2[pair] = k * k (the host's product): Huber r2 <= k2 ? 1 : k / sqrt(r2), Cauchy
//     1 / (1 + r2 / k2), Tukey r2 <= k2 ? (1 - r2/k2)^2 : 0, none 1.0 exactly.  r2 = +inf: 0 for all three.  weights[gi] = w.
//   terms: ICP_MOM_CNT = 1, ICP_MOM_W = w, every other slot the fused pass's term times w.  w = 1.0 multiplies exactly, so a
//     pair without a kernel has the rows of batch_trim_moments bit for bit.
// The block writes slots 1 .. ICP_MOM_W of its row -- zeros in the slots between the metric's last one and ICP_MOM_W, which no
// other launch writes -- and leaves ICP_MOM_ERR, the matching launch's.  A pair that takes part in the step without matching (the
// loop's error-only last pass) gets zeros throughout: nothing of an earlier pass's weight sum stays in the row.
// The point's terms are restated, not routed through ICP_BATCH_POINT_TERMS: the existing kernels keep their listings (see that
// macro's comment).  No LDS beyond block_sum_store's 4 x 29 doubles.
// ------------------------------------------------------------------------------------------------
template <typename F, int METRIC, bool MUTUAL>
__global__ __launch_bounds__(NN_BLOCK) void batch_robust_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                                 const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                                 const F* __restrict__ Q, const F* __restrict__ Nrm, long long q_plane,
                                                                 int32_t* __restrict__ idx_cur, const F* __restrict__ dist,
                                                                 const F* __restrict__ tau, const F* __restrict__ thr,
                                                                 const int* __restrict__ kind, const double* __restrict__ ks,
                                                                 const double* __restrict__ k2s, double* __restrict__ weights,
                                                                 double* __restrict__ partials, const int32_t* __restrict__ rev,
                                                                 const uint8_t* __restrict__ recip)
{
    constexpr int NACC = ICP_MOM_W + 1;
    static_assert(ICP_MOM_ERR == 0 && BatchAcc<METRIC>::N <= ICP_MOM_W && ICP_MOM_W < ICP_NMOM, "the weight sum sits behind every slot of either metric");
    const BatchItem it = items[blockIdx.x];
    const int pm = mode[it.pair];
    if (pm == 0) return;   // the pair takes no part in this step: its row is not read
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if ((pm & BATCH_MATCH) && w == 0 && lane < it.count) {
        const long long gi = pr.p_off + it.first + lane;
        const F* Qx = Q + pr.q_off;
        const F* Qy = Qx + q_plane;
        const F* Qz = Qx + 2 * q_plane;
        const int j = idx_cur[gi];   // in [0, m): the matching launch wrote it
        const bool kept = batch_kept<F, MUTUAL>(dist[gi], it.pair, tau, thr, recip, rev, pr.q_off + j, it.first + lane);
        double wgt = 0.0;
        if (!kept) {
            idx_cur[gi] = j | BATCH_IDX_REJECTED;   // (a rejected point adds nothing: every accumulator stays 0, the count included)
        } else {
            const double px = (double)P[gi], py = (double)P[p_plane + gi], pz = (double)P[2 * p_plane + gi];
            const double qx = (double)Qx[j], qy = (double)Qy[j], qz = (double)Qz[j];
            const int kd = kind[it.pair];
            const double kk = ks[it.pair], kk2 = k2s[it.pair];
            double r2, nx = 0.0, ny = 0.0, nz = 0.0, bi = 0.0;
            if constexpr (METRIC == ICP_POINT_TO_POINT) {
                const double dx = qx - px, dy = qy - py, dz = qz - pz;
                r2 = dx * dx + dy * dy + dz * dz;
            } else {
                const F* Nx = Nrm + pr.q_off;
                nx = (double)Nx[j]; ny = (double)Nx[q_plane + j]; nz = (double)Nx[2 * q_plane + j];
                bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
                r2 = bi * bi;
            }
            wgt = 1.0;
            if (kd == ICP_ROBUST_HUBER) {
                wgt = r2 <= kk2 ? 1.0 : kk / sqrt(r2);
            } else if (kd == ICP_ROBUST_CAUCHY) {
                wgt = 1.0 / (1.0 + r2 / kk2);
            } else if (kd == ICP_ROBUST_TUKEY) {
                const double u = 1.0 - r2 / kk2;
                wgt = r2 <= kk2 ? u * u : 0.0;
            }
            acc[ICP_MOM_CNT] = 1.0;
            acc[ICP_MOM_W] = wgt;
            if constexpr (METRIC == ICP_POINT_TO_POINT) {
                acc[ICP_MOM_SP + 0] = px * wgt; acc[ICP_MOM_SP + 1] = py * wgt; acc[ICP_MOM_SP + 2] = pz * wgt;
                acc[ICP_MOM_SQ + 0] = qx * wgt; acc[ICP_MOM_SQ + 1] = qy * wgt; acc[ICP_MOM_SQ + 2] = qz * wgt;
                acc[ICP_MOM_SQP + 0] = (qx * px) * wgt; acc[ICP_MOM_SQP + 1] = (qx * py) * wgt; acc[ICP_MOM_SQP + 2] = (qx * pz) * wgt;
                acc[ICP_MOM_SQP + 3] = (qy * px) * wgt; acc[ICP_MOM_SQP + 4] = (qy * py) * wgt; acc[ICP_MOM_SQP + 5] = (qy * pz) * wgt;
                acc[ICP_MOM_SQP + 6] = (qz * px) * wgt; acc[ICP_MOM_SQP + 7] = (qz * py) * wgt; acc[ICP_MOM_SQP + 8] = (qz * pz) * wgt;
                acc[ICP_MOM_SPP] = (px * px + py * py + pz * pz) * wgt;
                acc[ICP_MOM_SQQ] = (qx * qx + qy * qy + qz * qz) * wgt;
            } else {
                double cn[6];
                cn[0] = py * nz - pz * ny;
                cn[1] = pz * nx - px * nz;
                cn[2] = px * ny - py * nx;
                cn[3] = nx; cn[4] = ny; cn[5] = nz;
                int o = ICP_MOM_C;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c) acc[o++] += (cn[a] * cn[c]) * wgt;
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[ICP_MOM_B + a] -= (cn[a] * bi) * wgt;
            }
        }
        weights[gi] = wgt;
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}

// one block per pair: mom[pair] = the pair's item rows added up in a fixed order (thread (k, part) adds items part, part + 8, ...
// of slot k; the eight part sums are then added in part order -- finalize_kernel's scheme, over the pair's own items only).
// last = the metric's last slot: ICP_MOM_SQQ, or ICP_MOM_B + 5 for a plane loop; the slots behind it are written as zeros.
__global__ __launch_bounds__(256) void batch_finalize_kernel(const BatchPair* __restrict__ pairs, const int* __restrict__ mode,
                                                             const double* __restrict__ partials, int last, double* __restrict__ mom)
{
    __shared__ double red[8][ICP_NMOM];
    if (mode[blockIdx.x] == 0) return;
    const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int i0 = pairs[blockIdx.x].item0, i1 = pairs[blockIdx.x].item1;
    double s = 0.0;
    if (k <= last)
        for (int i = i0 + part; i < i1; i += 8) s += partials[(size_t)i * ICP_NMOM + k];
    red[part][k] = s;
    __syncthreads();
    if (threadIdx.x < ICP_NMOM) {
        double tot = red[0][k];
#pragma unroll
        for (int p = 1; p < 8; ++p) tot += red[p][k];
        mom[(size_t)blockIdx.x * ICP_NMOM + k] = tot;
    }
}

hipError_t launch_batch_pass(const BatchPassArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    const bool plane = a.metric == ICP_POINT_TO_PLANE;
    if (plane && !a.N_soa) return hipErrorInvalidValue;
    if (a.trim_rank && (!a.dist || !a.tau)) return hipErrorInvalidValue;
    if (a.recip && (!a.dist || !a.rev || !a.q_items || a.n_q_items <= 0)) return hipErrorInvalidValue;
    if (a.robust_kind && (!a.robust_k || !a.robust_k2 || !a.weights || !a.dist)) return hipErrorInvalidValue;
    if (a.metric == ICP_GENERALIZED || a.metric == ICP_COLORED || a.metric == ICP_SYMMETRIC) {
        // the generalized metric: matching without a decision (the point-to-point instantiation), [the reverse search,] [the K-th
        // distance of every pair,] then batch_gicp_moments (icp_k_gicp.hip): the decision and the terms of the 6 x 6 system.  The
        // colored metric: the same launches with batch_color_moments (icp_k_color.hip) in its place; the symmetric metric: with
        // batch_sym_moments (icp_k_sym.hip)
        if (a.robust_kind || !a.dist) return hipErrorInvalidValue;
#define ICP_LAUNCH_BATCH_GICP(F)                                                                                                 \
    do {                                                                                                                         \
        hipLaunchKernelGGL((nn_match_batch<F, ICP_POINT_TO_POINT, true, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items,  \
                           a.pairs, a.mode, (const RT<F>*)a.rt, (F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)nullptr,     \
                           a.q_plane, a.idx_prev, a.idx_cur, a.partials, (const F*)nullptr, (F*)a.dist);                          \
        if (a.recip)                                                                                                             \
            hipLaunchKernelGGL((nn_match_batch_rev<F>), dim3(a.n_q_items), dim3(NN_BLOCK), 0, st, a.q_items, a.pairs, a.mode,     \
                               a.recip, (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, a.q_plane, a.rev);                       \
        if (a.trim_rank)                                                                                                         \
            hipLaunchKernelGGL((batch_trim_select<F>), dim3(a.n_pairs), dim3(TRIM_BLOCK), 0, st, a.pairs, a.mode, a.trim_rank,    \
                               (const F*)a.dist, (F*)a.tau);                                                                      \
    } while (0)
        if (a.precision == ICP_F64) ICP_LAUNCH_BATCH_GICP(double); else ICP_LAUNCH_BATCH_GICP(float);
#undef ICP_LAUNCH_BATCH_GICP
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (hipError_t e = a.metric == ICP_COLORED     ? launch_batch_color_moments(a, st)
                           : a.metric == ICP_SYMMETRIC ? launch_batch_sym_moments(a, st)
                                                       : launch_batch_gicp_moments(a, st);
            e != hipSuccess)
            return e;
        hipLaunchKernelGGL(batch_finalize_kernel, dim3(a.n_pairs), dim3(256), 0, st, a.pairs, a.mode, (const double*)a.partials,
                           ICP_MOM_B + 5, a.mom);
        return hipGetLastError();
    }
#define ICP_LAUNCH_BATCH(F, MET, GATE)                                                                                          \
    hipLaunchKernelGGL((nn_match_batch<F, MET, GATE>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,          \
                       (const RT<F>*)a.rt, (F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx_prev,   \
                       a.idx_cur, a.partials, (const F*)a.thr, (F*)nullptr)
    // a batch that trims: matching without a decision, the K-th distance of every pair, then the decision and the terms
#define ICP_LAUNCH_BATCH_TRIM(F, MET)                                                                                            \
    do {                                                                                                                         \
        hipLaunchKernelGGL((nn_match_batch<F, MET, true, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs,        \
                           a.mode, (const RT<F>*)a.rt, (F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)nullptr, a.q_plane,   \
                           a.idx_prev, a.idx_cur, a.partials, (const F*)nullptr, (F*)a.dist);                                     \
        hipLaunchKernelGGL((batch_trim_select<F>), dim3(a.n_pairs), dim3(TRIM_BLOCK), 0, st, a.pairs, a.mode, a.trim_rank,        \
                           (const F*)a.dist, (F*)a.tau);                                                                          \
        hipLaunchKernelGGL((batch_trim_moments<F, MET>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,        \
                           (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx_cur,              \
                           (const F*)a.dist, (const F*)a.tau, (const F*)a.thr, a.partials);                                       \
    } while (0)
    // a batch with a reciprocal pair: matching without a decision, the reverse search, [the K-th distance of every pair where the
    // batch also trims,] then the decision -- mutual, trim, gate -- and the terms
#define ICP_LAUNCH_BATCH_RECIP(F, MET)                                                                                           \
    do {                                                                                                                         \
        hipLaunchKernelGGL((nn_match_batch<F, MET, true, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs,        \
                           a.mode, (const RT<F>*)a.rt, (F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)nullptr, a.q_plane,   \
                           a.idx_prev, a.idx_cur, a.partials, (const F*)nullptr, (F*)a.dist);                                     \
        hipLaunchKernelGGL((nn_match_batch_rev<F>), dim3(a.n_q_items), dim3(NN_BLOCK), 0, st, a.q_items, a.pairs, a.mode,         \
                           a.recip, (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, a.q_plane, a.rev);                           \
        if (a.trim_rank)                                                                                                         \
            hipLaunchKernelGGL((batch_trim_select<F>), dim3(a.n_pairs), dim3(TRIM_BLOCK), 0, st, a.pairs, a.mode, a.trim_rank,    \
                               (const F*)a.dist, (F*)a.tau);                                                                      \
        hipLaunchKernelGGL((batch_trim_moments<F, MET, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,  \
                           (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx_cur,              \
                           (const F*)a.dist, a.trim_rank ? (const F*)a.tau : (const F*)nullptr, (const F*)a.thr, a.partials,      \
                           (const int32_t*)a.rev, a.recip);                                                                       \
    } while (0)
    // a batch with a robust pair: matching without a decision, [the reverse search,] [the K-th distance of every pair,] then the
    // decision, the weights and the weighted terms
#define ICP_LAUNCH_BATCH_ROBUST(F, MET, MUT)                                                                                     \
    do {                                                                                                                         \
        hipLaunchKernelGGL((nn_match_batch<F, MET, true, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs,        \
                           a.mode, (const RT<F>*)a.rt, (F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)nullptr, a.q_plane,   \
                           a.idx_prev, a.idx_cur, a.partials, (const F*)nullptr, (F*)a.dist);                                     \
        if (MUT)                                                                                                                 \
            hipLaunchKernelGGL((nn_match_batch_rev<F>), dim3(a.n_q_items), dim3(NN_BLOCK), 0, st, a.q_items, a.pairs, a.mode,     \
                               a.recip, (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, a.q_plane, a.rev);                       \
        if (a.trim_rank)                                                                                                         \
            hipLaunchKernelGGL((batch_trim_select<F>), dim3(a.n_pairs), dim3(TRIM_BLOCK), 0, st, a.pairs, a.mode, a.trim_rank,    \
                               (const F*)a.dist, (F*)a.tau);                                                                      \
        hipLaunchKernelGGL((batch_robust_moments<F, MET, MUT>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs,         \
                           a.mode, (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx_cur,      \
                           (const F*)a.dist, a.trim_rank ? (const F*)a.tau : (const F*)nullptr, (const F*)a.thr, a.robust_kind,   \
                           a.robust_k, a.robust_k2, a.weights, a.partials, (const int32_t*)a.rev, a.recip);                       \
    } while (0)
#define ICP_LAUNCH_BATCH_F(F)                                                                                                  \
    do {                                                                                                                       \
        if (a.robust_kind && a.recip) {                                                                                        \
            if (plane) ICP_LAUNCH_BATCH_ROBUST(F, ICP_POINT_TO_PLANE, true); else ICP_LAUNCH_BATCH_ROBUST(F, ICP_POINT_TO_POINT, true); \
        } else if (a.robust_kind) {                                                                                            \
            if (plane) ICP_LAUNCH_BATCH_ROBUST(F, ICP_POINT_TO_PLANE, false); else ICP_LAUNCH_BATCH_ROBUST(F, ICP_POINT_TO_POINT, false); \
        } else if (a.recip) {                                                                                                         \
            if (plane) ICP_LAUNCH_BATCH_RECIP(F, ICP_POINT_TO_PLANE); else ICP_LAUNCH_BATCH_RECIP(F, ICP_POINT_TO_POINT);      \
        } else if (a.trim_rank) {                                                                                                   \
            if (plane) ICP_LAUNCH_BATCH_TRIM(F, ICP_POINT_TO_PLANE); else ICP_LAUNCH_BATCH_TRIM(F, ICP_POINT_TO_POINT);        \
        } else if (a.thr) {                                                                                                    \
            if (plane) ICP_LAUNCH_BATCH(F, ICP_POINT_TO_PLANE, true); else ICP_LAUNCH_BATCH(F, ICP_POINT_TO_POINT, true);      \
        } else {                                                                                                               \
            if (plane) ICP_LAUNCH_BATCH(F, ICP_POINT_TO_PLANE, false); else ICP_LAUNCH_BATCH(F, ICP_POINT_TO_POINT, false);    \
        }                                                                                                                      \
    } while (0)
    if (a.precision == ICP_F64) ICP_LAUNCH_BATCH_F(double); else ICP_LAUNCH_BATCH_F(float);
#undef ICP_LAUNCH_BATCH_F
#undef ICP_LAUNCH_BATCH_ROBUST
#undef ICP_LAUNCH_BATCH_RECIP
#undef ICP_LAUNCH_BATCH_TRIM
#undef ICP_LAUNCH_BATCH
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_finalize_kernel, dim3(a.n_pairs), dim3(256), 0, st, a.pairs, a.mode, (const double*)a.partials,
                       a.robust_kind ? ICP_MOM_W : plane ? ICP_MOM_B + 5 : ICP_MOM_SQQ, a.mom);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// evaluation (icp_batch_evaluate): how well every pair is registered where its moving cloud stands -- kept count, squared
// distances, and the sums a 6 x 6 information matrix is assembled from.  Three launches, none of which writes anything the loop
// reads again:
//   nn_match_batch<F, POINT, true, true>   the deferred matching instantiation, mode BATCH_MATCH alone: P is only read; the loop's
//                                          own idx and winning distance, into evaluation-only buffers
//   batch_eval_moments                     one block per work item: kept = d <= thr[pair] (thr == NULL: everything), marks idx, forms
//                                          the terms of the ICP_EVAL_* slots
//   batch_finalize_kernel                  as ever, into an evaluation-only vector per pair
// batch_trim_moments' block shape: wave 0 alone carries data, waves 1-3 add zeros, block_sum_store writes the whole row (slot 0
// included).  Every term is formed in double from the widened coordinates; a pair's bits depend on that pair and its threshold alone.
//   both metrics: ICP_EVAL_SD = |q - p|^2 with the differences in double (the front end's error arithmetic), ICP_EVAL_CNT = 1
//   point-to-point: ICP_EVAL_SQ = q, ICP_EVAL_SQQ = the upper triangle of q q^T
//   point-to-plane: ICP_MOM_C .. + 20 = cn cn^T, cn = (p x n, n) -- the statements of a plane pass's C, restated here so that the
//     loop's kernels keep their listings
// ------------------------------------------------------------------------------------------------
template <int METRIC> struct BatchEvalAcc { static constexpr int N = (METRIC == ICP_POINT_TO_POINT) ? ICP_EVAL_SQQ + 6 : ICP_MOM_C + 21; };

template <typename F, int METRIC>
__global__ __launch_bounds__(NN_BLOCK) void batch_eval_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                               const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                               const F* __restrict__ Q, const F* __restrict__ Nrm, long long q_plane,
                                                               int32_t* __restrict__ idx, const F* __restrict__ dist,
                                                               const F* __restrict__ thr, double* __restrict__ partials)
{
    constexpr int NACC = BatchEvalAcc<METRIC>::N;
    static_assert(ICP_EVAL_SD == 0 && ICP_EVAL_CNT == 1 && NACC <= ICP_NMOM, "the row is written from its first slot on");
    const BatchItem it = items[blockIdx.x];
    if (!(mode[it.pair] & BATCH_MATCH)) return;   // the pair is not evaluated: nothing was matched for it
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (w == 0 && lane < it.count) {
        const long long gi = pr.p_off + it.first + lane;
        const F b = dist[gi];
        const int j = idx[gi];   // in [0, m): the matching launch wrote it
        const bool kept = thr == nullptr || b <= thr[it.pair];
        if (!kept) {
            idx[gi] = j | BATCH_IDX_REJECTED;   // (a rejected point adds nothing: every accumulator stays 0, the count included)
        } else {
            const F* Qx = Q + pr.q_off;
            const F* Qy = Qx + q_plane;
            const F* Qz = Qx + 2 * q_plane;
            const double px = (double)P[gi], py = (double)P[p_plane + gi], pz = (double)P[2 * p_plane + gi];
            const double qx = (double)Qx[j], qy = (double)Qy[j], qz = (double)Qz[j];
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            acc[ICP_EVAL_SD] = dx * dx + dy * dy + dz * dz;
            acc[ICP_EVAL_CNT] = 1.0;
            if constexpr (METRIC == ICP_POINT_TO_POINT) {
                acc[ICP_EVAL_SQ + 0] = qx; acc[ICP_EVAL_SQ + 1] = qy; acc[ICP_EVAL_SQ + 2] = qz;
                acc[ICP_EVAL_SQQ + 0] = qx * qx; acc[ICP_EVAL_SQQ + 1] = qx * qy; acc[ICP_EVAL_SQQ + 2] = qx * qz;
                acc[ICP_EVAL_SQQ + 3] = qy * qy; acc[ICP_EVAL_SQQ + 4] = qy * qz; acc[ICP_EVAL_SQQ + 5] = qz * qz;
            } else {
                const F* Nx = Nrm + pr.q_off;
                const double nx = (double)Nx[j], ny = (double)Nx[q_plane + j], nz = (double)Nx[2 * q_plane + j];
                double cn[6];
                cn[0] = py * nz - pz * ny;
                cn[1] = pz * nx - px * nz;
                cn[2] = px * ny - py * nx;
                cn[3] = nx; cn[4] = ny; cn[5] = nz;
                int o = ICP_MOM_C;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c) acc[o++] += cn[a] * cn[c];
            }
        }
    }
    block_sum_store<NACC, NN_BLOCK>(acc, partials + (size_t)blockIdx.x * ICP_NMOM);
}

hipError_t launch_batch_evaluate(const BatchEvalArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    const bool plane = a.metric == ICP_POINT_TO_PLANE;
    if (plane && !a.N_soa) return hipErrorInvalidValue;
    if (!a.idx || !a.dist || !a.partials || !a.mom) return hipErrorInvalidValue;
    // (the matching launch reads neither rt nor idx_prev without BATCH_APPLY, and neither the normals nor thr when deferred)
#define ICP_LAUNCH_BATCH_EVAL(F, MET)                                                                                            \
    do {                                                                                                                         \
        hipLaunchKernelGGL((nn_match_batch<F, ICP_POINT_TO_POINT, true, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, \
                           a.pairs, a.mode, (const RT<F>*)nullptr, (F*)const_cast<void*>(a.P_soa), a.p_plane, (const F*)a.Q_soa,  \
                           (const F*)nullptr, a.q_plane, (const int32_t*)nullptr, a.idx, a.partials, (const F*)nullptr,           \
                           (F*)a.dist);                                                                                           \
        hipLaunchKernelGGL((batch_eval_moments<F, MET>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,        \
                           (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx,                  \
                           (const F*)a.dist, (const F*)a.thr, a.partials);                                                        \
    } while (0)
    if (a.precision == ICP_F64) {
        if (plane) ICP_LAUNCH_BATCH_EVAL(double, ICP_POINT_TO_PLANE); else ICP_LAUNCH_BATCH_EVAL(double, ICP_POINT_TO_POINT);
    } else {
        if (plane) ICP_LAUNCH_BATCH_EVAL(float, ICP_POINT_TO_PLANE); else ICP_LAUNCH_BATCH_EVAL(float, ICP_POINT_TO_POINT);
    }
#undef ICP_LAUNCH_BATCH_EVAL
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_finalize_kernel, dim3(a.n_pairs), dim3(256), 0, st, a.pairs, a.mode, (const double*)a.partials,
                       plane ? ICP_MOM_C + 20 : ICP_EVAL_SQQ + 5, a.mom);
    return hipGetLastError();
}

// the start cloud of every pair of a batch that holds initial transforms (icp_batch_begin): P = apply_rt(rt0[pair], P0) -- the
// front end's own arithmetic, so a loop from here is the loop of a batch created from this cloud -- or P0's bytes for a pair
// whose kind is BATCH_INIT_COPY (the exact identity: a -0.0 stays a -0.0).  Reads P0 and writes P, as the copy it replaces.
// One wave per work item (four items per block), one point per lane; the padding between the clouds is not touched.  A
// transformed point with a NaN or an infinite coordinate raises its pair's flag (zero before the launch): a plain vector store
// of 1 from every such lane, whoever comes last.
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_init_kernel(const BatchItem* __restrict__ items, int n_items,
                                                              const BatchPair* __restrict__ pairs, const int* __restrict__ kind,
                                                              const RT<F>* __restrict__ rt0, const F* __restrict__ P0,
                                                              F* __restrict__ P, long long p_plane, int* __restrict__ nonfinite)
{
    const int item = blockIdx.x * (NN_BLOCK / BATCH_ITEM) + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const BatchItem it = items[item];
    const int lane = threadIdx.x & 63;
    if (lane >= it.count) return;
    const long long gi = pairs[it.pair].p_off + it.first + lane;
    F x = P0[gi], y = P0[p_plane + gi], z = P0[2 * p_plane + gi];
    if (kind[it.pair] != BATCH_INIT_COPY) {
        apply_rt<F>(rt0[it.pair], x, y, z, x, y, z);
        // (x - x is 0 for every finite x, NaN for NaN and for +-inf)
        const bool finite = (x - x) == F(0) && (y - y) == F(0) && (z - z) == F(0);
        if (!finite) nonfinite[it.pair] = 1;
    }
    P[gi] = x;
    P[p_plane + gi] = y;
    P[2 * p_plane + gi] = z;
}

hipError_t launch_batch_init(int precision, const BatchItem* items, int n_items, const BatchPair* pairs, const int* kind, const void* rt0,
                             const void* P0, void* P, long long p_plane, int* nonfinite, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    const int nb = (n_items + NN_BLOCK / BATCH_ITEM - 1) / (NN_BLOCK / BATCH_ITEM);
    if (precision == ICP_F64)
        hipLaunchKernelGGL((batch_init_kernel<double>), dim3(nb), dim3(NN_BLOCK), 0, st, items, n_items, pairs, kind, (const RT<double>*)rt0,
                           (const double*)P0, (double*)P, p_plane, nonfinite);
    else
        hipLaunchKernelGGL((batch_init_kernel<float>), dim3(nb), dim3(NN_BLOCK), 0, st, items, n_items, pairs, kind, (const RT<float>*)rt0,
                           (const float*)P0, (float*)P, p_plane, nonfinite);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// voxel-grid downsampling of every cloud of a batch (icp_batch_downsample, icp_batch.cpp; the rule is stated in
// include/icp_mi355x.h and every step here is one statement of it).  Brute force, as the matching kernels: a cloud has at most
// ICP_BATCH_MAX_POINTS points, so nothing is sorted.
//   batch_voxel_keys    one block per cloud: lo, hi = the component-wise minimum and maximum (comparisons only: exact), the range
//                       check floor(((double)hi - (double)lo) / v) <= VOXEL_MAX_CELL per axis -> too_fine[cloud], and every point's
//                       key = cx | cy << 21 | cz << 42 with c = floor(((double)x - (double)lo) / v): one subtraction, one IEEE
//                       division (never a reciprocal), one floor, all in double
//   batch_voxel_group   one wave per work item, one point per lane: the lane scans its cloud's keys in ascending j through LDS
//                       tiles of VOXEL_TILE keys and points.  The first j with its key is its cell's first point (first[i]); a lane
//                       that is that point itself goes on and adds the later members as they come, s += (double)x_j from s = 0.0 in
//                       ascending j -- the sequential sum of the rule -- and leaves (F)(s / (double)c), or its own bytes where it
//                       is alone, in cent.  The wave stops when every lane knows its cell and none leads one.
//   batch_voxel_rank    one block per cloud: an exclusive scan of the flags first[i] == i in chunks of VOXEL_SCAN_BLOCK (a wave scan
//                       by shuffles, the four waves' totals through LDS, a running carry) -> rank, count[cloud]; then
//                       map[i] = rank[first[i]]
//   batch_voxel_compact one wave per work item: a leading point's cent goes to the new batch's planes at dst_off + rank
// No atomics of any kind: every output element has one writer and every sum one order.  v == 0.0: the cloud is copied -- every
// point leads its own cell: no keys, no search, and rank and map are the point's own index (no scan).  A cloud of too_fine is skipped by the later kernels (the host refuses the call).
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_voxel_keys(const BatchVoxelArgs a)
{
    __shared__ F s_lo[VOXEL_SCAN_BLOCK / 64][3], s_hi[VOXEL_SCAN_BLOCK / 64][3];
    const int cloud = blockIdx.x;
    const double v = a.voxel[cloud];
    if (v == 0.0) {
        if (threadIdx.x == 0) a.too_fine[cloud] = 0;
        return;
    }
    const VoxelCloud c = a.clouds[cloud];
    const long long sp = a.src_plane[c.side];
    const F* S = static_cast<const F*>(a.src[c.side]) + c.src_off;
    F lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = S[k * sp];
    for (int i = threadIdx.x; i < c.n; i += VOXEL_SCAN_BLOCK)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const F x = S[k * sp + i];
            lo[k] = x < lo[k] ? x : lo[k];
            hi[k] = x > hi[k] ? x : hi[k];
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const F ol = __shfl_xor(lo[k], off, 64), oh = __shfl_xor(hi[k], off, 64);
            lo[k] = ol < lo[k] ? ol : lo[k];
            hi[k] = oh > hi[k] ? oh : hi[k];
        }
        if ((threadIdx.x & 63) == 0) {
            s_lo[threadIdx.x >> 6][k] = lo[k];
            s_hi[threadIdx.x >> 6][k] = hi[k];
        }
    }
    __syncthreads();
    bool bad = false;
    double dlo[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = s_lo[0][k];
        hi[k] = s_hi[0][k];
#pragma unroll
        for (int w = 1; w < VOXEL_SCAN_BLOCK / 64; ++w) {
            lo[k] = s_lo[w][k] < lo[k] ? s_lo[w][k] : lo[k];
            hi[k] = s_hi[w][k] > hi[k] ? s_hi[w][k] : hi[k];
        }
        dlo[k] = (double)lo[k];
        const double top = floor(((double)hi[k] - dlo[k]) / v);   // (the largest index of the axis: every step is monotonic)
        bad = bad || !(top <= (double)VOXEL_MAX_CELL);
    }
    if (threadIdx.x == 0) a.too_fine[cloud] = bad ? 1 : 0;
    if (bad) return;
    unsigned long long* keys = a.keys + c.tmp_off;
    for (int i = threadIdx.x; i < c.n; i += VOXEL_SCAN_BLOCK) {
        unsigned long long key = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double cell = floor(((double)S[k * sp + i] - dlo[k]) / v);
            key |= (unsigned long long)cell << (21 * k);
        }
        keys[i] = key;
    }
}

template <typename F>
__global__ __launch_bounds__(BATCH_ITEM) void batch_voxel_group(const BatchVoxelArgs a)
{
    __shared__ unsigned long long s_key[VOXEL_TILE];
    __shared__ F s_x[3][VOXEL_TILE];
    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const int lane = threadIdx.x;
    const bool active = lane < it.count;
    const int i = it.first + lane;
    const long long sp = a.src_plane[c.side];
    const F* S = static_cast<const F*>(a.src[c.side]) + c.src_off;
    F* cent = static_cast<F*>(a.cent) + c.tmp_off;
    int32_t* first_out = a.first + c.tmp_off;
    if (a.voxel[it.pair] == 0.0) {   // copied: the point's bytes, every point its own cell
        if (active) {
            first_out[i] = i;
#pragma unroll
            for (int k = 0; k < 3; ++k) cent[k * a.tmp_plane + i] = S[k * sp + i];
        }
        return;
    }
    if (a.too_fine[it.pair]) return;
    const unsigned long long* keys = a.keys + c.tmp_off;
    const unsigned long long mine = active ? keys[i] : ~0ull;   // (a key has 63 bits: no point's cell is all ones)
    int first = -1, members = 0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int base = 0; base < c.n; base += VOXEL_TILE) {
        const int len = min(VOXEL_TILE, c.n - base);
        __syncthreads();
        for (int j = lane; j < len; j += BATCH_ITEM) {
            s_key[j] = keys[base + j];
#pragma unroll
            for (int k = 0; k < 3; ++k) s_x[k][j] = S[k * sp + base + j];
        }
        __syncthreads();
        for (int j = 0; j < len; ++j) {
            if (s_key[j] == mine) {
                if (first < 0) first = base + j;
                if (first == i) {   // this lane leads the cell: its own point first, then the later members as they come
#pragma unroll
                    for (int k = 0; k < 3; ++k) s[k] += (double)s_x[k][j];
                    ++members;
                }
            }
        }
        if (__all(!active || (first >= 0 && first != i))) break;   // (the whole wave: no barrier is skipped by a part of it)
    }
    if (!active) return;
    first_out[i] = first;
    if (first != i) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        cent[k * a.tmp_plane + i] = members == 1 ? S[k * sp + i] : (F)(s[k] / (double)members);
}

__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_voxel_rank(const BatchVoxelArgs a)
{
    __shared__ int s_wave[VOXEL_SCAN_BLOCK / 64];
    const int cloud = blockIdx.x;
    if (a.too_fine[cloud]) {
        if (threadIdx.x == 0) a.count[cloud] = 0;
        return;
    }
    const VoxelCloud c = a.clouds[cloud];
    const int32_t* first = a.first + c.tmp_off;
    int32_t* rank = a.rank + c.tmp_off;
    int32_t* map = a.map + c.tmp_off;
    if (a.voxel[cloud] == 0.0) {   // copied: every point leads its own cell, in its place -- nothing to scan
        for (int i = threadIdx.x; i < c.n; i += VOXEL_SCAN_BLOCK) rank[i] = map[i] = i;
        if (threadIdx.x == 0) a.count[cloud] = c.n;
        return;
    }
    const int cells = block_rank_flags(c.n, s_wave, [&](int i) { return first[i] == i ? 1 : 0; }, [&](int i, int, int r) { rank[i] = r; });
    if (threadIdx.x == 0) a.count[cloud] = cells;
    for (int i = threadIdx.x; i < c.n; i += VOXEL_SCAN_BLOCK) map[i] = rank[first[i]];   // (the block's ranks are written: the scan ends on a barrier)
}

template <typename F>
__global__ __launch_bounds__(BATCH_ITEM) void batch_voxel_compact(const BatchVoxelArgs a)
{
    const BatchItem it = a.items[blockIdx.x];
    const int lane = threadIdx.x;
    if (lane >= it.count) return;
    const VoxelCloud c = a.clouds[it.pair];
    const int i = it.first + lane;
    if (a.first[c.tmp_off + i] != i) return;
    const F* cent = static_cast<const F*>(a.cent) + c.tmp_off;
    F* D = static_cast<F*>(a.dst[c.side]) + c.dst_off + a.rank[c.tmp_off + i];
    const long long dp = a.dst_plane[c.side];
#pragma unroll
    for (int k = 0; k < 3; ++k) D[k * dp] = cent[k * a.tmp_plane + i];
}

hipError_t launch_batch_voxel_group(const BatchVoxelArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0 || a.n_items <= 0) return hipSuccess;
    if (a.precision == ICP_F64) {
        hipLaunchKernelGGL((batch_voxel_keys<double>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
        hipLaunchKernelGGL((batch_voxel_group<double>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    } else {
        hipLaunchKernelGGL((batch_voxel_keys<float>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
        hipLaunchKernelGGL((batch_voxel_group<float>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    }
    hipLaunchKernelGGL(batch_voxel_rank, dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_voxel_compact(const BatchVoxelArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_voxel_compact<double>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    else hipLaunchKernelGGL((batch_voxel_compact<float>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// statistical and radius outlier removal of every cloud of a batch (icp_batch_remove_outliers, icp_batch.cpp; the rule is stated
// in include/icp_mi355x.h and every step here is one statement of it).  The clouds and work items are the voxel call's.
//   batch_outlier_scan    one block of NN_BLOCK threads per work item, one query per lane: phase 1's steps (icp_device_batch.h)
//                         in a loop of its own, because the two rules share it.  Places past a quarter's end hold +inf (a list)
//                         or NaN (a count): such a distance enters nothing.  The rule is uniform per block.  A statistical cloud
//                         keeps the list of the k smallest dist2<F> -- distances only -- as kth_distance does, and then
//                         dbar = (sum of sqrt((double)d), ascending, from 0.0) / (double)k.
//                         A radius cloud counts dist2 <= thr2 per wave, the query included (its distance is exactly 0), and
//                         wave 0 adds the four counts and takes the query out.  score[i] = dbar or (double)c; 0.0 where copied.
//   batch_outlier_decide  one block per cloud: granule sums (64 consecutive points from 0.0 in ascending index, one thread per
//                         granule), thread 0 adds them from 0.0 in ascending order: S, then Qsum the same way; mean, std, thr;
//                         the keep flags, their exclusive scan, map, count, stats.
//   batch_outlier_compact one wave per work item: a kept point's bytes go to the new batch's planes at dst_off + map
// No atomics of any kind; nothing is fused (contraction is off for this file), nothing multiplied by a reciprocal.
// ------------------------------------------------------------------------------------------------
template <typename F, int CAP>
__global__ __launch_bounds__(NN_BLOCK) void batch_outlier_scan(const BatchOutlierArgs a)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK;
    constexpr size_t TILE_BYTES = sizeof(F) * 4 * 3 * TW, LIST_BYTES = sizeof(F) * 3 * CAP * BATCH_ITEM;
    static_assert(CAP >= 1 && CAP <= OUTLIER_MAX_K, "the list's capacity");
    // the sub-tiles during the scan, the lists of waves 1-3 after it
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[TILE_BYTES > LIST_BYTES ? TILE_BYTES : LIST_BYTES];
    __shared__ int s_cnt[4][BATCH_ITEM];
    F(*sq)[3][TW] = reinterpret_cast<F(*)[3][TW]>(s_raw);

    const BatchItem it = a.items[blockIdx.x];
    const OutlierRule rule = a.rules[it.pair];
    const VoxelCloud c = a.clouds[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);   // (lanes past the item's end repeat its first point: nothing of theirs is kept)
    double* score = a.score + c.tmp_off;
    if (rule.kind == ICP_OUTLIER_NONE) {
        if (w == 0 && live) score[i] = 0.0;
        return;
    }
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const WaveQuarter q = wave_quarter<F>(c.n, w);
    const bool radius = rule.kind == ICP_OUTLIER_RADIUS;
    const F thr2 = (F)(rule.value * rule.value);      // (the radius rule's; the product in double, rounded once)
    const int k = rule.neighbours;
    // places past a quarter's end: NaN for a count (such a distance is NaN and compares false, whatever thr2), +inf for a list
    // (such a distance is +inf, never NaN, and enters no list)
    const F pad = radius ? nan_<F>() : inf_<F>();
    int cnt = 0;
    F bd[CAP];
    knn_list_init<F, CAP>(bd, k);

    for (int t = 0; t < q.ntile; ++t) {
        const int t0 = q.first + t * TW;
        __syncthreads();
        load_subtile<F, TW>(sq[w], Sx, Sy, Sz, t0, q.end, pad);
        __syncthreads();
        const int len = min(TW, q.end - t0);   // <= 0: this wave's quarter is exhausted
        for (int cc = 0; cc < len; cc += C) {
            F dd[C];
            chunk_dist2<F, TW>(sq[w], cc, px, py, pz, dd);
            if (radius) {
#pragma unroll
                for (int kk = 0; kk < C; ++kk) cnt += (dd[kk] <= thr2) ? 1 : 0;
                continue;
            }
            knn_chunk<F, CAP>(bd, dd, t0 + cc, it, i);
        }
    }
    if (radius) {
        s_cnt[w][lane] = cnt;
        __syncthreads();
        if (w == 0 && live) score[i] = (double)(s_cnt[0][lane] + s_cnt[1][lane] + s_cnt[2][lane] + s_cnt[3][lane] - 1);
        return;
    }
    knn_merge<F, CAP>(s_raw, bd, k);
    if (w != 0) return;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < CAP; ++r) {
        const double t = s + sqrt((double)bd[r]);
        s = (r >= CAP - k) ? t : s;
    }
    if (live) score[i] = s / (double)k;
}

__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_outlier_decide(const BatchOutlierArgs a)
{
    __shared__ double s_g[OUTLIER_MAX_GRANULES];
    __shared__ double s_val[2];
    __shared__ int s_wave[VOXEL_SCAN_BLOCK / 64];
    const int cloud = blockIdx.x;
    const OutlierRule rule = a.rules[cloud];
    const VoxelCloud c = a.clouds[cloud];
    const double* score = a.score + c.tmp_off;
    int32_t* map = a.map + c.tmp_off;
    double* stats = a.stats + 4 * (size_t)cloud;
    const int n = c.n;
    if (rule.kind == ICP_OUTLIER_NONE) {   // copied: every point kept, in its place -- nothing to scan
        for (int i = threadIdx.x; i < n; i += VOXEL_SCAN_BLOCK) map[i] = i;
        if (threadIdx.x == 0) {
            a.count[cloud] = n;
            a.bad[cloud] = 0;
            stats[0] = stats[1] = stats[2] = 0.0;
            stats[3] = (double)n;
        }
        return;
    }
    double mean = 0.0, sd = 0.0, thr;
    if (rule.kind == ICP_OUTLIER_RADIUS) {
        const double r2 = rule.value * rule.value;
        thr = a.precision == ICP_F64 ? r2 : (double)(float)r2;
    } else {
        const int ng = (n + BATCH_ITEM - 1) / BATCH_ITEM;   // <= OUTLIER_MAX_GRANULES
        for (int g = threadIdx.x; g < ng; g += VOXEL_SCAN_BLOCK) {
            const int i1 = min(n, (g + 1) * BATCH_ITEM);
            double s = 0.0;
            for (int i = g * BATCH_ITEM; i < i1; ++i) s += score[i];
            s_g[g] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double S = 0.0;
            for (int g = 0; g < ng; ++g) S += s_g[g];
            s_val[0] = S / (double)n;
        }
        __syncthreads();
        mean = s_val[0];
        for (int g = threadIdx.x; g < ng; g += VOXEL_SCAN_BLOCK) {
            const int i1 = min(n, (g + 1) * BATCH_ITEM);
            double q = 0.0;
            for (int i = g * BATCH_ITEM; i < i1; ++i) {
                const double dev = score[i] - mean;
                const double qi = dev * dev;
                q += qi;
            }
            s_g[g] = q;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double Qs = 0.0;
            for (int g = 0; g < ng; ++g) Qs += s_g[g];
            s_val[1] = sqrt(Qs / (double)(n - 1));
        }
        __syncthreads();
        sd = s_val[1];
        const double scaled = rule.value * sd;
        thr = mean + scaled;
        if (!(isfinite(mean) && isfinite(sd))) {   // (the whole block: the host refuses the call)
            if (threadIdx.x == 0) {
                a.count[cloud] = 0;
                a.bad[cloud] = 1;
                stats[0] = mean;
                stats[1] = sd;
                stats[2] = thr;
                stats[3] = 0.0;
            }
            return;
        }
    }
    const bool radius = rule.kind == ICP_OUTLIER_RADIUS;
    const double least = (double)rule.neighbours;
    const int carry = block_rank_flags(
        n, s_wave,
        [&](int i) {
            const double sc = score[i];
            return (radius ? sc >= least : sc <= thr) ? 1 : 0;
        },
        [&](int i, int flag, int rank) { map[i] = flag ? rank : -1; });
    if (threadIdx.x == 0) {
        a.count[cloud] = carry;
        a.bad[cloud] = 0;
        stats[0] = mean;
        stats[1] = sd;
        stats[2] = thr;
        stats[3] = (double)carry;
    }
}

template <typename F>
__global__ __launch_bounds__(BATCH_ITEM) void batch_outlier_compact(const BatchOutlierArgs a)
{
    const BatchItem it = a.items[blockIdx.x];
    const int lane = threadIdx.x;
    if (lane >= it.count) return;
    const VoxelCloud c = a.clouds[it.pair];
    const int i = it.first + lane;
    const int32_t to = a.map[c.tmp_off + i];
    if (to < 0) return;
    copy_kept_point<F>(static_cast<const F*>(a.src[c.side]) + c.src_off + i, a.src_plane[c.side], static_cast<F*>(a.dst[c.side]) + c.dst_off + to,
                       a.dst_plane[c.side]);
}

hipError_t launch_batch_outlier_scan(const BatchOutlierArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0 || a.n_items <= 0) return hipSuccess;
    if (a.cap != 8 && a.cap != 16 && a.cap != 32) return hipErrorInvalidValue;
#define ICP_OUTLIER_SCAN(F, CAP) hipLaunchKernelGGL((batch_outlier_scan<F, CAP>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a)
    if (a.precision == ICP_F64) {
        if (a.cap == 8) ICP_OUTLIER_SCAN(double, 8);
        else if (a.cap == 16) ICP_OUTLIER_SCAN(double, 16);
        else ICP_OUTLIER_SCAN(double, 32);
    } else {
        if (a.cap == 8) ICP_OUTLIER_SCAN(float, 8);
        else if (a.cap == 16) ICP_OUTLIER_SCAN(float, 16);
        else ICP_OUTLIER_SCAN(float, 32);
    }
#undef ICP_OUTLIER_SCAN
    hipLaunchKernelGGL(batch_outlier_decide, dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_outlier_compact(const BatchOutlierArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_outlier_compact<double>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    else hipLaunchKernelGGL((batch_outlier_compact<float>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    return hipGetLastError();
}

}  // namespace icp
