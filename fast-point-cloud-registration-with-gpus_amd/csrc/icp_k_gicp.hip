// icp_k_gicp.hip -- gfx950 kernels of the generalized (plane-to-plane) metric of batched ICP (icp_batch.cpp): the per-point
// covariances of every cloud of a batch (batch_cov_kernel) and the decision and the terms of a generalized step
// (batch_gicp_moments, batch_robust_moments' sibling on the deferred route).  The rules are stated in include/icp_mi355x.h and
// restated in numpy (tests/batch_gicp_ref.py); every step here is one statement of them.  The kernels of icp_k_batch.hip keep
// their listings: what this file needs of them -- the statistical list of batch_outlier_scan, the kept decision of
// batch_trim_moments -- is restated, not shared.  Contraction is off for this file: nothing is fused.
#include "icp_device.h"
#include <math.h>

namespace icp {

template <typename F> struct GicpCfg;
template <> struct GicpCfg<float> { static constexpr int TW = 512; };    // points per wave and sub-tile (BatchCfg's: 6 KiB per wave)
template <> struct GicpCfg<double> { static constexpr int TW = 256; };
constexpr int COV_CHUNK = 8;   // points per early-out chunk

// batch_outlier_scan's list, restated: d into the ascending list bd[0 .. CAP-1], the largest entry falling off -- bd[r] =
// median(bd[r-1], d, bd[r]) from the top slot down.  Selections only; equal values change nothing of the multiset.
__device__ __forceinline__ float cov_med3(float lo, float d, float hi) { return __builtin_amdgcn_fmed3f(lo, d, hi); }
__device__ __forceinline__ double cov_med3(double lo, double d, double hi) { return __builtin_fmin(hi, __builtin_fmax(lo, d)); }
template <typename F, int CAP>
__device__ __forceinline__ void cov_insert(F (&bd)[CAP], F d)
{
#pragma unroll
    for (int r = CAP - 1; r >= 1; --r) bd[r] = cov_med3(bd[r - 1], d, bd[r]);
    bd[0] = fmin_(bd[0], d);
}

template <typename F> __device__ __forceinline__ F cov_nan();
template <> __device__ __forceinline__ float cov_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double cov_nan<double>() { return __builtin_nan(""); }

// ------------------------------------------------------------------------------------------------
// per-point covariances (icp_batch_estimate_covariances): one block of NN_BLOCK threads per work item, one query per lane.
//   phase 1  tau_i = the k-th smallest d2(i, j) over j != i by index: batch_outlier_scan's statistical list.  The four waves stream
//            the four contiguous quarters of the query's own cloud through their LDS sub-tiles (every lane reads the same address:
//            a broadcast), each keeping the k smallest distances ascending in the TOP k of CAP registers (the slots below hold -inf,
//            which nothing displaces: bd[CAP - 1] is the k-th smallest at a compile-time index); waves 1-3 leave their lists in LDS
//            and wave 0 inserts them into its own -- a multiset has one order.  Places past a quarter's end hold +inf.
//   phase 2  the block loads the cloud again, 4 * TW points per tile, and wave 0 walks every tile in ascending j: a point with
//            d2(i, j) <= tau_i -- the query itself included, at distance 0 -- adds e = x_j - x_i (in double) to s and e e^T to S.  One
//            lane, one query, one running sum: the order of the additions is ascending j whatever the cloud.  A chunk in which no
//            lane's test passes is skipped (wave-uniform).  Places past the cloud's end hold NaN: such a distance passes no test.
//   then     C = (S - s s^T / c) / c, the regularisation, and six stores into the cloud's covariance planes.
// The k of the block's cloud is uniform; the result depends on the cloud, its k and the two parameters alone -- not on CAP, which
// is the launch's (the largest k's capacity), nor on the other clouds.  No atomics.
// LDS: 4 x 3 x TW x sizeof(F) = 24 KiB of tiles, reused for the three lists (3 x CAP x 64 x sizeof(F) <= 48 KiB for CAP 32, fp64).
// ------------------------------------------------------------------------------------------------
template <typename F, int CAP>
__global__ __launch_bounds__(NN_BLOCK) void batch_cov_kernel(const BatchCovArgs a)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = GicpCfg<F>::TW, C = COV_CHUNK, T2 = 4 * TW;
    constexpr size_t TILE_BYTES = sizeof(F) * 4 * 3 * TW, LIST_BYTES = sizeof(F) * 3 * CAP * BATCH_ITEM;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM && TW % C == 0 && C % VN == 0, "one query per lane, four waves per item");
    static_assert(CAP >= 1 && CAP <= COV_MAX_K, "the list's capacity");
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[TILE_BYTES > LIST_BYTES ? TILE_BYTES : LIST_BYTES];
    F(*sq)[3][TW] = reinterpret_cast<F(*)[3][TW]>(s_raw);                    // phase 1: a sub-tile per wave
    F(*ld)[CAP][BATCH_ITEM] = reinterpret_cast<F(*)[CAP][BATCH_ITEM]>(s_raw);  // ... then the lists of waves 1-3
    F(*st)[T2] = reinterpret_cast<F(*)[T2]>(s_raw);                          // phase 2: one tile of the block

    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const int k = a.k[it.pair];   // in [ICP_COV_MIN_NEIGHBOURS, CAP], and the cloud holds at least k + 1 points (the host checked)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);   // (lanes past the item's end repeat its first point: nothing of theirs is kept)
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const int n = c.n;

    // ---- phase 1: the k-th smallest distance
    const int wseg = ((n + 3) / 4 + C - 1) / C * C;   // points per wave, whole chunks
    const int my0 = w * wseg, my1 = min(my0 + wseg, n);  // may be empty (my1 <= my0)
    const int ntile = (wseg + TW - 1) / TW;           // the same for every wave: the barriers pair up
    F bd[CAP];
#pragma unroll
    for (int r = 0; r < CAP; ++r) bd[r] = (r >= CAP - k) ? inf_<F>() : -inf_<F>();
    for (int t = 0; t < ntile; ++t) {
        const int t0 = my0 + t * TW;
        __syncthreads();
        for (int e = lane; e < TW; e += 64) {
            const int j = t0 + e;
            F qx = inf_<F>(), qy = inf_<F>(), qz = inf_<F>();
            if (j < my1) { qx = Sx[j]; qy = Sy[j]; qz = Sz[j]; }
            sq[w][0][e] = qx;
            sq[w][1][e] = qy;
            sq[w][2][e] = qz;
        }
        __syncthreads();
        const int len = min(TW, my1 - t0);   // <= 0: this wave's quarter is exhausted
        for (int cc = 0; cc < len; cc += C) {
            F dd[C];
#pragma unroll
            for (int kk = 0; kk < C; kk += VN) {
                const V qx = *reinterpret_cast<const V*>(&sq[w][0][cc + kk]);
                const V qy = *reinterpret_cast<const V*>(&sq[w][1][cc + kk]);
                const V qz = *reinterpret_cast<const V*>(&sq[w][2][cc + kk]);
#pragma unroll
                for (int v = 0; v < VN; ++v) dd[kk + v] = dist2<F>(px, py, pz, vget(qx, v), vget(qy, v), vget(qz, v));
            }
            const int j0 = t0 + cc;
            if (j0 + C > it.first && j0 < it.first + BATCH_ITEM) {   // (wave-uniform) the chunk holds queries of this item: j != i
#pragma unroll
                for (int kk = 0; kk < C; ++kk) dd[kk] = (j0 + kk == i) ? inf_<F>() : dd[kk];
            }
            F cmin = inf_<F>();
#pragma unroll
            for (int kk = 0; kk < C; ++kk) cmin = fmin_(cmin, dd[kk]);
            if (__builtin_amdgcn_ballot_w64(cmin < bd[CAP - 1]) == 0ull) continue;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) cov_insert<F, CAP>(bd, dd[kk]);
        }
    }
    __syncthreads();   // every wave has read its last sub-tile: the lists go over them
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < CAP; ++r) ld[w - 1][r][lane] = bd[r];
    }
    __syncthreads();
    F tau = inf_<F>();
    if (w == 0) {
        for (int ww = 0; ww < 3; ++ww) {
#pragma unroll 1
            for (int s = CAP - k; s < CAP; ++s) {
                const F d = ld[ww][s][lane];
                if (__builtin_amdgcn_ballot_w64(d < bd[CAP - 1]) == 0ull) break;   // (ascending lists: no later entry of this wave's enters any lane's)
                cov_insert<F, CAP>(bd, d);
            }
        }
        tau = bd[CAP - 1];
    }

    // ---- phase 2: the sums over the neighbourhood, ascending j, wave 0
    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, Sxx = 0.0, Sxy = 0.0, Sxz = 0.0, Syy = 0.0, Syz = 0.0, Szz = 0.0;
    int cnt = 0;
    const int ntile2 = (n + T2 - 1) / T2;
    for (int t = 0; t < ntile2; ++t) {
        const int t0 = t * T2;
        __syncthreads();   // (the first: wave 0 has read the lists)
        for (int e = threadIdx.x; e < T2; e += NN_BLOCK) {
            const int j = t0 + e;
            F qx = cov_nan<F>(), qy = cov_nan<F>(), qz = cov_nan<F>();
            if (j < n) { qx = Sx[j]; qy = Sy[j]; qz = Sz[j]; }
            st[0][e] = qx;
            st[1][e] = qy;
            st[2][e] = qz;
        }
        __syncthreads();
        if (w != 0) continue;
        const int len = min(T2, n - t0);
        for (int cc = 0; cc < len; cc += C) {
            F qq[3][C];
            bool in[C];
            bool any = false;
#pragma unroll
            for (int kk = 0; kk < C; kk += VN) {
                const V qx = *reinterpret_cast<const V*>(&st[0][cc + kk]);
                const V qy = *reinterpret_cast<const V*>(&st[1][cc + kk]);
                const V qz = *reinterpret_cast<const V*>(&st[2][cc + kk]);
#pragma unroll
                for (int v = 0; v < VN; ++v) {
                    qq[0][kk + v] = vget(qx, v);
                    qq[1][kk + v] = vget(qy, v);
                    qq[2][kk + v] = vget(qz, v);
                    in[kk + v] = dist2<F>(px, py, pz, qq[0][kk + v], qq[1][kk + v], qq[2][kk + v]) <= tau;   // (NaN: false)
                    any = any || in[kk + v];
                }
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) {
                if (in[kk]) {
                    const double ex = (double)qq[0][kk] - xi, ey = (double)qq[1][kk] - yi, ez = (double)qq[2][kk] - zi;
                    s0 += ex; s1 += ey; s2 += ez;
                    Sxx += ex * ex; Sxy += ex * ey; Sxz += ex * ez;
                    Syy += ey * ey; Syz += ey * ez; Szz += ez * ez;
                    cnt += 1;
                }
            }
        }
    }
    if (w != 0 || !live) return;
    const double dc = (double)cnt;   // >= k + 1
    double xx = (Sxx - (s0 * s0) / dc) / dc, xy = (Sxy - (s0 * s1) / dc) / dc, xz = (Sxz - (s0 * s2) / dc) / dc;
    double yy = (Syy - (s1 * s1) / dc) / dc, yz = (Syz - (s1 * s2) / dc) / dc, zz = (Szz - (s2 * s2) / dc) / dc;
    if (a.regularisation == ICP_COV_FROBENIUS) {
        const double f = sqrt(((xx * xx + yy * yy) + zz * zz) + 2.0 * ((xy * xy + xz * xz) + yz * yz));
        const double lam = a.lambda;
        if (f > 0.0) {
            xx = xx / f + lam; xy = xy / f; xz = xz / f;
            yy = yy / f + lam; yz = yz / f; zz = zz / f + lam;
        } else {
            xx = lam; xy = 0.0; xz = 0.0;
            yy = lam; yz = 0.0; zz = lam;
        }
    }
    double* cv = a.cov[c.side] + c.src_off + i;   // the planes are laid out as the cloud's
    cv[0] = xx; cv[sp] = xy; cv[2 * sp] = xz; cv[3 * sp] = yy; cv[4 * sp] = yz; cv[5 * sp] = zz;
}

hipError_t launch_batch_covariances(const BatchCovArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    if (!a.clouds || !a.items || !a.k) return hipErrorInvalidValue;
#define ICP_COV_LAUNCH(F, CAP) hipLaunchKernelGGL((batch_cov_kernel<F, CAP>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a)
#define ICP_COV_LAUNCH_F(F)                          \
    do {                                             \
        if (a.cap <= 8) ICP_COV_LAUNCH(F, 8);        \
        else if (a.cap <= 16) ICP_COV_LAUNCH(F, 16); \
        else ICP_COV_LAUNCH(F, 32);                  \
    } while (0)
    if (a.precision == ICP_F64) ICP_COV_LAUNCH_F(double); else ICP_COV_LAUNCH_F(float);
#undef ICP_COV_LAUNCH_F
#undef ICP_COV_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// the generalized step (icp_batch_begin with ICP_GENERALIZED): the decision and the terms of every kept match --
// batch_robust_moments' place on the deferred route, over the same items and in its block shape (wave 0 alone carries data, waves
// 1-3 add zeros, block_sum_store adds a row in the fused pass's order).
//   kept: batch_trim_moments' tests, restated -- (tau == NULL || d <= tau[pair]) && (thr == NULL || d <= thr[pair]), and with MUTUAL
//     (its own instantiations: the others never read rev or recip) && (recip[pair] == 0 || rev[idx[i]] == i) -- and det finite and
//     > 0.  A rejected point's idx entry gets BATCH_IDX_REJECTED.
//   terms, in double from the widened coordinates p (the moved point), q = Q[idx] and the covariances Cp (of point i, in the frame of
//     the cloud as uploaded) and Cq (of model point idx), with Rc = rot[pair], the rotation that carries that frame into the pass's:
//     Tm = Rc Cp, B = Tm Rc^T, S = Cq + B, M = adj(S) / det(S); u_a = M j_a for the six columns j_a of J = [-[p]x | I];
//     C(a, c) += j_a . u_c (a <= c), B(a) -= u_a . (p - q), CNT = 1.  Every dot product is (x*x' + y*y') + z*z', each operation
//     rounded on its own; with M = n n^T these are the plane pass's statements.
// The block writes slots 1 .. ICP_MOM_B + 5 of its row and leaves ICP_MOM_ERR, the matching launch's.  A pair that takes part in the
// step without matching (the loop's error-only last pass) gets zeros throughout.  No LDS beyond block_sum_store's.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gdot(double x, double y, double z, double a, double b, double c) { return (x * a + y * b) + z * c; }

template <typename F, bool MUTUAL>
__global__ __launch_bounds__(NN_BLOCK) void batch_gicp_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                               const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                               const F* __restrict__ Q, long long q_plane, int32_t* __restrict__ idx_cur,
                                                               const F* __restrict__ dist, const F* __restrict__ tau,
                                                               const F* __restrict__ thr, const double* __restrict__ cov_p,
                                                               const double* __restrict__ cov_q, const double* __restrict__ rot,
                                                               double* __restrict__ partials, const int32_t* __restrict__ rev,
                                                               const uint8_t* __restrict__ recip)
{
    constexpr int NACC = ICP_MOM_B + 6;
    static_assert(ICP_MOM_ERR == 0 && ICP_MOM_C == 2 && ICP_MOM_B == ICP_MOM_C + 21 && NACC <= ICP_NMOM, "a plane pass's slots");
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
        const F b = dist[gi];
        const int j = idx_cur[gi];   // in [0, m): the matching launch wrote it
        bool kept = (tau == nullptr || b <= tau[it.pair]) && (thr == nullptr || b <= thr[it.pair]);
        if constexpr (MUTUAL) kept = kept && (recip[it.pair] == 0 || rev[pr.q_off + j] == it.first + lane);
        if (kept) {
            const double* R = rot + 9 * (size_t)it.pair;
            const double* cp = cov_p + gi;
            const double* cq = cov_q + pr.q_off + j;
            const double pxx = cp[0], pxy = cp[p_plane], pxz = cp[2 * p_plane], pyy = cp[3 * p_plane], pyz = cp[4 * p_plane], pzz = cp[5 * p_plane];
            // Tm = Rc Cp, the full 3 x 3: row a of Rc against the columns of the symmetric Cp
            double Tm[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double r0 = R[3 * r], r1 = R[3 * r + 1], r2 = R[3 * r + 2];
                Tm[r][0] = gdot(r0, r1, r2, pxx, pxy, pxz);
                Tm[r][1] = gdot(r0, r1, r2, pxy, pyy, pyz);
                Tm[r][2] = gdot(r0, r1, r2, pxz, pyz, pzz);
            }
            // S = Cq + Tm Rc^T, the upper triangle
            const double S00 = cq[0] + gdot(Tm[0][0], Tm[0][1], Tm[0][2], R[0], R[1], R[2]);
            const double S01 = cq[q_plane] + gdot(Tm[0][0], Tm[0][1], Tm[0][2], R[3], R[4], R[5]);
            const double S02 = cq[2 * q_plane] + gdot(Tm[0][0], Tm[0][1], Tm[0][2], R[6], R[7], R[8]);
            const double S11 = cq[3 * q_plane] + gdot(Tm[1][0], Tm[1][1], Tm[1][2], R[3], R[4], R[5]);
            const double S12 = cq[4 * q_plane] + gdot(Tm[1][0], Tm[1][1], Tm[1][2], R[6], R[7], R[8]);
            const double S22 = cq[5 * q_plane] + gdot(Tm[2][0], Tm[2][1], Tm[2][2], R[6], R[7], R[8]);
            const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
            const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
            const double det = (S00 * c00 + S01 * c01) + S02 * c02;
            kept = det > 0.0 && det < __builtin_huge_val();   // (NaN fails both)
            if (kept) {
                const F* Qx = Q + pr.q_off;
                const double px = (double)P[gi], py = (double)P[p_plane + gi], pz = (double)P[2 * p_plane + gi];
                const double ex = px - (double)Qx[j], ey = py - (double)Qx[q_plane + j], ez = pz - (double)Qx[2 * q_plane + j];
                const double M[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
                const double J[6][3] = {{0.0, -pz, py}, {pz, 0.0, -px}, {-py, px, 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
                double u[6][3];
#pragma unroll
                for (int c = 0; c < 6; ++c)
#pragma unroll
                    for (int r = 0; r < 3; ++r) u[c][r] = gdot(M[r][0], M[r][1], M[r][2], J[c][0], J[c][1], J[c][2]);
                acc[ICP_MOM_CNT] = 1.0;
                int o = ICP_MOM_C;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) acc[o++] += gdot(J[r][0], J[r][1], J[r][2], u[c][0], u[c][1], u[c][2]);
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[ICP_MOM_B + r] -= gdot(u[r][0], u[r][1], u[r][2], ex, ey, ez);
            }
        }
        if (!kept) idx_cur[gi] = j | BATCH_IDX_REJECTED;   // (a rejected point adds nothing: every accumulator stays 0, the count included)
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}

hipError_t launch_batch_gicp_moments(const BatchPassArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    if (!a.cov_p || !a.cov_q || !a.rot || !a.dist) return hipErrorInvalidValue;
    if (a.recip && !a.rev) return hipErrorInvalidValue;
#define ICP_LAUNCH_GICP(F, MUT)                                                                                                  \
    hipLaunchKernelGGL((batch_gicp_moments<F, MUT>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,            \
                       (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, a.q_plane, a.idx_cur, (const F*)a.dist,                   \
                       a.trim_rank ? (const F*)a.tau : (const F*)nullptr, (const F*)a.thr, a.cov_p, a.cov_q, a.rot, a.partials,   \
                       (const int32_t*)a.rev, a.recip)
    if (a.precision == ICP_F64) {
        if (a.recip) ICP_LAUNCH_GICP(double, true); else ICP_LAUNCH_GICP(double, false);
    } else {
        if (a.recip) ICP_LAUNCH_GICP(float, true); else ICP_LAUNCH_GICP(float, false);
    }
#undef ICP_LAUNCH_GICP
    return hipGetLastError();
}

}  // namespace icp
