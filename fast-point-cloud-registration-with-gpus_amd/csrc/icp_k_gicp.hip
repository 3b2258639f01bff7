// icp_k_gicp.hip -- gfx950 kernels of the generalized (plane-to-plane) metric of batched ICP (icp_batch.cpp): the per-point
// covariances of every cloud of a batch (batch_cov_kernel) and the decision and the terms of a generalized step
// (batch_gicp_moments, batch_robust_moments' sibling on the deferred route).  The rules are stated in include/icp_mi355x.h and
// restated in numpy (tests/batch_gicp_ref.py); every step here is one statement of them.  The scan, the walk, the sums and the
// kept decision are icp_device_batch.h's.  Contraction is off for this file: nothing is fused.
#include "icp_device_batch.h"

namespace icp {

// ------------------------------------------------------------------------------------------------
// per-point covariances (icp_batch_estimate_covariances): one block of NN_BLOCK threads per work item, one query per lane.
//   phase 1  tau_i = kth_distance over the query's own cloud.
//   phase 2  walk_tiles, 4 * TW points per tile, wave 0: a point with d2(i, j) <= tau_i -- the query itself included, at distance
//            0 -- goes into the NeighbourSums of its lane, in ascending j.
//   then     C = (S - s s^T / c) / c, the regularisation, and six stores into the cloud's covariance planes.
// The k of the block's cloud is uniform; the result depends on the cloud, its k and the two parameters alone -- not on CAP, which
// is the launch's (the largest k's capacity), nor on the other clouds.  No atomics.
// LDS: 4 x 3 x TW x sizeof(F) = 24 KiB of tiles, reused for the three lists (3 x CAP x 64 x sizeof(F) <= 48 KiB for CAP 32, fp64).
// ------------------------------------------------------------------------------------------------
template <typename F, int CAP>
__global__ __launch_bounds__(NN_BLOCK) void batch_cov_kernel(const BatchCovArgs a)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK, T2 = 4 * TW;
    constexpr size_t TILE_BYTES = sizeof(F) * 4 * 3 * TW, LIST_BYTES = sizeof(F) * 3 * CAP * BATCH_ITEM;
    static_assert(CAP >= 1 && CAP <= COV_MAX_K, "the list's capacity");
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[TILE_BYTES > LIST_BYTES ? TILE_BYTES : LIST_BYTES];

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

    const F tau = kth_distance<F, CAP>(s_raw, Sx, Sy, Sz, c.n, k, it, i, px, py, pz);

    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    NeighbourSums sums;
    walk_tiles<F, T2>(
        reinterpret_cast<F(*)[T2]>(s_raw), Sx, Sy, Sz, c.n, px, py, pz, [&](F d, int) { return d <= tau; },
        [&](int, const bool(&in)[C], const F(&qq)[3][C]) {
#pragma unroll
            for (int kk = 0; kk < C; ++kk)
                if (in[kk]) sums.add((double)qq[0][kk] - xi, (double)qq[1][kk] - yi, (double)qq[2][kk] - zi);
        });
    if (w != 0 || !live) return;
    double xx, xy, xz, yy, yz, zz;
    sums.covariance(xx, xy, xz, yy, yz, zz);   // (the count is >= k + 1)
    if (a.regularisation == ICP_COV_FROBENIUS) {
        (void)range_scale6(xx, xy, xz, yy, yz, zz);   // the squares below stay in range; the quotients are scale-free
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
//   kept: batch_kept, and det finite and > 0.  A rejected point's idx entry gets BATCH_IDX_REJECTED.
//   terms, in double from the widened coordinates p (the moved point), q = Q[idx] and the covariances Cp (of point i, in the frame of
//     the cloud as uploaded) and Cq (of model point idx), with Rc = rot[pair], the rotation that carries that frame into the pass's:
//     Tm = Rc Cp, B = Tm Rc^T, S = Cq + B, M = adj(S) / det(S); u_a = M j_a for the six columns j_a of J = [-[p]x | I];
//     C(a, c) += j_a . u_c (a <= c), B(a) -= u_a . (p - q), CNT = 1.  Every dot product is dot3; with M = n n^T these are the plane
//     pass's statements.
// The block writes slots 1 .. ICP_MOM_B + 5 of its row and leaves ICP_MOM_ERR, the matching launch's.  A pair that takes part in the
// step without matching (the loop's error-only last pass) gets zeros throughout.  No LDS beyond block_sum_store's.
// ------------------------------------------------------------------------------------------------
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
        const int j = idx_cur[gi];   // in [0, m): the matching launch wrote it
        bool kept = batch_kept<F, MUTUAL>(dist[gi], it.pair, tau, thr, recip, rev, pr.q_off + j, it.first + lane);
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
                Tm[r][0] = dot3(r0, r1, r2, pxx, pxy, pxz);
                Tm[r][1] = dot3(r0, r1, r2, pxy, pyy, pyz);
                Tm[r][2] = dot3(r0, r1, r2, pxz, pyz, pzz);
            }
            // S = Cq + Tm Rc^T, the upper triangle
            const double S00 = cq[0] + dot3(Tm[0][0], Tm[0][1], Tm[0][2], R[0], R[1], R[2]);
            const double S01 = cq[q_plane] + dot3(Tm[0][0], Tm[0][1], Tm[0][2], R[3], R[4], R[5]);
            const double S02 = cq[2 * q_plane] + dot3(Tm[0][0], Tm[0][1], Tm[0][2], R[6], R[7], R[8]);
            const double S11 = cq[3 * q_plane] + dot3(Tm[1][0], Tm[1][1], Tm[1][2], R[3], R[4], R[5]);
            const double S12 = cq[4 * q_plane] + dot3(Tm[1][0], Tm[1][1], Tm[1][2], R[6], R[7], R[8]);
            const double S22 = cq[5 * q_plane] + dot3(Tm[2][0], Tm[2][1], Tm[2][2], R[6], R[7], R[8]);
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
                    for (int r = 0; r < 3; ++r) u[c][r] = dot3(M[r][0], M[r][1], M[r][2], J[c][0], J[c][1], J[c][2]);
                acc[ICP_MOM_CNT] = 1.0;
                int o = ICP_MOM_C;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) acc[o++] += dot3(J[r][0], J[r][1], J[r][2], u[c][0], u[c][1], u[c][2]);
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[ICP_MOM_B + r] -= dot3(u[r][0], u[r][1], u[r][2], ex, ey, ez);
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
