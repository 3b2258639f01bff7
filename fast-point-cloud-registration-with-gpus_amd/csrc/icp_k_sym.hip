// icp_k_sym.hip -- gfx950 kernel of the symmetric metric of batched ICP (icp_batch.cpp; Rusinkiewicz, SIGGRAPH 2019): the decision and
// the terms of a symmetric step (batch_sym_moments, batch_color_moments' sibling on the deferred route).  The rule is stated in
// include/icp_mi355x.h and restated in numpy (tests/batch_sym_ref.py); every step here is one statement of it.  The kept decision is
// icp_device_batch.h's.  Contraction is off for this file: nothing is fused.
#include "icp_device_batch.h"

namespace icp {

// ------------------------------------------------------------------------------------------------
// the symmetric step (icp_batch_begin with ICP_SYMMETRIC): the decision and the terms of every kept match -- batch_color_moments'
// place on the deferred route, over the same items and in its block shape (wave 0 alone carries data, waves 1-3 add zeros,
// block_sum_store adds a row in the fused pass's order).
//   kept: batch_kept.  A rejected point's idx entry gets BATCH_IDX_REJECTED.
//   terms, in double from the widened coordinates p (the moved point) and q = Q[idx], the stored point normal m0 of the moving
//     point (the frame of the cloud as uploaded), the stored point normal nq of model point idx and Rc = rot[pair]:
//     np_a = Rc[a] . m0; s = np . nq; n_a = s < 0 ? nq_a - np_a : nq_a + np_a; e = p - q, g = p + q, h = e . n; v = (g x n, n);
//     C(a, c) += v_a v_c (a <= c), B(a) -= v_a h, CNT = 1.  Every dot product is dot3.  A kept match whose n is exactly zero
//     counts and adds zeros.
// The block writes slots 1 .. ICP_MOM_B + 5 of its row and leaves ICP_MOM_ERR, the matching launch's.  A pair that takes part in the
// step without matching (the loop's error-only last pass) gets zeros throughout.  No LDS beyond block_sum_store's.
// ------------------------------------------------------------------------------------------------
template <typename F, bool MUTUAL>
__global__ __launch_bounds__(NN_BLOCK) void batch_sym_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                              const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                              const F* __restrict__ Q, long long q_plane, int32_t* __restrict__ idx_cur,
                                                              const F* __restrict__ dist, const F* __restrict__ tau,
                                                              const F* __restrict__ thr, const double* __restrict__ nrm_p,
                                                              const double* __restrict__ nrm_q, const double* __restrict__ rot,
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
        const bool kept = batch_kept<F, MUTUAL>(dist[gi], it.pair, tau, thr, recip, rev, pr.q_off + j, it.first + lane);
        if (kept) {
            const long long gj = pr.q_off + j;
            const double px = (double)P[gi], py = (double)P[p_plane + gi], pz = (double)P[2 * p_plane + gi];
            const double qx = (double)Q[gj], qy = (double)Q[q_plane + gj], qz = (double)Q[2 * q_plane + gj];
            const double mx = nrm_p[gi], my = nrm_p[p_plane + gi], mz = nrm_p[2 * p_plane + gi];
            const double ux = nrm_q[gj], uy = nrm_q[q_plane + gj], uz = nrm_q[2 * q_plane + gj];
            const double* Rc = rot + (size_t)it.pair * 9;
            const double ax = dot3(Rc[0], Rc[1], Rc[2], mx, my, mz);
            const double ay = dot3(Rc[3], Rc[4], Rc[5], mx, my, mz);
            const double az = dot3(Rc[6], Rc[7], Rc[8], mx, my, mz);
            const bool flip = dot3(ax, ay, az, ux, uy, uz) < 0.0;   // (the two normals point into opposite half spaces: their difference)
            const double nx = flip ? ux - ax : ux + ax, ny = flip ? uy - ay : uy + ay, nz = flip ? uz - az : uz + az;
            const double ex = px - qx, ey = py - qy, ez = pz - qz;
            const double gx = px + qx, gy = py + qy, gz = pz + qz;
            const double h = dot3(ex, ey, ez, nx, ny, nz);
            double v[6];
            v[0] = gy * nz - gz * ny;
            v[1] = gz * nx - gx * nz;
            v[2] = gx * ny - gy * nx;
            v[3] = nx; v[4] = ny; v[5] = nz;
            acc[ICP_MOM_CNT] = 1.0;
            int o = ICP_MOM_C;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[o++] += v[r] * v[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[ICP_MOM_B + r] -= v[r] * h;
        }
        if (!kept) idx_cur[gi] = j | BATCH_IDX_REJECTED;   // (a rejected point adds nothing: every accumulator stays 0, the count included)
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}

hipError_t launch_batch_sym_moments(const BatchPassArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    if (!a.nrm_p || !a.nrm_q || !a.rot || !a.dist) return hipErrorInvalidValue;
    if (a.recip && !a.rev) return hipErrorInvalidValue;
#define ICP_LAUNCH_SYM(F, MUT)                                                                                                     \
    hipLaunchKernelGGL((batch_sym_moments<F, MUT>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,              \
                       (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, a.q_plane, a.idx_cur, (const F*)a.dist,                    \
                       a.trim_rank ? (const F*)a.tau : (const F*)nullptr, (const F*)a.thr, a.nrm_p, a.nrm_q, a.rot, a.partials,    \
                       (const int32_t*)a.rev, a.recip)
    if (a.precision == ICP_F64) {
        if (a.recip) ICP_LAUNCH_SYM(double, true); else ICP_LAUNCH_SYM(double, false);
    } else {
        if (a.recip) ICP_LAUNCH_SYM(float, true); else ICP_LAUNCH_SYM(float, false);
    }
#undef ICP_LAUNCH_SYM
    return hipGetLastError();
}

}  // namespace icp
