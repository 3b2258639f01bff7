// icp_k_color.hip -- gfx950 kernels of the colored metric of batched ICP (icp_batch.cpp; Park, Zhou, Koltun, ICCV 2017): the
// per-point intensity gradients of every model of a batch (batch_intensity_gradient_kernel) and the decision and the terms of a
// colored step (batch_color_moments, batch_gicp_moments' sibling on the deferred route).  The rules are stated in
// include/icp_mi355x.h and restated in numpy (tests/batch_color_ref.py); every step here is one statement of them.  The scan, the
// walk and the kept decision are icp_device_batch.h's.  Contraction is off for this file: nothing is fused.
#include "icp_device_batch.h"

namespace icp {

// ------------------------------------------------------------------------------------------------
// per-point intensity gradients (icp_batch_estimate_intensity_gradients): one block of NN_BLOCK threads per work item of a model,
// one query per lane -- batch_cov_kernel's shape.
//   phase 1  tau_i = kth_distance over the query's own model.
//   phase 2  walk_tiles, 4 * TW points per tile and their intensities beside them (a fourth LDS plane of doubles: the neighbour's
//            intensity comes from the tile, as its coordinates do), wave 0: a point j != i with d2(i, j) <= tau_i adds u u^T to A
//            and u g to r, u the part of e = q_j - q_i across the normal of i, g = I_j - I_i -- nine running sums per lane,
//            ascending j by construction.
//   then     A += c^2 n n^T (the gradient has no part along the normal), d = A^-1 r by cofactors, (0, 0, 0) where det is not finite
//            and > 0 or a component is not finite, and three stores into the model's gradient planes.
// The k of the block's model is uniform; the result depends on the model, its normals, its intensities and its k alone -- not on
// CAP, which is the launch's, nor on the other pairs.  No atomics.
// LDS: 4 x 3 x TW x sizeof(F) = 24 KiB of coordinate tiles + 4 x TW doubles of intensities (16 / 8 KiB); the three lists of phase 1
// (3 x CAP x 64 x sizeof(F) <= 48 KiB) lie over them.
// ------------------------------------------------------------------------------------------------
template <typename F, int CAP>
__global__ __launch_bounds__(NN_BLOCK) void batch_intensity_gradient_kernel(const BatchGradArgs a)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK, T2 = 4 * TW;
    constexpr size_t TILE_BYTES = sizeof(F) * 4 * 3 * TW, INT_BYTES = sizeof(double) * T2, LIST_BYTES = sizeof(F) * 3 * CAP * BATCH_ITEM;
    static_assert(CAP >= 1 && CAP <= COV_MAX_K && TILE_BYTES % 16 == 0, "the list's capacity");
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[TILE_BYTES + INT_BYTES > LIST_BYTES ? TILE_BYTES + INT_BYTES : LIST_BYTES];
    double* si = reinterpret_cast<double*>(s_raw + TILE_BYTES);   // phase 2: the tile's intensities, behind its coordinates

    const BatchItem it = a.items[blockIdx.x];
    const BatchPair pr = a.pairs[it.pair];
    const int k = a.k[it.pair];   // in [ICP_COV_MIN_NEIGHBOURS, CAP], and the model holds at least k + 1 points (the host checked)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);   // (lanes past the item's end repeat its first point: nothing of theirs is kept)
    const long long sp = a.q_plane;
    const F* Sx = static_cast<const F*>(a.Q_soa) + pr.q_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const double* SI = a.int_q + pr.q_off;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const int n = pr.m;

    const F tau = kth_distance<F, CAP>(s_raw, Sx, Sy, Sz, n, k, it, i, px, py, pz);

    const F* Nx = static_cast<const F*>(a.N_soa) + pr.q_off;
    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    const double nx = (double)Nx[i], ny = (double)Nx[sp + i], nz = (double)Nx[2 * sp + i];
    const double Ii = SI[i];
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    int cnt = 0;
    walk_tiles<F, T2>(
        reinterpret_cast<F(*)[T2]>(s_raw), Sx, Sy, Sz, n, px, py, pz, [&](int e, int j, bool inside) { si[e] = inside ? SI[j] : 0.0; },
        [&](F d, int j) { return d <= tau && j != i; },
        [&](int cc, const bool(&in)[C], const F(&qq)[3][C]) {
#pragma unroll
            for (int kk = 0; kk < C; ++kk) {
                if (in[kk]) {
                    const double ex = (double)qq[0][kk] - xi, ey = (double)qq[1][kk] - yi, ez = (double)qq[2][kk] - zi;
                    const double h = dot3(ex, ey, ez, nx, ny, nz);
                    const double ux = ex - h * nx, uy = ey - h * ny, uz = ez - h * nz;
                    const double g = si[cc + kk] - Ii;
                    A00 += ux * ux; A01 += ux * uy; A02 += ux * uz;
                    A11 += uy * uy; A12 += uy * uz; A22 += uz * uz;
                    r0 += ux * g; r1 += uy * g; r2 += uz * g;
                    cnt += 1;
                }
            }
        });
    if (w != 0 || !live) return;
    const double wn = (double)cnt * (double)cnt;   // the tangent constraint's weight
    A00 += wn * (nx * nx); A01 += wn * (nx * ny); A02 += wn * (nx * nz);
    A11 += wn * (ny * ny); A12 += wn * (ny * nz); A22 += wn * (nz * nz);
    const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
    const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
    const double det = (A00 * c00 + A01 * c01) + A02 * c02;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (det > 0.0 && det < __builtin_huge_val()) {   // (NaN fails both)
        const double M00 = c00 / det, M01 = c01 / det, M02 = c02 / det, M11 = c11 / det, M12 = c12 / det, M22 = c22 / det;
        d0 = dot3(M00, M01, M02, r0, r1, r2);
        d1 = dot3(M01, M11, M12, r0, r1, r2);
        d2 = dot3(M02, M12, M22, r0, r1, r2);
        if (!(finite_(d0) && finite_(d1) && finite_(d2))) { d0 = 0.0; d1 = 0.0; d2 = 0.0; }
    }
    double* gv = a.grad + pr.q_off + i;   // the planes are laid out as the model's
    gv[0] = d0; gv[sp] = d1; gv[2 * sp] = d2;
}

hipError_t launch_batch_intensity_gradients(const BatchGradArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    if (!a.items || !a.pairs || !a.k || !a.Q_soa || !a.N_soa || !a.int_q || !a.grad) return hipErrorInvalidValue;
#define ICP_GRAD_LAUNCH(F, CAP) hipLaunchKernelGGL((batch_intensity_gradient_kernel<F, CAP>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a)
#define ICP_GRAD_LAUNCH_F(F)                          \
    do {                                              \
        if (a.cap <= 8) ICP_GRAD_LAUNCH(F, 8);        \
        else if (a.cap <= 16) ICP_GRAD_LAUNCH(F, 16); \
        else ICP_GRAD_LAUNCH(F, 32);                  \
    } while (0)
    if (a.precision == ICP_F64) ICP_GRAD_LAUNCH_F(double); else ICP_GRAD_LAUNCH_F(float);
#undef ICP_GRAD_LAUNCH_F
#undef ICP_GRAD_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// the colored step (icp_batch_begin with ICP_COLORED): the decision and the terms of every kept match -- batch_gicp_moments' place
// on the deferred route, over the same items and in its block shape (wave 0 alone carries data, waves 1-3 add zeros,
// block_sum_store adds a row in the fused pass's order).
//   kept: batch_kept.  A rejected point's idx entry gets BATCH_IDX_REJECTED.
//   terms, in double from the widened coordinates p (the moved point), q = Q[idx], the normal n and the gradient d of model point
//     idx and the two intensities: e = p - q, h = e . n, s = d . n, m = d - s n, u = e - h n, rI = (Iq + d . u) - Ip; G_a = j_a . n,
//     K_a = j_a . m for the six columns j_a of J = [-[p]x | I]; lg = lambda[pair], lp = 1.0 - lg;
//     C(a, c) += lg (G_a G_c) + lp (K_a K_c) (a <= c), B(a) -= lg (G_a h) + lp (K_a rI), CNT = 1.  Every dot product is dot3; with
//     lg == 1 these are the plane pass's statements.
// The block writes slots 1 .. ICP_MOM_B + 5 of its row and leaves ICP_MOM_ERR, the matching launch's.  A pair that takes part in the
// step without matching (the loop's error-only last pass) gets zeros throughout.  No LDS beyond block_sum_store's.
// ------------------------------------------------------------------------------------------------
template <typename F, bool MUTUAL>
__global__ __launch_bounds__(NN_BLOCK) void batch_color_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                                const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                                const F* __restrict__ Q, const F* __restrict__ N, long long q_plane,
                                                                int32_t* __restrict__ idx_cur, const F* __restrict__ dist,
                                                                const F* __restrict__ tau, const F* __restrict__ thr,
                                                                const double* __restrict__ int_p, const double* __restrict__ int_q,
                                                                const double* __restrict__ grad_q, const double* __restrict__ color_w,
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
            const double ex = px - (double)Q[gj], ey = py - (double)Q[q_plane + gj], ez = pz - (double)Q[2 * q_plane + gj];
            const double nx = (double)N[gj], ny = (double)N[q_plane + gj], nz = (double)N[2 * q_plane + gj];
            const double dx = grad_q[gj], dy = grad_q[q_plane + gj], dz = grad_q[2 * q_plane + gj];
            const double h = dot3(ex, ey, ez, nx, ny, nz);
            const double s = dot3(dx, dy, dz, nx, ny, nz);
            const double mx = dx - s * nx, my = dy - s * ny, mz = dz - s * nz;
            const double ux = ex - h * nx, uy = ey - h * ny, uz = ez - h * nz;
            const double rI = (int_q[gj] + dot3(dx, dy, dz, ux, uy, uz)) - int_p[gi];
            const double lg = color_w[it.pair], lp = 1.0 - lg;
            const double J[6][3] = {{0.0, -pz, py}, {pz, 0.0, -px}, {-py, px, 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
            double G[6], K[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                G[c] = dot3(J[c][0], J[c][1], J[c][2], nx, ny, nz);
                K[c] = dot3(J[c][0], J[c][1], J[c][2], mx, my, mz);
            }
            acc[ICP_MOM_CNT] = 1.0;
            int o = ICP_MOM_C;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[o++] += lg * (G[r] * G[c]) + lp * (K[r] * K[c]);
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[ICP_MOM_B + r] -= lg * (G[r] * h) + lp * (K[r] * rI);
        }
        if (!kept) idx_cur[gi] = j | BATCH_IDX_REJECTED;   // (a rejected point adds nothing: every accumulator stays 0, the count included)
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}

hipError_t launch_batch_color_moments(const BatchPassArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    if (!a.N_soa || !a.int_p || !a.int_q || !a.grad_q || !a.color_w || !a.dist) return hipErrorInvalidValue;
    if (a.recip && !a.rev) return hipErrorInvalidValue;
#define ICP_LAUNCH_COLOR(F, MUT)                                                                                                 \
    hipLaunchKernelGGL((batch_color_moments<F, MUT>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.mode,           \
                       (const F*)a.P_soa, a.p_plane, (const F*)a.Q_soa, (const F*)a.N_soa, a.q_plane, a.idx_cur, (const F*)a.dist, \
                       a.trim_rank ? (const F*)a.tau : (const F*)nullptr, (const F*)a.thr, a.int_p, a.int_q, a.grad_q, a.color_w,  \
                       a.partials, (const int32_t*)a.rev, a.recip)
    if (a.precision == ICP_F64) {
        if (a.recip) ICP_LAUNCH_COLOR(double, true); else ICP_LAUNCH_COLOR(double, false);
    } else {
        if (a.recip) ICP_LAUNCH_COLOR(float, true); else ICP_LAUNCH_COLOR(float, false);
    }
#undef ICP_LAUNCH_COLOR
    return hipGetLastError();
}

}  // namespace icp
