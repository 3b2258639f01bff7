// icp_k_feat.hip -- gfx950 kernels of batched global registration (icp_batch.cpp): the 33-bin FPFH descriptor of every point of
// every cloud of a batch (batch_spfh_kernel, batch_fpfh_kernel), the nearest descriptor of the other cloud (batch_feature_match)
// and the inlier count of candidate poses over a correspondence list (batch_score_transforms); the sums of one iteration of Fast
// Global Registration over a used list, and its weights (batch_fgr_terms, batch_fgr_finalize).  The rules are stated in
// include/icp_mi355x.h and restated in numpy (tests/batch_feature_ref.py, tests/batch_fgr_ref.py); every step here is one statement of them.  The scan
// and the walk are icp_device_batch.h's.  Contraction is off for this file: nothing is fused.  No atomics anywhere.
#include "icp_device_batch.h"

namespace icp {

constexpr int FEAT_TILE = 512;    // points per LDS tile of the neighbourhood walks: coordinates (and, in batch_spfh_kernel, normals)

// bin(val, lo, width) = clamp((int)floor((11.0 * (val - lo)) / width), 0, 10); the clamp is taken in double, a NaN lands in bin 0
__device__ __forceinline__ int feat_bin(double val, double lo, double width)
{
    const double f = floor((11.0 * (val - lo)) / width);
    return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);
}

// ------------------------------------------------------------------------------------------------
// SPFH of every point (icp_batch_compute_features, first launch): one block of NN_BLOCK threads per work item, one query per lane.
//   phase 1  tau_i = kth_distance over the query's own cloud.
//   phase 2  load_tile, FEAT_TILE points per tile with their normals (always double), and a walk of its own by wave 0 (a chunk in
//            which no lane's test passes is skipped; through walk_tiles the kernel needs more registers): a point with d2(i, j) <= tau_i gives
//            one pair term (the query itself has r2 == 0 and is skipped with every other coincident point), three bins, three
//            integer counters of the lane's 33 in LDS (s_cnt[bin][lane]: a lane owns a bank).  Counts have no order.  The chunk's
//            points are read from the tile one by one (a rolled loop: no runtime-indexed register array).
//   then     S_i[b] = (100.0 * (double)cnt_b) / (double)c, or zeros where c == 0; tau_i is stored for the second launch.
// LDS: phase 1 as batch_cov_kernel (24 KiB of sub-tiles, reused for the lists: <= 48 KiB for CAP 32, fp64); phase 2 over the same
// bytes FEAT_TILE x (3 sizeof(F) + 24) = 18 / 24 KiB; beside them the counters, 33 x 64 x 4 = 8.25 KiB.
// ------------------------------------------------------------------------------------------------
template <typename F, int CAP>
__global__ __launch_bounds__(NN_BLOCK) void batch_spfh_kernel(const BatchFeatArgs a)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK, T2 = FEAT_TILE;
    constexpr size_t TILE_BYTES = sizeof(F) * 4 * 3 * TW, LIST_BYTES = sizeof(F) * 3 * CAP * BATCH_ITEM;
    constexpr size_t WALK_BYTES = (sizeof(F) + sizeof(double)) * 3 * T2;
    constexpr size_t RAW_A = TILE_BYTES > LIST_BYTES ? TILE_BYTES : LIST_BYTES, RAW = RAW_A > WALK_BYTES ? RAW_A : WALK_BYTES;
    static_assert(CAP >= 1 && CAP <= COV_MAX_K, "the list's capacity");
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[RAW];
    __shared__ int s_cnt[ICP_FEATURE_BINS][BATCH_ITEM];
    double(*sn)[T2] = reinterpret_cast<double(*)[T2]>(s_raw);                // phase 2: the tile's normals ...
    F(*st)[T2] = reinterpret_cast<F(*)[T2]>(s_raw + sizeof(double) * 3 * T2);  // ... and its coordinates

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
    const double* Nx = a.nrm[c.side] + c.src_off;
    const double* Ny = Nx + sp;
    const double* Nz = Nx + 2 * sp;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const int n = c.n;

    const F tau = kth_distance<F, CAP>(s_raw, Sx, Sy, Sz, n, k, it, i, px, py, pz);
    if (w == 0) {
#pragma unroll 1
        for (int b = 0; b < ICP_FEATURE_BINS; ++b) s_cnt[b][lane] = 0;
    }

    // ---- phase 2: the pair terms of the neighbourhood, wave 0
    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    const double nix = Nx[i], niy = Ny[i], niz = Nz[i];
    int cnt = 0;
    const int ntile = (n + T2 - 1) / T2;
    for (int t = 0; t < ntile; ++t) {
        const int t0 = t * T2;
        load_tile<F, T2>(st, Sx, Sy, Sz, t0, n, [&](int e, int j, bool inside) {
            sn[0][e] = inside ? Nx[j] : 0.0;
            sn[1][e] = inside ? Ny[j] : 0.0;
            sn[2][e] = inside ? Nz[j] : 0.0;
        });
        if (w != 0) continue;
        const int len = min(T2, n - t0);
        for (int cc = 0; cc < len; cc += C) {
            F dd[C];
            chunk_dist2<F, T2>(st, cc, px, py, pz, dd);
            unsigned in = 0u;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) in |= (dd[kk] <= tau) ? (1u << kk) : 0u;   // (NaN: false)
            if (__builtin_amdgcn_ballot_w64(in != 0u) == 0ull) continue;
#pragma unroll 1
            for (int kk = 0; kk < C; ++kk) {
                if (!((in >> kk) & 1u)) continue;
                const int e = cc + kk;
                double dx = (double)st[0][e] - xi, dy = (double)st[1][e] - yi, dz = (double)st[2][e] - zi;
                const double r2 = dot3(dx, dy, dz, dx, dy, dz);
                if (r2 == 0.0 || !finite_(r2)) continue;
                const double r = sqrt(r2);
                const double njx = sn[0][e], njy = sn[1][e], njz = sn[2][e];
                const double a1 = dot3(nix, niy, niz, dx, dy, dz) / r, a2 = dot3(njx, njy, njz, dx, dy, dz) / r;
                double n1x, n1y, n1z, n2x, n2y, n2z, f3;
                if (__builtin_fabs(a1) < __builtin_fabs(a2)) {
                    n1x = njx; n1y = njy; n1z = njz; n2x = nix; n2y = niy; n2z = niz;
                    dx = -dx; dy = -dy; dz = -dz;
                    f3 = -a2;
                } else {
                    n1x = nix; n1y = niy; n1z = niz; n2x = njx; n2y = njy; n2z = njz;
                    f3 = a1;
                }
                double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
                const double vv = dot3(vx, vy, vz, vx, vy, vz);
                if (vv == 0.0 || !finite_(vv)) continue;
                const double sv = sqrt(vv);
                vx = vx / sv; vy = vy / sv; vz = vz / sv;
                const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
                const double f2 = dot3(vx, vy, vz, n2x, n2y, n2z);
                const double x = dot3(n1x, n1y, n1z, n2x, n2y, n2z), y = dot3(wx, wy, wz, n2x, n2y, n2z);
                const double s = __builtin_fabs(x) + __builtin_fabs(y);
                double tt = 0.0;
                if (!(s == 0.0)) {
                    const double q = y / s;
                    tt = x >= 0.0 ? q : (y >= 0.0 ? 2.0 - q : -2.0 - q);
                }
                s_cnt[feat_bin(tt, -2.0, 4.0)][lane] += 1;
                s_cnt[11 + feat_bin(f2, -1.0, 2.0)][lane] += 1;
                s_cnt[22 + feat_bin(f3, -1.0, 2.0)][lane] += 1;
                cnt += 1;
            }
        }
    }
    if (w != 0 || !live) return;
    static_cast<F*>(a.tau[c.side])[c.src_off + i] = tau;
    double* S = a.spfh[c.side] + (size_t)(c.src_off + i) * ICP_FEATURE_BINS;
    const double dc = (double)cnt;
#pragma unroll 1
    for (int b = 0; b < ICP_FEATURE_BINS; ++b) S[b] = cnt > 0 ? (100.0 * (double)s_cnt[b][lane]) / dc : 0.0;
}

// ------------------------------------------------------------------------------------------------
// FPFH of every point (second launch): the same work items, the same walk.  A[b] += S_j[b] * (1.0 / (double)d2(i, j)) over the
// neighbourhood in ascending j, a point at d2 == 0 skipped (the query itself among them).  One lane, one query, one running sum per
// bin, ascending j: wave w carries the bins w, w + 4, w + 8, ... (nine running sums; every wave walks the whole cloud), so the order
// of the additions of a bin is ascending j whatever the cloud.  S_j is read at a wave-uniform address.  Then wave 0 normalises each
// sub-histogram of 11 bins: s = the sequential sum from 0.0 in ascending b, F_i[b] = (A[b] * 100.0) / s, or 0.0 where s is not > 0 or
// not finite.  LDS: the tile's coordinates, FEAT_TILE x 3 sizeof(F) = 6 / 12 KiB, and the 33 sums of 64 lanes, 16.5 KiB.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_fpfh_kernel(const BatchFeatArgs a)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int C = KNN_CHUNK, T2 = FEAT_TILE, NB = (ICP_FEATURE_BINS + 3) / 4;
    static_assert(T2 % C == 0 && C % VN == 0, "whole chunks, whole vectors");
    __shared__ __attribute__((aligned(16))) F st[3][T2];
    __shared__ double s_acc[ICP_FEATURE_BINS][BATCH_ITEM];

    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const double* SP = a.spfh[c.side] + (size_t)c.src_off * ICP_FEATURE_BINS;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const F tau = static_cast<const F*>(a.tau[c.side])[c.src_off + i];
    const int n = c.n;
    double A[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) A[b] = 0.0;
    const int ntile = (n + T2 - 1) / T2;
    for (int t = 0; t < ntile; ++t) {
        const int t0 = t * T2;
        load_tile<F, T2>(st, Sx, Sy, Sz, t0, n);
        const int len = min(T2, n - t0);
        for (int cc = 0; cc < len; cc += C) {
            bool any = false;   // (the test alone, vector by vector: with chunk_dist2's eight distances held, the kernel needs 19 registers more)
#pragma unroll
            for (int kk = 0; kk < C; kk += VN) {
                const V qx = *reinterpret_cast<const V*>(&st[0][cc + kk]);
                const V qy = *reinterpret_cast<const V*>(&st[1][cc + kk]);
                const V qz = *reinterpret_cast<const V*>(&st[2][cc + kk]);
#pragma unroll
                for (int v = 0; v < VN; ++v) any = any || dist2<F>(px, py, pz, vget(qx, v), vget(qy, v), vget(qz, v)) <= tau;   // (NaN: false)
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
#pragma unroll 1
            for (int kk = 0; kk < C; ++kk) {
                const int e = cc + kk;
                const F d = dist2<F>(px, py, pz, st[0][e], st[1][e], st[2][e]);
                if (!(d <= tau) || d == (F)0) continue;
                const double wgt = 1.0 / (double)d;
                const double* Sj = SP + (size_t)(t0 + e) * ICP_FEATURE_BINS;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int bin = w + 4 * b;   // (wave-uniform)
                    if (bin < ICP_FEATURE_BINS) A[b] += Sj[bin] * wgt;
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int bin = w + 4 * b;
        if (bin < ICP_FEATURE_BINS) s_acc[bin][lane] = A[b];
    }
    __syncthreads();
    if (w != 0 || !live) return;
    double* Fo = a.feat[c.side] + (size_t)(c.src_off + i) * ICP_FEATURE_BINS;
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        double s = 0.0;
#pragma unroll 1
        for (int b = 0; b < 11; ++b) s += s_acc[11 * h + b][lane];
        const bool ok = s > 0.0 && s < __builtin_huge_val();   // (NaN fails both)
#pragma unroll 1
        for (int b = 0; b < 11; ++b) Fo[11 * h + b] = ok ? (s_acc[11 * h + b][lane] * 100.0) / s : 0.0;
    }
}

hipError_t launch_batch_features(const BatchFeatArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    if (!a.clouds || !a.items || !a.k || !a.nrm[0] || !a.nrm[1] || !a.tau[0] || !a.tau[1] || !a.spfh[0] || !a.spfh[1] || !a.feat[0] || !a.feat[1])
        return hipErrorInvalidValue;
#define ICP_SPFH_LAUNCH(F, CAP) hipLaunchKernelGGL((batch_spfh_kernel<F, CAP>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a)
#define ICP_SPFH_LAUNCH_F(F)                          \
    do {                                              \
        if (a.cap <= 8) ICP_SPFH_LAUNCH(F, 8);        \
        else if (a.cap <= 16) ICP_SPFH_LAUNCH(F, 16); \
        else ICP_SPFH_LAUNCH(F, 32);                  \
    } while (0)
    if (a.precision == ICP_F64) ICP_SPFH_LAUNCH_F(double); else ICP_SPFH_LAUNCH_F(float);
#undef ICP_SPFH_LAUNCH_F
#undef ICP_SPFH_LAUNCH
    if (hipError_t e = hipGetLastError()) return e;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_fpfh_kernel<double>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((batch_fpfh_kernel<float>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// descriptor matching (icp_batch_match_features): one block per 64 queries of one pair, one query per lane, its 33 doubles in
// registers; the other cloud's descriptors stream through an LDS tile of FMATCH_TILE points (every lane reads the same address: a
// broadcast), wave w taking a quarter of every tile.  D(i, j) = the sum of (F_i[b] - G_j[b])^2 from 0.0 in ascending b; a wave
// meets its j in ascending order and takes a strictly smaller D only; wave 0 then takes of the four (D, j) the smallest D and,
// among equal D, the smallest j: the lowest j that minimises D.  A NaN never wins; where no D is below +inf the answer is 0.
// swap = 0: queries are the moving clouds (-> fwd, laid out as the moving clouds); 1: the models (-> rev).
// LDS: FMATCH_TILE x 33 x 8 = 16.5 KiB, and 3 KiB for the four candidates of every lane.
// ------------------------------------------------------------------------------------------------
constexpr int FMATCH_TILE = 64;
__global__ __launch_bounds__(NN_BLOCK) void batch_feature_match(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                                const double* __restrict__ fq, const double* __restrict__ fo, int swap,
                                                                int32_t* __restrict__ out)
{
    constexpr int NB = ICP_FEATURE_BINS, TJ = FMATCH_TILE, WJ = TJ / 4;
    __shared__ double g[TJ * NB];
    __shared__ double s_d[4][BATCH_ITEM];
    __shared__ int s_j[4][BATCH_ITEM];
    const BatchItem it = items[blockIdx.x];
    const BatchPair pr = pairs[it.pair];
    const long long qoff = swap ? pr.q_off : pr.p_off, ooff = swap ? pr.p_off : pr.q_off;
    const int no = swap ? pr.n : pr.m;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);
    double f[NB];
    {
        const double* src = fq + (size_t)(qoff + i) * NB;
#pragma unroll
        for (int b = 0; b < NB; ++b) f[b] = src[b];
    }
    double best = __builtin_huge_val();
    int bj = 0;
    for (int t0 = 0; t0 < no; t0 += TJ) {
        const int len = min(TJ, no - t0);
        const double* src = fo + (size_t)(ooff + t0) * NB;
        __syncthreads();
        for (int e = threadIdx.x; e < TJ * NB; e += NN_BLOCK) g[e] = e < len * NB ? src[e] : 0.0;
        __syncthreads();
        const int j1 = min(WJ * (w + 1), len);
        for (int jj = WJ * w; jj < j1; ++jj) {
            const double* gj = &g[jj * NB];
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double d = f[b] - gj[b];
                s = s + d * d;
            }
            if (s < best) {
                best = s;
                bj = t0 + jj;
            }
        }
    }
    s_d[w][lane] = best;
    s_j[w][lane] = bj;
    __syncthreads();
    if (w != 0 || !live) return;
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
        const double d = s_d[ww][lane];
        const int j = s_j[ww][lane];
        if (d < best || (d == best && j < bj)) {
            best = d;
            bj = j;
        }
    }
    out[qoff + i] = bj;
}

hipError_t launch_batch_feature_match(const BatchFeatMatchArgs& a, hipStream_t st)
{
    if (!a.pairs || !a.feat[0] || !a.feat[1] || !a.fwd || !a.rev || !a.items[0] || !a.items[1]) return hipErrorInvalidValue;
    if (a.n_items[0] > 0)
        hipLaunchKernelGGL(batch_feature_match, dim3(a.n_items[0]), dim3(NN_BLOCK), 0, st, a.items[0], a.pairs, a.feat[0], a.feat[1], 0, a.fwd);
    if (a.n_items[1] > 0)
        hipLaunchKernelGGL(batch_feature_match, dim3(a.n_items[1]), dim3(NN_BLOCK), 0, st, a.items[1], a.pairs, a.feat[1], a.feat[0], 1, a.rev);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// inlier counts of candidate poses over every pair's correspondence list (icp_batch_score_transforms, icp_batch_ransac): one block
// per (pair, group of SCORE_GROUP candidates).  A thread gathers the points of its list entries once -- p = P0[ci[e]], q = Q[cj[e]]
// -- and moves p by every candidate of the group in the front end's arithmetic (apply_rt); an entry counts iff the moved point is
// finite and dist2(moved, q) <= thr[pair].  Per wave a ballot and a popcount per candidate; the four waves' integers are added in
// LDS.  Integers have no order: the count is exact.  A candidate whose valid byte is 0 is not scored (its count is 0).
// ------------------------------------------------------------------------------------------------
constexpr int SCORE_GROUP = 16;
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_score_transforms(const BatchPair* __restrict__ pairs, const int* __restrict__ cn,
                                                                   const int32_t* __restrict__ ci, const int32_t* __restrict__ cj,
                                                                   const F* __restrict__ P0, long long p_plane, const F* __restrict__ Q,
                                                                   long long q_plane, const RT<F>* __restrict__ cand,
                                                                   const uint8_t* __restrict__ valid, const F* __restrict__ thr, int per_pair,
                                                                   int groups, int32_t* __restrict__ counts)
{
    constexpr int G = SCORE_GROUP;
    __shared__ RT<F> s_rt[G];
    __shared__ int s_ok[G];
    __shared__ int s_wc[4][G];
    const int pair = blockIdx.x / groups, g0 = (blockIdx.x % groups) * G;
    const int ng = min(G, per_pair - g0);
    const BatchPair pr = pairs[pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < G) {
        const int g = threadIdx.x;
        const size_t at = (size_t)pair * per_pair + g0 + (g < ng ? g : 0);
        s_rt[g] = cand[at];
        s_ok[g] = g < ng && (valid == nullptr || valid[at] != 0) ? 1 : 0;
    }
    __syncthreads();
    const int C = cn[pair];
    const F th = thr[pair];
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) cnt[g] = 0;
    for (int e0 = 0; e0 < C; e0 += NN_BLOCK) {
        const int e = e0 + threadIdx.x;
        const bool have = e < C;
        F x = 0, y = 0, z = 0, qx = 0, qy = 0, qz = 0;
        if (have) {
            const long long pi = pr.p_off + ci[pr.p_off + e], qi = pr.q_off + cj[pr.p_off + e];   // (indices within [0, n) and [0, m): the host made the list)
            x = P0[pi]; y = P0[p_plane + pi]; z = P0[2 * p_plane + pi];
            qx = Q[qi]; qy = Q[q_plane + qi]; qz = Q[2 * q_plane + qi];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (!s_ok[g]) continue;   // (block-uniform)
            F mx, my, mz;
            apply_rt<F>(s_rt[g], x, y, z, mx, my, mz);
            const F d = dist2<F>(mx, my, mz, qx, qy, qz);
            const bool hit = have && finite_(mx) && finite_(my) && finite_(mz) && d <= th;
            cnt[g] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) s_wc[w][g] = cnt[g];
    }
    __syncthreads();
    if (threadIdx.x < ng) {
        const int g = threadIdx.x;
        counts[(size_t)pair * per_pair + g0 + g] = ((s_wc[0][g] + s_wc[1][g]) + s_wc[2][g]) + s_wc[3][g];
    }
}

hipError_t launch_batch_score(const BatchScoreArgs& a, hipStream_t st)
{
    if (a.n_pairs <= 0 || a.per_pair <= 0) return hipSuccess;
    if (!a.pairs || !a.cn || !a.ci || !a.cj || !a.P0 || !a.Q || !a.cand || !a.thr || !a.counts) return hipErrorInvalidValue;
    const int groups = (a.per_pair + SCORE_GROUP - 1) / SCORE_GROUP;
    if ((long long)groups * a.n_pairs > 0x7fffffffLL) return hipErrorInvalidValue;
#define ICP_SCORE_LAUNCH(F)                                                                                                       \
    hipLaunchKernelGGL((batch_score_transforms<F>), dim3(groups * a.n_pairs), dim3(NN_BLOCK), 0, st, a.pairs, a.cn, a.ci, a.cj,   \
                       (const F*)a.P0, a.p_plane, (const F*)a.Q, a.q_plane, (const RT<F>*)a.cand, a.valid, (const F*)a.thr,       \
                       a.per_pair, groups, a.counts)
    if (a.precision == ICP_F64) ICP_SCORE_LAUNCH(double); else ICP_SCORE_LAUNCH(float);
#undef ICP_SCORE_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Fast Global Registration (icp_batch_fgr): the terms of one Gauss-Newton step of the Geman-McClure objective over every pair's
// used list, in batch_gicp_moments' block shape -- one block per 64 list entries, wave 0 alone carries data, waves 1-3 add zeros,
// block_sum_store writes the row.  Entry e of the pair's list: p0 = P0[ui[e]], q = Q[uj[e]], widened once; everything after that
// is the header's rule in double, one operation per statement:
//   p_a = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3], e = p - q, r2 = (ex*ex + ey*ey) + ez*ez, s = mu / (mu + r2), l = s*s;
//   cn_x = (0, pz, -py, 1, 0, 0), cn_y = (-pz, 0, px, 0, 1, 0), cn_z = (py, -px, 0, 0, 0, 1), w_a[r] = l * cn_a[r];
//   C(r, c) += (w_x[r]*cn_x[c] + w_y[r]*cn_y[c]) + w_z[r]*cn_z[c] (r <= c), B(r) -= (w_x[r]*ex + w_y[r]*ey) + w_z[r]*ez,
//   CNT += 1, W += l, ERR += l*r2 + mu*((1 - s)*(1 - s)).
// An entry whose p or r2 is not finite adds nothing.  The products with the constant zeros and ones stay as written: 0 * x is +-0
// for every finite x, and the statement is the rule numpy restates.  WEIGHTS: the same l at the pair's final pose into
// weights[p_off + ui[e]] (0.0 for an entry that does not count) and nothing else -- the list holds a moving point once, so no two
// lanes write one address.  A pair whose flag in ctl is 0.0 takes no part.  No LDS beyond block_sum_store's 4 x 30 doubles.
// ------------------------------------------------------------------------------------------------
template <typename F, bool WEIGHTS>
__global__ __launch_bounds__(NN_BLOCK) void batch_fgr_terms(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                            const int32_t* __restrict__ ui, const int32_t* __restrict__ uj,
                                                            const F* __restrict__ P0, long long p_plane, const F* __restrict__ Q,
                                                            long long q_plane, const double* __restrict__ ctl,
                                                            double* __restrict__ partials, double* __restrict__ weights)
{
    constexpr int NACC = ICP_MOM_W + 1;
    static_assert(ICP_MOM_ERR == 0 && ICP_MOM_CNT == 1 && ICP_MOM_C == 2 && ICP_MOM_B == ICP_MOM_C + 21 && ICP_MOM_W == ICP_MOM_B + 6 && NACC <= ICP_NMOM,
                  "a plane pass's slots, then the sum of the weights");
    const BatchItem it = items[blockIdx.x];
    const double* c = ctl + (size_t)FGR_CTL * it.pair;
    if (c[FGR_CTL_RUN] == 0.0) return;   // (block-uniform)
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (w == 0 && lane < it.count) {
        const long long e = pr.p_off + it.first + lane;            // (first + count <= U_p <= n: the host made the items from the list)
        const long long gi = pr.p_off + ui[e], gj = pr.q_off + uj[e];   // (indices within [0, n) and [0, m): the host made the list)
        const double x = (double)P0[gi], y = (double)P0[p_plane + gi], z = (double)P0[2 * p_plane + gi];
        const double mu = c[FGR_CTL_MU];
        double p[3], ev[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = ((c[4 * a] * x + c[4 * a + 1] * y) + c[4 * a + 2] * z) + c[4 * a + 3];
            ev[a] = p[a] - (double)Q[a * q_plane + gj];
        }
        const double r2 = (ev[0] * ev[0] + ev[1] * ev[1]) + ev[2] * ev[2];
        const double s = mu / (mu + r2);
        const double l = s * s;
        const bool ok = finite_(p[0]) && finite_(p[1]) && finite_(p[2]) && finite_(r2);
        if constexpr (WEIGHTS) {
            weights[gi] = ok ? l : 0.0;
        } else if (ok) {
            const double cn[3][6] = {{0.0, p[2], -p[1], 1.0, 0.0, 0.0}, {-p[2], 0.0, p[0], 0.0, 1.0, 0.0}, {p[1], -p[0], 0.0, 0.0, 0.0, 1.0}};
            double wr[3][6];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int r = 0; r < 6; ++r) wr[a][r] = l * cn[a][r];
            int o = ICP_MOM_C;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = r; cc < 6; ++cc) acc[o++] = (wr[0][r] * cn[0][cc] + wr[1][r] * cn[1][cc]) + wr[2][r] * cn[2][cc];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[ICP_MOM_B + r] -= (wr[0][r] * ev[0] + wr[1][r] * ev[1]) + wr[2][r] * ev[2];
            const double d = 1.0 - s;
            acc[ICP_MOM_ERR] = l * r2 + mu * (d * d);
            acc[ICP_MOM_CNT] = 1.0;
            acc[ICP_MOM_W] = l;
        }
    }
    if constexpr (!WEIGHTS) block_sum_store<NACC, NN_BLOCK>(acc, partials + (size_t)blockIdx.x * ICP_NMOM);
}

// one block per pair: batch_finalize_kernel's scheme and order over the pair's FGR items -- thread (k, part) adds items part,
// part + 8, ... of slot k, the eight part sums are then added in part order; the slots behind ICP_MOM_W are written as zeros
__global__ __launch_bounds__(256) void batch_fgr_finalize(const int* __restrict__ item0, const double* __restrict__ ctl,
                                                          const double* __restrict__ partials, double* __restrict__ mom)
{
    __shared__ double red[8][ICP_NMOM];
    if (ctl[(size_t)FGR_CTL * blockIdx.x + FGR_CTL_RUN] == 0.0) return;
    const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int i0 = item0[blockIdx.x], i1 = item0[blockIdx.x + 1];
    double s = 0.0;
    if (k <= ICP_MOM_W)
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

static bool fgr_args_ok(const BatchFgrArgs& a)
{
    return a.items && a.pairs && a.item0 && a.ui && a.uj && a.P0 && a.Q && a.ctl;
}

hipError_t launch_batch_fgr_terms(const BatchFgrArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    if (!fgr_args_ok(a) || !a.partials || !a.mom) return hipErrorInvalidValue;
#define ICP_FGR_LAUNCH(F)                                                                                                      \
    hipLaunchKernelGGL((batch_fgr_terms<F, false>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.ui, a.uj,      \
                       (const F*)a.P0, a.p_plane, (const F*)a.Q, a.q_plane, a.ctl, a.partials, (double*)nullptr)
    if (a.precision == ICP_F64) ICP_FGR_LAUNCH(double); else ICP_FGR_LAUNCH(float);
#undef ICP_FGR_LAUNCH
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_fgr_finalize, dim3(a.n_pairs), dim3(256), 0, st, a.item0, a.ctl, (const double*)a.partials, a.mom);
    return hipGetLastError();
}

hipError_t launch_batch_fgr_weights(const BatchFgrArgs& a, hipStream_t st)
{
    if (a.n_items <= 0 || a.n_pairs <= 0) return hipSuccess;
    if (!fgr_args_ok(a) || !a.weights) return hipErrorInvalidValue;
#define ICP_FGR_LAUNCH(F)                                                                                                      \
    hipLaunchKernelGGL((batch_fgr_terms<F, true>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a.items, a.pairs, a.ui, a.uj,       \
                       (const F*)a.P0, a.p_plane, (const F*)a.Q, a.q_plane, a.ctl, (double*)nullptr, a.weights)
    if (a.precision == ICP_F64) ICP_FGR_LAUNCH(double); else ICP_FGR_LAUNCH(float);
#undef ICP_FGR_LAUNCH
    return hipGetLastError();
}

}  // namespace icp
