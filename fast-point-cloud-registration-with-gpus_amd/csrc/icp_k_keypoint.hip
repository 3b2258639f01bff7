// icp_k_keypoint.hip -- gfx950 kernels of keypoint selection for batched global registration (icp_batch_select_keypoints,
// icp_batch.cpp): the ISS saliency of every point of every cloud of a batch (batch_iss_saliency), the non-maximum suppression
// (batch_iss_select), the ranks of the kept points (batch_keypoint_rank) and the compaction of their coordinates and descriptors
// into a new batch (batch_keypoint_compact).  The rule is stated in include/icp_mi355x.h and restated in numpy
// (tests/batch_keypoint_ref.py); every step here is one statement of it.  The kernels of icp_k_gicp.hip and icp_k_batch.hip keep
// their listings: what this file needs of them -- the neighbourhood sums of batch_cov_kernel's phase 2, the scan of
// batch_outlier_decide, the copy of batch_outlier_compact -- is restated, not shared; icp_eigh3's Jacobi (icp_host_math.cpp) is
// restated in named scalars.  Contraction is off for this file: nothing is fused.
//
// Launches of one call: four -- batch_iss_saliency and batch_iss_select (one block of NN_BLOCK threads per 64 points of every
// cloud), batch_keypoint_rank (one block of VOXEL_SCAN_BLOCK threads per cloud), batch_keypoint_compact (one wave per 64 points).
// LDS per block: batch_iss_saliency 3 x 4 x TW x sizeof(F) = 24 KiB (one tile of the block); batch_iss_select 4 sub-tiles of
// 3 x TW x sizeof(F) + TW x 8 bytes (coordinates and saliencies) = 40 KiB fp32, 32 KiB fp64, plus 2 KiB for the waves' counts and
// flags; batch_keypoint_rank 16 bytes; batch_keypoint_compact none.  No atomics of any kind.
#include "icp_device.h"
#include <math.h>

namespace icp {

template <typename F> struct KeypointCfg;
template <> struct KeypointCfg<float> { static constexpr int TW = 512; };    // points per wave and sub-tile (GicpCfg's: 6 KiB per wave)
template <> struct KeypointCfg<double> { static constexpr int TW = 256; };
constexpr int KP_CHUNK = 8;   // points per early-out chunk

template <typename F> __device__ __forceinline__ F kp_nan();
template <> __device__ __forceinline__ float kp_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double kp_nan<double>() { return __builtin_nan(""); }

// one rotation of icp_eigh3's sweep on the pair (p, q), r the remaining index: app = a[p][p], aqq = a[q][q], apq = a[p][q],
// arp = a[r][p], arq = a[r][q].  The statements and their order are the host's; the eigenvectors are not formed.
__device__ __forceinline__ void kp_rotate(double& app, double& aqq, double& apq, double& arp, double& arq)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double p0 = app, q0 = aqq, rp = arp, rq = arq;
    app = p0 - t * apq;
    aqq = q0 + t * apq;
    apq = 0.0;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
}

// ------------------------------------------------------------------------------------------------
// ISS saliency: one block of NN_BLOCK threads per work item, one query per lane -- batch_cov_kernel's phase 2 with the fixed
// threshold ts = (F)(salient_radius * salient_radius) in tau's place.  The block loads the cloud 4 * TW points per tile and wave 0
// walks every tile in ascending j: a point with d2(i, j) <= ts -- the query itself included, at distance 0 -- adds e = x_j - x_i (in
// double) to s and e e^T to S.  One lane, one query, one running sum: the order of the additions is ascending j whatever the
// cloud.  A chunk in which no lane's test passes is skipped (wave-uniform).  Places past the cloud's end hold NaN: such a distance
// passes no test.  Then C = (S - s s^T / c) / c, the Jacobi on six named doubles (no runtime-indexed array, no scratch), the
// ascending order, the four tests, and one store of sal.  A copied cloud (ICP_KEYPOINT_NONE) gets 0.0.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_iss_saliency(const BatchKeypointArgs a)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = KeypointCfg<F>::TW, C = KP_CHUNK, T2 = 4 * TW;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM && TW % C == 0 && C % VN == 0, "one query per lane, four waves per item");
    __shared__ __attribute__((aligned(16))) F st[3][T2];

    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const KeypointRule rule = a.rules[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);   // (lanes past the item's end repeat its first point: nothing of theirs is kept)
    double* sal = a.sal + c.tmp_off;
    if (rule.kind == ICP_KEYPOINT_NONE) {   // (the whole block)
        if (w == 0 && live) sal[i] = 0.0;
        return;
    }
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const int n = c.n;
    const double rs2 = rule.salient_radius * rule.salient_radius;
    const F ts = (F)rs2;   // the product formed in double and rounded once (the gate's rule)

    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, Sxx = 0.0, Sxy = 0.0, Sxz = 0.0, Syy = 0.0, Syz = 0.0, Szz = 0.0;
    int cnt = 0;
    const int ntile = (n + T2 - 1) / T2;
    for (int t = 0; t < ntile; ++t) {
        const int t0 = t * T2;
        __syncthreads();   // (wave 0 has read the tile before)
        for (int e = threadIdx.x; e < T2; e += NN_BLOCK) {
            const int j = t0 + e;
            F qx = kp_nan<F>(), qy = kp_nan<F>(), qz = kp_nan<F>();
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
                    in[kk + v] = dist2<F>(px, py, pz, qq[0][kk + v], qq[1][kk + v], qq[2][kk + v]) <= ts;   // (NaN: false)
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
    const double dc = (double)cnt;
    double a00 = (Sxx - (s0 * s0) / dc) / dc, a01 = (Sxy - (s0 * s1) / dc) / dc, a02 = (Sxz - (s0 * s2) / dc) / dc;
    double a11 = (Syy - (s1 * s1) / dc) / dc, a12 = (Syz - (s1 * s2) / dc) / dc, a22 = (Szz - (s2 * s2) / dc) / dc;
    // icp_eigh3: cyclic Jacobi over (0,1), (0,2), (1,2), at most 64 sweeps
#pragma unroll 1
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a01 * a01 + a02 * a02 + a12 * a12;
        const double dia = a00 * a00 + a11 * a11 + a22 * a22;
        if (off <= 1e-34 * dia || off == 0.0) break;
        kp_rotate(a00, a11, a01, a02, a12);   // (0, 1), r = 2
        kp_rotate(a00, a22, a02, a01, a12);   // (0, 2), r = 1
        kp_rotate(a11, a22, a12, a01, a02);   // (1, 2), r = 0
    }
    double w0 = a00, w1 = a11, w2 = a22, tmp;   // ... and its ascending order: three compare-and-swaps
    if (w1 < w0) { tmp = w0; w0 = w1; w1 = tmp; }
    if (w2 < w0) { tmp = w0; w0 = w2; w2 = tmp; }
    if (w2 < w1) { tmp = w1; w1 = w2; w2 = tmp; }
    const bool salient = cnt >= rule.min_neighbours && (w1 / w2) < rule.gamma_21 && (w0 / w1) < rule.gamma_32 && w0 > 0.0;   // (NaN fails each)
    sal[i] = salient ? w0 : 0.0;
}

// ------------------------------------------------------------------------------------------------
// non-maximum suppression: the same items, one query per lane.  |M_i| and "some j of M_i has sal_j > sal_i" are an integer count and a
// comparison -- no summation order -- so the four waves stream the four contiguous quarters of the query's own cloud through their
// own LDS sub-tiles (coordinates and saliencies; every lane reads the same address: a broadcast), leave their count and flag in LDS,
// and wave 0 combines them: flag = sal_i > 0 && |M_i| >= min_neighbours && no higher saliency within tn.  The flag goes into map
// (1 / 0), which batch_keypoint_rank turns into ranks.  Places past a quarter's end hold NaN.  A copied cloud is left to the rank.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_iss_select(const BatchKeypointArgs a)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = KeypointCfg<F>::TW, C = KP_CHUNK;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM && TW % C == 0 && C % VN == 0, "one query per lane, four waves per item");
    __shared__ __attribute__((aligned(16))) F sq[4][3][TW];
    __shared__ __attribute__((aligned(16))) double ss[4][TW];
    __shared__ int s_cnt[4][BATCH_ITEM];
    __shared__ int s_gt[4][BATCH_ITEM];

    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const KeypointRule rule = a.rules[it.pair];
    if (rule.kind == ICP_KEYPOINT_NONE) return;   // (the whole block)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const double* sal = a.sal + c.tmp_off;
    const F px = Sx[i], py = Sy[i], pz = Sz[i];
    const double si = sal[i];
    const int n = c.n;
    const double rn2 = rule.non_max_radius * rule.non_max_radius;
    const F tn = (F)rn2;

    const int wseg = ((n + 3) / 4 + C - 1) / C * C;      // points per wave, whole chunks
    const int my0 = w * wseg, my1 = min(my0 + wseg, n);  // may be empty (my1 <= my0)
    const int ntile = (wseg + TW - 1) / TW;              // the same for every wave: the barriers pair up
    int cnt = 0, gt = 0;
    for (int t = 0; t < ntile; ++t) {
        const int t0 = my0 + t * TW;
        __syncthreads();
        for (int e = lane; e < TW; e += 64) {
            const int j = t0 + e;
            F qx = kp_nan<F>(), qy = kp_nan<F>(), qz = kp_nan<F>();
            double sj = 0.0;
            if (j < my1) { qx = Sx[j]; qy = Sy[j]; qz = Sz[j]; sj = sal[j]; }
            sq[w][0][e] = qx;
            sq[w][1][e] = qy;
            sq[w][2][e] = qz;
            ss[w][e] = sj;
        }
        __syncthreads();
        const int len = min(TW, my1 - t0);   // <= 0: this wave's quarter is exhausted
        for (int cc = 0; cc < len; cc += C) {
            bool in[C];
            bool any = false;
#pragma unroll
            for (int kk = 0; kk < C; kk += VN) {
                const V qx = *reinterpret_cast<const V*>(&sq[w][0][cc + kk]);
                const V qy = *reinterpret_cast<const V*>(&sq[w][1][cc + kk]);
                const V qz = *reinterpret_cast<const V*>(&sq[w][2][cc + kk]);
#pragma unroll
                for (int v = 0; v < VN; ++v) {
                    in[kk + v] = dist2<F>(px, py, pz, vget(qx, v), vget(qy, v), vget(qz, v)) <= tn;   // (NaN: false)
                    any = any || in[kk + v];
                }
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) {
                const double sj = ss[w][cc + kk];
                cnt += in[kk] ? 1 : 0;
                gt |= (in[kk] && sj > si) ? 1 : 0;
            }
        }
    }
    s_cnt[w][lane] = cnt;
    s_gt[w][lane] = gt;
    __syncthreads();
    if (w != 0 || !live) return;
    const int size = (s_cnt[0][lane] + s_cnt[1][lane]) + (s_cnt[2][lane] + s_cnt[3][lane]);
    const int higher = (s_gt[0][lane] | s_gt[1][lane]) | (s_gt[2][lane] | s_gt[3][lane]);
    a.map[c.tmp_off + i] = (si > 0.0 && size >= rule.min_neighbours && higher == 0) ? 1 : 0;
}

// one block per cloud: the flags batch_iss_select left in map become the index of a kept point in its new cloud, -1 otherwise
// (batch_outlier_decide's scan, restated); a copied cloud gets 0 .. n-1; count[cloud] = the kept points.
__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_keypoint_rank(const BatchKeypointArgs a)
{
    __shared__ int s_wave[VOXEL_SCAN_BLOCK / 64];
    const int cloud = blockIdx.x;
    const KeypointRule rule = a.rules[cloud];
    const VoxelCloud c = a.clouds[cloud];
    int32_t* map = a.map + c.tmp_off;
    const int n = c.n;
    if (rule.kind == ICP_KEYPOINT_NONE) {   // copied: every point kept, in its place
        for (int i = threadIdx.x; i < n; i += VOXEL_SCAN_BLOCK) map[i] = i;
        if (threadIdx.x == 0) a.count[cloud] = n;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += VOXEL_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const int flag = i < n ? map[i] : 0;
        int incl = flag;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < VOXEL_SCAN_BLOCK / 64; ++w) {
            before += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (i < n) map[i] = flag ? carry + before + incl - flag : -1;
        carry += total;
        __syncthreads();   // (s_wave is rewritten by the next chunk)
    }
    if (threadIdx.x == 0) a.count[cloud] = carry;
}

// one wave per work item: a kept point's coordinates go to the new batch's planes at dst_off + map (batch_outlier_compact's copy),
// and, where the source holds descriptors on the cloud's side, its ICP_FEATURE_BINS doubles go to the new batch's descriptors at
// (dst_off + map) * ICP_FEATURE_BINS -- as 64-bit words, byte for byte; the item's 64 x 33 words are dealt over the lanes in order.
template <typename F>
__global__ __launch_bounds__(BATCH_ITEM) void batch_keypoint_compact(const BatchKeypointArgs a)
{
    const BatchItem it = a.items[blockIdx.x];
    const int lane = threadIdx.x;
    const VoxelCloud c = a.clouds[it.pair];
    const int32_t* map = a.map + c.tmp_off + it.first;
    if (lane < it.count) {
        const int32_t to = map[lane];
        if (to >= 0) {
            const F* S = static_cast<const F*>(a.src[c.side]) + c.src_off + it.first + lane;
            F* D = static_cast<F*>(a.dst[c.side]) + c.dst_off + to;
            const long long sp = a.src_plane[c.side], dp = a.dst_plane[c.side];
#pragma unroll
            for (int k = 0; k < 3; ++k) D[k * dp] = S[k * sp];
        }
    }
    const unsigned long long* fs = a.src_feat[c.side];
    if (fs == nullptr) return;   // (the whole block)
    unsigned long long* fd = a.dst_feat[c.side];
    fs += (size_t)(c.src_off + it.first) * ICP_FEATURE_BINS;
    for (int e = lane; e < it.count * ICP_FEATURE_BINS; e += BATCH_ITEM) {
        const int pt = e / ICP_FEATURE_BINS, b = e - pt * ICP_FEATURE_BINS;
        const int32_t to = map[pt];
        if (to >= 0) fd[(size_t)(c.dst_off + to) * ICP_FEATURE_BINS + b] = fs[e];
    }
}

hipError_t launch_batch_keypoint_select(const BatchKeypointArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0 || a.n_items <= 0) return hipSuccess;
    if (!a.clouds || !a.items || !a.rules || !a.sal || !a.map || !a.count) return hipErrorInvalidValue;
    if (a.precision == ICP_F64) {
        hipLaunchKernelGGL((batch_iss_saliency<double>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
        hipLaunchKernelGGL((batch_iss_select<double>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
    } else {
        hipLaunchKernelGGL((batch_iss_saliency<float>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
        hipLaunchKernelGGL((batch_iss_select<float>), dim3(a.n_items), dim3(NN_BLOCK), 0, st, a);
    }
    hipLaunchKernelGGL(batch_keypoint_rank, dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_keypoint_compact(const BatchKeypointArgs& a, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    for (int sd = 0; sd < 2; ++sd)
        if (!a.dst[sd] || (a.src_feat[sd] && !a.dst_feat[sd])) return hipErrorInvalidValue;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_keypoint_compact<double>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    else hipLaunchKernelGGL((batch_keypoint_compact<float>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    return hipGetLastError();
}

}  // namespace icp
