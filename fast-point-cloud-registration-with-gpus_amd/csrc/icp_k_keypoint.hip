// icp_k_keypoint.hip -- gfx950 kernels of keypoint selection for batched global registration (icp_batch_select_keypoints,
// icp_batch.cpp): the ISS saliency of every point of every cloud of a batch (batch_iss_saliency), the non-maximum suppression
// (batch_iss_select), the ranks of the kept points (batch_keypoint_rank) and the compaction of their coordinates and descriptors
// into a new batch (batch_keypoint_compact).  The rule is stated in include/icp_mi355x.h and restated in numpy
// (tests/batch_keypoint_ref.py); every step here is one statement of it.  The walk, the neighbourhood sums, the Jacobi, the quarter
// loader, the flag scan and the point copy are icp_device_batch.h's.  Contraction is off for this file: nothing is fused.
//
// Launches of one call: four -- batch_iss_saliency and batch_iss_select (one block of NN_BLOCK threads per 64 points of every
// cloud), batch_keypoint_rank (one block of VOXEL_SCAN_BLOCK threads per cloud), batch_keypoint_compact (one wave per 64 points).
// LDS per block: batch_iss_saliency 3 x 4 x TW x sizeof(F) = 24 KiB (one tile of the block); batch_iss_select 4 sub-tiles of
// 3 x TW x sizeof(F) + TW x 8 bytes (coordinates and saliencies) = 40 KiB fp32, 32 KiB fp64, plus 2 KiB for the waves' counts and
// flags; batch_keypoint_rank 16 bytes; batch_keypoint_compact none.  No atomics of any kind.
#include "icp_device_batch.h"

namespace icp {

// ------------------------------------------------------------------------------------------------
// ISS saliency: one block of NN_BLOCK threads per work item, one query per lane -- batch_cov_kernel's phase 2 with the fixed
// threshold ts = (F)(salient_radius * salient_radius) in tau's place.  Then the covariance, the Jacobi without eigenvectors, the
// ascending order, the four tests, and one store of sal.  A copied cloud (ICP_KEYPOINT_NONE) gets 0.0.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_iss_saliency(const BatchKeypointArgs a)
{
    constexpr int C = KNN_CHUNK, T2 = 4 * BatchCfg<F>::TW;
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
    const double rs2 = rule.salient_radius * rule.salient_radius;
    const F ts = (F)rs2;   // the product formed in double and rounded once (the gate's rule)

    const double xi = (double)px, yi = (double)py, zi = (double)pz;
    NeighbourSums sums;
    walk_tiles<F, T2>(
        st, Sx, Sy, Sz, c.n, px, py, pz, [&](F d, int) { return d <= ts; },
        [&](int, const bool(&in)[C], const F(&qq)[3][C]) {
#pragma unroll
            for (int kk = 0; kk < C; ++kk)
                if (in[kk]) sums.add((double)qq[0][kk] - xi, (double)qq[1][kk] - yi, (double)qq[2][kk] - zi);
        });
    if (w != 0 || !live) return;
    double a00, a01, a02, a11, a12, a22;
    sums.covariance(a00, a01, a02, a11, a12, a22);
    EigenVectors3 none;
    const double unscale = jacobi_eigh3<false>(a00, a01, a02, a11, a12, a22, none);
    double w0 = a00, w1 = a11, w2 = a22, tmp;   // ... and its ascending order: three compare-and-swaps
    if (w1 < w0) { tmp = w0; w0 = w1; w1 = tmp; }
    if (w2 < w0) { tmp = w0; w0 = w2; w2 = tmp; }
    if (w2 < w1) { tmp = w1; w1 = w2; w2 = tmp; }
    w0 *= unscale; w1 *= unscale; w2 *= unscale;   // (the range rule: 1.0 for every matrix within 2^+-400)
    const bool salient = sums.cnt >= rule.min_neighbours && (w1 / w2) < rule.gamma_21 && (w0 / w1) < rule.gamma_32 && w0 > 0.0;   // (NaN fails each)
    sal[i] = salient ? w0 : 0.0;
}

// ------------------------------------------------------------------------------------------------
// non-maximum suppression: the same items, one query per lane.  |M_i| and "some j of M_i has sal_j > sal_i" are an integer count and a
// comparison -- no summation order -- so the four waves stream their quarters of the query's own cloud through their own LDS
// sub-tiles (phase 1's loader, the saliencies beside the coordinates), leave their count and flag in LDS, and wave 0 combines them:
// flag = sal_i > 0 && |M_i| >= min_neighbours && no higher saliency within tn.  The flag goes into map (1 / 0), which
// batch_keypoint_rank turns into ranks.  Places past a quarter's end hold NaN.  A copied cloud is left to the rank.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_iss_select(const BatchKeypointArgs a)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK;
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
    const double rn2 = rule.non_max_radius * rule.non_max_radius;
    const F tn = (F)rn2;

    const WaveQuarter q = wave_quarter<F>(c.n, w);
    int cnt = 0, gt = 0;
    for (int t = 0; t < q.ntile; ++t) {
        const int t0 = q.first + t * TW;
        __syncthreads();
        load_subtile<F, TW>(sq[w], Sx, Sy, Sz, t0, q.end, nan_<F>(), [&](int e, int j, bool inside) { ss[w][e] = inside ? sal[j] : 0.0; });
        __syncthreads();
        const int len = min(TW, q.end - t0);   // <= 0: this wave's quarter is exhausted
        for (int cc = 0; cc < len; cc += C) {
            F dd[C];
            chunk_dist2<F, TW>(sq[w], cc, px, py, pz, dd);
            bool any = false;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) any = any || dd[kk] <= tn;   // (NaN: false)
            if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) {
                const double sj = ss[w][cc + kk];
                const bool in = dd[kk] <= tn;
                cnt += in ? 1 : 0;
                gt |= (in && sj > si) ? 1 : 0;
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

// one block per cloud: the flags batch_iss_select left in map become the index of a kept point in its new cloud, -1 otherwise;
// a copied cloud gets 0 .. n-1; count[cloud] = the kept points.
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
    const int kept = block_rank_flags(n, s_wave, [=](int i) { return map[i]; }, [=](int i, int flag, int rank) { map[i] = flag ? rank : -1; });
    if (threadIdx.x == 0) a.count[cloud] = kept;
}

// one wave per work item: a kept point's coordinates go to the new batch's planes at dst_off + map, and, where the source holds
// descriptors on the cloud's side, its ICP_FEATURE_BINS doubles go to the new batch's descriptors at
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
        if (to >= 0)
            copy_kept_point<F>(static_cast<const F*>(a.src[c.side]) + c.src_off + it.first + lane, a.src_plane[c.side],
                               static_cast<F*>(a.dst[c.side]) + c.dst_off + to, a.dst_plane[c.side]);
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
