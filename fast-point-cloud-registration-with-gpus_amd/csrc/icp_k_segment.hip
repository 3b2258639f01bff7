// icp_k_segment.hip -- gfx950 kernels of plane segmentation for a batch (icp_batch_segment_plane, icp_batch.cpp): the inlier counts
// of every cloud's plane hypotheses (batch_plane_score), the centroid and the centred second moments of the winner's inliers
// (batch_plane_refit), and the decision of every point with its rank in the new cloud (batch_plane_decide).  The rule is stated in
// include/icp_mi355x.h and restated in numpy (tests/batch_segment_ref.py); every step here is one statement of it.  The flag scan is
// icp_device_batch.h's; the compaction into the new batch is the outlier call's kernel (launch_batch_outlier_compact), whose
// arguments fit as they are.  Contraction is off for this file: nothing is fused, nothing is multiplied by a reciprocal.
//
// Launches of one call: one batch_plane_score per PLANE_CHUNK hypotheses (icp_batch.cpp), then batch_plane_refit, batch_plane_decide
// and the compaction.  LDS per block: batch_plane_score 512 bytes (the four waves' counts), batch_plane_refit 48 KiB (six granule
// sums of up to OUTLIER_MAX_GRANULES granules) + 24 bytes, batch_plane_decide 16 bytes.  The only atomics are integer adds of a
// block's counts into its cloud's (exact in any order); no floating-point atomics.
#include "icp_device_batch.h"

namespace icp {

// point i of a cloud lies on the plane (nx, ny, nz, d) iff fabs(((nx*x + ny*y) + nz*z) + d) <= dist, in double on the widened
// coordinates; a NaN is out
__device__ __forceinline__ bool on_plane(double nx, double ny, double nz, double d, double x, double y, double z, double dist)
{
    const double s = ((nx * x + ny * y) + nz * z) + d;
    return fabs(s) <= dist;
}

// ------------------------------------------------------------------------------------------------
// the counts: one block of NN_BLOCK threads per slice of PLANE_SLICE points of one cloud and per group of PLANE_GROUP hypotheses.
// The group's planes are read at an address that is uniform over the block (scalar loads); a lane walks its points, widened once,
// and keeps one integer per hypothesis; the wave adds its lanes' integers, the block its waves' in LDS, and one integer add per
// hypothesis brings the block's count into the cloud's.  A group without a valid hypothesis costs its blocks a few loads.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_plane_score(const BatchPlaneArgs a)
{
    constexpr int G = PLANE_GROUP;
    __shared__ int s_cnt[NN_BLOCK / 64][G];
    const BatchItem sl = a.slices[blockIdx.x];
    const size_t h0 = (size_t)sl.pair * a.per + (size_t)blockIdx.y * G;
    const uint8_t* __restrict__ valid = a.valid + h0;
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; ++g) any = any || valid[g] != 0;
    if (!any) return;   // (the whole block)
    const VoxelCloud c = a.clouds[sl.pair];
    const double dist = a.distance[sl.pair];
    const double* __restrict__ pl = a.planes + h0 * 4;
    const long long sp = a.src_plane[c.side];
    const F* __restrict__ Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* __restrict__ Sy = Sx + sp;
    const F* __restrict__ Sz = Sx + 2 * sp;
    const int end = sl.first + sl.count;
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) cnt[g] = 0;
    for (int i = sl.first + (int)threadIdx.x; i < end; i += NN_BLOCK) {
        const double x = (double)Sx[i], y = (double)Sy[i], z = (double)Sz[i];
#pragma unroll
        for (int g = 0; g < G; ++g) cnt[g] += on_plane(pl[4 * g], pl[4 * g + 1], pl[4 * g + 2], pl[4 * g + 3], x, y, z, dist) ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        int v = cnt[g];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) s_cnt[w][g] = v;
    }
    __syncthreads();
    if (threadIdx.x < G && valid[threadIdx.x]) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < NN_BLOCK / 64; ++k) total += s_cnt[k][threadIdx.x];
        if (total) atomicAdd(&a.counts[h0 + threadIdx.x], total);
    }
}

// ------------------------------------------------------------------------------------------------
// the refit's sums: one block per cloud.  Granules of 64 consecutive points from the cloud's first point, one thread per granule:
// the coordinates of the winner's inliers added from 0.0 in ascending index; the granule sums added from 0.0 in ascending order (one
// thread per axis); c = S / (double)k; then the six centred products the same way, each sum divided once by (double)k.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_plane_refit(const BatchPlaneArgs a)
{
    __shared__ double s_g[6][OUTLIER_MAX_GRANULES];
    __shared__ double s_c[3];
    const int cloud = blockIdx.x;
    const PlaneJob job = a.jobs[cloud];
    double* out = a.moments + 9 * (size_t)cloud;
    if (job.kind == ICP_PLANE_NONE || !job.has_plane || job.win_count < 3) {   // (the whole block) nothing to refit
        if (threadIdx.x < 9) out[threadIdx.x] = 0.0;
        return;
    }
    const VoxelCloud c = a.clouds[cloud];
    const long long sp = a.src_plane[c.side];
    const F* __restrict__ Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* __restrict__ Sy = Sx + sp;
    const F* __restrict__ Sz = Sx + 2 * sp;
    const int n = c.n;
    const int ng = (n + BATCH_ITEM - 1) / BATCH_ITEM;   // <= OUTLIER_MAX_GRANULES
    const double k = (double)job.win_count;
    const double nx = job.win[0], ny = job.win[1], nz = job.win[2], d = job.win[3], dist = job.distance;
    for (int g = threadIdx.x; g < ng; g += VOXEL_SCAN_BLOCK) {
        const int i1 = min(n, (g + 1) * BATCH_ITEM);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int i = g * BATCH_ITEM; i < i1; ++i) {
            const double x = (double)Sx[i], y = (double)Sy[i], z = (double)Sz[i];
            if (!on_plane(nx, ny, nz, d, x, y, z, dist)) continue;
            sx += x;
            sy += y;
            sz += z;
        }
        s_g[0][g] = sx;
        s_g[1][g] = sy;
        s_g[2][g] = sz;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double S = 0.0;
        for (int g = 0; g < ng; ++g) S += s_g[threadIdx.x][g];
        s_c[threadIdx.x] = S / k;
    }
    __syncthreads();
    const double cx = s_c[0], cy = s_c[1], cz = s_c[2];
    for (int g = threadIdx.x; g < ng; g += VOXEL_SCAN_BLOCK) {
        const int i1 = min(n, (g + 1) * BATCH_ITEM);
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0, q5 = 0.0;
        for (int i = g * BATCH_ITEM; i < i1; ++i) {
            const double x = (double)Sx[i], y = (double)Sy[i], z = (double)Sz[i];
            if (!on_plane(nx, ny, nz, d, x, y, z, dist)) continue;
            const double ex = x - cx, ey = y - cy, ez = z - cz;
            const double xx = ex * ex, xy = ex * ey, xz = ex * ez, yy = ey * ey, yz = ey * ez, zz = ez * ez;
            q0 += xx;
            q1 += xy;
            q2 += xz;
            q3 += yy;
            q4 += yz;
            q5 += zz;
        }
        s_g[0][g] = q0;
        s_g[1][g] = q1;
        s_g[2][g] = q2;
        s_g[3][g] = q3;
        s_g[4][g] = q4;
        s_g[5][g] = q5;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double Q = 0.0;
        for (int g = 0; g < ng; ++g) Q += s_g[threadIdx.x][g];
        out[3 + threadIdx.x] = Q / k;
    }
    if (threadIdx.x < 3) out[threadIdx.x] = s_c[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------
// the decision: one block per cloud.  The refit, where there is one, is counted and returned if its count is at least the winner's;
// mask[i] = point i lies on the returned plane; the keep flags by kind (DETECT: all, REMOVE: the points off the plane, KEEP: those
// on it), their exclusive scan, map, count.  A cloud without a plane -- not searched, or no valid hypothesis -- has an all-zero mask
// and is copied; under KEEP it keeps nothing and the host refuses the call.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void batch_plane_decide(const BatchPlaneArgs a)
{
    __shared__ int s_wave[VOXEL_SCAN_BLOCK / 64];
    const int cloud = blockIdx.x;
    const PlaneJob job = a.jobs[cloud];
    const VoxelCloud c = a.clouds[cloud];
    int32_t* map = a.map + c.tmp_off;
    uint8_t* mask = a.mask + c.tmp_off;
    const int n = c.n;
    if (job.kind == ICP_PLANE_NONE || !job.has_plane) {   // (the whole block)
        const bool keep = job.kind != ICP_PLANE_KEEP;
        for (int i = threadIdx.x; i < n; i += VOXEL_SCAN_BLOCK) {
            mask[i] = 0;
            map[i] = keep ? i : -1;
        }
        if (threadIdx.x == 0) {
            a.count[cloud] = keep ? n : 0;
            a.inliers[cloud] = 0;
            a.chosen[cloud] = -1;
        }
        return;
    }
    const long long sp = a.src_plane[c.side];
    const F* __restrict__ Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* __restrict__ Sy = Sx + sp;
    const F* __restrict__ Sz = Sx + 2 * sp;
    const double dist = job.distance;
    double nx = job.win[0], ny = job.win[1], nz = job.win[2], d = job.win[3];
    int inl = job.win_count, chosen = 0;
    if (job.fit_ok) {
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += VOXEL_SCAN_BLOCK)
            mine += on_plane(job.fit[0], job.fit[1], job.fit[2], job.fit[3], (double)Sx[i], (double)Sy[i], (double)Sz[i], dist) ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int w = 0; w < VOXEL_SCAN_BLOCK / 64; ++w) total += s_wave[w];
        __syncthreads();   // (s_wave is rewritten by the scan)
        if (total >= job.win_count) {
            nx = job.fit[0], ny = job.fit[1], nz = job.fit[2], d = job.fit[3];
            inl = total;
            chosen = 1;
        }
    }
    const int kind = job.kind;
    const int kept = block_rank_flags(
        n, s_wave,
        [&](int i) {
            const int in = on_plane(nx, ny, nz, d, (double)Sx[i], (double)Sy[i], (double)Sz[i], dist) ? 1 : 0;
            mask[i] = (uint8_t)in;
            return kind == ICP_PLANE_DETECT ? 1 : kind == ICP_PLANE_REMOVE ? 1 - in : in;
        },
        [&](int i, int flag, int rank) { map[i] = flag ? rank : -1; });
    if (threadIdx.x == 0) {
        a.count[cloud] = kept;
        a.inliers[cloud] = inl;
        a.chosen[cloud] = chosen;
    }
}

hipError_t launch_batch_plane_score(const BatchPlaneArgs& a, hipStream_t st)
{
    if (a.n_slices <= 0 || a.per <= 0) return hipSuccess;
    if (a.per % PLANE_GROUP != 0 || !a.slices || !a.clouds || !a.planes || !a.valid || !a.distance || !a.counts) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_slices, (unsigned)(a.per / PLANE_GROUP));
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_plane_score<double>), grid, dim3(NN_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((batch_plane_score<float>), grid, dim3(NN_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_plane_refit(const BatchPlaneArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0) return hipSuccess;
    if (!a.clouds || !a.jobs || !a.moments) return hipErrorInvalidValue;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_plane_refit<double>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((batch_plane_refit<float>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_plane_decide(const BatchPlaneArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0) return hipSuccess;
    if (!a.clouds || !a.jobs || !a.map || !a.count || !a.mask || !a.inliers || !a.chosen) return hipErrorInvalidValue;
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_plane_decide<double>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((batch_plane_decide<float>), dim3(a.n_clouds), dim3(VOXEL_SCAN_BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace icp
