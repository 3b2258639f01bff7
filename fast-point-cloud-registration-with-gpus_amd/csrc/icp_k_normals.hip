// icp_k_normals.hip -- gfx950 kernels of the point normals of batched global registration (icp_batch_estimate_point_normals,
// icp_batch.cpp): every cloud's centroid (batch_centroid_kernel, for ICP_ORIENT_CENTROID alone) and every point's normal from its
// stored covariance (batch_point_normals_kernel).  The rule is stated in include/icp_mi355x.h and restated in numpy
// (tests/batch_normals_ref.py); every step here is one statement of it.  The Jacobi is icp_device_batch.h's, with its
// eigenvectors.  Contraction is off for this file: nothing is fused.
//
// Launches of one call: one (batch_point_normals_kernel, one wave per 64 points of every cloud of both sides), two with
// ICP_ORIENT_CENTROID (batch_centroid_kernel first, one block of CENTROID_BLOCK threads per cloud).  LDS per block: 6 KiB
// (centroid), none (normals).  No atomics of any kind.  Both kernels are latency-sized: a point costs nine loads, a few hundred
// dependent double operations and three stores.
#include "icp_device_batch.h"

namespace icp {

constexpr int CENTROID_BLOCK = 256;   // the rule's 256 partial sums per axis

// ------------------------------------------------------------------------------------------------
// centroid: one block of CENTROID_BLOCK threads per cloud.  Thread t adds the widened coordinates of the points t, t + 256, ... in
// registers, from 0.0; the three partial sums go to LDS; threads 0, 1 and 2 add the 256 partials of their axis in ascending t and
// divide by (double)n.  One thread, one running sum: the order is the rule's whatever the cloud.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(CENTROID_BLOCK) void batch_centroid_kernel(const BatchNormalsArgs a)
{
    __shared__ double part[3][CENTROID_BLOCK];
    const int cloud = blockIdx.x;
    const VoxelCloud c = a.clouds[cloud];
    const long long sp = a.src_plane[c.side];
    const F* Sx = static_cast<const F*>(a.src[c.side]) + c.src_off;
    const F* Sy = Sx + sp;
    const F* Sz = Sx + 2 * sp;
    const int n = c.n, t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = t; j < n; j += CENTROID_BLOCK) {
        s0 += (double)Sx[j];
        s1 += (double)Sy[j];
        s2 += (double)Sz[j];
    }
    part[0][t] = s0;
    part[1][t] = s1;
    part[2][t] = s2;
    __syncthreads();
    if (t >= 3) return;
    double total = 0.0;
#pragma unroll 8
    for (int k = 0; k < CENTROID_BLOCK; ++k) total += part[t][k];
    a.cent[(size_t)cloud * 3 + t] = total / (double)n;
}

// ------------------------------------------------------------------------------------------------
// normals: one wave per work item, one point per lane.  Six plane loads of the covariance and three of the coordinates, the Jacobi on
// six named doubles for a and nine for v (no runtime-indexed array, no scratch), every lane under its own stop test, the ascending
// order's three compare-and-swaps with the column carried along by selects, the finiteness test, the flip towards the cloud's
// viewpoint (a wave-uniform address: a.view holds three doubles per cloud, given or made by batch_centroid_kernel), three plane
// stores.  Lanes past the item's end repeat its first point and store nothing.
// ------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(BATCH_ITEM) void batch_point_normals_kernel(const BatchNormalsArgs a)
{
    static_assert(BATCH_ITEM == 64, "one point per lane");
    const BatchItem it = a.items[blockIdx.x];
    const VoxelCloud c = a.clouds[it.pair];
    const int lane = threadIdx.x;
    const bool live = lane < it.count;
    const int i = it.first + (live ? lane : 0);
    const long long sp = a.src_plane[c.side];
    const double* C = a.cov[c.side] + c.src_off + i;
    double a00 = C[0], a01 = C[sp], a02 = C[2 * sp], a11 = C[3 * sp], a12 = C[4 * sp], a22 = C[5 * sp];
    EigenVectors3 v;
    (void)jacobi_eigh3<true>(a00, a01, a02, a11, a12, a22, v);   // (the factor that scales the eigenvalues back: the order needs none)
    // ... its ascending order: three compare-and-swaps with the strict <, every column with its eigenvalue
    double w0 = a00, w1 = a11, w2 = a22;
    double nx = v.v00, ny = v.v10, nz = v.v20;     // column ord[0]
    double mx = v.v01, my = v.v11, mz = v.v21;     // column ord[1]
    double lx = v.v02, ly = v.v12, lz = v.v22;     // column ord[2]
    {
        const bool sw = w1 < w0;
        const double tw = w0, tx = nx, ty = ny, tz = nz;
        w0 = sw ? w1 : w0; nx = sw ? mx : nx; ny = sw ? my : ny; nz = sw ? mz : nz;
        w1 = sw ? tw : w1; mx = sw ? tx : mx; my = sw ? ty : my; mz = sw ? tz : mz;
    }
    {
        const bool sw = w2 < w0;
        const double tw = w0, tx = nx, ty = ny, tz = nz;
        w0 = sw ? w2 : w0; nx = sw ? lx : nx; ny = sw ? ly : ny; nz = sw ? lz : nz;
        w2 = sw ? tw : w2; lx = sw ? tx : lx; ly = sw ? ty : ly; lz = sw ? tz : lz;
    }
    {   // (ord[1] and ord[2]: the normal does not depend on them)
        const bool sw = w2 < w1;
        const double tw = w1;
        w1 = sw ? w2 : w1;
        w2 = sw ? tw : w2;
    }
    if (!(__builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz))) nx = ny = nz = 0.0;
    if (a.orient != ICP_ORIENT_NONE) {   // (the whole launch)
        const F* S = static_cast<const F*>(a.src[c.side]) + c.src_off + i;
        const double* view = a.view + (size_t)it.pair * 3;
        const double tox = view[0] - (double)S[0], toy = view[1] - (double)S[sp], toz = view[2] - (double)S[2 * sp];
        const double dt = (nx * tox + ny * toy) + nz * toz;
        if (dt < 0.0) { nx = -nx; ny = -ny; nz = -nz; }   // (dt == 0 and NaN keep the normal)
    }
    if (!live) return;
    double* N = a.nrm[c.side] + c.src_off + i;
    N[0] = nx;
    N[sp] = ny;
    N[2 * sp] = nz;
}

hipError_t launch_batch_point_normals(const BatchNormalsArgs& a, hipStream_t st)
{
    if (a.n_clouds <= 0 || a.n_items <= 0) return hipSuccess;
    if (!a.clouds || !a.items || !a.src[0] || !a.src[1] || !a.cov[0] || !a.cov[1] || !a.nrm[0] || !a.nrm[1]) return hipErrorInvalidValue;
    if (a.orient != ICP_ORIENT_NONE && !a.view) return hipErrorInvalidValue;
    if (a.orient == ICP_ORIENT_CENTROID) {
        if (!a.cent) return hipErrorInvalidValue;
        if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_centroid_kernel<double>), dim3(a.n_clouds), dim3(CENTROID_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((batch_centroid_kernel<float>), dim3(a.n_clouds), dim3(CENTROID_BLOCK), 0, st, a);
    }
    if (a.precision == ICP_F64) hipLaunchKernelGGL((batch_point_normals_kernel<double>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    else hipLaunchKernelGGL((batch_point_normals_kernel<float>), dim3(a.n_items), dim3(BATCH_ITEM), 0, st, a);
    return hipGetLastError();
}

}  // namespace icp
