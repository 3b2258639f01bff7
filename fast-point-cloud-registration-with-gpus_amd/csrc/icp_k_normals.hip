// icp_k_normals.hip -- gfx950 kernels of the point normals of batched global registration (icp_batch_estimate_point_normals,
// icp_batch.cpp): every cloud's centroid (batch_centroid_kernel, for ICP_ORIENT_CENTROID alone) and every point's normal from its
// stored covariance (batch_point_normals_kernel).  The rule is stated in include/icp_mi355x.h and restated in numpy
// (tests/batch_normals_ref.py); every step here is one statement of it.  icp_eigh3's Jacobi (icp_host_math.cpp) is restated in
// named scalars, its eigenvectors included -- batch_iss_saliency (icp_k_keypoint.hip) keeps its own restatement without them, and
// its listing.  Contraction is off for this file: nothing is fused.
//
// Launches of one call: one (batch_point_normals_kernel, one wave per 64 points of every cloud of both sides), two with
// ICP_ORIENT_CENTROID (batch_centroid_kernel first, one block of CENTROID_BLOCK threads per cloud).  LDS per block: 6 KiB
// (centroid), none (normals).  No atomics of any kind.  Both kernels are latency-sized: a point costs nine loads, a few hundred
// dependent double operations and three stores.
#include "icp_device.h"
#include <math.h>

namespace icp {

constexpr int CENTROID_BLOCK = 256;   // the rule's 256 partial sums per axis

// one rotation of icp_eigh3's sweep on the pair (p, q), r the remaining index: app = a[p][p], aqq = a[q][q], apq = a[p][q],
// arp = a[r][p], arq = a[r][q]; v0p .. v2p and v0q .. v2q are columns p and q of v.  The statements and their order are the host's.
__device__ __forceinline__ void nrm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                           double& v0p, double& v1p, double& v2p, double& v0q, double& v1q, double& v2q)
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
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0;
    v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1;
    v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2;
    v2q = s * a2 + c * b2;
}

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
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
    // icp_eigh3: cyclic Jacobi over (0,1), (0,2), (1,2), at most 64 sweeps
#pragma unroll 1
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a01 * a01 + a02 * a02 + a12 * a12;
        const double dia = a00 * a00 + a11 * a11 + a22 * a22;
        if (off <= 1e-34 * dia || off == 0.0) break;
        nrm_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);   // (0, 1), r = 2
        nrm_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);   // (0, 2), r = 1
        nrm_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);   // (1, 2), r = 0
    }
    // ... its ascending order: three compare-and-swaps with the strict <, every column with its eigenvalue
    double w0 = a00, w1 = a11, w2 = a22;
    double nx = v00, ny = v10, nz = v20;     // column ord[0]
    double mx = v01, my = v11, mz = v21;     // column ord[1]
    double lx = v02, ly = v12, lz = v22;     // column ord[2]
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
