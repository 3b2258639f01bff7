// icp_device_batch.h -- device-side pieces shared by the batched neighbourhood kernels (icp_k_batch.hip, icp_k_gicp.hip,
// icp_k_color.hip, icp_k_feat.hip, icp_k_keypoint.hip, icp_k_normals.hip): the list behind the k-th smallest distance and the scan
// that fills it ("phase 1"), the block-wide walk over a cloud's tiles ("phase 2"), the neighbourhood sums behind a covariance, the
// cyclic Jacobi of icp_eigh3 with its range rule (a matrix beyond 2^+-400 is solved times an exact power of two, the eigenvalues
// scaled back; the Frobenius regularisation forms its norm the same way), the exclusive scan of keep flags, the copy of a kept point and the kept decision of a deferred step.
// ONE definition each: a kernel states what is its own -- its pointers, its per-chunk body, its closing arithmetic, its stores.
// Everything here is constexpr or __device__ __forceinline__, and rounds every operation on its own (icp_device.h turns contraction
// off).  Internal to libicp_mi355x.so.
#pragma once
#include "icp_device.h"
#include <math.h>

namespace icp {

// ------------------------------------------------------------------------------------------------
// constants and scalars
// ------------------------------------------------------------------------------------------------
template <typename F> struct BatchCfg;
template <> struct BatchCfg<float> { static constexpr int TW = 512; };    // points per wave and LDS sub-tile: 6 KiB per wave
template <> struct BatchCfg<double> { static constexpr int TW = 256; };
constexpr int KNN_CHUNK = 8;   // points per early-out chunk of the neighbourhood scans and walks

template <typename F> __device__ __forceinline__ F nan_();
template <> __device__ __forceinline__ float nan_<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double nan_<double>() { return __builtin_nan(""); }

// (x*a + y*b) + z*c, each operation rounded on its own
__device__ __forceinline__ double dot3(double x, double y, double z, double a, double b, double c) { return (x * a + y * b) + z * c; }
__device__ __forceinline__ bool finite_(double v) { return __builtin_fabs(v) < __builtin_huge_val(); }   // (NaN: false)
__device__ __forceinline__ bool finite_(float v) { return __builtin_fabsf(v) < __builtin_huge_valf(); }

// ------------------------------------------------------------------------------------------------
// the list of the k smallest distances: ascending in the TOP k of CAP registers, the slots below holding -inf, which nothing
// displaces -- bd[CAP - 1] is the k-th smallest at a compile-time index.  knn_insert puts d into the list, the largest entry
// falling off: bd[r] = median(bd[r-1], d, bd[r]) -- bd[r-1] where d lies below it, d where it lies between the two, bd[r] where
// it lies above -- from the top slot down, so that every step reads its lower neighbour as it was.  One v_med3_f32, or one max and
// one min in double, per slot: selections only, no branch, no predicate; equal values change nothing of the multiset.  d is never
// NaN here (+inf: the list is left as it is).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float med3(float lo, float d, float hi) { return __builtin_amdgcn_fmed3f(lo, d, hi); }
__device__ __forceinline__ double med3(double lo, double d, double hi) { return __builtin_fmin(hi, __builtin_fmax(lo, d)); }

template <typename F, int CAP>
__device__ __forceinline__ void knn_list_init(F (&bd)[CAP], int k)
{
#pragma unroll
    for (int r = 0; r < CAP; ++r) bd[r] = (r >= CAP - k) ? inf_<F>() : -inf_<F>();
}

template <typename F, int CAP>
__device__ __forceinline__ void knn_insert(F (&bd)[CAP], F d)
{
#pragma unroll
    for (int r = CAP - 1; r >= 1; --r) bd[r] = med3(bd[r - 1], d, bd[r]);
    bd[0] = fmin_(bd[0], d);
}

// ------------------------------------------------------------------------------------------------
// phase 1: one block of NN_BLOCK threads per work item, one query per lane, the same query in all four waves.  Wave w streams the
// w-th contiguous quarter of the query's own cloud (whole chunks of KNN_CHUNK points) through its own LDS sub-tile of TW points;
// every lane reads the same address, a broadcast.  The steps below are what every such scan is made of.
// ------------------------------------------------------------------------------------------------
struct WaveQuarter {
    int first, end;   // the wave's points [first, end): may be empty (end <= first)
    int ntile;        // sub-tiles per quarter: the same for every wave, so the barriers pair up
};
template <typename F>
__device__ __forceinline__ WaveQuarter wave_quarter(int n, int w)
{
    constexpr int C = KNN_CHUNK, TW = BatchCfg<F>::TW;
    const int wseg = ((n + 3) / 4 + C - 1) / C * C;   // points per wave, whole chunks
    return {w * wseg, min(w * wseg + wseg, n), (wseg + TW - 1) / TW};
}

// the wave's sub-tile from point t0 on, `pad` in the places past the quarter's end; extra(e, j, inside) fills place e of the
// caller's planes beside the coordinates (inside: j < end).  The caller puts a barrier before and after.
template <typename F, int W, typename Extra>
__device__ __forceinline__ void load_subtile(F (*sq)[W], const F* Sx, const F* Sy, const F* Sz, int t0, int end, F pad, Extra extra)
{
    for (int e = threadIdx.x & 63; e < W; e += 64) {
        const int j = t0 + e;
        F qx = pad, qy = pad, qz = pad;
        if (j < end) { qx = Sx[j]; qy = Sy[j]; qz = Sz[j]; }
        sq[0][e] = qx;
        sq[1][e] = qy;
        sq[2][e] = qz;
        extra(e, j, j < end);
    }
}
template <typename F, int W>
__device__ __forceinline__ void load_subtile(F (*sq)[W], const F* Sx, const F* Sy, const F* Sz, int t0, int end, F pad)
{
    load_subtile(sq, Sx, Sy, Sz, t0, end, pad, [](int, int, bool) {});
}

// the distances from (px, py, pz) of the chunk of KNN_CHUNK points at place cc of a tile, read as 16-byte vectors
template <typename F, int W>
__device__ __forceinline__ void chunk_dist2(const F (*tile)[W], int cc, F px, F py, F pz, F (&dd)[KNN_CHUNK])
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    static_assert(W % KNN_CHUNK == 0 && KNN_CHUNK % VN == 0, "whole chunks, whole vectors");
#pragma unroll
    for (int kk = 0; kk < KNN_CHUNK; kk += VN) {
        const V qx = *reinterpret_cast<const V*>(&tile[0][cc + kk]);
        const V qy = *reinterpret_cast<const V*>(&tile[1][cc + kk]);
        const V qz = *reinterpret_cast<const V*>(&tile[2][cc + kk]);
#pragma unroll
        for (int v = 0; v < VN; ++v) dd[kk + v] = dist2<F>(px, py, pz, vget(qx, v), vget(qy, v), vget(qz, v));
    }
}

// the chunk's distances dd, of the points j0 .. j0 + KNN_CHUNK - 1, into the list: the query itself (j == i, by index: a coincident
// point counts) is masked to +inf in the chunks that overlap the item, a wave-uniform test; the list is entered only where the
// chunk's minimum lies below some lane's k-th smallest, a wave-uniform test again.
template <typename F, int CAP>
__device__ __forceinline__ void knn_chunk(F (&bd)[CAP], F (&dd)[KNN_CHUNK], int j0, const BatchItem& it, int i)
{
    constexpr int C = KNN_CHUNK;
    if (j0 + C > it.first && j0 < it.first + BATCH_ITEM) {   // (wave-uniform) the chunk holds queries of this item: j != i
#pragma unroll
        for (int kk = 0; kk < C; ++kk) dd[kk] = (j0 + kk == i) ? inf_<F>() : dd[kk];
    }
    F cmin = inf_<F>();
#pragma unroll
    for (int kk = 0; kk < C; ++kk) cmin = fmin_(cmin, dd[kk]);
    if (__builtin_amdgcn_ballot_w64(cmin < bd[CAP - 1]) == 0ull) return;
#pragma unroll
    for (int kk = 0; kk < C; ++kk) knn_insert<F, CAP>(bd, dd[kk]);
}

// the four waves' lists into wave 0's: waves 1-3 leave theirs in LDS, over the sub-tiles (s_raw holds 3 x CAP x 64 values), and
// wave 0 inserts them into its own -- a multiset has one order.  The whole block calls this: two barriers, the first because every
// wave must have read its last sub-tile before the lists overwrite it.
template <typename F, int CAP>
__device__ __forceinline__ void knn_merge(unsigned char* s_raw, F (&bd)[CAP], int k)
{
    F(*ld)[CAP][BATCH_ITEM] = reinterpret_cast<F(*)[CAP][BATCH_ITEM]>(s_raw);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    __syncthreads();
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < CAP; ++r) ld[w - 1][r][lane] = bd[r];
    }
    __syncthreads();
    if (w != 0) return;
    for (int ww = 0; ww < 3; ++ww) {
#pragma unroll 1
        for (int s = CAP - k; s < CAP; ++s) {
            const F d = ld[ww][s][lane];
            if (__builtin_amdgcn_ballot_w64(d < bd[CAP - 1]) == 0ull) break;   // (ascending lists: no later entry of this wave's enters any lane's)
            knn_insert<F, CAP>(bd, d);
        }
    }
}

// tau_i = the k-th smallest d2(i, j) over j != i by index, of the cloud (Sx, Sy, Sz) of n >= k + 1 points: the list initialised to
// the top k of CAP, the four waves over their quarters (places past a quarter's end hold +inf: such a distance is +inf, never NaN,
// and enters no list), the merge.  s_raw: max(4 x 3 x TW, 3 x CAP x 64) values of F, 16-byte aligned.  The whole block calls this
// with the block's k; wave 0 gets tau_i, the others +inf.  The result depends on the cloud and k alone, not on CAP.
template <typename F, int CAP>
__device__ __forceinline__ F kth_distance(unsigned char* s_raw, const F* Sx, const F* Sy, const F* Sz, int n, int k, const BatchItem& it,
                                          int i, F px, F py, F pz)
{
    constexpr int TW = BatchCfg<F>::TW, C = KNN_CHUNK;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM && TW % C == 0, "one query per lane, four waves per item");
    F(*sq)[3][TW] = reinterpret_cast<F(*)[3][TW]>(s_raw);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const WaveQuarter q = wave_quarter<F>(n, w);
    F bd[CAP];
    knn_list_init<F, CAP>(bd, k);
    for (int t = 0; t < q.ntile; ++t) {
        const int t0 = q.first + t * TW;
        __syncthreads();
        load_subtile<F, TW>(sq[w], Sx, Sy, Sz, t0, q.end, inf_<F>());
        __syncthreads();
        const int len = min(TW, q.end - t0);   // <= 0: this wave's quarter is exhausted
        for (int cc = 0; cc < len; cc += C) {
            F dd[C];
            chunk_dist2<F, TW>(sq[w], cc, px, py, pz, dd);
            knn_chunk<F, CAP>(bd, dd, t0 + cc, it, i);
        }
    }
    knn_merge<F, CAP>(s_raw, bd, k);
    return w == 0 ? bd[CAP - 1] : inf_<F>();
}

// ------------------------------------------------------------------------------------------------
// phase 2: the block loads the cloud again, T2 points per tile, and wave 0 visits every tile's chunks in ascending j.
// ------------------------------------------------------------------------------------------------
// the block's tile from point t0 on, between two barriers -- the first also ends whatever read the bytes under the tile before (the
// tile before, phase 1's lists).  Places past the cloud's end hold NaN: such a distance passes no test.  extra(e, j, inside) fills
// place e of the caller's planes beside the coordinates (intensities, normals; inside: j < n).
template <typename F, int T2, typename Extra>
__device__ __forceinline__ void load_tile(F (*st)[T2], const F* Sx, const F* Sy, const F* Sz, int t0, int n, Extra extra)
{
    __syncthreads();
    for (int e = threadIdx.x; e < T2; e += NN_BLOCK) {
        const int j = t0 + e;
        F qx = nan_<F>(), qy = nan_<F>(), qz = nan_<F>();
        if (j < n) { qx = Sx[j]; qy = Sy[j]; qz = Sz[j]; }
        st[0][e] = qx;
        st[1][e] = qy;
        st[2][e] = qz;
        extra(e, j, j < n);
    }
    __syncthreads();
}
template <typename F, int T2>
__device__ __forceinline__ void load_tile(F (*st)[T2], const F* Sx, const F* Sy, const F* Sz, int t0, int n)
{
    load_tile<F, T2>(st, Sx, Sy, Sz, t0, n, [](int, int, bool) {});
}

// the walk of wave 0 with the chunk's points in registers: a chunk in which no lane accepts a point is skipped (wave-uniform); for
// the others body(cc, in, qq) runs once -- cc the chunk's place in the tile, in[kk] = accept(d2(i, j), j) for its kk-th point j,
// qq its coordinates.  One lane, one query, one running sum: a body that adds in ascending kk adds in ascending j whatever the
// cloud.  (batch_spfh_kernel and batch_fpfh_kernel walk load_tile's tiles themselves: their bodies read the points from the tile
// again in a rolled loop, and through this function they need registers beyond their waves-per-SIMD step.)
template <typename F, int T2, typename Extra, typename Accept, typename Body>
__device__ __forceinline__ void walk_tiles(F (*st)[T2], const F* Sx, const F* Sy, const F* Sz, int n, F px, F py, F pz, Extra extra,
                                           Accept accept, Body body)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int C = KNN_CHUNK;
    static_assert(T2 % C == 0 && C % VN == 0, "whole chunks, whole vectors");
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (n + T2 - 1) / T2;
    for (int t = 0; t < ntile; ++t) {
        const int t0 = t * T2;
        load_tile<F, T2>(st, Sx, Sy, Sz, t0, n, extra);
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
                    in[kk + v] = accept(dist2<F>(px, py, pz, qq[0][kk + v], qq[1][kk + v], qq[2][kk + v]), t0 + cc + kk + v);   // (NaN: false)
                    any = any || in[kk + v];
                }
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
            body(cc, in, qq);
        }
    }
}
template <typename F, int T2, typename Accept, typename Body>
__device__ __forceinline__ void walk_tiles(F (*st)[T2], const F* Sx, const F* Sy, const F* Sz, int n, F px, F py, F pz, Accept accept,
                                           Body body)
{
    walk_tiles<F, T2>(st, Sx, Sy, Sz, n, px, py, pz, [](int, int, bool) {}, accept, body);
}

// the sums over a neighbourhood behind its covariance: e = x_j - x_i (in double) into s, e e^T into S, the count.  Then
// C = (S - s s^T / c) / c, the upper triangle.
struct NeighbourSums {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, Sxx = 0.0, Sxy = 0.0, Sxz = 0.0, Syy = 0.0, Syz = 0.0, Szz = 0.0;
    int cnt = 0;
    __device__ __forceinline__ void add(double ex, double ey, double ez)
    {
        s0 += ex; s1 += ey; s2 += ez;
        Sxx += ex * ex; Sxy += ex * ey; Sxz += ex * ez;
        Syy += ey * ey; Syz += ey * ez; Szz += ez * ez;
        cnt += 1;
    }
    __device__ __forceinline__ void covariance(double& xx, double& xy, double& xz, double& yy, double& yz, double& zz) const
    {
        const double dc = (double)cnt;
        xx = (Sxx - (s0 * s0) / dc) / dc; xy = (Sxy - (s0 * s1) / dc) / dc; xz = (Sxz - (s0 * s2) / dc) / dc;
        yy = (Syy - (s1 * s1) / dc) / dc; yz = (Syz - (s1 * s2) / dc) / dc; zz = (Szz - (s2 * s2) / dc) / dc;
    }
};

// ------------------------------------------------------------------------------------------------
// icp_eigh3's cyclic Jacobi (icp_host_math.cpp) on named doubles -- no runtime-indexed array, no scratch.  The statements and their
// order are the host's, the range rule in front included.  The eigenvectors are formed with VECTORS alone.
// ------------------------------------------------------------------------------------------------
struct EigenVectors3 {   // v[row][column], the identity before the first sweep
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
};

// one rotation on the pair (p, q), r the remaining index: app = a[p][p], aqq = a[q][q], apq = a[p][q], arp = a[r][p],
// arq = a[r][q]; v0p .. v2p and v0q .. v2q are columns p and q of v
template <bool VECTORS>
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v1p,
                                              double& v2p, double& v0q, double& v1q, double& v2q)
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
    if constexpr (VECTORS) {
        const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
        v0p = c * a0 - s * b0;
        v0q = s * a0 + c * b0;
        v1p = c * a1 - s * b1;
        v1q = s * a1 + c * b1;
        v2p = c * a2 - s * b2;
        v2q = s * a2 + c * b2;
    }
}

// the range rule of icp_eigh3 and of the Frobenius regularisation: whatever squares the six entries of a symmetric matrix leaves the
// double range once they pass 2^+-400 (the Jacobi's stop test then sees off = inf or 0 and ends at once, with the identity for
// eigenvectors; the Frobenius norm is inf or 0).  With amax the largest magnitude of the six, amax > 2^400 multiplies them by 2^-600
// and 0 < amax < 2^-400 by 2^+600: an exact power of two, which changes no rotation and no quotient.  Returns the factor that
// scales an eigenvalue back (2^+600, 2^-600), 1.0 where the matrix is left as it is: amax within [2^-400, 2^400], amax == 0, and
// every matrix with an entry that is not finite -- those go through bit for bit.
__device__ __forceinline__ double range_scale6(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22)
{
    const double amax = fmax(fmax(fmax(fabs(a00), fabs(a01)), fmax(fabs(a02), fabs(a11))), fmax(fabs(a12), fabs(a22)));   // (fmax drops a NaN)
    if (!(amax > 0x1p+400 || (amax < 0x1p-400 && amax > 0.0))) return 1.0;
    if (!(finite_(a00) && finite_(a01) && finite_(a02) && finite_(a11) && finite_(a12) && finite_(a22))) return 1.0;
    const double sc = amax > 1.0 ? 0x1p-600 : 0x1p+600;
    a00 *= sc; a01 *= sc; a02 *= sc; a11 *= sc; a12 *= sc; a22 *= sc;
    return amax > 1.0 ? 0x1p+600 : 0x1p-600;
}

// the sweeps over (0,1), (0,2), (1,2), at most 64, every lane under its own stop test, on the matrix range_scale6 leaves: the
// eigenvalues are left on the diagonal, to be multiplied by the factor returned once their ascending order is fixed (the
// eigenvectors need nothing)
template <bool VECTORS>
__device__ __forceinline__ double jacobi_eigh3(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22, EigenVectors3& v)
{
    const double unscale = range_scale6(a00, a01, a02, a11, a12, a22);
#pragma unroll 1
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a01 * a01 + a02 * a02 + a12 * a12;
        const double dia = a00 * a00 + a11 * a11 + a22 * a22;
        if (off <= 1e-34 * dia || off == 0.0) break;
        jacobi_rotate<VECTORS>(a00, a11, a01, a02, a12, v.v00, v.v10, v.v20, v.v01, v.v11, v.v21);   // (0, 1), r = 2
        jacobi_rotate<VECTORS>(a00, a22, a02, a01, a12, v.v00, v.v10, v.v20, v.v02, v.v12, v.v22);   // (0, 2), r = 1
        jacobi_rotate<VECTORS>(a11, a22, a12, a01, a02, v.v01, v.v11, v.v21, v.v02, v.v12, v.v22);   // (1, 2), r = 0
    }
    return unscale;
}

// ------------------------------------------------------------------------------------------------
// ranks, copies, decisions
// ------------------------------------------------------------------------------------------------
// one block of VOXEL_SCAN_BLOCK threads: the exclusive scan of the flags flag(i) of the points 0 .. n-1, VOXEL_SCAN_BLOCK at a
// time with a running carry; store(i, flag, rank) gets the number of flagged points before i.  Returns the number of flagged
// points, in every thread.  s_wave: VOXEL_SCAN_BLOCK / 64 ints of LDS.  Ends on a barrier: what store wrote is the block's to read.
template <typename Flag, typename Store>
__device__ __forceinline__ int block_rank_flags(int n, int* s_wave, Flag flag, Store store)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += VOXEL_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const int f = i < n ? flag(i) : 0;
        int incl = f;
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
        if (i < n) store(i, f, carry + before + incl - f);
        carry += total;
        __syncthreads();   // (s_wave is rewritten by the next chunk)
    }
    return carry;
}

// a kept point's coordinates from the planes of its cloud to those of the new batch
template <typename F>
__device__ __forceinline__ void copy_kept_point(const F* S, long long sp, F* D, long long dp)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) D[k * dp] = S[k * sp];
}

// the decision of a deferred step for moving point `self` of its pair, matched at distance b to the model point at rev[qj]:
// kept = (tau == NULL || b <= tau[pair]) && (thr == NULL || b <= thr[pair]), and with MUTUAL (its own instantiations: the others
// never read rev or recip) && (recip[pair] == 0 || rev[qj] == self).  TAU_GIVEN: tau is read without the NULL test.  The caller
// gives a rejected point's idx entry BATCH_IDX_REJECTED.
template <typename F, bool MUTUAL, bool TAU_GIVEN = false>
__device__ __forceinline__ bool batch_kept(F b, int pair, const F* tau, const F* thr, const uint8_t* recip, const int32_t* rev, long long qj,
                                           int self)
{
    bool kept;
    if constexpr (TAU_GIVEN) kept = b <= tau[pair];
    else kept = tau == nullptr || b <= tau[pair];
    kept = kept && (thr == nullptr || b <= thr[pair]);
    if constexpr (MUTUAL) kept = kept && (recip[pair] == 0 || rev[qj] == self);
    return kept;
}

}  // namespace icp
