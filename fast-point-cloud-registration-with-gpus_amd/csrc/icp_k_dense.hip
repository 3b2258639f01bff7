// icp_k_dense.hip -- gfx950 kernels that touch every point or every pair: layout conversion, the dense matching kernels (generic
// thread-per-point: fp64 fallback; packed fp32 v2: fallback + roofline reference), merge, fused moments, transform + error,
// finalize.  Reference statements: nn_match_* Matching<<<>>> src/CUDA/GPU_point_to_point_real.cu:38-79 / src/ICP_CPU.c:220-234;
// moments_kernel src/ICP_point_to_point.cu:308-357, src/CUDA/GPU_point_to_plane_real.cu:246-288,532-549; transform_error_kernel
// src/ICP_point_to_point.cu:81-88,403-416.
#include "icp_device.h"
#include <math.h>
#include <stdlib.h>
#include <cstring>

namespace icp {

// ------------------------------------------------------------------------------------------------
// layout conversion
// ------------------------------------------------------------------------------------------------
// `nonfinite` (pinned host memory, or NULL): counts the points with a NaN or an infinite coordinate -- icp_set_* refuse such a
// cloud (include/icp_mi355x.h).  Written only when there is something to count.
template <typename F>
__global__ void aos_to_soa_kernel(const F* __restrict__ aos, int n, int n_pad, F* __restrict__ soa, unsigned int* nonfinite, F* __restrict__ soa2, unsigned int* __restrict__ enc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n_pad;
    const int s = i < n ? i : n - 1;  // padding replicates the last real point
    F x = F(0), y = F(0), z = F(0);
    // the block's 256 points are 768 contiguous values: fetched as 16-byte vectors, coalesced (the source may be pinned HOST memory read
    // over PCIe -- the short set-up -- where three strided 4-byte loads per thread were 15 us for 196 KB), handed out through LDS; a block
    // that reaches beyond the cloud (its tail, the padding) reads its points one by one
    __shared__ __attribute__((aligned(16))) F buf[768];
    const size_t b0 = (size_t)blockIdx.x * 256;
    const bool whole = b0 + 256 <= (size_t)n;
    if (whole) {
        constexpr int PER = 16 / (int)sizeof(F), NV = 768 / PER;
        using V = typename Vec16<F>::type;
        const V* src = reinterpret_cast<const V*>(aos + 3 * b0);
        for (int k = threadIdx.x; k < NV; k += 256) reinterpret_cast<V*>(buf)[k] = src[k];
    }
    __syncthreads();
    if (in) {
        if (whole) { x = buf[3 * threadIdx.x]; y = buf[3 * threadIdx.x + 1]; z = buf[3 * threadIdx.x + 2]; }
        else { x = aos[3 * (size_t)s + 0]; y = aos[3 * (size_t)s + 1]; z = aos[3 * (size_t)s + 2]; }
        soa[i] = x;
        soa[(size_t)n_pad + i] = y;
        soa[2 * (size_t)n_pad + i] = z;
        if (soa2 != nullptr) { soa2[i] = x; soa2[(size_t)n_pad + i] = y; soa2[2 * (size_t)n_pad + i] = z; }
    }
    // (x - x is 0 for every finite x, NaN for NaN and for +-inf)
    const bool finite = (x - x) == F(0) && (y - y) == F(0) && (z - z) == F(0);
    if (in && nonfinite != nullptr && i < n && !finite)
        __hip_atomic_fetch_add(nonfinite, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if constexpr (sizeof(F) == 4) {
        // the bounding cube of the finite points, for the spatial order: a wave's minima and maxima, then six ordered-integer atomics
        if (enc != nullptr) {
            const bool use = in && i < n && finite;
            const float binf = __builtin_huge_valf();
            float lo[3] = {use ? (float)x : binf, use ? (float)y : binf, use ? (float)z : binf};
            float hi[3] = {use ? (float)x : -binf, use ? (float)y : -binf, use ? (float)z : -binf};
#pragma unroll
            for (int a = 0; a < 3; ++a)
                for (int off = 32; off > 0; off >>= 1) {
                    lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off, 64));
                    hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
                }
            if ((threadIdx.x & 63) == 0 && hi[0] >= lo[0]) {
                auto ord = [](float f) { const unsigned int b = __float_as_uint(f == 0.f ? 0.f : f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); };
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    atomicMax(&enc[a], ~ord(lo[a]));
                    atomicMax(&enc[3 + a], ord(hi[a]));
                }
            }
        }
    }
}

template <typename F>
__global__ void soa_to_aos_kernel(const F* __restrict__ soa, int n, int n_pad, F* __restrict__ aos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aos[3 * (size_t)i + 0] = soa[i];
    aos[3 * (size_t)i + 1] = soa[(size_t)n_pad + i];
    aos[3 * (size_t)i + 2] = soa[2 * (size_t)n_pad + i];
}

// ------------------------------------------------------------------------------------------------
// matching
//
// grid = (n_pad / (256*T), S).  A block owns 256*T moving points (T per lane, in registers) and one
// segment [q0, q1) of the model.  The segment streams through LDS in SoA tiles; every lane reads the
// SAME LDS address (broadcast, conflict-free), 16 bytes per ds_read.
//
// The inner loop keeps only the running MINIMUM per moving point (8 rounding-exact VALU ops per
// pair + a min), not the arg-min: per NN_CHUNK model points one compare records the id of the
// chunk that last lowered the minimum.  Because the compare is strict, that is the FIRST chunk
// holding the final minimum; the index is recovered afterwards by re-evaluating just that chunk
// (16 pairs per moving point) and taking the lowest j with d_j == min.  Same answer as the
// reference's ascending strict-< scan, ~25% fewer VALU ops per pair.
// ------------------------------------------------------------------------------------------------
template <typename F, int T, int TQ>
__global__ __launch_bounds__(NN_BLOCK) void nn_match_kernel(const F* __restrict__ P, int n_pad,
                                                            const F* __restrict__ Q, int m_pad, int seg_len,
                                                            F* __restrict__ part_d, int32_t* __restrict__ part_idx)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int C = NN_CHUNK;
    __shared__ __attribute__((aligned(16))) F sq[3 * TQ];

    const int q0 = blockIdx.y * seg_len;
    const int q1 = min(q0 + seg_len, m_pad);
    const int ibase = blockIdx.x * (NN_BLOCK * T) + threadIdx.x;

    F px[T], py[T], pz[T], best[T];
    int cst[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = ibase + t * NN_BLOCK;
        px[t] = P[i];
        py[t] = P[(size_t)n_pad + i];
        pz[t] = P[2 * (size_t)n_pad + i];
        best[t] = inf_<F>();
        cst[t] = q0 / C;
    }

    for (int tile = q0; tile < q1; tile += TQ) {
        const int len = min(TQ, q1 - tile);  // multiple of C
        __syncthreads();
        for (int e = threadIdx.x * VN; e < len; e += NN_BLOCK * VN) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
                *reinterpret_cast<V*>(&sq[a * TQ + e]) =
                    *reinterpret_cast<const V*>(&Q[(size_t)a * m_pad + tile + e]);
        }
        __syncthreads();

        for (int c = 0; c < len; c += C) {
            F bo[T];
#pragma unroll
            for (int t = 0; t < T; ++t) bo[t] = best[t];
#pragma unroll
            for (int k = 0; k < C; k += VN) {
                const V qx = *reinterpret_cast<const V*>(&sq[c + k]);
                const V qy = *reinterpret_cast<const V*>(&sq[TQ + c + k]);
                const V qz = *reinterpret_cast<const V*>(&sq[2 * TQ + c + k]);
#pragma unroll
                for (int v = 0; v < VN; ++v) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const F d = dist2<F>(px[t], py[t], pz[t], vget(qx, v), vget(qy, v), vget(qz, v));
                        best[t] = fmin_(best[t], d);
                    }
                }
            }
            const int cid = (tile + c) / C;
#pragma unroll
            for (int t = 0; t < T; ++t) cst[t] = (best[t] < bo[t]) ? cid : cst[t];
        }
    }

    // index recovery inside the winning chunk (global memory, L2-resident)
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int base = cst[t] * C;
        int idx = base;
        const F b = best[t];
        for (int k = C - 1; k >= 0; --k) {
            const int j = base + k;
            const F d = dist2<F>(px[t], py[t], pz[t], Q[j], Q[(size_t)m_pad + j], Q[2 * (size_t)m_pad + j]);
            idx = (d == b) ? j : idx;
        }
        const size_t o = (size_t)blockIdx.y * n_pad + ibase + t * NN_BLOCK;
        part_d[o] = b;
        part_idx[o] = idx;
    }
}

// ------------------------------------------------------------------------------------------------
// matching, fp32, v2 -- the shipped fp32 kernel.
//
// What the gfx950 VALU probe (profiles/r1/valu_rate_gfx950.txt) says and how the kernel answers:
//   * one wave issues a VALU instruction only every ~6 cycles whatever its ILP; a SIMD saturates
//     at ~8 resident waves  -> <= 64 VGPRs (launch_bounds(256, 8)), 16 KB LDS per block;
//   * v_pk_add/mul_f32 retire 2 results per issue slot (70 T results/s vs 51 T for plain ops)
//     -> every sub/mul/add of the distance is a packed op over TWO MOVING POINTS of the lane; the
//     model coordinate is broadcast into both halves with op_sel straight from the LDS quad,
//     no v_mov.  Each half is an ordinary IEEE add/mul, so rounding is identical to the scalar form;
//   * v_cndmask (VCC read) costs ~9 issue slots -> the chunk-id update sits behind a wave-uniform
//     branch that is skipped while no lane's minimum moved.
// Small clouds cannot fill 8 waves x 1024 SIMDs along the moving axis, so the model range is split
// twice: grid.y segments (merged later from the partials) and, inside a block, one contiguous
// quarter of the segment per wave (merged through LDS in ascending order, strict <, so the lowest
// index still wins).  All four waves of a block own the SAME 64*T moving points.
// ------------------------------------------------------------------------------------------------

template <int T /*2 or 4*/, int C /*chunk: 8 or 16*/, int CULL /*0: plain; 1: seeded bound + box/xy early-out over LDS tiles*/, int TAIL = 0>
__global__ __launch_bounds__(NN_BLOCK, (T == 2 ? 8 : 4)) void nn_match_f32_v2(const float* __restrict__ P, int n_pad,
                                                               const float* __restrict__ Q, int m_pad, int seg_len,
                                                               float* __restrict__ part_d,
                                                               int32_t* __restrict__ part_idx, RT<float> rt,
                                                               NNFuse fuse, NNTail tail)
{
    constexpr int TP = T / 2;  // packed pairs of moving points per lane
    // one raw LDS block, carved by hand: the tail's transpose buffer overlays the tile + merge scratch
    constexpr int SQ_BYTES = 4 * 3 * NN2_TQW * 4, MD_BYTES = 4 * 64 * T * 4;
    constexpr int TR_BYTES = TAIL ? (TAIL == 2 ? 28 : 18) * 65 * 8 : 0;
    constexpr int LDS_BYTES = (SQ_BYTES + 2 * MD_BYTES + 16) > TR_BYTES ? (SQ_BYTES + 2 * MD_BYTES + 16) : TR_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    float (*sq)[3][NN2_TQW] = reinterpret_cast<float (*)[3][NN2_TQW]>(lds_raw);
    float (*md)[64 * T] = reinterpret_cast<float (*)[64 * T]>(lds_raw + SQ_BYTES);
    int (*mi)[64 * T] = reinterpret_cast<int (*)[64 * T]>(lds_raw + SQ_BYTES + MD_BYTES);
    int* s_flag = reinterpret_cast<int*>(lds_raw + SQ_BYTES + 2 * MD_BYTES);

    const int lane = threadIdx.x & 63;
    // the wave id as a SCALAR: everything derived from it (ranges, loop bounds, the box addresses) then lives in
    // SGPRs, the loops are scalar loops and the per-chunk boxes arrive through the scalar cache
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int phase_pass_ = 0, phase_nw_ = 4;  // (phase log)
    constexpr bool phase_diag_ = true;
    const int wseg = seg_len >> 2;              // model points per wave (multiple of C)
    const int q0 = blockIdx.y * seg_len;
    const int my0 = q0 + w * wseg;
    const int my1 = min(my0 + wseg, m_pad);     // may be <= my0: this wave's range is empty
    const int ibase = blockIdx.x * (64 * T) + lane;

    f2 px[TP], py[TP], pz[TP];
    float best[T];
    int cst[T];
    ICP_PHASE(0)
#pragma unroll
    for (int u = 0; u < TP; ++u) {
        const int i0 = ibase + (2 * u) * 64, i1 = i0 + 64;
        px[u] = f2{P[i0], P[i1]};
        py[u] = f2{P[(size_t)n_pad + i0], P[(size_t)n_pad + i1]};
        pz[u] = f2{P[2 * (size_t)n_pad + i0], P[2 * (size_t)n_pad + i1]};
    }
    if (fuse.apply) {
        // every block re-derives the moved points in registers (same instructions => same bits);
        // the grid.y == 0 row stores them and accounts the error of the pass that produced (R, t)
        double err = 0.0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int u = t >> 1;
            float x = (t & 1) ? px[u].y : px[u].x, y = (t & 1) ? py[u].y : py[u].x, z = (t & 1) ? pz[u].y : pz[u].x;
            apply_rt<float>(rt, x, y, z, x, y, z);
            if (t & 1) { px[u].y = x; py[u].y = y; pz[u].y = z; } else { px[u].x = x; py[u].x = y; pz[u].x = z; }
            if (blockIdx.y == 0 && w == 0) {
                const int i = ibase + t * 64;
                fuse.P_out[i] = x;
                fuse.P_out[(size_t)n_pad + i] = y;
                fuse.P_out[2 * (size_t)n_pad + i] = z;
                if (i < fuse.n) {
                    const int j = fuse.idx_prev[i];
                    const float* Qg = fuse.Q_gather;
                    const double ex = (double)Qg[j] - (double)x;
                    const double ey = (double)Qg[(size_t)m_pad + j] - (double)y;
                    const double ez = (double)Qg[2 * (size_t)m_pad + j] - (double)z;
                    err += ex * ex + ey * ey + ez * ez;
                }
            }
        }
        if (blockIdx.y == 0 && w == 0) {
            err = wave_sum(err);
            if (lane == 0) {
                if constexpr (TAIL != 0)  // read by whichever block closes this row: agent-scope store, drained before our ticket
                    __hip_atomic_store(&tail.err_tile[blockIdx.x], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    fuse.err_rows[blockIdx.x] = err;
            }
        }
    }
    ICP_PHASE(1)
#pragma unroll
    for (int t = 0; t < T; ++t) { best[t] = inf_<float>(); cst[t] = -1; }
    if constexpr (CULL) {
        // Seeded bound: start from the distance to ANY model point (last pass's match) bumped by one ulp.
        // The true minimum is <= that distance < bound, so the ordinary ascending strict-< scan still ends
        // on the first index of the minimum -- the seed changes how much work is skipped, never the answer.
        if (fuse.seed_idx) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int u = t >> 1;
                const float x = (t & 1) ? px[u].y : px[u].x, y = (t & 1) ? py[u].y : py[u].x, z = (t & 1) ? pz[u].y : pz[u].x;
                // padding lanes (i >= n) have no previous match, and a seed is trusted only if it is a
                // real model index: anything else simply starts unbounded
                const int i = ibase + t * 64;
                int j = (i < fuse.n) ? fuse.seed_idx[i] : -1;
                const bool ok = (unsigned)j < (unsigned)fuse.m;
                j = ok ? j : 0;
                const float* Qg = fuse.Q_gather;
                const float d = dist2<float>(x, y, z, Qg[j], Qg[(size_t)m_pad + j], Qg[2 * (size_t)m_pad + j]);
                // next float above d (d >= 0, finite): bit pattern + 1; inf stays inf
                best[t] = (ok && d < inf_<float>()) ? __uint_as_float(__float_as_uint(d) + 1u) : inf_<float>();
                // padding lanes can never improve on a bound of zero: they cost no chunk visits (their result,
                // "nothing found", is never read)
                best[t] = (i < fuse.n) ? best[t] : 0.f;
            }
        }
    }

    ICP_PHASE(2)
    {
    const int ntile = (wseg + NN2_TQW - 1) / NN2_TQW;
    for (int k = 0; k < ntile; ++k) {
        __syncthreads();
        // cooperative fill of the four per-wave sub-tiles: 4 x 3 x 256 floats = 768 float4, 3 per thread
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int v = threadIdx.x + r * NN_BLOCK;      // 0..767
            const int ww = v / 192, rem = v % 192;         // 192 float4 per wave sub-tile
            const int a = rem / 64, e = (rem % 64) * 4;    // coordinate array, element offset
            const int off = k * NN2_TQW + e;               // offset inside the wave's range
            const int src = q0 + ww * wseg + off;
            if (off < wseg && src < m_pad)
                *reinterpret_cast<float4*>(&sq[ww][a][e]) = *reinterpret_cast<const float4*>(&Q[(size_t)a * m_pad + src]);
        }
        __syncthreads();

        const int tile0 = my0 + k * NN2_TQW;
        const int len = min(NN2_TQW, my1 - tile0);  // multiple of C, <= 0 when exhausted
        for (int c = 0; c < len; c += C) {
            float bo[T];
#pragma unroll
            for (int t = 0; t < T; ++t) bo[t] = best[t];
            if constexpr (CULL) {
                // level 0: the chunk's bounding box (precomputed once per model over the scan copy): ~20 VALU ops
                // per chunk and lane pair instead of ~50, wave-uniform skip; then the xy early-out
                if (fuse.boxes) {
                    const float* bx = fuse.boxes + (size_t)((tile0 + c) / C) * 8;  // scalar address -> s_load
                    if (__builtin_amdgcn_ballot_w64(box_may_improve<TP>(bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], px, py, pz, best)) == 0ull)
                        continue;
                }
                scan_chunk_xy_cull<TP, C>(&sq[w][0][c], &sq[w][1][c], &sq[w][2][c], px, py, pz, best);
            } else {
#pragma unroll
                for (int kk = 0; kk < C; kk += 4) {
                    const float4 qx4 = *reinterpret_cast<const float4*>(&sq[w][0][c + kk]);
                    const float4 qy4 = *reinterpret_cast<const float4*>(&sq[w][1][c + kk]);
                    const float4 qz4 = *reinterpret_cast<const float4*>(&sq[w][2][c + kk]);
                    const f2 qxa = f2{qx4.x, qx4.y}, qxb = f2{qx4.z, qx4.w};
                    const f2 qya = f2{qy4.x, qy4.y}, qyb = f2{qy4.z, qy4.w};
                    const f2 qza = f2{qz4.x, qz4.y}, qzb = f2{qz4.z, qz4.w};
#pragma unroll
                    for (int u = 0; u < TP; ++u) {
                        const f2 d0 = pk_dist2<0>(qxa, qya, qza, px[u], py[u], pz[u]);
                        const f2 d1 = pk_dist2<1>(qxa, qya, qza, px[u], py[u], pz[u]);
                        const f2 d2 = pk_dist2<0>(qxb, qyb, qzb, px[u], py[u], pz[u]);
                        const f2 d3 = pk_dist2<1>(qxb, qyb, qzb, px[u], py[u], pz[u]);
                        best[2 * u] = fmin_(fmin_(best[2 * u], d0.x), d1.x);
                        best[2 * u] = fmin_(fmin_(best[2 * u], d2.x), d3.x);
                        best[2 * u + 1] = fmin_(fmin_(best[2 * u + 1], d0.y), d1.y);
                        best[2 * u + 1] = fmin_(fmin_(best[2 * u + 1], d2.y), d3.y);
                    }
                }
            }
            bool any = false;
#pragma unroll
            for (int t = 0; t < T; ++t) any |= best[t] < bo[t];
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {  // wave-uniform: skipped while no minimum moved
                const int cid = (tile0 + c) / C;
#pragma unroll
                for (int t = 0; t < T; ++t) cst[t] = (best[t] < bo[t]) ? cid : cst[t];
            }
        }
    }
    }  // tile scan
    ICP_PHASE(3)

    // index recovery inside the winning chunk (lowest j with d_j == min), then the in-block merge
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float pxt = (t & 1) ? px[t >> 1].y : px[t >> 1].x;
        const float pyt = (t & 1) ? py[t >> 1].y : py[t >> 1].x;
        const float pzt = (t & 1) ? pz[t >> 1].y : pz[t >> 1].x;
        const bool found = cst[t] >= 0;  // this wave's range lowered the (possibly seeded) bound at least once
        const int base = found ? cst[t] * C : 0;
        int idx = 0x7fffffff;
        const float b = found ? best[t] : inf_<float>();
        if (found) {
            idx = base;
#pragma unroll 4
            for (int kk = C - 1; kk >= 0; --kk) {
                const int j = base + kk;
                const float d = dist2<float>(pxt, pyt, pzt, Q[j], Q[(size_t)m_pad + j], Q[2 * (size_t)m_pad + j]);
                idx = (d == b) ? j : idx;
            }
        }
        md[w][lane + t * 64] = b;
        mi[w][lane + t * 64] = idx;
    }
    ICP_PHASE(4)
    __syncthreads();
    ICP_PHASE(5)
    if (threadIdx.x < 64 * T) {
        float b = md[0][threadIdx.x];
        int bi = mi[0][threadIdx.x];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
            const float d = md[ww][threadIdx.x];
            const int j = mi[ww][threadIdx.x];
            if (d < b) { b = d; bi = j; }
        }
        if constexpr (TAIL == 0) {
            const size_t o = (size_t)blockIdx.y * n_pad + (size_t)blockIdx.x * (64 * T) + threadIdx.x;
            part_d[o] = b;
            part_idx[o] = bi;
        } else {
            const unsigned long long key = ((unsigned long long)__float_as_uint(b) << 32) | (unsigned int)bi;
            __hip_atomic_fetch_min(&tail.keys[(size_t)blockIdx.x * (64 * T) + threadIdx.x], key, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (TAIL != 0) {
        static_assert(TAIL == 0 || T == 2, "the fused tail is written for two moving points per lane");
        // every wave drains its atomics, the block meets, one lane draws the row's ticket
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ICP_PHASE(6)
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int ticket = __hip_atomic_fetch_add(&tail.tickets[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *s_flag = (ticket == gridDim.y - 1) ? 1 : 0;
        }
        __syncthreads();
        ICP_PHASE(7)
        if (*s_flag == 0 || w != 0) return;  // only wave 0 of the row's last block goes on (the LDS is all its own now)

        constexpr int NACC = TAIL == 2 ? 28 : 18;
        double acc[NACC];
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
        const float* Qg = fuse.Q_gather;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int i = ibase + t * 64;
            const unsigned long long key = __hip_atomic_load(&tail.keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tail.keys[i] = ~0ull;  // ready for the next launch (nobody touches this row again in this one)
            int j = (int)(unsigned int)(key & 0xffffffffull);
            j = ((unsigned)j < (unsigned)fuse.m) ? j : fuse.m - 1;  // unreachable clamp, keeps idx in range by construction
            if (i < fuse.n) {
                tail.idx_out[i] = j;
                const double ppx = (double)(t ? px[0].y : px[0].x), ppy = (double)(t ? py[0].y : py[0].x),
                             ppz = (double)(t ? pz[0].y : pz[0].x);
                const double qx = (double)Qg[j], qy = (double)Qg[(size_t)m_pad + j], qz = (double)Qg[2 * (size_t)m_pad + j];
                acc[0] += 1.0;
                if constexpr (TAIL == 1) {
                    acc[1] += ppx; acc[2] += ppy; acc[3] += ppz;
                    acc[4] += qx; acc[5] += qy; acc[6] += qz;
                    acc[7] += qx * ppx; acc[8] += qx * ppy; acc[9] += qx * ppz;
                    acc[10] += qy * ppx; acc[11] += qy * ppy; acc[12] += qy * ppz;
                    acc[13] += qz * ppx; acc[14] += qz * ppy; acc[15] += qz * ppz;
                    acc[16] += ppx * ppx + ppy * ppy + ppz * ppz;
                    acc[17] += qx * qx + qy * qy + qz * qz;
                } else {
                    const double nx = (double)tail.Nrm[j], ny = (double)tail.Nrm[(size_t)m_pad + j],
                                 nz = (double)tail.Nrm[2 * (size_t)m_pad + j];
                    double cn[6];
                    cn[0] = ppy * nz - ppz * ny;
                    cn[1] = ppz * nx - ppx * nz;
                    cn[2] = ppx * ny - ppy * nx;
                    cn[3] = nx; cn[4] = ny; cn[5] = nz;
                    const double bb = (ppx - qx) * nx + (ppy - qy) * ny + (ppz - qz) * nz;
                    int o = 1;
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int c2 = a; c2 < 6; ++c2) acc[o++] += cn[a] * cn[c2];
#pragma unroll
                    for (int a = 0; a < 6; ++a) acc[22 + a] -= cn[a] * bb;
                }
            }
        }
        // one wave: transpose through LDS (rows padded to 65 doubles), lane k adds slot k in lane order
        double (*tr)[65] = reinterpret_cast<double (*)[65]>(lds_raw);
#pragma unroll
        for (int k = 0; k < NACC; ++k) tr[k][lane] = acc[k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // same wave: DS ops are in order; this pins the compiler
        double* row = tail.rows + (size_t)blockIdx.x * ICP_NMOM;
        if (lane < NACC) {
            double sum = 0.0;
#pragma unroll 8
            for (int l = 0; l < 64; ++l) sum += tr[lane][l];
            row[1 + lane] = sum;
        }
        if (lane == 0) {
            row[ICP_MOM_ERR] = fuse.apply ? __hip_atomic_load(&tail.err_tile[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            tail.tickets[blockIdx.x] = 0u;
        }
        __threadfence_system();  // the row is visible to a polling host before its tag
        if (lane == 0) __hip_atomic_store(&row[ICP_NMOM - 1], tail.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        ICP_PHASE(8)
    }
}

// lexicographic (d, j) minimum over the S segment partials: segments are ascending model ranges,
// so the first strict minimum in segment order is the lowest index.
template <typename F>
__device__ __forceinline__ int merge_partials(const F* __restrict__ part_d, const int32_t* __restrict__ part_idx,
                                              int S, int n_pad, int i)
{
    F best = part_d[i];
    int bi = part_idx[i];
    int s = 1;
    for (; s + 8 <= S; s += 8) {  // 16 independent loads in flight, then the ordered compare chain
        F d[8];
        int j[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            d[u] = part_d[(size_t)(s + u) * n_pad + i];
            j[u] = part_idx[(size_t)(s + u) * n_pad + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (d[u] < best) { best = d[u]; bi = j[u]; }
    }
    if (s < S) {  // tail: same 16 loads in flight, out-of-range slots replaced by +inf
        F d[8];
        int j[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ss = s + u < S ? s + u : S - 1;
            d[u] = part_d[(size_t)ss * n_pad + i];
            j[u] = part_idx[(size_t)ss * n_pad + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s + u < S && d[u] < best) { best = d[u]; bi = j[u]; }
    }
    return bi;
}

template <typename F>
__global__ void merge_kernel(const F* __restrict__ part_d, const int32_t* __restrict__ part_idx, int S, int n_pad,
                             int n, int m, int32_t* __restrict__ idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int j = merge_partials<F>(part_d, part_idx, S, n_pad, i);
    idx[i] = j < m ? j : m - 1;  // unreachable clamp (padding never wins); keeps idx in range by construction
}

// ------------------------------------------------------------------------------------------------
// fused merge + gather + moments.  HBM-bound: per moving point 12 B (p) + 8*S B (partials)
// + 4 B (idx store) + 12 B gathered (q) [+ 12 B normals], accumulated in fp64.
// ------------------------------------------------------------------------------------------------
constexpr int MOM_BLOCK = 64;  // one wave per block: no LDS, no barrier; 256 blocks already at 16 384 points

template <typename F, int METRIC>
__global__ __launch_bounds__(MOM_BLOCK) void moments_kernel(const F* __restrict__ P, int n, int n_pad,
                                                            const F* __restrict__ Q, int m, int m_pad,
                                                            const F* __restrict__ Nrm,
                                                            const F* __restrict__ part_d,
                                                            const int32_t* __restrict__ part_idx, int S,
                                                            int32_t* __restrict__ idx_out,
                                                            double* __restrict__ partials, double tag,
                                                            const double* __restrict__ err_rows, int err_count)
{
    constexpr int NACC = (METRIC == ICP_POINT_TO_POINT) ? 18 : 28;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;

    for (int i = blockIdx.x * MOM_BLOCK + threadIdx.x; i < n; i += gridDim.x * MOM_BLOCK) {
        int j = merge_partials<F>(part_d, part_idx, S, n_pad, i);
        j = j < m ? j : m - 1;
        idx_out[i] = j;
        const double px = (double)P[i], py = (double)P[(size_t)n_pad + i], pz = (double)P[2 * (size_t)n_pad + i];
        const double qx = (double)Q[j], qy = (double)Q[(size_t)m_pad + j], qz = (double)Q[2 * (size_t)m_pad + j];
        acc[0] += 1.0;
        if constexpr (METRIC == ICP_POINT_TO_POINT) {
            acc[1] += px; acc[2] += py; acc[3] += pz;
            acc[4] += qx; acc[5] += qy; acc[6] += qz;
            acc[7] += qx * px; acc[8] += qx * py; acc[9] += qx * pz;
            acc[10] += qy * px; acc[11] += qy * py; acc[12] += qy * pz;
            acc[13] += qz * px; acc[14] += qz * py; acc[15] += qz * pz;
            acc[16] += px * px + py * py + pz * pz;
            acc[17] += qx * qx + qy * qy + qz * qz;
        } else {
            const double nx = (double)Nrm[j], ny = (double)Nrm[(size_t)m_pad + j], nz = (double)Nrm[2 * (size_t)m_pad + j];
            double cn[6];
            cn[0] = py * nz - pz * ny;
            cn[1] = pz * nx - px * nz;
            cn[2] = px * ny - py * nx;
            cn[3] = nx; cn[4] = ny; cn[5] = nz;
            const double bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
            int o = 1;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c) acc[o++] += cn[a] * cn[c];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[22 + a] -= cn[a] * bi;
        }
    }
    // slot 0 of the moment vector is the error of the preceding transform (written by finalize)
    block_sum_store<NACC, MOM_BLOCK>(acc, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
    // slot 0: this block's share of the error rows the preceding transform (fused into the matching
    // kernel, or its own launch) left in device memory -- fixed assignment, fixed order
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int r = blockIdx.x; r < err_count; r += gridDim.x) e += err_rows[r];
        partials[(size_t)blockIdx.x * ICP_NMOM + ICP_MOM_ERR] = e;
    }
    // completion tag for a host that polls the (pinned, mapped) rows instead of synchronising the
    // stream: the row's data is released to system scope before the tag becomes visible
    static_assert(MOM_BLOCK == 64, "the tag protocol assumes one wave per block");
    __threadfence_system();
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * ICP_NMOM + (ICP_NMOM - 1)] = tag;
}

// ------------------------------------------------------------------------------------------------
// in-place transform + error.  HBM-bound: 12 B read + 12 B written per moving point, + 4 B idx
// + 12 B gathered q.  The products and sums are rounded separately in the storage precision
// ((r0*x + r1*y) + r2*z) + t, the association of RyT (src/ICP_point_to_point.cu:85).
// ------------------------------------------------------------------------------------------------
constexpr int TR_BLOCK = 256;

template <typename F>
__global__ __launch_bounds__(TR_BLOCK) void transform_error_kernel(F* __restrict__ P, int n, int n_pad, RT<F> rt,
                                                                    const F* __restrict__ Q, int m_pad,
                                                                    const int32_t* __restrict__ idx,
                                                                    double* __restrict__ err_partials)
{
    double acc[1] = {0.0};
    for (int i = blockIdx.x * TR_BLOCK + threadIdx.x; i < n_pad; i += gridDim.x * TR_BLOCK) {
        const F x = P[i], y = P[(size_t)n_pad + i], z = P[2 * (size_t)n_pad + i];
        F o[3];
        apply_rt<F>(rt, x, y, z, o[0], o[1], o[2]);
        P[i] = o[0];
        P[(size_t)n_pad + i] = o[1];
        P[2 * (size_t)n_pad + i] = o[2];
        if (i < n) {
            const int j = idx[i];
            const double dx = (double)Q[j] - (double)o[0];
            const double dy = (double)Q[(size_t)m_pad + j] - (double)o[1];
            const double dz = (double)Q[2 * (size_t)m_pad + j] - (double)o[2];
            acc[0] += dx * dx + dy * dy + dz * dz;
        }
    }
    block_sum_store<1, TR_BLOCK>(acc, err_partials + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// finalize: one block, fixed-order sums of the per-block partials -> the ICP_NMOM vector.
// thread (k = tid % 32, part = tid / 32) sums blocks part, part+8, ... of slot k.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void finalize_kernel(double* __restrict__ mom, const double* __restrict__ mom_partials,
                                                       int mom_blocks, const double* __restrict__ err_partials,
                                                       int err_blocks, int rows_have_err)
{
    __shared__ double red[8][ICP_NMOM];
    const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
    double s = 0.0;
    if (k == 0) {
        for (int b = part; b < err_blocks; b += 8) s += err_partials[b];
        if (rows_have_err)
            for (int b = part; b < mom_blocks; b += 8) s += mom_partials[(size_t)b * ICP_NMOM];
    } else if (k == ICP_NMOM - 1) {
        s = 0.0;  // the rows' completion-tag slot is not a moment
    } else {
        for (int b = part; b < mom_blocks; b += 8) s += mom_partials[(size_t)b * ICP_NMOM + k];
    }
    red[part][k] = s;
    __syncthreads();
    if (threadIdx.x < ICP_NMOM) {
        double tot = red[0][k];
#pragma unroll
        for (int p = 1; p < 8; ++p) tot += red[p][k];
        mom[k] = tot;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
template <typename F> struct NNCfg;
template <> struct NNCfg<float> { static constexpr int T = 4; static constexpr int TQ = 2048; };
template <> struct NNCfg<double> { static constexpr int T = 2; static constexpr int TQ = 1024; };

template <typename F>
hipError_t launch_nn_t(const NNPlan& pl, const void* P, const void* Q, void* part_d, int32_t* part_idx,
                              hipStream_t st)
{
    constexpr int TQ = NNCfg<F>::TQ;
    dim3 grid(pl.blocks_x, pl.splits);
#define ICP_LAUNCH_NN(TT)                                                                                          \
    hipLaunchKernelGGL((nn_match_kernel<F, TT, TQ>), grid, dim3(NN_BLOCK), 0, st, (const F*)P, pl.n_pad, (const F*)Q, \
                       pl.m_pad, pl.seg_len, (F*)part_d, part_idx)
    switch (pl.pts_per_thread) {
        case 1: ICP_LAUNCH_NN(1); break;
        case 2: ICP_LAUNCH_NN(2); break;
        case 8: if constexpr (sizeof(F) == 4) { ICP_LAUNCH_NN(8); break; }
        default: ICP_LAUNCH_NN(4); break;
    }
#undef ICP_LAUNCH_NN
    return hipGetLastError();
}

hipError_t launch_merge(const NNPlan& pl, const void* part_d, const int32_t* part_idx, int32_t* idx, hipStream_t st)
{
    if (pl.n <= 0 || pl.m <= 0) return hipSuccess;
    const int blocks = (pl.n + 255) / 256;
    if (pl.precision == ICP_F64)
        hipLaunchKernelGGL((merge_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)part_d, part_idx,
                           pl.splits, pl.n_pad, pl.n, pl.m, idx);
    else
        hipLaunchKernelGGL((merge_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)part_d, part_idx,
                           pl.splits, pl.n_pad, pl.n, pl.m, idx);
    return hipGetLastError();
}

hipError_t launch_moments(const NNPlan& pl, int metric, const void* P, const void* Q, const void* Nrm,
                          const void* part_d, const int32_t* part_idx, int32_t* idx, double* partials, int* blocks,
                          double tag, const double* err_rows, int err_count, hipStream_t st)
{
    int nb = (pl.n + MOM_BLOCK - 1) / MOM_BLOCK;
    if (nb > MOM_MAX_BLOCKS) nb = MOM_MAX_BLOCKS;
    *blocks = nb;
    if (nb <= 0) return hipSuccess;
#define ICP_LAUNCH_MOM(F, MET)                                                                                     \
    hipLaunchKernelGGL((moments_kernel<F, MET>), dim3(nb), dim3(MOM_BLOCK), 0, st, (const F*)P, pl.n, pl.n_pad,      \
                       (const F*)Q, pl.m, pl.m_pad, (const F*)Nrm, (const F*)part_d, part_idx, pl.splits, idx, partials, tag, err_rows, err_count)
    if (pl.precision == ICP_F64) {
        if (metric == ICP_POINT_TO_PLANE) ICP_LAUNCH_MOM(double, ICP_POINT_TO_PLANE);
        else ICP_LAUNCH_MOM(double, ICP_POINT_TO_POINT);
    } else {
        if (metric == ICP_POINT_TO_PLANE) ICP_LAUNCH_MOM(float, ICP_POINT_TO_PLANE);
        else ICP_LAUNCH_MOM(float, ICP_POINT_TO_POINT);
    }
#undef ICP_LAUNCH_MOM
    return hipGetLastError();
}

hipError_t launch_transform_error(int precision, void* P, int n, int n_pad, const double* R9, const double* t3,
                                  const void* Q, int m_pad, const int32_t* idx, double* err_partials, int* blocks,
                                  hipStream_t st)
{
    int nb = (n_pad + TR_BLOCK - 1) / TR_BLOCK;
    if (nb > MOM_MAX_BLOCKS) nb = MOM_MAX_BLOCKS;
    *blocks = nb;
    if (nb <= 0) return hipSuccess;
    if (precision == ICP_F64) {
        RT<double> rt;
        for (int k = 0; k < 9; ++k) rt.r[k] = R9[k];
        for (int k = 0; k < 3; ++k) rt.t[k] = t3[k];
        hipLaunchKernelGGL((transform_error_kernel<double>), dim3(nb), dim3(TR_BLOCK), 0, st, (double*)P, n, n_pad, rt,
                           (const double*)Q, m_pad, idx, err_partials);
    } else {
        RT<float> rt;
        for (int k = 0; k < 9; ++k) rt.r[k] = (float)R9[k];
        for (int k = 0; k < 3; ++k) rt.t[k] = (float)t3[k];
        hipLaunchKernelGGL((transform_error_kernel<float>), dim3(nb), dim3(TR_BLOCK), 0, st, (float*)P, n, n_pad, rt,
                           (const float*)Q, m_pad, idx, err_partials);
    }
    return hipGetLastError();
}

// many rows (a cloud of millions of points: 78 125 rows for 10 M): one block walking all of them is milliseconds -- the
// RCCL route of configs[4] spent 5.6 ms per iteration there.  Stage 1: up to 256 blocks each add a contiguous range of
// rows, in the same fixed order, into one row of `scratch`; stage 2: the block above adds those.  Fixed ranges, fixed
// order: the same bits on every rank and every run.
__global__ __launch_bounds__(256) void finalize_ranges_kernel(double* __restrict__ scratch, const double* __restrict__ mom_partials, int mom_blocks,
                                                              int per, int rows_have_err)
{
    __shared__ double red[8][ICP_NMOM];
    const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int b0 = (int)blockIdx.x * per, b1 = min(b0 + per, mom_blocks);
    double s = 0.0;
    if (k != ICP_NMOM - 1 && (k != 0 || rows_have_err))
        for (int b = b0 + part; b < b1; b += 8) s += mom_partials[(size_t)b * ICP_NMOM + k];
    red[part][k] = s;
    __syncthreads();
    if (threadIdx.x < ICP_NMOM) {
        double tot = red[0][k];
#pragma unroll
        for (int p = 1; p < 8; ++p) tot += red[p][k];
        scratch[(size_t)blockIdx.x * ICP_NMOM + k] = tot;
    }
}

hipError_t launch_finalize(double* mom_out, const double* mom_partials, int mom_blocks, const double* err_partials,
                           int err_blocks, int rows_have_err, hipStream_t st, double* scratch)
{
    if (scratch != nullptr && mom_blocks > 2048) {
        const int groups = 256, per = (mom_blocks + groups - 1) / groups;
        hipLaunchKernelGGL(finalize_ranges_kernel, dim3(groups), dim3(256), 0, st, scratch, mom_partials, mom_blocks, per, rows_have_err);
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, st, mom_out, scratch, groups, err_partials, err_blocks, rows_have_err);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, st, mom_out, mom_partials, mom_blocks, err_partials,
                       err_blocks, rows_have_err);
    return hipGetLastError();
}

hipError_t launch_aos_to_soa(int precision, const void* aos, int n, int n_pad, void* soa, hipStream_t st, unsigned int* nonfinite, void* soa2, unsigned int* enc)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (n_pad + 255) / 256;
    if (precision == ICP_F64)
        hipLaunchKernelGGL((aos_to_soa_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)aos, n, n_pad,
                           (double*)soa, nonfinite, (double*)soa2, (unsigned int*)nullptr);
    else
        hipLaunchKernelGGL((aos_to_soa_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)aos, n, n_pad,
                           (float*)soa, nonfinite, (float*)soa2, enc);
    return hipGetLastError();
}

hipError_t launch_soa_to_aos(int precision, const void* soa, int n, int n_pad, void* aos, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (n + 255) / 256;
    if (precision == ICP_F64)
        hipLaunchKernelGGL((soa_to_aos_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)soa, n, n_pad,
                           (double*)aos);
    else
        hipLaunchKernelGGL((soa_to_aos_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)soa, n, n_pad,
                           (float*)aos);
    return hipGetLastError();
}


template hipError_t launch_nn_t<float>(const NNPlan&, const void*, const void*, void*, int32_t*, hipStream_t);
template hipError_t launch_nn_t<double>(const NNPlan&, const void*, const void*, void*, int32_t*, hipStream_t);

// the packed fp32 kernel nn_match_f32_v2 (the plan is the dense one's: pl.sparse == 0); tl: 0 no fused tail, 1 point-to-point, 2 point-to-plane
hipError_t launch_dense_v2(const NNPlan& pl, const void* P, const void* Qscan, void* part_d, int32_t* part_idx, const RT<float>& rt, const NNFuse& fuse,
                           const NNTail& tail, int tl, bool cull, hipStream_t st)
{
    const dim3 grid(pl.blocks_x, pl.splits);
#define ICP_LAUNCH_NN2T(CU, TL)                                                                                     \
    hipLaunchKernelGGL((nn_match_f32_v2<2, 8, CU, TL>), grid, dim3(NN_BLOCK), 0, st, (const float*)P, pl.n_pad,      \
                       (const float*)Qscan, pl.m_pad, pl.seg_len, (float*)part_d, part_idx, rt, fuse, tail)
#define ICP_LAUNCH_NN2(TT, CC, CU)                                                                                  \
    hipLaunchKernelGGL((nn_match_f32_v2<TT, CC, CU, 0>), grid, dim3(NN_BLOCK), 0, st, (const float*)P, pl.n_pad,     \
                       (const float*)Qscan, pl.m_pad, pl.seg_len, (float*)part_d, part_idx, rt, fuse, tail)
    if (tl != 0) {
        const bool plane = tl == 2;
        if (cull) { if (plane) ICP_LAUNCH_NN2T(1, 2); else ICP_LAUNCH_NN2T(1, 1); }
        else { if (plane) ICP_LAUNCH_NN2T(0, 2); else ICP_LAUNCH_NN2T(0, 1); }
    } else if (pl.pts_per_thread == 4) {
        if (pl.chunk == 8) ICP_LAUNCH_NN2(4, 8, 0); else ICP_LAUNCH_NN2(4, 16, 0);
    } else if (cull) {
        if (pl.chunk == 8) ICP_LAUNCH_NN2(2, 8, 1); else ICP_LAUNCH_NN2(2, 16, 1);
    } else {
        if (pl.chunk == 8) ICP_LAUNCH_NN2(2, 8, 0); else ICP_LAUNCH_NN2(2, 16, 0);
    }
#undef ICP_LAUNCH_NN2
#undef ICP_LAUNCH_NN2T
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// batched ICP (icp_batch.cpp): the pass of every running pair of a batch in one launch.
//
// grid = one block per work item: BATCH_ITEM moving points of one pair, cut from that pair's first point.  All four waves
// hold the item's points (one per lane); wave w scans the w-th contiguous quarter of the pair's model through its own LDS
// sub-tile (every lane reads the same address), keeping the running minimum and the first chunk that lowered it, as
// nn_match_kernel does; the index is recovered inside that chunk, and the quarters are merged in ascending order with a
// strict <: the lowest index wins ties, as in the reference's ascending scan.
//   front end (pass >= 1): the pair's previous R, t by apply_rt -- every wave moves its copy of the points with the same
//     instructions; wave 0 stores them and adds |p_new - q[idx_prev]|^2 in double (transform_error_kernel's arithmetic);
//   tail: wave 0 stores idx, gathers q[idx] and forms moments_kernel's point-to-point terms in double; block_sum_store
//     writes the item's row partials[item][0 .. ICP_MOM_SQQ] (error in slot ICP_MOM_ERR).
//   METRIC == ICP_POINT_TO_PLANE (its own instantiation: the point-to-point one has no branch on the metric): wave 0 gathers
//     n[idx] too, from the normal planes laid out as the model's, and forms moments_kernel's plane terms statement for
//     statement -- cn = (p x n, n), bi = (p - q) . n, C += cn cn^T, b -= cn bi -- into slots ICP_MOM_CNT, ICP_MOM_C ..
//     ICP_MOM_B + 5.  The front end and the error-only last pass are the same code.
//   GATE (its own instantiations: the ungated ones have no branch on it and never read thr): wave 0 keeps the match only if
//     the merged minimum b -- the dist2<F> the scan already holds, nothing recomputed -- is <= thr[pair], the pair's squared
//     maximum correspondence distance in F (+inf: not gated).  A rejected point leaves every accumulator 0, ICP_MOM_CNT
//     included, and its idx entry carries BATCH_IDX_REJECTED above the nearest neighbour's index; the next pass's front end
//     reads that entry anyway (idx_prev) and adds the point's error only if the bit is clear.  Downloads strip the bit.
// A pair's blocks, their geometry and every sum depend on that pair alone (no atomics): its bits do not depend on the batch.
// ------------------------------------------------------------------------------------------------
template <typename F> struct BatchCfg;
template <> struct BatchCfg<float> { static constexpr int TW = 512; };    // model points per wave and tile: 6 KiB per wave
template <> struct BatchCfg<double> { static constexpr int TW = 256; };
static_assert(sizeof(RT<float>) == 12 * sizeof(float) && sizeof(RT<double>) == 12 * sizeof(double), "the host writes R, t as 12 values per pair");

// slots of the moment vector a batch pass fills: error, count, sum p, sum q, sum q p^T, |p|^2, |q|^2 -- or error, count, C (21), b (6)
template <int METRIC> struct BatchAcc { static constexpr int N = (METRIC == ICP_POINT_TO_POINT) ? ICP_MOM_SQQ + 1 : ICP_MOM_B + 6; };

// What one moving point (x, y, z), matched to model point j of its pair, adds to the accumulators acc[] of its lane (all zero
// before): nothing if the match was not kept.  ONE definition for the fused tail of nn_match_batch and for batch_trim_moments,
// so that the two cannot drift and a pair that is not trimmed has the same bits on either route.  A macro, not a function: a
// __device__ function, force-inlined, is simplified on its own before it is inlined, and the eight fused instantiations then
// come out with other register numbers and commuted operands than the kernels whose timings DESIGN.md records (tried: by value,
// by reference, into a local array).  As statements they compile to the listings they always had.  To be used inside a template
// with METRIC in scope; Qx_, Qy_, Qz_: the pair's model planes, Nrm_ + q_off_: its normal planes (read for the plane metric only).
#define ICP_BATCH_POINT_TERMS(acc, kept_, x_, y_, z_, j_, Qx_, Qy_, Qz_, Nrm_, q_off_, q_plane_)                              \
    {                                                                                                                        \
        const double px = (double)(x_), py = (double)(y_), pz = (double)(z_);                                                \
        const double qx = (double)(Qx_)[j_], qy = (double)(Qy_)[j_], qz = (double)(Qz_)[j_];                                 \
        if (!(kept_)) {                                                                                                      \
            /* (a rejected point adds nothing: every accumulator stays 0, the count included) */                             \
        } else if constexpr (METRIC == ICP_POINT_TO_POINT) {                                                                 \
            acc[ICP_MOM_CNT] = 1.0;                                                                                          \
            acc[ICP_MOM_SP + 0] = px; acc[ICP_MOM_SP + 1] = py; acc[ICP_MOM_SP + 2] = pz;                                    \
            acc[ICP_MOM_SQ + 0] = qx; acc[ICP_MOM_SQ + 1] = qy; acc[ICP_MOM_SQ + 2] = qz;                                    \
            acc[ICP_MOM_SQP + 0] = qx * px; acc[ICP_MOM_SQP + 1] = qx * py; acc[ICP_MOM_SQP + 2] = qx * pz;                  \
            acc[ICP_MOM_SQP + 3] = qy * px; acc[ICP_MOM_SQP + 4] = qy * py; acc[ICP_MOM_SQP + 5] = qy * pz;                  \
            acc[ICP_MOM_SQP + 6] = qz * px; acc[ICP_MOM_SQP + 7] = qz * py; acc[ICP_MOM_SQP + 8] = qz * pz;                  \
            acc[ICP_MOM_SPP] = px * px + py * py + pz * pz;                                                                  \
            acc[ICP_MOM_SQQ] = qx * qx + qy * qy + qz * qz;                                                                  \
        } else {                                                                                                             \
            acc[ICP_MOM_CNT] = 1.0;                                                                                          \
            const F* Nx = (Nrm_) + (q_off_);                                                                                 \
            const double nx = (double)Nx[j_], ny = (double)Nx[(q_plane_) + j_], nz = (double)Nx[2 * (q_plane_) + j_];        \
            double cn[6];                                                                                                    \
            cn[0] = py * nz - pz * ny;                                                                                       \
            cn[1] = pz * nx - px * nz;                                                                                       \
            cn[2] = px * ny - py * nx;                                                                                       \
            cn[3] = nx; cn[4] = ny; cn[5] = nz;                                                                              \
            const double bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;                                              \
            int o = ICP_MOM_C;                                                                                               \
            _Pragma("unroll") for (int a = 0; a < 6; ++a)                                                                    \
                _Pragma("unroll") for (int c = a; c < 6; ++c) acc[o++] += cn[a] * cn[c];                                     \
            _Pragma("unroll") for (int a = 0; a < 6; ++a) acc[ICP_MOM_B + a] -= cn[a] * bi;                                  \
        }                                                                                                                    \
    }

// DEFER (its own instantiations, <F, METRIC, true, true>, for a batch that trims: see batch_trim_select below): the gated front
// end and the same search, and a tail in which wave 0 only stores idx_cur[gi] = j and dist[gi] = the merged minimum b -- no
// decision, no terms; the row carries ICP_MOM_ERR and zeros.  The fused instantiations never touch dist.
template <typename F, int METRIC, bool GATE, bool DEFER = false>
__global__ __launch_bounds__(NN_BLOCK) void nn_match_batch(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                           const int* __restrict__ mode, const RT<F>* __restrict__ rts,
                                                           F* __restrict__ P, long long p_plane, const F* __restrict__ Q,
                                                           const F* __restrict__ Nrm, long long q_plane,
                                                           const int32_t* __restrict__ idx_prev, int32_t* __restrict__ idx_cur,
                                                           double* __restrict__ partials, const F* __restrict__ thr,
                                                           F* __restrict__ dist)
{
    using V = typename Vec16<F>::type;
    constexpr int VN = Vec16<F>::N;
    constexpr int TW = BatchCfg<F>::TW, C = NN_CHUNK;
    constexpr int NACC = BatchAcc<METRIC>::N;
    static_assert(BATCH_ITEM == 64 && NN_BLOCK == 4 * BATCH_ITEM, "one point per lane, four waves per item");
    __shared__ __attribute__((aligned(16))) F sq[4][3][TW];
    __shared__ F md[4][BATCH_ITEM];
    __shared__ int mi[4][BATCH_ITEM];

    const BatchItem it = items[blockIdx.x];
    const int pm = mode[it.pair];
    if (pm == 0) return;   // the pair has ended (or takes no part in this pass): the whole block leaves
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = lane < it.count;
    const long long gi = pr.p_off + it.first + (live ? lane : 0);   // (lanes past the item's end work on its first point: nothing of theirs is kept)
    const F* Qx = Q + pr.q_off;
    const F* Qy = Qx + q_plane;
    const F* Qz = Qx + 2 * q_plane;

    F x = P[gi], y = P[p_plane + gi], z = P[2 * p_plane + gi];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    __syncthreads();   // every wave holds its points before wave 0 overwrites them

    if (pm & BATCH_APPLY) {
        apply_rt<F>(rts[it.pair], x, y, z, x, y, z);
        if (w == 0 && live) {
            P[gi] = x;
            P[p_plane + gi] = y;
            P[2 * p_plane + gi] = z;
            const int jr = idx_prev[gi];
            const int j = GATE ? (jr & BATCH_IDX_MASK) : jr;
            const double dx = (double)Qx[j] - (double)x;
            const double dy = (double)Qy[j] - (double)y;
            const double dz = (double)Qz[j] - (double)z;
            if (!GATE || jr >= 0) acc[ICP_MOM_ERR] = dx * dx + dy * dy + dz * dz;   // (only a point kept by that matching pass)
        }
    }

    if (pm & BATCH_MATCH) {
        const int m = pr.m;
        const int wseg = ((m + 3) / 4 + C - 1) / C * C;   // model points per wave, whole chunks
        const int my0 = w * wseg, my1 = min(my0 + wseg, m);  // may be empty (my1 <= my0)
        const int ntile = (wseg + TW - 1) / TW;           // the same for every wave: the barriers pair up
        F best = inf_<F>();
        int cst = -1;   // first model index of the chunk that last lowered `best`
        for (int k = 0; k < ntile; ++k) {
            const int t0 = my0 + k * TW;
            __syncthreads();
            // this wave's sub-tile; places past the quarter's end hold +inf, which never lowers a minimum
            for (int e = lane; e < TW; e += 64) {
                const int j = t0 + e;
                F qx = inf_<F>(), qy = inf_<F>(), qz = inf_<F>();
                if (j < my1) { qx = Qx[j]; qy = Qy[j]; qz = Qz[j]; }
                sq[w][0][e] = qx;
                sq[w][1][e] = qy;
                sq[w][2][e] = qz;
            }
            __syncthreads();
            const int len = min(TW, my1 - t0);   // <= 0: this wave's quarter is exhausted
            for (int c = 0; c < len; c += C) {
                const F bo = best;
#pragma unroll
                for (int kk = 0; kk < C; kk += VN) {
                    const V qx = *reinterpret_cast<const V*>(&sq[w][0][c + kk]);
                    const V qy = *reinterpret_cast<const V*>(&sq[w][1][c + kk]);
                    const V qz = *reinterpret_cast<const V*>(&sq[w][2][c + kk]);
#pragma unroll
                    for (int v = 0; v < VN; ++v) best = fmin_(best, dist2<F>(x, y, z, vget(qx, v), vget(qy, v), vget(qz, v)));
                }
                cst = (best < bo) ? t0 + c : cst;
            }
        }
        // the lowest j of the winning chunk with d_j == min (global memory, L2-resident)
        int bi = 0x7fffffff;
        if (cst >= 0) {
            bi = cst;
            for (int kk = C - 1; kk >= 0; --kk) {
                const int j = cst + kk;
                if (j < my1) {
                    const F d = dist2<F>(x, y, z, Qx[j], Qy[j], Qz[j]);
                    bi = (d == best) ? j : bi;
                }
            }
        }
        md[w][lane] = cst >= 0 ? best : inf_<F>();
        mi[w][lane] = bi;
        __syncthreads();
        if (w == 0 && live) {
            F b = md[0][lane];
            int j = mi[0][lane];
#pragma unroll
            for (int ww = 1; ww < 4; ++ww)
                if (md[ww][lane] < b) { b = md[ww][lane]; j = mi[ww][lane]; }
            j = ((unsigned)j < (unsigned)m) ? j : 0;   // (nothing found only if every distance overflowed: idx stays in range)
            if constexpr (DEFER) {
                // (the deferred route: batch_trim_select ranks the pair's distances, batch_trim_moments decides and forms the terms)
                idx_cur[gi] = j;
                dist[gi] = b;
            } else {
                const bool kept = !GATE || b <= thr[it.pair];
                idx_cur[gi] = kept ? j : (j | BATCH_IDX_REJECTED);
                ICP_BATCH_POINT_TERMS(acc, kept, x, y, z, j, Qx, Qy, Qz, Nrm, pr.q_off, q_plane)
            }
        }
    }
    // (waves 1-3 add zeros: the row is wave 0's 64 lanes, summed in lane order)
    block_sum_store<NACC, NN_BLOCK>(acc, partials + (size_t)blockIdx.x * ICP_NMOM);
}

// ------------------------------------------------------------------------------------------------
// trimmed rejection (icp_batch_set_trim): a pair keeps the K closest of its n matches (and every match tied with the K-th).  The
// K-th smallest distance of a pair is known only when every one of its points has been matched -- by other blocks, for a
// pair of more than one work item -- so the fused pass cannot decide; a step of a batch that trims runs four launches:
//   nn_match_batch<.., DEFER>   front end + search as the gated pass; wave 0 stores idx and the winning distance, no terms
//   batch_trim_select         one block per pair: tau[pair] = the K-th smallest of the pair's n distances
//   batch_trim_moments        one block per work item: kept = d <= tau[pair] (and d <= thr[pair]); marks idx, forms the terms
//   batch_finalize_kernel     as ever
// A pair's tau, its masks and its sums depend on that pair alone: integer counts, fixed summation order, no floating-point
// atomics.  A pair that is not trimmed (rank 0, tau = +inf, written once by the host) keeps everything, and its rows are the
// fused pass's bit for bit: the same terms (ICP_BATCH_POINT_TERMS) in the same lanes through the same block_sum_store.
// ------------------------------------------------------------------------------------------------
// the values are >= +0 and never NaN (a sum of squares of finite differences, +inf on overflow): their bit patterns, read as
// unsigned integers, sort as the values do
template <typename F> struct TrimKey;
template <> struct TrimKey<float> {
    using U = unsigned int;
    static __device__ __forceinline__ U key(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(U k) { return __uint_as_float(k); }
};
template <> struct TrimKey<double> {
    using U = unsigned long long;
    static __device__ __forceinline__ U key(double v) { return (U)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(U k) { return __longlong_as_double((long long)k); }
};

// one block per pair: tau[pair] = the rank[pair]-th smallest of dist[p_off .. p_off + n), one of those values bit for bit.
// Most-significant-digit radix select, 8 bits per round (4 rounds for fp32, 8 for fp64): every thread adds the values that
// still carry the prefix found so far to a 256-bin LDS histogram of their next digit (integer LDS atomics: the counts do not
// depend on the order of the adds), wave 0 scans the bins for the one that holds the remaining rank, and that digit joins the
// prefix.  Each round re-reads the pair's at most ICP_BATCH_MAX_POINTS values (L2-resident).  rank 0: the pair is not trimmed.
constexpr int TRIM_BLOCK = 256;
template <typename F>
__global__ __launch_bounds__(TRIM_BLOCK) void batch_trim_select(const BatchPair* __restrict__ pairs, const int* __restrict__ mode,
                                                                const int* __restrict__ rank, const F* __restrict__ dist,
                                                                F* __restrict__ tau)
{
    using K = TrimKey<F>;
    using U = typename K::U;
    constexpr int BITS = 8 * (int)sizeof(U);
    __shared__ unsigned int hist[256];
    __shared__ U s_prefix;
    __shared__ unsigned int s_rest;
    const int pair = blockIdx.x;
    if (!(mode[pair] & BATCH_MATCH)) return;
    const int kth = rank[pair];
    const int n = pairs[pair].n;
    if (kth < 1 || kth > n) return;   // not trimmed (a trimmed pair's rank lies in [1, n])
    const F* d = dist + pairs[pair].p_off;
    const int lane = threadIdx.x & 63;
    U prefix = 0;
    unsigned int rest = (unsigned int)(kth - 1);   // values below the wanted one among those that carry the prefix
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0u;
        __syncthreads();
        // (a shift by the type's width is undefined: the first round, where every value carries the empty prefix, has no mask)
        const U high = (shift + 8 < BITS) ? (~U(0) << ((shift + 8) & (BITS - 1))) : U(0);
        for (int i = threadIdx.x; i < n; i += TRIM_BLOCK) {
            const U k = K::key(d[i]);
            if ((k & high) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // lane l holds bins 4l .. 4l + 3; an inclusive scan over the lanes finds the lane, then the bin, that holds `rest`
            const unsigned int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const unsigned int mine = c0 + c1 + c2 + c3;
            unsigned int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const unsigned int excl = incl - mine;
            if (excl <= rest && rest < incl) {   // exactly one lane: the bins hold more than `rest` values between them
                unsigned int r = rest - excl, bin = 4u * lane;
                if (r >= c0) { r -= c0; ++bin; if (r >= c1) { r -= c1; ++bin; if (r >= c2) { r -= c2; ++bin; } } }
                s_prefix = prefix | ((U)bin << shift);
                s_rest = r;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rest = s_rest;
    }
    if (threadIdx.x == 0) tau[pair] = K::value(prefix);
}

// one block per work item, over nn_match_batch's items and in its block shape (wave 0 alone carries data, waves 1-3 add zeros, so
// that block_sum_store adds a row in the fused pass's order): kept = d <= tau[pair] && (no gate || d <= thr[pair]); a rejected
// point's idx entry gets BATCH_IDX_REJECTED; the kept points' terms go to slots 1 .. of the item's row.  Slot ICP_MOM_ERR, which
// nn_match_batch<.., DEFER> wrote, is not touched.
template <typename F, int METRIC>
__global__ __launch_bounds__(NN_BLOCK) void batch_trim_moments(const BatchItem* __restrict__ items, const BatchPair* __restrict__ pairs,
                                                               const int* __restrict__ mode, const F* __restrict__ P, long long p_plane,
                                                               const F* __restrict__ Q, const F* __restrict__ Nrm, long long q_plane,
                                                               int32_t* __restrict__ idx_cur, const F* __restrict__ dist,
                                                               const F* __restrict__ tau, const F* __restrict__ thr,
                                                               double* __restrict__ partials)
{
    constexpr int NACC = BatchAcc<METRIC>::N;
    static_assert(ICP_MOM_ERR == 0, "the row's slots behind the error are written as one run");
    const BatchItem it = items[blockIdx.x];
    if (!(mode[it.pair] & BATCH_MATCH)) return;   // nothing was matched for this pair: the row stays the error and zeros
    const BatchPair pr = pairs[it.pair];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (w == 0 && lane < it.count) {
        const long long gi = pr.p_off + it.first + lane;
        const F* Qx = Q + pr.q_off;
        const F b = dist[gi];
        const int j = idx_cur[gi];
        const bool kept = b <= tau[it.pair] && (thr == nullptr || b <= thr[it.pair]);
        if (!kept) idx_cur[gi] = j | BATCH_IDX_REJECTED;
        const F* Qy = Qx + q_plane;
        const F* Qz = Qx + 2 * q_plane;
        const F x = P[gi], y = P[p_plane + gi], z = P[2 * p_plane + gi];
        ICP_BATCH_POINT_TERMS(acc, kept, x, y, z, j, Qx, Qy, Qz, Nrm, pr.q_off, q_plane)
    }
    double tail[NACC - 1];
#pragma unroll
    for (int k = 1; k < NACC; ++k) tail[k - 1] = acc[k];
    block_sum_store<NACC - 1, NN_BLOCK>(tail, partials + (size_t)blockIdx.x * ICP_NMOM + 1);
}
#undef ICP_BATCH_POINT_TERMS

// one block per pair: mom[pair] = the pair's item rows added up in a fixed order (thread (k, part) adds items part, part + 8, ...
// of slot k; the eight part sums are then added in part order -- finalize_kernel's scheme, over the pair's own items only).
// last = the metric's last slot: ICP_MOM_SQQ, or ICP_MOM_B + 5 for a plane loop; the slots behind it are written as zeros.
__global__ __launch_bounds__(256) void batch_finalize_kernel(const BatchPair* __restrict__ pairs, const int* __restrict__ mode,
                                                             const double* __restrict__ partials, int last, double* __restrict__ mom)
{
    __shared__ double red[8][ICP_NMOM];
    if (mode[blockIdx.x] == 0) return;
    const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int i0 = pairs[blockIdx.x].item0, i1 = pairs[blockIdx.x].item1;
    double s = 0.0;
    if (k <= last)
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

hipError_t launch_batch_pass(int precision, int metric, const BatchItem* items, int n_items, const BatchPair* pairs, int n_pairs,
                             const int* mode, const void* rt, void* P, long long p_plane, const void* Q, const void* Nrm,
                             long long q_plane, const int32_t* idx_prev, int32_t* idx_cur, double* partials, double* mom,
                             const void* thr, const int* trim_rank, void* dist, void* tau, hipStream_t st)
{
    if (n_items <= 0 || n_pairs <= 0) return hipSuccess;
    const bool plane = metric == ICP_POINT_TO_PLANE;
    if (plane && !Nrm) return hipErrorInvalidValue;
    if (trim_rank && (!dist || !tau)) return hipErrorInvalidValue;
#define ICP_LAUNCH_BATCH(F, MET, GATE)                                                                                             \
    hipLaunchKernelGGL((nn_match_batch<F, MET, GATE>), dim3(n_items), dim3(NN_BLOCK), 0, st, items, pairs, mode, (const RT<F>*)rt, \
                       (F*)P, p_plane, (const F*)Q, (const F*)Nrm, q_plane, idx_prev, idx_cur, partials, (const F*)thr, (F*)nullptr)
    // a batch that trims: matching without a decision, the K-th distance of every pair, then the decision and the terms
#define ICP_LAUNCH_BATCH_TRIM(F, MET)                                                                                                      \
    do {                                                                                                                                   \
        hipLaunchKernelGGL((nn_match_batch<F, MET, true, true>), dim3(n_items), dim3(NN_BLOCK), 0, st, items, pairs, mode,                 \
                           (const RT<F>*)rt, (F*)P, p_plane, (const F*)Q, (const F*)nullptr, q_plane, idx_prev, idx_cur, partials,         \
                           (const F*)nullptr, (F*)dist);                                                                                   \
        hipLaunchKernelGGL((batch_trim_select<F>), dim3(n_pairs), dim3(TRIM_BLOCK), 0, st, pairs, mode, trim_rank, (const F*)dist,         \
                           (F*)tau);                                                                                                       \
        hipLaunchKernelGGL((batch_trim_moments<F, MET>), dim3(n_items), dim3(NN_BLOCK), 0, st, items, pairs, mode, (const F*)P, p_plane,   \
                           (const F*)Q, (const F*)Nrm, q_plane, idx_cur, (const F*)dist, (const F*)tau, (const F*)thr, partials);          \
    } while (0)
#define ICP_LAUNCH_BATCH_F(F)                                                                                                  \
    do {                                                                                                                       \
        if (trim_rank) {                                                                                                       \
            if (plane) ICP_LAUNCH_BATCH_TRIM(F, ICP_POINT_TO_PLANE); else ICP_LAUNCH_BATCH_TRIM(F, ICP_POINT_TO_POINT);        \
        } else if (thr) {                                                                                                      \
            if (plane) ICP_LAUNCH_BATCH(F, ICP_POINT_TO_PLANE, true); else ICP_LAUNCH_BATCH(F, ICP_POINT_TO_POINT, true);      \
        } else {                                                                                                               \
            if (plane) ICP_LAUNCH_BATCH(F, ICP_POINT_TO_PLANE, false); else ICP_LAUNCH_BATCH(F, ICP_POINT_TO_POINT, false);    \
        }                                                                                                                      \
    } while (0)
    if (precision == ICP_F64) ICP_LAUNCH_BATCH_F(double); else ICP_LAUNCH_BATCH_F(float);
#undef ICP_LAUNCH_BATCH_F
#undef ICP_LAUNCH_BATCH_TRIM
#undef ICP_LAUNCH_BATCH
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_finalize_kernel, dim3(n_pairs), dim3(256), 0, st, pairs, mode, (const double*)partials,
                       plane ? ICP_MOM_B + 5 : ICP_MOM_SQQ, mom);
    return hipGetLastError();
}

// the start cloud of every pair of a batch that holds initial transforms (icp_batch_begin): P = apply_rt(rt0[pair], P0) -- the
// front end's own arithmetic, so a loop from here is the loop of a batch created from this cloud -- or P0's bytes for a pair
// whose kind is BATCH_INIT_COPY (the exact identity: a -0.0 stays a -0.0).  Reads P0 and writes P, as the copy it replaces.
// One wave per work item (four items per block), one point per lane; the padding between the clouds is not touched.  A
// transformed point with a NaN or an infinite coordinate raises its pair's flag (zero before the launch): a plain vector store
// of 1 from every such lane, whoever comes last.
template <typename F>
__global__ __launch_bounds__(NN_BLOCK) void batch_init_kernel(const BatchItem* __restrict__ items, int n_items,
                                                              const BatchPair* __restrict__ pairs, const int* __restrict__ kind,
                                                              const RT<F>* __restrict__ rt0, const F* __restrict__ P0,
                                                              F* __restrict__ P, long long p_plane, int* __restrict__ nonfinite)
{
    const int item = blockIdx.x * (NN_BLOCK / BATCH_ITEM) + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const BatchItem it = items[item];
    const int lane = threadIdx.x & 63;
    if (lane >= it.count) return;
    const long long gi = pairs[it.pair].p_off + it.first + lane;
    F x = P0[gi], y = P0[p_plane + gi], z = P0[2 * p_plane + gi];
    if (kind[it.pair] != BATCH_INIT_COPY) {
        apply_rt<F>(rt0[it.pair], x, y, z, x, y, z);
        // (x - x is 0 for every finite x, NaN for NaN and for +-inf)
        const bool finite = (x - x) == F(0) && (y - y) == F(0) && (z - z) == F(0);
        if (!finite) nonfinite[it.pair] = 1;
    }
    P[gi] = x;
    P[p_plane + gi] = y;
    P[2 * p_plane + gi] = z;
}

hipError_t launch_batch_init(int precision, const BatchItem* items, int n_items, const BatchPair* pairs, const int* kind, const void* rt0,
                             const void* P0, void* P, long long p_plane, int* nonfinite, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    const int nb = (n_items + NN_BLOCK / BATCH_ITEM - 1) / (NN_BLOCK / BATCH_ITEM);
    if (precision == ICP_F64)
        hipLaunchKernelGGL((batch_init_kernel<double>), dim3(nb), dim3(NN_BLOCK), 0, st, items, n_items, pairs, kind, (const RT<double>*)rt0,
                           (const double*)P0, (double*)P, p_plane, nonfinite);
    else
        hipLaunchKernelGGL((batch_init_kernel<float>), dim3(nb), dim3(NN_BLOCK), 0, st, items, n_items, pairs, kind, (const RT<float>*)rt0,
                           (const float*)P0, (float*)P, p_plane, nonfinite);
    return hipGetLastError();
}

}  // namespace icp
