// icp_batch_clouds.h -- the clouds of a batch as the per-cloud kernels see them, and the packed buffer that carries them: host
// arithmetic only, no device call (tests/batch_clouds_check.cpp runs it as a program of its own).
//
// The per-cloud calls of icp_batch.cpp (downsampling, outlier removal, keypoints, covariances, descriptors, point normals) all
// number the 2 * count clouds of a batch moving clouds first, cut every cloud into work items of BATCH_ITEM points and give it a
// stretch of the call's per-point temporaries: list_clouds states that once.  The kernels that keep no per-point temporaries
// (covariances, descriptors, point normals) do not read tmp_off, so they take the same list.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "icp_kernels.h"

namespace icp {

struct CloudList {
    std::vector<VoxelCloud> clouds;   // 2 * count: cloud k < count is the moving cloud of pair k, the others the model of pair k - count (dst_off: 0)
    std::vector<BatchItem> items;     // the wanted sides' work items, in cloud order, then point order (BatchItem::pair = the cloud's number)
    long long tmp_plane = 0;          // elements of a per-point temporary: every cloud, wanted or not, at a multiple of BATCH_ALIGN
};

// the clouds of `pairs` and the work items of the sides asked for (want[0]: the moving clouds, want[1]: the models).
// false: more than INT_MAX work items -- one launch cannot number them
inline bool list_clouds(const std::vector<BatchPair>& pairs, const bool want[2], CloudList& out)
{
    const int count = (int)pairs.size();
    out.clouds.resize(2 * (size_t)count);
    out.items.clear();
    out.tmp_plane = 0;
    for (int k = 0; k < 2 * count; ++k) {
        const int side = k < count ? 0 : 1;
        const BatchPair& pr = pairs[(size_t)(k - side * count)];
        VoxelCloud& cl = out.clouds[(size_t)k];
        cl = VoxelCloud{side ? pr.q_off : pr.p_off, out.tmp_plane, 0, side ? pr.m : pr.n, side};
        out.tmp_plane += round_up(cl.n, BATCH_ALIGN);
        for (int first = 0; want[side] && first < cl.n; first += BATCH_ITEM)
            out.items.push_back(BatchItem{k, first, std::min(BATCH_ITEM, cl.n - first), 0});
    }
    return out.items.size() <= (size_t)INT_MAX;
}

// one side of a batch -- the moving clouds or the models: the caller's offsets, where each cloud starts in its plane, the plane
struct Side {
    const int64_t* off;
    std::vector<long long> dst;
    long long plane;
};

inline Side make_side(const std::vector<BatchPair>& pairs, const int64_t* off, long long plane, bool model)
{
    Side s{off, std::vector<long long>(pairs.size()), plane};
    for (size_t p = 0; p < pairs.size(); ++p) s.dst[p] = model ? pairs[p].q_off : pairs[p].p_off;
    return s;
}

// `width` values of `esize` bytes (float or double) per point of one side -- coordinates, normals, covariances, intensities,
// gradients, descriptors.  The caller holds them point after point, the clouds concatenated; the device holds them packed: as
// `width` padded planes, value k of point i of cloud p at k * plane + dst[p] + i, or as rows, at (dst[p] + i) * width + k.  The
// padding between the clouds is all-zero bytes (0.0 in both precisions, never read).
enum Layout { PLANES, ROWS };

struct Format {
    int width;
    Layout layout;
    size_t esize;
    size_t bytes(long long plane) const { return (size_t)width * (size_t)plane * esize; }
};

namespace codec {

template <typename E, int V, bool ENCODE>   // V == 0: any width, read at run time
void planes(const Side& s, int width, E* packed, E* own)
{
    const int v = V ? V : width;
    for (size_t p = 0; p < s.dst.size(); ++p)
        for (int64_t i = 0; i < s.off[p + 1] - s.off[p]; ++i)
            for (int k = 0; k < v; ++k) {
                E& in_planes = packed[(size_t)(k * s.plane + s.dst[p] + i)];
                E& in_own = own[v * (s.off[p] + i) + k];
                if (ENCODE) in_planes = in_own;
                else in_own = in_planes;
            }
}

template <typename E, bool ENCODE>
void run(const Format& f, const Side& s, void* packed_v, void* own_v)
{
    E* packed = static_cast<E*>(packed_v);
    E* own = static_cast<E*>(own_v);
    if (f.layout == ROWS) {   // a cloud's rows are one stretch on both sides
        for (size_t p = 0; p < s.dst.size(); ++p) {
            E* a = packed + (size_t)f.width * (size_t)s.dst[p];
            E* b = own + (size_t)f.width * (size_t)s.off[p];
            const size_t bytes = (size_t)f.width * (size_t)(s.off[p + 1] - s.off[p]) * sizeof(E);
            if (ENCODE) std::memcpy(a, b, bytes);
            else std::memcpy(b, a, bytes);
        }
        return;
    }
    switch (f.width) {   // (the widths the batch has, each with its own inner loop)
    case 1: return planes<E, 1, ENCODE>(s, 1, packed, own);
    case 3: return planes<E, 3, ENCODE>(s, 3, packed, own);
    case 6: return planes<E, 6, ENCODE>(s, 6, packed, own);
    default: return planes<E, 0, ENCODE>(s, f.width, packed, own);
    }
}

}  // namespace codec

// the caller's values -> `raw`, packed (resized, the padding zeroed), and packed values -> the caller's array
inline void encode(const Format& f, const Side& s, const void* own, std::vector<char>& raw)
{
    raw.assign(f.bytes(s.plane), 0);
    if (f.esize == sizeof(double)) codec::run<double, true>(f, s, raw.data(), const_cast<void*>(own));
    else codec::run<float, true>(f, s, raw.data(), const_cast<void*>(own));
}

inline void decode(const Format& f, const Side& s, const void* packed, void* own)
{
    if (f.esize == sizeof(double)) codec::run<double, false>(f, s, const_cast<void*>(packed), own);
    else codec::run<float, false>(f, s, const_cast<void*>(packed), own);
}

// one buffer for a launch's clouds, its work items and n_ints ints (every cloud's k; 0: none): where each region starts -- at a
// 16-byte boundary -- and the bytes of the whole
struct ArgsLayout {
    size_t off_items, off_ints, bytes;
};

inline ArgsLayout lay_out_args(size_t n_clouds, size_t n_items, size_t n_ints)
{
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    ArgsLayout l{};
    l.off_items = up16(n_clouds * sizeof(VoxelCloud));
    l.off_ints = l.off_items + up16(n_items * sizeof(BatchItem));
    l.bytes = l.off_ints + n_ints * sizeof(int);
    return l;
}

}  // namespace icp
