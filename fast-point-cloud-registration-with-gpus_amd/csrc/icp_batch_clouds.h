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
