"""What the voxel-grid tests share (tests/test_batch_voxel_ref.py, tests/test_gpu_batch_voxel.py): the rule of
icp_batch_downsample in numpy, bit for bit as include/icp_mi355x.h states it, a plain Python loop that says the same thing more
slowly, and the clouds both files use.  Nothing here touches a device.

    cell        c = floor(((double)x - (double)lo) / v) per axis, lo the component-wise minimum: numpy's float64 subtract, true
                divide and floor are one IEEE operation each
    cells       ordered by first occurrence: np.unique(key, return_index, return_inverse), re-ordered by return_index
    sums        np.bincount(rank, weights=x.astype(float64)) adds sequentially in input order starting from 0.0 -- the rule.
                (np.sum and np.add.reduceat add pairwise: not used)
    points      (F)(s / (double)c); a cell of one point gets that point's bytes instead
"""
import numpy as np

import batch_ref

MAX_CELL = 2097151   # 21 bits per axis
TILE = 512           # VOXEL_TILE: keys per LDS tile of batch_voxel_group (csrc/icp_kernels.h)
SCAN = 256           # VOXEL_SCAN_BLOCK: a chunk of batch_voxel_rank's scan
MAX_POINTS = 65536   # ICP_BATCH_MAX_POINTS


def cells(X, v):
    """(n, 3) int64: the cell of every point"""
    lo = X.min(axis=0)
    q = (X.astype(np.float64) - lo.astype(np.float64)) / np.float64(v)
    return np.floor(q).astype(np.int64)


def top_cell(X, v):
    """the largest cell index of any axis, as the library's range check computes it (a float: it may be inf)"""
    lo, hi = X.min(axis=0).astype(np.float64), X.max(axis=0).astype(np.float64)
    with np.errstate(over="ignore"):
        return float(np.floor((hi - lo) / np.float64(v)).max())


def downsample(X, v):
    """(Y, map, population): the thinned cloud, every source point's output index (int32), every output point's member count"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    if v == 0:
        return X.copy(), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int64)
    assert np.isfinite(v) and v > 0
    c = cells(X, v)
    assert c.min() >= 0 and c.max() <= MAX_CELL and top_cell(X, v) == c.max()
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # the sorted cells, by first occurrence
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    m = rank[inv.reshape(-1)]
    pop = np.bincount(m, minlength=order.size)
    Y = np.empty((order.size, 3), dtype=X.dtype)
    for k in range(3):
        s = np.bincount(m, weights=X[:, k].astype(np.float64), minlength=order.size)
        Y[:, k] = (s / pop.astype(np.float64)).astype(X.dtype)
    src = first[order]
    Y[pop == 1] = X[src[pop == 1]]                    # copied, not computed
    return Y, m.astype(np.int32), pop


def downsample_loop(X, v):
    """the same rule as a Python loop over the points (small clouds only)"""
    X = np.ascontiguousarray(X)
    F = X.dtype.type
    if v == 0:
        return X.copy(), np.arange(X.shape[0], dtype=np.int32)
    lo = [float(X[:, k].min()) for k in range(3)]
    seen, members = {}, []
    m = np.empty(X.shape[0], dtype=np.int32)
    for i in range(X.shape[0]):
        cell = tuple(int(np.floor((float(X[i, k]) - lo[k]) / float(v))) for k in range(3))
        if cell not in seen:
            seen[cell] = len(members)
            members.append([])
        m[i] = seen[cell]
        members[m[i]].append(i)
    Y = np.empty((len(members), 3), dtype=X.dtype)
    for r, mem in enumerate(members):
        if len(mem) == 1:
            Y[r] = X[mem[0]]
            continue
        for k in range(3):
            s = 0.0
            for i in mem:
                s += float(X[i, k])
            Y[r, k] = F(s / float(len(mem)))
    return Y, m


def downsample_pairs(pairs, vm, vq):
    """the reference of a whole batch: [(Y_D, Y_M)], [map_D], [map_M]"""
    out, mm, qm = [], [], []
    for (D, M), a, b in zip(pairs, vm, vq):
        YD, mD, _ = downsample(D, a)
        YM, mM, _ = downsample(M, b)
        out.append((YD, YM))
        mm.append(mD)
        qm.append(mM)
    return out, mm, qm


def offsets(clouds):
    return np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------
def normal(n, seed, dtype):
    X = np.random.default_rng(seed).standard_normal((n, 3))
    return np.ascontiguousarray(X.astype(dtype))     # (fp64: all 53 bits random; fp32: rounded once)


def identity_voxel(X):
    """extent / 2e6: every cell index stays inside the 21 bits, and distinct random points are all alone"""
    lo, hi = X.min(axis=0).astype(np.float64), X.max(axis=0).astype(np.float64)
    return float((hi - lo).max() / 2e6)


# 1. granules: a work item of 64 points, the key tile, a chunk of the scan
GRANULE_N = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, SCAN - 1, SCAN + 1)
GRANULE_V = 0.5   # standard normal points: the cells near the origin hold up to about ten points, the outer ones a single one


def granule_pairs(dtype):
    """one pair per size; the models cycle through other sizes of the same list"""
    k = len(GRANULE_N)
    return [(normal(n, 100 + b, dtype), normal(GRANULE_N[(b + 4) % k], 200 + b, dtype)) for b, n in enumerate(GRANULE_N)]


# 2. extremes
def coincident(dtype):
    """300 points of which 40 coincide (batch_ref.knn_models' last cloud)"""
    return np.ascontiguousarray(batch_ref.knn_models(dtype, sizes=())[-1].astype(dtype))


def signed_zeros(dtype):
    """normal points with -0.0 coordinates: one point with a single one, one with two, one that is (-0.0, -0.0, -0.0), and a
    far point that is alone in its cell at GRANULE_V and carries one"""
    X = normal(200, 77, dtype)
    X[5, 1] = -0.0
    X[9, 0] = X[9, 2] = -0.0
    X[17] = -0.0
    X[33] = (7.25, -0.0, -6.5)
    return X


# 3. boundaries
def half_lattice(dtype):
    """k * 0.5 on a 9 x 9 x 5 lattice, shuffled; with v = 1.0 every quotient is exact: 5 x 5 x 3 cells of 1, 2, 4 or 8 points"""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 3) * 0.5
    return np.ascontiguousarray(np.random.default_rng(3).permutation(g).astype(dtype))


def tenth_lattice(dtype):
    """(X, K): k * 0.1, formed in double, on a 48 x 6 x 2 lattice, shuffled, and the integers k; with v = 0.1 some quotients round
    below the integer (in double the first is k = 43: 4.3 / 0.1 = 42.99..., in fp32 already k = 7): the cell is not k everywhere"""
    K = np.stack(np.meshgrid(np.arange(48), np.arange(6), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    K = np.random.default_rng(4).permutation(K)
    return np.ascontiguousarray((K * 0.1).astype(dtype)), K


def far(dtype):
    """normal points carried 1e4 from the origin"""
    return np.ascontiguousarray((np.random.default_rng(8).standard_normal((400, 3)) + 1e4).astype(dtype))


def negative(dtype):
    return np.ascontiguousarray((np.random.default_rng(9).standard_normal((400, 3)) - np.array([50.0, 3.0, 0.5])).astype(dtype))
