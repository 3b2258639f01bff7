"""What the outlier-removal tests share (tests/test_batch_outlier_ref.py, tests/test_gpu_batch_outlier.py): the rules of
icp_batch_remove_outliers in numpy, bit for bit as include/icp_mi355x.h states them, and the clouds both files use.  Nothing
here touches a device.

    distance    d2(i, j) = (dx*dx + dy*dy) + dz*dz on arrays of the cloud's own dtype F: numpy rounds every elementwise operation
                separately.  Row blocks of a distance matrix; the diagonal (j == i, by index) is taken out, so a coincident point
                counts at distance 0
    k smallest  np.partition + np.sort: a multiset has one ascending order whatever the ties
    dbar        the k values widened to float64, np.sqrt (correctly rounded), added from the smallest to the largest from 0.0 in
                an explicit loop over k, divided once by float64(k)
    sums        explicit Python loops: a granule of 64 consecutive points from 0.0 in ascending index, the granule sums from 0.0
                in ascending granule order.  (np.sum adds pairwise: not used)
    statistic   mean = S / n, dev = dbar - mean, q = dev * dev, std = sqrt(Qsum / (n - 1)), thr = mean + a * std; keep dbar <= thr
    radius      thr2 = F(r * r) with the product in float64; c = #{j != i: d2 <= thr2}; keep c >= min
"""
import numpy as np

import batch_ref
import batch_voxel_ref as vr

GRANULE = 64          # BATCH_ITEM: the work item and the granule of the ordered sums
MAX_K = 32            # ICP_OUTLIER_MAX_NEIGHBOURS
MAX_POINTS = vr.MAX_POINTS
ROWS = 256            # rows per block of the distance matrix


def d2_rows(X, i0, i1):
    """(i1 - i0, n) of dtype F: the squared distances of points i0 .. i1-1 to every point, the matching's expression"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = X[i0:i1, None, :] - X[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dbar(X, k, rows=None):
    """float64 per point (or per point of `rows`): the mean distance to the k nearest other points"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    assert 1 <= k <= MAX_K and n >= k + 1
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.empty(rows.size, dtype=np.float64)
    for b in range(0, rows.size, ROWS):
        r = rows[b:b + ROWS]
        d = np.stack([d2_rows(X, i, i + 1)[0] for i in r]) if rows.size != n else d2_rows(X, b, min(b + ROWS, n))
        d[np.arange(r.size), r] = np.inf                               # j != i, by index
        small = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)  # the k smallest, ascending
        with np.errstate(invalid="ignore"):
            root = np.sqrt(small.astype(np.float64))
        s = np.zeros(r.size, dtype=np.float64)
        for j in range(k):                                             # from the smallest to the largest, starting at 0.0
            s = s + root[:, j]
        out[b:b + ROWS] = s / np.float64(k)
    return out


def counts(X, r):
    """(int64 per point, thr2 as F): the other points within r"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    with np.errstate(over="ignore"):
        thr2 = X.dtype.type(np.float64(r) * np.float64(r))
    c = np.empty(n, dtype=np.int64)
    for b in range(0, n, ROWS):
        d = d2_rows(X, b, min(b + ROWS, n))
        inside = d <= thr2
        inside[np.arange(d.shape[0]), np.arange(b, b + d.shape[0])] = False   # j != i
        c[b:b + ROWS] = inside.sum(axis=1)
    return c, thr2


def ordered_sum(x, granule=GRANULE):
    """the sum of the float64 values x in the order of the rule"""
    total = 0.0
    for g in range(0, len(x), granule):
        s = 0.0
        for v in x[g:g + granule].tolist():
            s += v
        total += s
    return total


def statistic(score, a, granule=GRANULE):
    """(mean, std, thr, keep) of a statistical cloud from its dbar"""
    score = np.asarray(score, dtype=np.float64)
    n = score.size
    with np.errstate(over="ignore", invalid="ignore"):
        mean = np.float64(ordered_sum(score, granule)) / np.float64(n)
        dev = score - mean
        q = dev * dev
        std = np.sqrt(np.float64(ordered_sum(q, granule)) / np.float64(n - 1))
        scaled = np.float64(a) * std
        thr = mean + scaled
    return float(mean), float(std), float(thr), score <= thr


def remove(X, rule, score=None):
    """(Y, map int32, score float64, stats [mean, std, thr, kept]) of one cloud; rule: None, ("statistical", k, a) or
    ("radius", r, min).  score: use these scores instead of computing them (the largest cloud: the device's own)"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    if rule is None:
        return X.copy(), np.arange(n, dtype=np.int32), np.zeros(n), np.array([0.0, 0.0, 0.0, float(n)])
    if rule[0] == "statistical":
        _, k, a = rule
        score = dbar(X, k) if score is None else np.asarray(score, dtype=np.float64)
        mean, std, thr, keep = statistic(score, a)
        assert np.isfinite(mean) and np.isfinite(std)
    else:
        _, r, least = rule
        assert rule[0] == "radius" and np.isfinite(r) and r > 0 and 1 <= least <= 65535
        c, thr2 = counts(X, r)
        score = c.astype(np.float64) if score is None else np.asarray(score, dtype=np.float64)
        mean, std, thr, keep = 0.0, 0.0, float(thr2), score >= float(least)
    m = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return X[keep].copy(), m, score, np.array([mean, std, thr, float(keep.sum())])


def per_pair(rules, count):
    one = rules is None or (isinstance(rules, tuple) and len(rules) == 3 and isinstance(rules[0], str))
    return [rules] * count if one else list(rules)


def remove_pairs(pairs, moving, model):
    """the reference of a whole batch: clouds [(Y_D, Y_M)], maps and scores per side, stats (2 * count, 4) moving clouds first"""
    rm, rq = per_pair(moving, len(pairs)), per_pair(model, len(pairs))
    D = [remove(p[0], r) for p, r in zip(pairs, rm)]
    M = [remove(p[1], r) for p, r in zip(pairs, rq)]
    return dict(clouds=[(d[0], m[0]) for d, m in zip(D, M)], moving_map=[d[1] for d in D], model_map=[m[1] for m in M],
                moving_score=[d[2] for d in D], model_score=[m[2] for m in M], stats=np.stack([d[3] for d in D] + [m[3] for m in M]))


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------
normal = vr.normal


def lattice(dtype, side=8, step=0.5):
    """side^3 points k * step in index order: every distance is exact, and every quarter boundary carries equal distances"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3) * step
    return np.ascontiguousarray(g.astype(dtype))


SHEET_SIDE, SHEET_PLANTED = 24, 30


def sheet(seed, dtype):
    """(X, planted): a jittered 24 x 24 sheet z = x^2 - y^2 over [-1, 1]^2 plus 30 far points planted at 2.5 to 12 from the
    origin in random directions, 606 points in all, shuffled; planted[i]: point i is a planted one"""
    rng = np.random.default_rng(seed)
    u = np.linspace(-1.0, 1.0, SHEET_SIDE)
    x, y = [a.reshape(-1) + rng.normal(0.0, 0.01, SHEET_SIDE * SHEET_SIDE) for a in np.meshgrid(u, u, indexing="ij")]
    S = np.stack([x, y, x * x - y * y + rng.normal(0.0, 0.005, x.size)], -1)
    v = rng.standard_normal((SHEET_PLANTED, 3))
    P = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.5, 12.0, (SHEET_PLANTED, 1))
    X = np.concatenate([S, P])
    planted = np.arange(X.shape[0]) >= S.shape[0]
    order = rng.permutation(X.shape[0])
    return np.ascontiguousarray(X[order].astype(dtype)), planted[order]


def coincident(dtype):
    """300 points of which 40 coincide (batch_ref.knn_models' last cloud)"""
    return vr.coincident(dtype)


def far(dtype):
    """normal points carried 1e4 from the origin"""
    return vr.far(dtype)


def order_sensitive():
    """130 float64 scores whose sum depends on the order: the granule order gives another last bit of the mean than one running
    sum over all points or numpy's pairwise sum"""
    x = np.full(130, 0.1)
    x[0] = 1e16
    x[64] = -1e16
    x[65:] = 0.3
    return x


def threshold_cloud(dtype):
    """points on the integer lattice 5 x 5 x 5 with r = 1, sqrt(2) and sqrt(3) rounded: counts decided by d2 == thr2 exactly (1) or
    by how r * r rounds to F (2 and 3)"""
    return lattice(dtype, side=5, step=1.0)
