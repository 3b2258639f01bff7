"""What the keypoint tests share (tests/test_batch_keypoint_ref.py, test_batch_keypoint_abi.py, test_gpu_batch_keypoint.py): the
ISS rule of icp_batch_select_keypoints in numpy, bit for bit as include/icp_mi355x.h states it, and the dense bunny pair both the
CPU and the GPU end-to-end tests use.  Nothing here touches a device.

    distance    d2(i, j) = (dx*dx + dy*dy) + dz*dz on arrays of the cloud's own dtype F (batch_outlier_ref.d2_rows), in row blocks;
                ts = F(rs * rs) and tn = F(rn * rn) with the products in float64; the diagonal stays in: i belongs to both of its
                neighbourhoods, at distance 0
    sums        np.nonzero lists a row's neighbours in ascending j; the r-th neighbour of every row is added in step r, so each
                row's nine sums run in ascending j from 0.0.  (np.sum adds pairwise: not used)
    covariance  C_ab = (S_ab - (s_a * s_b) / c) / c, one numpy operation per rounding
    Jacobi      icp_eigh3's statements on six arrays a00 .. a22, every point at once: a point that has met the stop test, and a
                rotation whose apq is exactly 0, keep their values through np.where -- elementwise IEEE operations keep the bits
    range       a matrix whose largest magnitude lies beyond 2^+-400 is solved times 2^-+600 and its eigenvalues are scaled back
                after the ascending order is fixed (range_scale): sal_i and the two ratio tests see the scaled-back values
    selection   integer counts and comparisons over the non-max neighbourhood
"""
import os

import numpy as np

import batch_feature_ref as fr
import batch_outlier_ref as orf

NONE, ISS = 0, 1            # ICP_KEYPOINT_NONE, ICP_KEYPOINT_ISS
ROWS = 256                  # rows per block of the distance matrix
SWEEPS = 64


def rule(salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbours=5):
    """the tuple Batch.keypoints takes, with its defaults"""
    return (float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbours))


def threshold(dtype, r):
    """F(r * r), the product formed in float64 and rounded once"""
    with np.errstate(over="ignore"):
        return np.dtype(dtype).type(np.float64(r) * np.float64(r))


def within(X, r):
    """(n, n) bool: d2(i, j) <= F(r * r), the diagonal included"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    t = threshold(X.dtype, r)
    out = np.empty((n, n), dtype=bool)
    for b in range(0, n, ROWS):
        out[b:b + ROWS] = orf.d2_rows(X, b, min(b + ROWS, n)) <= t   # (a NaN distance: False)
    return out


def covariances(X, inside):
    """(c (n,) int64, C (6, n) float64: xx, xy, xz, yy, yz, zz) over the neighbourhoods `inside`, the sums in ascending j"""
    n = X.shape[0]
    X64 = X.astype(np.float64)
    ii, jj = np.nonzero(inside)                                  # row-major: ascending j within a row
    start = np.searchsorted(ii, np.arange(n))
    count = np.bincount(ii, minlength=n)
    s = np.zeros((3, n))
    S = np.zeros((6, n))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r in range(int(count.max()) if n else 0):
            rows = np.flatnonzero(count > r)
            j = jj[start[rows] + r]
            e = [X64[j, a] - X64[rows, a] for a in range(3)]
            for a in range(3):
                s[a, rows] = s[a, rows] + e[a]
            for o, (a, b) in enumerate(pairs):
                S[o, rows] = S[o, rows] + e[a] * e[b]
        c = count.astype(np.float64)
        C = np.stack([(S[o] - (s[a] * s[b]) / c) / c for o, (a, b) in enumerate(pairs)])
    return count, C


def range_scale(a6):
    """(the six arrays times sc, unscale (n,)): the range rule of icp_eigh3 and of the Frobenius regularisation.  amax = the largest
    magnitude of the six entries; a matrix with six finite entries and amax > 2^400 is multiplied by 2^-600, one with
    0 < amax < 2^-400 by 2^+600 (sc), and unscale = 1 / sc scales an eigenvalue back; sc = unscale = 1.0 for every other matrix,
    whose bits a multiplication by 1.0 keeps"""
    a6 = [np.asarray(a, dtype=np.float64) for a in a6]
    amax = np.zeros(a6[0].shape)
    finite = np.ones(a6[0].shape, dtype=bool)
    for a in a6:
        amax = np.fmax(amax, np.fabs(a))                          # (fmax drops a NaN)
        finite &= np.isfinite(a)
    big = finite & (amax > 2.0 ** 400)
    small = finite & (amax < 2.0 ** -400) & (amax > 0.0)
    sc = np.where(big, 2.0 ** -600, np.where(small, 2.0 ** 600, 1.0))
    unscale = np.where(big, 2.0 ** 600, np.where(small, 2.0 ** -600, 1.0))
    scaled = [np.where(big | small, a * sc, a) for a in a6]       # (the others: not multiplied at all)
    return scaled, unscale


def jacobi_eigenvalues(C, _scale=True):
    """(3, n) float64, ascending per point: icp_eigh3's eigenvalues of the symmetric matrices given as (6, n) xx, xy, xz, yy, yz, zz.
    _scale=False leaves the range rule out (the statements as they were before it: the anchor of tests/test_batch_range_ref.py)"""
    a00, a01, a02, a11, a12, a22 = (np.array(C[o], dtype=np.float64, copy=True) for o in range(6))
    unscale = 1.0
    if _scale:
        (a00, a01, a02, a11, a12, a22), unscale = range_scale((a00, a01, a02, a11, a12, a22))
    live = np.ones(a00.shape, dtype=bool)                        # the point has not met the stop test yet

    def rotate(live, apq, app, aqq, arp, arq):
        """one rotation's statements where `live` and apq != 0: (app', aqq', apq', arp', arq')"""
        do = live & ~(apq == 0.0)                                # (a NaN apq rotates, as the C loop does)
        theta = (aqq - app) / (2.0 * apq)
        t = np.copysign(1.0, theta) / (np.fabs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        return (np.where(do, app - t * apq, app), np.where(do, aqq + t * apq, aqq), np.where(do, 0.0, apq),
                np.where(do, c * arp - s * arq, arp), np.where(do, s * arp + c * arq, arq))

    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        for _ in range(SWEEPS):
            off = a01 * a01 + a02 * a02 + a12 * a12
            dia = a00 * a00 + a11 * a11 + a22 * a22
            live = live & ~((off <= 1e-34 * dia) | (off == 0.0))
            if not live.any():
                break
            a00, a11, a01, a02, a12 = rotate(live, a01, a00, a11, a02, a12)   # (0, 1), r = 2
            a00, a22, a02, a01, a12 = rotate(live, a02, a00, a22, a01, a12)   # (0, 2), r = 1
            a11, a22, a12, a01, a02 = rotate(live, a12, a11, a22, a01, a02)   # (1, 2), r = 0
        w0, w1, w2 = a00, a11, a22
        lt = w1 < w0                                             # the ascending order, icp_eigh3's three compare-and-swaps
        w0, w1 = np.where(lt, w1, w0), np.where(lt, w0, w1)
        lt = w2 < w0
        w0, w2 = np.where(lt, w2, w0), np.where(lt, w0, w2)
        lt = w2 < w1
        w1, w2 = np.where(lt, w2, w1), np.where(lt, w1, w2)
        if _scale:                                               # scaled back once the order is fixed
            w0, w1, w2 = w0 * unscale, w1 * unscale, w2 * unscale
    return np.stack([w0, w1, w2])


def saliency(X, r):
    """(n,) float64: sal_i of every point of the cloud X under the rule r"""
    rs, _, g21, g32, least = r
    X = np.ascontiguousarray(X)
    c, C = covariances(X, within(X, rs))
    w = jacobi_eigenvalues(C)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ok = (c >= least) & ((w[1] / w[2]) < g21) & ((w[0] / w[1]) < g32) & (w[0] > 0)
    return np.where(ok, w[0], 0.0)


def select(X, r, sal=None):
    """(keep (n,) bool, sal (n,) float64) of one cloud under the rule r"""
    _, rn, _, _, least = r
    X = np.ascontiguousarray(X)
    sal = saliency(X, r) if sal is None else np.asarray(sal, dtype=np.float64)
    M = within(X, rn)
    size = M.sum(axis=1)
    higher = (M & (sal[None, :] > sal[:, None])).any(axis=1)
    return (sal > 0) & (size >= least) & ~higher, sal


def keypoints(X, r):
    """(Y, map int32, sal float64) of one cloud; r: None (copy) or a rule"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    if r is None:
        return X.copy(), np.arange(n, dtype=np.int32), np.zeros(n)
    keep, sal = select(X, r)
    m = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return X[keep].copy(), m, sal


def per_pair(rules, count):
    one = rules is None or (isinstance(rules, tuple) and len(rules) > 0 and np.isscalar(rules[0]))   # one rule: a tuple of numbers
    return [rules] * count if one else list(rules)


def keypoint_pairs(pairs, moving, model):
    """the reference of a whole batch: clouds [(Y_D, Y_M)], maps and saliencies per side, counts (2 * count,) moving clouds first"""
    rm, rq = per_pair(moving, len(pairs)), per_pair(model, len(pairs))
    D = [keypoints(p[0], r) for p, r in zip(pairs, rm)]
    M = [keypoints(p[1], r) for p, r in zip(pairs, rq)]
    return dict(clouds=[(d[0], m[0]) for d, m in zip(D, M)], moving_map=[d[1] for d in D], model_map=[m[1] for m in M],
                moving_saliency=[d[2] for d in D], model_saliency=[m[2] for m in M],
                counts=np.array([d[0].shape[0] for d in D] + [m[0].shape[0] for m in M], dtype=np.int32))


# ---- the dense bunny pair ----------------------------------------------------------------------------------------------------------
DENSE_STEP = 6
DENSE_RULE = rule(0.007, 0.00525, 0.975, 0.975, 5)


def dense_bunny_pair(golden):
    """every 6th point of the bunny from 0, turned 149 degrees about (1, 2, 3) and shifted by batch_feature_ref.BUNNY_T, against
    every 6th from 3 -- 5 992 and 5 991 points, disjoint samples.  (moving, model, T_true): T_true carries the moving cloud onto
    the model"""
    B = np.fromfile(os.path.join(golden, "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::DENSE_STEP], np.ascontiguousarray(B[3::DENSE_STEP])
    R = fr.rodrigues((1.0, 2.0, 3.0), 149.0)
    moving = np.ascontiguousarray((src.astype(np.float64) @ R.T + fr.BUNNY_T).astype(np.float32))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ fr.BUNNY_T
    return moving, model, T


_DENSE = {}


def dense_bunny_keypoints(golden):
    """[(Y, map, sal) of the moving cloud, of the model] under DENSE_RULE, computed once per session and left unchanged"""
    if "kept" not in _DENSE:
        A, M, _ = dense_bunny_pair(golden)
        _DENSE["kept"] = [keypoints(A, DENSE_RULE), keypoints(M, DENSE_RULE)]
    return _DENSE["kept"]
