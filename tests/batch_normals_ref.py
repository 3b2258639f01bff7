"""What the point-normal tests share (tests/test_batch_normals_ref.py, test_batch_normals_abi.py, test_gpu_batch_normals.py): the rule
of icp_batch_estimate_point_normals in numpy, bit for bit as include/icp_mi355x.h states it.  Nothing here touches a device.

    Jacobi      icp_eigh3's statements on six arrays a00 .. a22 and nine arrays v00 .. v22, every point at once, in the manner of
                batch_keypoint_ref.jacobi_eigenvalues: a point that has met the stop test, and a rotation whose apq is exactly 0,
                keep their values through np.where -- elementwise IEEE operations keep the bits
    column      the three compare-and-swaps of the order with the strict <, the column carried along by np.where
    non-finite  a normal with a component that is not finite is exactly (0.0, 0.0, 0.0)
    flip        to = v - x in float64, dt = (nx*tox + ny*toy) + nz*toz, negated iff dt < 0
    centroid    256 strided partial sums per axis, each from 0.0 in ascending j, added from 0.0 in ascending t, divided by n
                (np.add.accumulate adds sequentially; np.sum adds pairwise: not used)
"""
import numpy as np

from batch_keypoint_ref import SWEEPS, range_scale

NONE, VIEWPOINT, CENTROID = 0, 1, 2   # ICP_ORIENT_NONE, ICP_ORIENT_VIEWPOINT, ICP_ORIENT_CENTROID
LANES = 256                            # the partial sums of the centroid


def jacobi(C, _scale=True):
    """(w (3, n) ascending, n (3, n): column ord[0] of v, Z (3, 3, n): v's columns in the order of w) of the symmetric matrices given
    as (6, n) xx, xy, xz, yy, yz, zz -- icp_eigh3's statements with the updates of v, behind its range rule
    (batch_keypoint_ref.range_scale; w is scaled back).  _scale=False leaves the range rule out (the statements as they were before
    it: the anchor of tests/test_batch_range_ref.py)"""
    a00, a01, a02, a11, a12, a22 = (np.array(C[o], dtype=np.float64, copy=True) for o in range(6))
    unscale = 1.0
    if _scale:
        (a00, a01, a02, a11, a12, a22), unscale = range_scale((a00, a01, a02, a11, a12, a22))
    one, zero = np.ones(a00.shape), np.zeros(a00.shape)
    v = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]   # v[row][column]
    live = np.ones(a00.shape, dtype=bool)

    def rotate(live, apq, app, aqq, arp, arq, p, q):
        """one rotation's statements where `live` and apq != 0: (app', aqq', apq', arp', arq'); columns p and q of v in place"""
        do = live & ~(apq == 0.0)                                # (a NaN apq rotates, as the C loop does)
        theta = (aqq - app) / (2.0 * apq)
        t = np.copysign(1.0, theta) / (np.fabs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        for k in range(3):
            vp, vq = v[k][p], v[k][q]
            v[k][p], v[k][q] = np.where(do, c * vp - s * vq, vp), np.where(do, s * vp + c * vq, vq)
        return (np.where(do, app - t * apq, app), np.where(do, aqq + t * apq, aqq), np.where(do, 0.0, apq),
                np.where(do, c * arp - s * arq, arp), np.where(do, s * arp + c * arq, arq))

    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        for _ in range(SWEEPS):
            off = a01 * a01 + a02 * a02 + a12 * a12
            dia = a00 * a00 + a11 * a11 + a22 * a22
            live = live & ~((off <= 1e-34 * dia) | (off == 0.0))
            if not live.any():
                break
            a00, a11, a01, a02, a12 = rotate(live, a01, a00, a11, a02, a12, 0, 1)   # (0, 1), r = 2
            a00, a22, a02, a01, a12 = rotate(live, a02, a00, a22, a01, a12, 0, 2)   # (0, 2), r = 1
            a11, a22, a12, a01, a02 = rotate(live, a12, a11, a22, a01, a02, 1, 2)   # (1, 2), r = 0
        w = [a00, a11, a22]
        col = [np.stack([v[0][k], v[1][k], v[2][k]]) for k in range(3)]
        for i, j in ((0, 1), (0, 2), (1, 2)):                    # the ascending order, icp_eigh3's three compare-and-swaps
            lt = w[j] < w[i]
            w[i], w[j] = np.where(lt, w[j], w[i]), np.where(lt, w[i], w[j])
            col[i], col[j] = np.where(lt[None, :], col[j], col[i]), np.where(lt[None, :], col[i], col[j])
        if _scale:                                               # scaled back once the order is fixed
            w = [x * unscale for x in w]
    return np.stack(w), col[0], np.stack(col, axis=1)


def centroid(X):
    """(3,) float64: the rule's centroid of one cloud"""
    X64 = np.asarray(X).astype(np.float64)
    n = X64.shape[0]
    out = np.empty(3)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            part = np.zeros(LANES)
            for t in range(min(LANES, n)):
                part[t] = np.add.accumulate(np.concatenate([[0.0], X64[t::LANES, a]]))[-1]
            total = np.add.accumulate(np.concatenate([[0.0], part]))[-1]
            out[a] = total / np.float64(n)
    return out


def normals(X, cov6, orient=CENTROID, viewpoint=None):
    """(n, 3) float64: the rule's normals of one cloud X (n, 3) with the covariances cov6 (n, 6); viewpoint (3,) with VIEWPOINT"""
    X = np.asarray(X)
    _, nv, _ = jacobi(np.asarray(cov6, dtype=np.float64).T)
    ok = np.isfinite(nv).all(axis=0)
    nv = np.where(ok[None, :], nv, 0.0)
    if orient != NONE:
        view = centroid(X) if orient == CENTROID else np.asarray(viewpoint, dtype=np.float64)
        X64 = X.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            to = [view[a] - X64[:, a] for a in range(3)]
            dt = (nv[0] * to[0] + nv[1] * to[1]) + nv[2] * to[2]
        nv = np.where((dt < 0)[None, :], -nv, nv)
    return np.ascontiguousarray(nv.T)


def normals_pairs(pairs, covs_m, covs_q, orient=CENTROID, viewpoints=None):
    """the reference of a whole batch: (moving, model), per pair the (points, 3) normals; viewpoints: (moving, model), each (count, 3)"""
    vm = [None] * len(pairs) if viewpoints is None else viewpoints[0]
    vq = [None] * len(pairs) if viewpoints is None else viewpoints[1]
    return ([normals(p[0], c, orient, v) for p, c, v in zip(pairs, covs_m, vm)],
            [normals(p[1], c, orient, v) for p, c, v in zip(pairs, covs_q, vq)])
