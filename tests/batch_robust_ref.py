"""What the tests of a batch's robust kernels share (tests/test_batch_robust_ref.py, test_batch_robust_abi.py,
test_gpu_batch_robust.py): the weight functions and the residuals as include/icp_mi355x.h states them (icp_batch_set_robust), exact
weighted moment sums, a numpy loop of iteratively re-weighted least squares for both metrics, and the two bounds the GPU tests
hold the device to.  Everything else comes from batch_ref.py and ref_moments.py, which this module only imports.

The rule.  Every kept match (p, q = Q[idx], n = N[idx]) of a robust pair has a residual, formed in double from the widened
coordinates -- point-to-point r2 = dx*dx + dy*dy + dz*dz with d = q - p, point-to-plane r2 = bi*bi with bi = (px-qx)*nx +
(py-qy)*ny + (pz-qz)*nz -- and a weight, formed in double with k2 = k*k:

    huber   r2 <= k2 ? 1 : k / sqrt(r2)          cauchy   1 / (1 + r2 / k2)          tukey   r2 <= k2 ? (1 - r2/k2)^2 : 0

CNT stays the kept count, W = sum w, every other slot of the pass is the term ref_moments states times the point's w.

Bound 1 -- the sums against the device's OWN downloaded weights.  A double weight is an integer times a power of two, as the
coordinates are, so sum w_i term_i is formed exactly in Python integers and rounded once (weighted()).  Its majorant is
ref_moments' majorant with every term scaled by w_i >= 0.  The device forms the term as ref_moments describes (at most 8 roundings)
and multiplies it by w: one rounding more, 9 per term, then adds n terms in some fixed order: (n - 1) + 9 roundings of at most u
A_s each to first order.  ref_moments.tolerance books 2 (n + 16) u A_s for (n - 1) + 8; with the one multiplication more

    tol_s = 2 (n + 17) 2^-53 A_s                                                                                  (tolerance())

W itself is a sum of n given numbers: no term rounding at all, inside the same bound with A_W = sum w.

Bound 2 -- the weights against the formula.  w_ref is the formula applied to r2 formed exactly (Python integers) and rounded once
(residual_sq_exact).  Two things separate the device's weight from it:
  * the device's r: every operation of the residual rounded in double.  Point-to-point: the three differences (u each, relative),
    three squares, two additions, every term >= 0, so r2_dev = r2 (1 + e), |e| <= 6u, and r_dev = r (1 + e / 2): |dr| <= 3u r <=
    3u A_r with A_r = sqrt(sum (|q_a| + |p_a|)^2) >= r.  Point-to-plane: bi is three differences, three products and two additions,
    |d bi| <= 5u A_r with A_r = sum (|p_a| + |q_a|) |n_a|, ref_moments.plane_terms_abs's majorant of bi; r = |bi| and the square
    adds u r / 2.  Either way |dr| <= 8u A_r.
  * the formula itself, evaluated in double from r2: at most a division, an addition, a subtraction and a product or a square
    root and a division, each u relative on values <= 1 -- below 8u absolute, the rounding of w_ref included.
|dw/dr| is at most 1/k for Huber (k / r^2 at r = k), 0.65/k for Cauchy ((2 r / k^2) / (1 + r^2/k^2)^2 at r = k / sqrt 3) and
1.54/k for Tukey ((4 r / k^2)(1 - r^2/k^2) at r = k / sqrt 3): 2/k bounds all three.  Hence

    |w_dev - w_ref| <= 8u + (2 / k) 8u A_r                                                                   (weight_tolerance())

Huber's and Tukey's branch r2 <= k2 needs no care: both are continuous there (1 and k / r meet at r = k; (1 - r2/k2)^2 and 0 meet
at 0 with slope 0), so a point whose rounded r2 falls on the other side of k2 moves its weight by the same dw/dr dr.
"""
from fractions import Fraction

import numpy as np

import ref_moments as rm
import ref_numpy
from batch_ref import hom

NONE, HUBER, CAUCHY, TUKEY = 0, 1, 2, 3
KINDS = {"huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY}
MOM_W = 29
U = rm.U
_NORMALS = {}


# ---- the weight functions -----------------------------------------------------------------------------------------------------
def weight(kind, r2, k):
    """w(r2) in double, k2 = k * k formed once; r2 = +inf gives 0 for every kernel"""
    r2 = np.asarray(r2, dtype=np.float64)
    if kind == NONE:
        return np.ones_like(r2)
    k = float(k)
    k2 = k * k
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == HUBER:
            return np.where(r2 <= k2, 1.0, k / np.sqrt(r2))
        if kind == CAUCHY:
            return 1.0 / (1.0 + r2 / k2)
        if kind == TUKEY:
            u = 1.0 - r2 / k2
            return np.where(r2 <= k2, u * u, 0.0)
    raise ValueError(kind)


# ---- the residuals ----------------------------------------------------------------------------------------------------------------
def residual_sq(plane, P, M, idx, nrm=None):
    """r2 per point in double, the operations in the order of the header: what the device forms, up to its roundings"""
    P64, G = np.asarray(P, dtype=np.float64), np.asarray(M, dtype=np.float64)[idx]
    if not plane:
        d = G - P64
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    N = np.asarray(nrm, dtype=np.float64)[idx]
    bi = (P64[:, 0] - G[:, 0]) * N[:, 0] + (P64[:, 1] - G[:, 1]) * N[:, 1] + (P64[:, 2] - G[:, 2]) * N[:, 2]
    return bi * bi


def residual_sq_exact(plane, P, M, idx, nrm=None):
    """(r2, A_r): r2 per point formed exactly and rounded once to double; A_r the residual's majorant (module docstring)"""
    P, G = np.asarray(P), np.asarray(M)[idx]
    aP, aG = np.abs(P.astype(np.float64)), np.abs(G.astype(np.float64))
    if not plane:
        (p, q), e = rm._exact_ints([P, G])
        d = q - p
        tot = (d * d).sum(axis=1)
        r2 = np.array([float(Fraction(int(v)) * Fraction(2) ** (2 * e)) for v in tot])
        return r2, np.sqrt(((aP + aG) ** 2).sum(axis=1))
    N = np.asarray(nrm)[idx]
    (p, q, n), e = rm._exact_ints([P, G, N])
    bi = ((p - q) * n).sum(axis=1)
    r2 = np.array([float(Fraction(int(v) * int(v)) * Fraction(2) ** (4 * e)) for v in bi])
    return r2, ((aP + aG) * np.abs(N.astype(np.float64))).sum(axis=1)


def weight_tolerance(k, A_r):
    """8u + (2 / k) 8u A_r, per point"""
    return 8.0 * U + (2.0 / float(k)) * 8.0 * U * np.asarray(A_r, dtype=np.float64)


# ---- exact weighted sums ------------------------------------------------------------------------------------------------------------
def _weight_ints(w):
    (wi,), ew = rm._exact_ints([np.asarray(w, dtype=np.float64)])
    return wi, ew


def weighted(plane, P, M, nrm, idx, w):
    """(moments[32], majorants[32]) of a robust pass over the KEPT points P (n x 3) matched to M[idx] with the weights w (n,):
    CNT = n, W = sum w, every other slot sum w_i term_i with ref_moments' terms, exact and rounded once; the majorants are
    ref_moments' with every term scaled by w_i.  ERR stays 0: the front end's error is unweighted (ref_moments.sq_error)"""
    P, M, idx, w = np.asarray(P), np.asarray(M), np.asarray(idx), np.asarray(w, dtype=np.float64)
    n = P.shape[0]
    assert w.shape == (n,) and (w >= 0).all() and np.isfinite(w).all()
    mom, maj = np.zeros(rm.NMOM), np.zeros(rm.NMOM)
    mom[rm.CNT] = maj[rm.CNT] = float(n)
    if n == 0:
        return mom, maj
    wi, ew = _weight_ints(w)
    mom[MOM_W] = rm._round_once(rm._osum(wi), ew)
    maj[MOM_W] = w.sum()
    G = M[idx]
    if not plane:
        (p, q), e = rm._exact_ints([P, G])
        aP, aG = np.abs(P.astype(np.float64)), np.abs(G.astype(np.float64))
        for a in range(3):
            mom[rm.SP + a] = rm._round_once(rm._osum(wi * p[:, a]), e + ew)
            mom[rm.SQ + a] = rm._round_once(rm._osum(wi * q[:, a]), e + ew)
            maj[rm.SP + a] = (w * aP[:, a]).sum()
            maj[rm.SQ + a] = (w * aG[:, a]).sum()
            for b in range(3):
                mom[rm.SQP + 3 * a + b] = rm._round_once(rm._osum(wi * q[:, a] * p[:, b]), 2 * e + ew)
                maj[rm.SQP + 3 * a + b] = (w * aG[:, a] * aP[:, b]).sum()
        mom[rm.SPP] = rm._round_once(rm._osum(wi * (p * p).sum(axis=1)), 2 * e + ew)
        mom[rm.SQQ] = rm._round_once(rm._osum(wi * (q * q).sum(axis=1)), 2 * e + ew)
        maj[rm.SPP], maj[rm.SQQ] = (w * (aP * aP).sum(axis=1)).sum(), (w * (aG * aG).sum(axis=1)).sum()
        return mom, maj
    N = np.asarray(nrm)[idx]
    (p, q, nr), e = rm._exact_ints([P, G, N])
    assert e <= 0
    one = 1 << (-e)
    (px, py, pz), (qx, qy, qz), (nx, ny, nz) = rm._cols(p), rm._cols(q), rm._cols(nr)
    cn = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx * one, ny * one, nz * one]
    bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz
    acn, abi = rm.plane_terms_abs(P, G, N)
    o = rm.MC
    for a in range(6):
        for c in range(a, 6):
            mom[o] = rm._round_once(rm._osum(wi * cn[a] * cn[c]), 4 * e + ew)
            maj[o] = (w * acn[:, a] * acn[:, c]).sum()
            o += 1
    for a in range(6):
        mom[rm.MB + a] = rm._round_once(-rm._osum(wi * cn[a] * bi), 4 * e + ew)
        maj[rm.MB + a] = (w * acn[:, a] * abi).sum()
    return mom, maj


def weighted_longdouble(plane, P, M, nrm, idx, w):
    """the same sums in np.longdouble (a second opinion on the integer arithmetic): moments[32]"""
    L = np.longdouble
    P, G, w = np.asarray(P).astype(L), np.asarray(M)[idx].astype(L), np.asarray(w).astype(L)
    mom = np.zeros(rm.NMOM, dtype=L)
    mom[rm.CNT] = P.shape[0]
    mom[MOM_W] = w.sum()
    if not plane:
        for a in range(3):
            mom[rm.SP + a], mom[rm.SQ + a] = (w * P[:, a]).sum(), (w * G[:, a]).sum()
            for b in range(3):
                mom[rm.SQP + 3 * a + b] = (w * G[:, a] * P[:, b]).sum()
        mom[rm.SPP], mom[rm.SQQ] = (w * (P * P).sum(axis=1)).sum(), (w * (G * G).sum(axis=1)).sum()
        return mom
    N = np.asarray(nrm)[idx].astype(L)
    cn = np.concatenate([np.cross(P, N), N], axis=1)
    bi = ((P - G) * N).sum(axis=1)
    o = rm.MC
    for a in range(6):
        for c in range(a, 6):
            mom[o] = (w * cn[:, a] * cn[:, c]).sum()
            o += 1
    for a in range(6):
        mom[rm.MB + a] = -(w * cn[:, a] * bi).sum()
    return mom


def tolerance(maj, n):
    """tol_s = 2 (n + 17) 2^-53 A_s (module docstring: ref_moments.tolerance with one rounding more per term)"""
    return 2.0 * (n + 17) * U * np.asarray(maj, dtype=np.float64)


def slots(plane):
    return (rm.PLANE_SLOTS if plane else rm.P2P_SLOTS) + (MOM_W,)


def check_weighted_sums(plane, P, M, nrm, idx, mask, w, mom, what):
    """the slots of a robust pass's vector against the exact weighted sums over the kept points, with the weights the device
    reported; CNT exactly.  Returns the largest |device - exact| / tol"""
    want, maj = weighted(plane, P[mask], M, nrm, idx[mask], w[mask])
    tol = tolerance(maj, P.shape[0])
    assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}, kept {int(mask.sum())}"
    worst = 0.0
    for s in slots(plane):
        dev = abs(mom[s] - want[s])
        assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
        if tol[s] > 0:
            worst = max(worst, dev / tol[s])
    return worst


def with_cnt_from_w(mom):
    """the vector the host solves on: a copy whose CNT slot holds W"""
    out = np.array(mom, dtype=np.float64, copy=True)
    out[rm.CNT] = out[MOM_W]
    return out


# ---- normals --------------------------------------------------------------------------------------------------------------------
def robust_normals(M):
    """ref_numpy.knn4 + normals_longdouble of the model, in the model's dtype; computed once per model"""
    M = np.ascontiguousarray(M)
    key = (M.dtype.str, M.shape[0], M.tobytes())
    if key not in _NORMALS:
        _NORMALS[key] = ref_numpy.normals_longdouble(M, ref_numpy.knn4(M))[0].astype(M.dtype)
    return _NORMALS[key]


# ---- the weighted minimisations and the loop ---------------------------------------------------------------------------------------
def minimize_weighted(P, M, idx, w):
    """the weighted Kabsch solve: centroids and cross-covariance with the weights, R = U Vt (no reflection fix, as
    ref_numpy.minimize)"""
    P, G, w = np.asarray(P, dtype=np.float64), np.asarray(M, dtype=np.float64)[idx], np.asarray(w, dtype=np.float64)
    W = w.sum()
    pb, qb = (w[:, None] * P).sum(0) / W, (w[:, None] * G).sum(0) / W
    N = ((G - qb) * w[:, None]).T @ (P - pb)
    Uu, _, Vt = np.linalg.svd(N)
    R = Uu @ Vt
    return R, qb - R @ pb


def p2plane_minimize_weighted(P, M, idx, nrm, w):
    """ref_numpy.p2plane_minimize with C = sum w cn cn^T, b = -sum w cn bi"""
    P, G, N = np.asarray(P, dtype=np.float64), np.asarray(M, dtype=np.float64)[idx], np.asarray(nrm, dtype=np.float64)[idx]
    cn = np.concatenate([np.cross(P, N), N], axis=1)
    bi = ((P - G) * N).sum(axis=1)
    x = np.linalg.solve((cn * w[:, None]).T @ cn, -(cn * (w * bi)[:, None]).sum(axis=0))
    cx, cy, cz, sx, sy, sz = np.cos(x[0]), np.cos(x[1]), np.cos(x[2]), np.sin(x[0]), np.sin(x[1]), np.sin(x[2])
    R = np.array([[cy * cz, cz * sx * sy - cx * sz, cx * cz * sy + sx * sz],
                  [cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx],
                  [-sy, cy * sx, cx * cy]])
    return R, x[3:6].copy()


def robust_loop(orc, A, M, kind, k, max_iter, tol, nrm=None):
    """batch_ref.reference_loop as iteratively re-weighted least squares, no gate and no trim: orc.nn, the residuals, the weights, a
    weighted minimise (point-to-plane where nrm is given); the error unweighted over the kept points -- all of them -- divided by
    their count.  A pass whose weights add up to nothing ends the loop.  kind NONE: the plain loop.  weights: every pass's (the
    last: the most recent matching pass); idx, moved: the last matches and the final cloud"""
    plane = nrm is not None
    P = A.copy()
    E, T, i, weights = [0.0], np.eye(4), 0, []
    while True:
        idx = orc.nn(P, M)
        w = weight(kind, residual_sq(plane, P, M, idx, nrm), k)
        weights.append(w)
        if not w.sum() > 0:
            break
        R, t = p2plane_minimize_weighted(P, M, idx, nrm, w) if plane else minimize_weighted(P, M, idx, w)
        P = (P.astype(np.float64) @ R.T + t).astype(A.dtype)
        T = hom(R, t) @ T
        diff = M[idx].astype(np.float64) - P.astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / P.shape[0])))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, weights=weights, idx=idx, moved=P)


def inlier_rms(moved, M, idx, is_out):
    """RMS distance of the true inliers to their matches"""
    d = np.asarray(M, dtype=np.float64)[idx][~is_out] - np.asarray(moved, dtype=np.float64)[~is_out]
    return float(np.sqrt((d ** 2).sum() / (~is_out).sum()))
