"""What the tests of the generalized (plane-to-plane) metric share (tests/test_batch_gicp_ref.py, test_batch_gicp_abi.py,
test_gpu_batch_gicp.py): the covariance rule of icp_batch_estimate_covariances in numpy, bit for bit as include/icp_mi355x.h states
it, the per-match terms of a generalized pass with every operation in the stated order, their exact sums, and a reference loop in
double.  Nothing here touches a device.

    distance      d2(i, j) = (dx*dx + dy*dy) + dz*dz on arrays of the cloud's own dtype F (batch_outlier_ref.d2_rows)
    tau_i         the k-th smallest d2(i, j) over j != i by index: the diagonal is taken out, np.partition picks the k-th
    neighbourhood every j with d2(i, j) <= tau_i, the diagonal (exactly 0) included
    sums          in float64 from 0.0 in ascending j.  A point outside the neighbourhood contributes +0.0, which changes no running
                  sum: the sum starts at +0.0 and a sum of doubles is never -0.0 unless every addend is, so np.cumsum over all j
                  behind one leading 0.0 is the rule's sequential sum.  (np.sum adds pairwise: not used.)
    covariance    C_ab = (S_ab - (s_a * s_b) / c) / c, every elementwise operation rounded separately
    frobenius     f = sqrt(((xx*xx + yy*yy) + zz*zz) + 2.0 * ((xy*xy + xz*xz) + yz*yz)); f > 0: C / f + lam on the diagonal, else lam I;
                  f and the quotients are formed on the matrix the range rule of icp_eigh3 leaves (batch_keypoint_ref.range_scale:
                  times 2^-+600 where the largest magnitude lies beyond 2^+-400), so no square leaves the double range

The per-match terms (terms()) use +, -, *, / on float64 arrays only, one numpy operation per rounding, in the order of the header;
the device forms the same expressions, so a pass's vector is a sum of these terms up to the order of its additions.  The bound on
that (tolerance()) is ref_moments.tolerance: (n - 1) additions of at most u A_s each, A_s = sum |term|, inside 2 (n + 16) u A_s.
"""
import math

import numpy as np

import batch_outlier_ref as orf
from batch_keypoint_ref import range_scale
import ref_moments as rm
from batch_ref import hom, sq_dist

GENERALIZED = 2
COV_NONE, COV_FROBENIUS = 0, 1
MIN_K, MAX_K = 3, 32
ROWS = 128          # rows per block of the distance matrix


# ---- the covariance rule ---------------------------------------------------------------------------------------------------------
def _seq_sum(terms):
    """(rows,) the sum of every row of `terms` (rows, n) from 0.0 in ascending column"""
    z = np.zeros((terms.shape[0], 1))
    return np.cumsum(np.concatenate([z, terms], axis=1), axis=1)[:, -1]


def covariances(X, k, regularisation=COV_FROBENIUS, lam=1e-3, rows=None):
    """(n, 6) float64 -- xx, xy, xz, yy, yz, zz -- of every point of X (or of the points `rows`), and the neighbourhood sizes c"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    assert MIN_K <= k <= MAX_K and n >= k + 1
    rows = np.arange(n) if rows is None else np.asarray(rows)
    X64 = X.astype(np.float64)
    out = np.empty((rows.size, 6))
    cnt = np.empty(rows.size, dtype=np.int64)
    for b in range(0, rows.size, ROWS):
        r = rows[b:b + ROWS]
        d = np.stack([orf.d2_rows(X, i, i + 1)[0] for i in r])
        off = d.copy()
        off[np.arange(r.size), r] = np.inf                                     # j != i, by index
        tau = np.partition(off, k - 1, axis=1)[:, k - 1]                       # the k-th smallest
        inside = d <= tau[:, None]                                             # i itself is in: d2(i, i) == 0
        e = X64[None, :, :] - X64[r, None, :]                                  # against the query
        c = inside.sum(axis=1).astype(np.float64)
        s = [_seq_sum(np.where(inside, e[..., a], 0.0)) for a in range(3)]
        k6 = 0
        for a in range(3):
            for bb in range(a, 3):
                S = _seq_sum(np.where(inside, e[..., a] * e[..., bb], 0.0))
                out[b:b + ROWS, k6] = (S - (s[a] * s[bb]) / c) / c
                k6 += 1
        cnt[b:b + ROWS] = inside.sum(axis=1)
    if regularisation == COV_FROBENIUS:
        out = frobenius(out, lam)
    return out, cnt


def frobenius(C, lam):
    C = np.asarray(C, dtype=np.float64)
    (xx, xy, xz, yy, yz, zz), _ = range_scale([C[:, a] for a in range(6)])   # the squares stay in range; the quotients are scale-free
    C = np.stack([xx, xy, xz, yy, yz, zz], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.sqrt(((xx * xx + yy * yy) + zz * zz) + 2.0 * ((xy * xy + xz * xz) + yz * yz))
    pos = f > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(pos[:, None], C / f[:, None], 0.0)
    lam = np.float64(lam)
    for a in (0, 3, 5):
        out[:, a] = np.where(pos, out[:, a] + lam, lam)
    return out


def from_normals(N, eps=1e-3):
    """I - (1 - eps) n n^T (engine.covariances_from_normals, restated)"""
    N = np.asarray(N, dtype=np.float64)
    s = 1.0 - float(eps)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.stack([1.0 - s * x * x, -s * x * y, -s * x * z, 1.0 - s * y * y, -s * y * z, 1.0 - s * z * z], axis=1)


def full(C6):
    """(n, 6) -> (n, 3, 3) symmetric"""
    C6 = np.asarray(C6, dtype=np.float64)
    ix = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return C6[:, ix]


# ---- the terms of a generalized pass ---------------------------------------------------------------------------------------------
def _dot(x, y, z, a, b, c):
    return (x * a + y * b) + z * c


def terms(P, M, idx, Cp, Cq, R):
    """(terms (n, 32), valid (n,) bool, Minv (n, 3, 3)): what every match i -> idx[i] adds to each slot of a generalized pass, in
    float64 with the operations of the header in their order; valid: det finite and > 0 (the terms of the others are not to be
    used).  Cp (n, 6): the moving covariances in the uploaded cloud's frame; Cq (m, 6); R (3, 3): the pass's rotation Rc"""
    P64, G = np.asarray(P, dtype=np.float64), np.asarray(M, dtype=np.float64)[np.asarray(idx)]
    n = P64.shape[0]
    R = np.asarray(R, dtype=np.float64)
    cp, cq = full(Cp), np.asarray(Cq, dtype=np.float64)[np.asarray(idx)]
    with np.errstate(all="ignore"):
        Tm = [[_dot(R[a, 0], R[a, 1], R[a, 2], cp[:, 0, b], cp[:, 1, b], cp[:, 2, b]) for b in range(3)] for a in range(3)]
        B = {(a, b): _dot(Tm[a][0], Tm[a][1], Tm[a][2], R[b, 0], R[b, 1], R[b, 2]) for a in range(3) for b in range(a, 3)}
        S00, S01, S02 = cq[:, 0] + B[0, 0], cq[:, 1] + B[0, 1], cq[:, 2] + B[0, 2]
        S11, S12, S22 = cq[:, 3] + B[1, 1], cq[:, 4] + B[1, 2], cq[:, 5] + B[2, 2]
        c00, c01, c02 = S11 * S22 - S12 * S12, S02 * S12 - S01 * S22, S01 * S12 - S02 * S11
        c11, c12, c22 = S00 * S22 - S02 * S02, S01 * S02 - S00 * S12, S00 * S11 - S01 * S01
        det = (S00 * c00 + S01 * c01) + S02 * c02
        valid = np.isfinite(det) & (det > 0)
        Mi = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
        px, py, pz = P64[:, 0], P64[:, 1], P64[:, 2]
        e = (px - G[:, 0], py - G[:, 1], pz - G[:, 2])
        zero, one = np.zeros(n), np.ones(n)
        J = [(zero, -pz, py), (pz, zero, -px), (-py, px, zero), (one, zero, zero), (zero, one, zero), (zero, zero, one)]
        u = [[_dot(Mi[r][0], Mi[r][1], Mi[r][2], J[c][0], J[c][1], J[c][2]) for r in range(3)] for c in range(6)]
        t = np.zeros((n, rm.NMOM))
        t[:, rm.CNT] = 1.0
        o = rm.MC
        for a in range(6):
            for c in range(a, 6):
                t[:, o] = _dot(J[a][0], J[a][1], J[a][2], u[c][0], u[c][1], u[c][2])
                o += 1
        for a in range(6):
            t[:, rm.MB + a] = -_dot(u[a][0], u[a][1], u[a][2], e[0], e[1], e[2])
    Minv = np.stack([np.stack(row, axis=-1) for row in Mi], axis=-2)
    return t, valid, Minv


def exact_sums(t, kept):
    """(moments[32], majorants[32]) of the kept rows of t: every slot math.fsum of its terms, the majorant math.fsum of |term|"""
    mom, maj = np.zeros(rm.NMOM), np.zeros(rm.NMOM)
    rows = t[np.asarray(kept, dtype=bool)]
    for s in (rm.CNT,) + rm.PLANE_SLOTS:
        mom[s] = math.fsum(rows[:, s].tolist())
        maj[s] = math.fsum(np.abs(rows[:, s]).tolist())
    return mom, maj


def tolerance(maj, n):
    """ref_moments.tolerance for a pair of n moving points"""
    return rm.tolerance(maj, n)


def check_sums(P, M, idx, mask, Cp, Cq, R, mom, what):
    """every slot of a generalized pass's vector against the exact sum of the numpy terms over the kept points; CNT exactly.  The
    kept points must all have a valid det.  Returns the largest |device - exact| / tol"""
    t, valid, _ = terms(P, M, idx, Cp, Cq, R)
    assert valid[mask].all(), what
    want, maj = exact_sums(t, mask)
    tol = tolerance(maj, P.shape[0])
    assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}, kept {int(mask.sum())}"
    worst = 0.0
    for s in rm.PLANE_SLOTS:
        dev = abs(mom[s] - want[s])
        assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
        if tol[s] > 0:
            worst = max(worst, dev / tol[s])
    for s in range(rm.MB + 6, rm.NMOM):
        assert mom[s] == 0.0, (what, s)
    return worst


# ---- the solve and the loop ------------------------------------------------------------------------------------------------------
def solve(mom):
    """the 6 x 6 system of a vector's slots C, B -> (R, t): x = C^-1 b, R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6] (the plane solve's
    variables; batch_robust_ref.p2plane_minimize_weighted's rotation)"""
    Cm = np.zeros((6, 6))
    o = rm.MC
    for a in range(6):
        for c in range(a, 6):
            Cm[a, c] = Cm[c, a] = mom[o]
            o += 1
    x = np.linalg.solve(Cm, np.asarray(mom[rm.MB:rm.MB + 6], dtype=np.float64))
    cx, cy, cz, sx, sy, sz = np.cos(x[0]), np.cos(x[1]), np.cos(x[2]), np.sin(x[0]), np.sin(x[1]), np.sin(x[2])
    R = np.array([[cy * cz, cz * sx * sy - cx * sz, cx * cz * sy + sx * sz],
                  [cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx],
                  [-sy, cy * sx, cx * cy]])
    return R, x[3:6].copy()


def gicp_loop(orc, A, M, Cp, Cq, max_iter, tol, keep=None, T0=None):
    """batch_ref.reference_loop for the generalized metric: orc.nn, keep(the winning squared distances) where a rule is given, the
    det test, the terms with Rc = the rotation of the motions applied so far (T0's included), the 6 x 6 solve; the error Euclidean
    over the kept points, divided by their count.  A pass that keeps nothing ends the loop (empty=True)."""
    P = A.copy()
    T = np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64).copy()
    E, i, kept, empty = [0.0], 0, [], False
    while True:
        idx = orc.nn(P, M)
        t, valid, _ = terms(P, M, idx, Cp, Cq, T[:3, :3])
        mask = valid if keep is None else (valid & keep(sq_dist(P, M, idx)))
        kept.append(int(mask.sum()))
        if not mask.any():
            empty = True
            break
        R, tr = solve(t[mask].sum(axis=0))
        P = (P.astype(np.float64) @ R.T + tr).astype(A.dtype)
        T = hom(R, tr) @ T
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, idx=idx, moved=P, empty=empty)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
def blob(seed, n, dtype, scale=1.0):
    return np.ascontiguousarray((np.random.default_rng(seed).standard_normal((n, 3)) * scale).astype(dtype))


def surface(seed, n, dtype):
    """n points of a non-planar sheet z = 0.3 sin(2x) + 0.2 cos(3y) + 0.1 x y over [-1, 1]^2, jittered"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    z = 0.3 * np.sin(2 * x) + 0.2 * np.cos(3 * y) + 0.1 * x * y + rng.normal(0, 0.002, n)
    return np.ascontiguousarray(np.stack([x, y, z], -1).astype(dtype))
