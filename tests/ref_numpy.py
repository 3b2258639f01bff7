"""Independent numpy/LAPACK restatement of the reference's point-to-point iteration, used only to
cross-check the C oracle (a second opinion written against the same reference lines,
src/ICP_CPU.c:217-271, with numpy's LAPACK gesdd standing in for MKL's gesvd)."""
import numpy as np


def nn(P, Q):
    P = np.asarray(P)
    Q = np.asarray(Q, dtype=P.dtype)
    idx = np.empty(P.shape[0], dtype=np.int32)
    for i in range(P.shape[0]):
        d = Q - P[i]              # vdSub
        d = d * d                 # vdSqr
        s = d[:, 0] + d[:, 1]     # vdAdd
        s = s + d[:, 2]           # vdAdd
        idx[i] = int(np.argmin(s))  # first minimum
    return idx


def minimize(P, Q, idx):
    P = np.asarray(P, dtype=np.float64)
    Qi = np.asarray(Q, dtype=np.float64)[idx]
    pb, qb = P.mean(0), Qi.mean(0)
    N = (Qi - qb).T @ (P - pb)
    U, _, Vt = np.linalg.svd(N)
    R = U @ Vt
    return R, qb - R @ pb


def icp(D, M, max_iter, tol, fixed=False):
    P = np.array(D, dtype=np.float64)
    Q = np.asarray(M, dtype=np.float64)
    E = [0.0]
    T = np.eye(4)
    i = 0
    while True:
        idx = nn(P, Q)
        R, t = minimize(P, Q, idx)
        P = P @ R.T + t
        Tk = np.eye(4)
        Tk[:3, :3], Tk[:3, 3] = R, t
        T = Tk @ T
        E.append(float(np.sqrt(((Q[idx] - P) ** 2).sum() / P.shape[0])))
        if not fixed and (E[-1] < tol or abs(E[-1] - E[-2]) < tol):
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, idx=idx, moved=P)


# ---- point-to-plane: a second opinion on the oracle's kNN(4), covariance, minimisation and loop -----------------------------------
def _sq_dist_rows(Pc, Q):
    """(len(Pc), len(Q)) distances (dx*dx + dy*dy) + dz*dz, every operation rounded in the clouds' dtype"""
    acc = None
    for a in range(3):
        d = np.subtract.outer(Pc[:, a], Q[:, a])   # (the sign of a difference does not reach its square)
        np.multiply(d, d, out=d)
        acc = d if acc is None else np.add(acc, d, out=acc)
    return acc


def nn_chunked(P, Q, chunk=1024):
    """nn() a block of moving points at a time.  |p|^2 + |q|^2 - 2 p.q (one matrix product) only picks the candidates -- the model
    points within 1e-9 (|coordinates|^2 + 1) of that row's smallest value, a band a million times the product's own rounding
    error --; among them the decision is nn()'s: (dx*dx + dy*dy) + dz*dz, every operation rounded, first minimum"""
    P = np.ascontiguousarray(P)
    Q = np.ascontiguousarray(Q, dtype=P.dtype)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    qn = (Q64 * Q64).sum(axis=1)
    band = 1e-9 * (max(np.abs(P64).max(), np.abs(Q64).max()) ** 2 + 1.0)
    idx = np.empty(P.shape[0], dtype=np.int32)
    for s in range(0, P.shape[0], chunk):
        approx = qn[None, :] - 2.0 * (P64[s:s + chunk] @ Q64.T)          # (|p|^2 is the same along a row)
        rows, cols = np.nonzero(approx <= approx.min(axis=1, keepdims=True) + band)   # row-major: cols ascend within a row
        d = Q[cols] - P[s + rows]
        d = d * d
        d = (d[:, 0] + d[:, 1]) + d[:, 2]
        assert d.dtype == P.dtype
        best = np.full(min(chunk, P.shape[0] - s), np.inf)
        np.minimum.at(best, rows, d)
        first = np.flatnonzero(d == best[rows])
        keep = np.ones(first.size, dtype=bool)
        keep[1:] = rows[first][1:] != rows[first][:-1]                    # the first of a row's minima
        idx[s + rows[first][keep]] = cols[first][keep]
    return idx


def knn4(Q, chunk=256):
    """the first five of the (d, j)-ascending order of Q for every point of Q, rank 0 dropped: brute force in Q's dtype, stable sort"""
    Q = np.ascontiguousarray(Q)
    out = np.empty((Q.shape[0], 4), dtype=np.int32)
    for s in range(0, Q.shape[0], chunk):
        d = _sq_dist_rows(Q[s:s + chunk], Q)
        assert d.dtype == Q.dtype
        out[s:s + chunk] = np.argsort(d, axis=1, kind="stable")[:, 1:5]
    return out


def covariance4(Q, nbr):
    """(m, 9) row-major, upper triangle filled: bar = (sum of the 4 neighbours) * 0.25, A += (x - bar)(y - bar) neighbour by neighbour,
    every operation rounded in Q's dtype (the statements of orc_normals_f32 / _f64)"""
    Q = np.ascontiguousarray(Q)
    G = Q[np.asarray(nbr)]                              # (m, 4, 3)
    bar = np.zeros((Q.shape[0], 3), dtype=Q.dtype)
    for j in range(4):
        bar = bar + G[:, j]
    bar = bar * Q.dtype.type(0.25)
    A = np.zeros((Q.shape[0], 9), dtype=Q.dtype)
    for j in range(4):
        d = G[:, j] - bar
        for e, (a, b) in zip((0, 1, 2, 4, 5, 8), ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            A[:, e] = A[:, e] + d[:, a] * d[:, b]
    assert A.dtype == Q.dtype
    return A


def symmetric(A9):
    """(m, 9) upper triangles -> (m, 3, 3) symmetric, double"""
    A = np.asarray(A9, dtype=np.float64).reshape(-1, 3, 3)
    return np.triu(A) + np.transpose(np.triu(A, 1), (0, 2, 1))


def smallest_magnitude_eigenvectors(Asym):
    """LAPACK's eigh of (m, 3, 3): (w ascending, the eigenvector of the first eigenvalue of smallest magnitude)"""
    w, Z = np.linalg.eigh(Asym)
    k = np.abs(w).argmin(axis=1)
    return w, Z[np.arange(len(w)), :, k]


def normals_longdouble(Q, nbr):
    """mean and covariance of the four neighbours in np.longdouble, rounded to double once, LAPACK's eigh: (normals, A (m,3,3))"""
    G = np.asarray(Q, dtype=np.longdouble)[np.asarray(nbr)]
    d = G - G.mean(axis=1, keepdims=True)
    A = np.einsum("mja,mjb->mab", d, d).astype(np.float64)
    return smallest_magnitude_eigenvectors(A)[1], A


def normals_float_cast(Q, nbr):
    """what a kernel gives that casts the neighbours to float and forms mean and covariance in float (eigen-solve in double)"""
    A = symmetric(covariance4(np.asarray(Q).astype(np.float32), nbr))
    return smallest_magnitude_eigenvectors(A)[1]


def angle_deg(a, b):
    """angle between directions (sign ignored), degrees, per row"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = np.abs((a * b).sum(axis=1))
    s = np.linalg.norm(np.cross(a, b), axis=1)
    return np.degrees(np.arctan2(s, c))


def p2plane_minimize(P, Q, idx, Nrm):
    """C = sum cn cn^T, b = -sum cn ((p - q) . n), cn = (p x n, n); LAPACK's solve; R = Rz Ry Rx"""
    P, G, N = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)[idx], np.asarray(Nrm, dtype=np.float64)[idx]
    cn = np.concatenate([np.cross(P, N), N], axis=1)
    bi = ((P - G) * N).sum(axis=1)
    x = np.linalg.solve(cn.T @ cn, -(cn * bi[:, None]).sum(axis=0))
    cx, cy, cz, sx, sy, sz = np.cos(x[0]), np.cos(x[1]), np.cos(x[2]), np.sin(x[0]), np.sin(x[1]), np.sin(x[2])
    R = np.array([[cy * cz, cz * sx * sy - cx * sz, cx * cz * sy + sx * sz],
                  [cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx],
                  [-sy, cy * sx, cx * cy]])
    return R, x[3:6].copy()


def icp_p2plane(D, M, Nrm, max_iter, tol, fixed=False):
    """the loop of orc_icp_p2plane_f64 on float64 clouds; idx_passes: the correspondences of every pass"""
    import ref_moments
    P = np.array(D, dtype=np.float64)
    Q = np.asarray(M, dtype=np.float64)
    E, T, it, idx_passes = [0.0], np.eye(4), 0, []
    while it < max_iter:
        idx = nn_chunked(P, Q)
        idx_passes.append(idx)
        R, t = p2plane_minimize(P, Q, idx, Nrm)
        P = ref_moments.apply_rt(P, R, t)
        Tk = np.eye(4)
        Tk[:3, :3], Tk[:3, 3] = R, t
        T = Tk @ T
        E.append(float(np.sqrt(((Q[idx] - P) ** 2).sum() / P.shape[0])))
        if not fixed and (E[-1] < tol or abs(E[-1] - E[-2]) < tol):
            break
        it += 1
    return dict(iterations=it, passes=len(idx_passes), err=np.array(E), T=T, idx=idx_passes[-1], idx_passes=idx_passes, moved=P)


# measurement L (test_oracle.test_plane_loop_f64_against_numpy): the largest difference between orc_icp_p2plane_f64 and icp_p2plane
# above in T, the error series and the moved cloud over the five widened pairs: 2.5e-16, 1.7e-15, 2.7e-15
PLANE_F64_L = 2.7e-15


# ---- what a fused multiply-add in the fp64 distance would change (exact rationals, rounded once) -----------------------------------
FUSED_FORMS = ("fma(dx,dx,dy*dy) + dz*dz", "fma(dz,dz, dx*dx+dy*dy)")


def _fused_distance(form, dx, dy, dz):
    from fractions import Fraction
    if form == 0:
        return float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy)) + dz * dz
    return float(Fraction(dz) * Fraction(dz) + Fraction(dx * dx + dy * dy))


def order_fused(P, Q, form, keep):
    """for every point of P (float64): the first `keep` model indices of the (d, j)-ascending order with d evaluated in the fused
    form FUSED_FORMS[form] -- the fused product exact, the sum rounded once (float(Fraction) rounds correctly).  Only candidates within
    1e-9 (relative) of the keep-th separately rounded distance are re-evaluated: a fused form moves a distance by a few 2^-53."""
    P, Q = np.ascontiguousarray(P), np.ascontiguousarray(Q)
    assert P.dtype == Q.dtype == np.float64
    out = np.empty((P.shape[0], keep), dtype=np.int32)
    for i in range(P.shape[0]):
        diff = Q - P[i]
        sep = ((diff * diff)[:, 0] + (diff * diff)[:, 1]) + (diff * diff)[:, 2]
        cand = np.flatnonzero(sep <= np.partition(sep, keep - 1)[keep - 1] * (1 + 1e-9))
        d = [_fused_distance(form, *(float(v) for v in diff[c])) for c in cand]
        out[i] = [c for _, c in sorted(zip(d, cand.tolist()))][:keep]
    return out
