"""What the tests of the colored metric share (tests/test_batch_color_ref.py, test_batch_color_abi.py, test_gpu_batch_color.py): the
gradient rule of icp_batch_estimate_intensity_gradients in numpy, bit for bit as include/icp_mi355x.h states it, the per-match
terms of a colored pass with every operation in the stated order, their exact sums, a reference loop in double, and the textured
surfaces the recovery tests use.  Nothing here touches a device.

    distance      d2(i, j) = (dx*dx + dy*dy) + dz*dz on arrays of the cloud's own dtype F (batch_outlier_ref.d2_rows)
    tau_i         the k-th smallest d2(i, j) over j != i by index: the diagonal is taken out, np.partition picks the k-th
    neighbourhood every j != i with d2(i, j) <= tau_i (the FPFH rule's)
    sums          in float64 from 0.0 in ascending j; a point outside the neighbourhood contributes +0.0, which changes no running
                  sum that started at +0.0 (batch_gicp_ref._seq_sum: np.cumsum behind one leading 0.0)
    solve         the cofactor statements of the generalized metric on A + c^2 n n^T; (0, 0, 0) where det is not finite and > 0
                  or a component is not finite

The per-match terms (terms()) use +, -, * on float64 arrays only, one numpy operation per rounding, in the order of the header;
the device forms the same expressions, so a pass's vector is a sum of these terms up to the order of its additions.  The bound on
that is ref_moments.tolerance: (n - 1) additions of at most u A_s each, A_s = sum |term|, inside 2 (n + 16) u A_s.
"""
import numpy as np

import batch_gicp_ref as gr
import batch_outlier_ref as orf
import ref_moments as rm
from batch_ref import hom, rot, sq_dist

COLORED = 3
LAMBDA_DEFAULT = 0.968
MIN_K, MAX_K = gr.MIN_K, gr.MAX_K
ROWS = 128          # rows per block of the distance matrix


def _dot(x, y, z, a, b, c):
    return (x * a + y * b) + z * c


# ---- the gradient rule -----------------------------------------------------------------------------------------------------------
def gradients(X, N, I, k, rows=None):
    """((n, 3) float64 gradients of every point of X (or of the points `rows`), the neighbourhood sizes c).  N: the normals, of X's
    dtype; I: the intensities, float64"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    assert MIN_K <= k <= MAX_K and n >= k + 1
    rows = np.arange(n) if rows is None else np.asarray(rows)
    X64, N64, I = X.astype(np.float64), np.asarray(N).astype(np.float64), np.asarray(I, dtype=np.float64)
    out = np.zeros((rows.size, 3))
    cnt = np.empty(rows.size, dtype=np.int64)
    for b in range(0, rows.size, ROWS):
        r = rows[b:b + ROWS]
        d = np.stack([orf.d2_rows(X, i, i + 1)[0] for i in r])
        off = d.copy()
        off[np.arange(r.size), r] = np.inf                                     # j != i, by index
        tau = np.partition(off, k - 1, axis=1)[:, k - 1]                       # the k-th smallest
        inside = d <= tau[:, None]
        inside[np.arange(r.size), r] = False                                   # i itself is out
        nx, ny, nz = (N64[r, a][:, None] for a in range(3))
        with np.errstate(all="ignore"):
            e = [X64[None, :, a] - X64[r, None, a] for a in range(3)]          # against the query
            h = _dot(e[0], e[1], e[2], nx, ny, nz)
            u = [e[0] - h * nx, e[1] - h * ny, e[2] - h * nz]
            g = I[None, :] - I[r, None]
            A = {(a, c): gr._seq_sum(np.where(inside, u[a] * u[c], 0.0)) for a in range(3) for c in range(a, 3)}
            rr = [gr._seq_sum(np.where(inside, u[a] * g, 0.0)) for a in range(3)]
            c = inside.sum(axis=1)
            w = c.astype(np.float64) * c.astype(np.float64)
            nn = (nx[:, 0], ny[:, 0], nz[:, 0])
            for a in range(3):
                for cc in range(a, 3):
                    A[a, cc] = A[a, cc] + w * (nn[a] * nn[cc])
            A00, A01, A02, A11, A12, A22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
            c00, c01, c02 = A11 * A22 - A12 * A12, A02 * A12 - A01 * A22, A01 * A12 - A02 * A11
            c11, c12, c22 = A00 * A22 - A02 * A02, A01 * A02 - A00 * A12, A00 * A11 - A01 * A01
            det = (A00 * c00 + A01 * c01) + A02 * c02
            M = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
            dd = np.stack([(M[a][0] * rr[0] + M[a][1] * rr[1]) + M[a][2] * rr[2] for a in range(3)], axis=1)
        ok = np.isfinite(det) & (det > 0) & np.isfinite(dd).all(axis=1)
        out[b:b + ROWS] = np.where(ok[:, None], dd, 0.0)
        cnt[b:b + ROWS] = c
    return out, cnt


# ---- the terms of a colored pass -------------------------------------------------------------------------------------------------
def terms(P, M, Nrm, idx, Ip, Iq, D, lam):
    """(n, 32): what every match i -> idx[i] adds to each slot of a colored pass, in float64 with the operations of the header in
    their order.  Nrm (m, 3): the model normals (the batch's dtype); Ip (n,), Iq (m,): the intensities; D (m, 3): the model's
    intensity gradients; lam: the pair's lambda"""
    idx = np.asarray(idx)
    P64, G = np.asarray(P, dtype=np.float64), np.asarray(M, dtype=np.float64)[idx]
    N = np.asarray(Nrm).astype(np.float64)[idx]
    d = np.asarray(D, dtype=np.float64)[idx]
    iq, ip = np.asarray(Iq, dtype=np.float64)[idx], np.asarray(Ip, dtype=np.float64)
    n = P64.shape[0]
    px, py, pz = P64[:, 0], P64[:, 1], P64[:, 2]
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        ex, ey, ez = px - G[:, 0], py - G[:, 1], pz - G[:, 2]
        h = _dot(ex, ey, ez, nx, ny, nz)
        s = _dot(dx, dy, dz, nx, ny, nz)
        mx, my, mz = dx - s * nx, dy - s * ny, dz - s * nz
        ux, uy, uz = ex - h * nx, ey - h * ny, ez - h * nz
        rI = (iq + _dot(dx, dy, dz, ux, uy, uz)) - ip
        lg = np.float64(lam)
        lp = np.float64(1.0) - lg
        zero, one = np.zeros(n), np.ones(n)
        J = [(zero, -pz, py), (pz, zero, -px), (-py, px, zero), (one, zero, zero), (zero, one, zero), (zero, zero, one)]
        Gm = [_dot(J[a][0], J[a][1], J[a][2], nx, ny, nz) for a in range(6)]
        K = [_dot(J[a][0], J[a][1], J[a][2], mx, my, mz) for a in range(6)]
        t = np.zeros((n, rm.NMOM))
        t[:, rm.CNT] = 1.0
        o = rm.MC
        for a in range(6):
            for c in range(a, 6):
                t[:, o] = lg * (Gm[a] * Gm[c]) + lp * (K[a] * K[c])
                o += 1
        for a in range(6):
            t[:, rm.MB + a] = -(lg * (Gm[a] * h) + lp * (K[a] * rI))
    return t


def check_sums(P, M, Nrm, idx, mask, Ip, Iq, D, lam, mom, what):
    """every slot of a colored pass's vector against the exact sum (math.fsum) of the numpy terms over the kept points; CNT
    exactly.  Returns the largest |device - exact| / tol"""
    t = terms(P, M, Nrm, idx, Ip, Iq, D, lam)
    want, maj = gr.exact_sums(t, mask)
    tol = rm.tolerance(maj, P.shape[0])
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


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def color_loop(orc, A, M, Nrm, Ip, Iq, D, lam, max_iter, tol, keep=None, T0=None):
    """batch_ref.reference_loop for the colored metric: orc.nn, keep(the winning squared distances) where a rule is given, the
    terms, the 6 x 6 solve (batch_gicp_ref.solve); the error Euclidean over the kept points, divided by their count.  A pass that
    keeps nothing ends the loop (empty=True); a singular system ends it too (singular=True).  lam = 1.0 is the point-to-plane
    loop."""
    P = A.copy()
    T = np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64).copy()
    E, i, kept, empty, singular = [0.0], 0, [], False, False
    while True:
        idx = orc.nn(P, M)
        t = terms(P, M, Nrm, idx, Ip, Iq, D, lam)
        mask = np.ones(P.shape[0], dtype=bool) if keep is None else keep(sq_dist(P, M, idx))
        kept.append(int(mask.sum()))
        if not mask.any():
            empty = True
            break
        try:
            R, tr = gr.solve(t[mask].sum(axis=0))
        except np.linalg.LinAlgError:
            singular = True
            break
        P = (P.astype(np.float64) @ R.T + tr).astype(A.dtype)
        T = hom(R, tr) @ T
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, idx=idx, moved=P, empty=empty, singular=singular)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
K_TEX, GATE_TEX, ITER_TEX = 8, 0.07, 40
T_OFF = hom(rot("z", 0.02) @ rot("x", 0.01), np.array([0.02, -0.015, 0.01]))   # what the moving cloud was moved by


def field(x, y):
    """the texture: I = 0.5 + 0.25 sin 6x + 0.25 cos(5y + 2x)"""
    return 0.5 + 0.25 * np.sin(6.0 * x) + 0.25 * np.cos(5.0 * y + 2.0 * x)


def textured(c, dtype=np.float64, seed=0, m=900, n=250):
    """a textured pair on the surface z = c (x^2 - y^2) over the unit square: dict(A, M, N, Ip, Iq, S) -- the model's m random
    samples M with their analytic unit normals N (exactly (0, 0, 1) for c = 0) and intensities Iq; the moving cloud A: n other
    samples S of the same surface moved by T_OFF, with the intensities Ip of the samples.  The registration sought is T_OFF^-1."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, (m, 2))
    M = np.stack([xy[:, 0], xy[:, 1], c * (xy[:, 0] ** 2 - xy[:, 1] ** 2)], -1)
    N = np.stack([-2.0 * c * xy[:, 0], 2.0 * c * xy[:, 1], np.ones(m)], -1)
    N = N / np.linalg.norm(N, axis=1, keepdims=True)
    sx = rng.uniform(0.0, 1.0, (n, 2))
    S = np.stack([sx[:, 0], sx[:, 1], c * (sx[:, 0] ** 2 - sx[:, 1] ** 2)], -1)
    A = S @ T_OFF[:3, :3].T + T_OFF[:3, 3]
    M, N, A = (np.ascontiguousarray(v.astype(dtype)) for v in (M, N, A))
    return dict(A=A, M=M, N=N, Ip=field(sx[:, 0], sx[:, 1]), Iq=field(xy[:, 0], xy[:, 1]), S=S)


def pose_error(T, pair):
    """the largest distance between a moving point carried by T and the sample it was made from (T = identity: about 0.03)"""
    A = pair["A"].astype(np.float64)
    return float(np.linalg.norm(A @ T[:3, :3].T + T[:3, 3] - pair["S"], axis=1).max())
