"""What the tests of the symmetric metric share (tests/test_batch_sym_ref.py, test_batch_sym_abi.py, test_gpu_batch_sym.py): the
per-match terms of a symmetric pass with every operation in the order include/icp_mi355x.h states ("the symmetric metric"), their
exact sums, the solve with its two half rotations, a reference loop in the batch's dtype for moving and matching, and the scene the
recovery tests use.  Nothing here touches a device.

    terms    np = Rc m0, s = np . nq, n = s < 0 ? nq - np : nq + np, e = p - q, g = p + q, h = e . n, v = (g x n, n);
             C(a, c) += v_a v_c, B(a) -= v_a h, CNT = 1 -- float64 arrays, one numpy operation per rounding
    solve    x = C^-1 b; a = x[0:3], tt = x[3:6]; l2 = |a|^2, c = 1 / sqrt(1 + l2), k = c c / (1 + c);
             Ra = c (I + [a]x) + k a a^T; R = Ra Ra, t = Ra (c tt) -- motion(x), in Python floats, statement by statement

The device forms the same expressions, so a pass's vector is a sum of these terms up to the order of its additions.  The bound on
that is ref_moments.tolerance: (n - 1) additions of at most u A_s each, A_s = sum |term|, inside 2 (n + 16) u A_s.
"""
import math

import numpy as np

import batch_gicp_ref as gr
import ref_moments as rm
from batch_ref import hom, sq_dist

SYMMETRIC = 4


def _dot(x, y, z, a, b, c):
    return (x * a + y * b) + z * c


# ---- the terms of a symmetric pass -----------------------------------------------------------------------------------------------
def residual(P, Q, Np0, Nq, idx, Rc):
    """(n (three (n,) arrays), h (n,), g (three arrays)): the direction every match i -> idx[i] pulls along, its residual and p + q.
    Np0 (n, 3): the moving point normals in the frame of the cloud as uploaded; Nq (m, 3): the model's; Rc (3, 3): the rotation of
    the motions applied to the cloud so far"""
    idx = np.asarray(idx)
    P64, G = np.asarray(P).astype(np.float64), np.asarray(Q).astype(np.float64)[idx]
    m0, nq = np.asarray(Np0, dtype=np.float64), np.asarray(Nq, dtype=np.float64)[idx]
    Rc = np.asarray(Rc, dtype=np.float64)
    with np.errstate(all="ignore"):
        npx = [_dot(Rc[a, 0], Rc[a, 1], Rc[a, 2], m0[:, 0], m0[:, 1], m0[:, 2]) for a in range(3)]
        s = _dot(npx[0], npx[1], npx[2], nq[:, 0], nq[:, 1], nq[:, 2])
        flip = s < 0
        n = [np.where(flip, nq[:, a] - npx[a], nq[:, a] + npx[a]) for a in range(3)]
        e = [P64[:, a] - G[:, a] for a in range(3)]
        g = [P64[:, a] + G[:, a] for a in range(3)]
        h = _dot(e[0], e[1], e[2], n[0], n[1], n[2])
    return n, h, g


def terms(P, Q, Np0, Nq, idx, Rc):
    """(n, 32): what every match i -> idx[i] adds to each slot of a symmetric pass, in float64 with the operations of the header in
    their order"""
    n, h, g = residual(P, Q, Np0, Nq, idx, Rc)
    with np.errstate(all="ignore"):
        v = [g[1] * n[2] - g[2] * n[1], g[2] * n[0] - g[0] * n[2], g[0] * n[1] - g[1] * n[0], n[0], n[1], n[2]]
        t = np.zeros((h.shape[0], rm.NMOM))
        t[:, rm.CNT] = 1.0
        o = rm.MC
        for a in range(6):
            for c in range(a, 6):
                t[:, o] = v[a] * v[c]
                o += 1
        for a in range(6):
            t[:, rm.MB + a] = -(v[a] * h)
    return t


def check_sums(P, Q, Np0, Nq, idx, mask, Rc, mom, what):
    """every slot of a symmetric pass's vector against the exact sum (math.fsum) of the numpy terms over the kept points; CNT
    exactly; the slots behind B are zero.  Returns the largest |device - exact| / tol"""
    t = terms(P, Q, Np0, Nq, idx, Rc)
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


# ---- the solve -------------------------------------------------------------------------------------------------------------------
def motion(x):
    """(R (3, 3), t (3,)) from x = (a, tt) by the header's statements, every one a Python float operation"""
    a = [float(x[0]), float(x[1]), float(x[2])]
    tt = [float(x[3]), float(x[4]), float(x[5])]
    l2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    c = 1.0 / math.sqrt(1.0 + l2)
    k = (c * c) / (1.0 + c)
    E = [[1.0, -a[2], a[1]], [a[2], 1.0, -a[0]], [-a[1], a[0], 1.0]]
    Ra = [[c * E[r][s] + k * (a[r] * a[s]) for s in range(3)] for r in range(3)]
    tp = [c * tt[r] for r in range(3)]
    R = np.array([[(Ra[r][0] * Ra[0][s] + Ra[r][1] * Ra[1][s]) + Ra[r][2] * Ra[2][s] for s in range(3)] for r in range(3)])
    t = np.array([(Ra[r][0] * tp[0] + Ra[r][1] * tp[1]) + Ra[r][2] * tp[2] for r in range(3)])
    return R, t


def system(mom):
    Cm = np.zeros((6, 6))
    o = rm.MC
    for a in range(6):
        for c in range(a, 6):
            Cm[a, c] = Cm[c, a] = mom[o]
            o += 1
    return Cm, np.asarray(mom[rm.MB:rm.MB + 6], dtype=np.float64)


def solve(mom):
    """the 6 x 6 system of a vector's slots C, B -> (R, t, x): x = C^-1 b, then motion(x).  numpy.linalg.LinAlgError where the
    system is singular or the solution is not finite"""
    Cm, b = system(mom)
    x = np.linalg.solve(Cm, b)
    if not np.isfinite(x).all():
        raise np.linalg.LinAlgError("the solution is not finite")
    R, t = motion(x)
    return R, t, x


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def angle_deg(Ra, Rb):
    """the angle of Ra Rb^T in degrees, from |Ra - Rb|_F^2 = 8 sin^2(angle / 2): well conditioned near 0, where the arc cosine of the
    trace loses half the digits (a T composed of motions rounded to fp32 is orthonormal to 1e-7 only)"""
    d = float(np.linalg.norm(np.asarray(Ra, dtype=np.float64) - np.asarray(Rb, dtype=np.float64)))
    return float(np.degrees(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0))))))


def reference_loop(orc, A, M, Np0, Nq, max_iter, tol, keep=None, T0=None, metric="symmetric", truth=None):
    """batch_ref.reference_loop for the symmetric metric: orc.nn on the cloud in its own dtype, keep(the winning squared distances)
    where a rule is given, the terms with Rc = the rotation of the motions applied so far (T0's included), solve; the cloud is moved
    in double and rounded to its dtype; the error Euclidean over the kept points, divided by their count.  A pass that keeps nothing
    ends the loop (empty=True); a singular system ends it too (singular=True).  metric="plane": the point-to-plane loop on the
    model normals Nq (ref_moments.plane_point_terms, batch_gicp_ref.solve) -- what the symmetric loop is compared against.
    truth: a (3, 3) rotation; ang then holds the angle in degrees between it and T's rotation after every pass."""
    P = A.copy()
    T = np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64).copy()
    E, i, kept, ang, empty, singular = [0.0], 0, [], [], False, False
    while True:
        idx = orc.nn(P, M)
        if metric == "symmetric":
            t = terms(P, M, Np0, Nq, idx, T[:3, :3])
        else:
            t = rm.plane_point_terms(P, M, Nq, idx)
        mask = np.ones(P.shape[0], dtype=bool) if keep is None else keep(sq_dist(P, M, idx))
        kept.append(int(mask.sum()))
        if not mask.any():
            empty = True
            break
        try:
            R, tr = solve(t[mask].sum(axis=0))[:2] if metric == "symmetric" else gr.solve(t[mask].sum(axis=0))
        except np.linalg.LinAlgError:
            singular = True
            break
        P = (P.astype(np.float64) @ R.T + tr).astype(A.dtype)
        T = hom(R, tr) @ T
        if truth is not None:
            ang.append(angle_deg(T[:3, :3], truth))
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, idx=idx, moved=P, empty=empty, singular=singular, ang=ang)


# ---- the scene -------------------------------------------------------------------------------------------------------------------
SHIFT = np.array([0.15, -0.1, 0.05])
ITER_SCENE = 30


def surf(n, seed, jitter=0.3):
    """(points (n*n, 3), unit normals): an n x n grid over [-1, 1]^2, every point jittered by up to jitter / n, lifted onto
    z = 0.25 sin(3x) cos(2.5y) + 0.2 x^2, with the surface's analytic normals"""
    r = np.random.default_rng(seed)
    g = np.linspace(-1, 1, n)
    x, y = np.meshgrid(g, g)
    x = x.ravel() + jitter * r.uniform(-1, 1, n * n) / n
    y = y.ravel() + jitter * r.uniform(-1, 1, n * n) / n
    z = 0.25 * np.sin(3 * x) * np.cos(2.5 * y) + 0.2 * x * x
    zx = 0.75 * np.cos(3 * x) * np.cos(2.5 * y) + 0.4 * x
    zy = -0.625 * np.sin(3 * x) * np.sin(2.5 * y)
    N = np.stack([-zx, -zy, np.ones_like(x)], 1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return np.stack([x, y, z], 1), N


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(dtype=np.float64, deg=40.0, axis=(0.0, 0.0, 1.0), model=40, moving=33):
    """dict(A, M, Np, Nq, R): the model, surf(model, 1); the moving cloud, the points of the independently jittered surf(moving, 2)
    with |x|, |y| < 0.8 (625 of 33 x 33) carried by the inverse of (R, SHIFT), R the rotation by deg about axis -- the registration
    sought is (R, SHIFT); Np, Nq: the analytic unit normals, float64, Np in the moving cloud's frame.  model=20, moving=17: the
    scene at a quarter of its size"""
    Q, Nq = surf(model, 1)
    X, Nx = surf(moving, 2)
    keep = (np.abs(X[:, 0]) < 0.8) & (np.abs(X[:, 1]) < 0.8)
    X, Nx = X[keep], Nx[keep]
    R = rodrigues(axis, deg)
    A, Np = (X - SHIFT) @ R, Nx @ R
    return dict(A=np.ascontiguousarray(A.astype(dtype)), M=np.ascontiguousarray(Q.astype(dtype)), Np=np.ascontiguousarray(Np),
                Nq=np.ascontiguousarray(Nq), R=R)
