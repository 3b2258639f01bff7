"""Exact reference of the ICP_NMOM moment vector of one ICP pass (include/icp_mi355x.h, ICP_MOM_*), in plain Python / numpy.

Every slot is a sum over the moving points of a polynomial in the points' coordinates.  A float (fp32 or fp64) is an integer
times a power of two, so the sum is formed EXACTLY -- Python integers on one common scale -- and rounded ONCE to double
(fractions.Fraction -> float is correctly rounded).  Nothing here knows how the device orders its additions.

    point-to-point   ERR CNT SP(3) SQ(3) SQP(9) SPP SQQ      p = P[i], q = Q[idx[i]]
    point-to-plane   ERR CNT C(21) B(6)                       the kernels' statements: cn = (p x n, n), bi = (p - q) . n,
                                                              C += cn cn^T (upper triangle, row-major), b -= cn * bi
    ERR = sum |P_new[i] - Q[idx_prev[i]]|^2 of the transform applied in front of the pass (0 without one)

Beside each value comes its MAJORANT A_s: the same expression with every operand replaced by its absolute value and every
subtraction by an addition.  The device forms every term in double and adds the terms in SOME fixed order; whatever the order,
the forward error of such a sum is at most (n - 1) u sum|terms| to first order, u = 2^-53, and forming a term costs at most 8
more roundings (none for sum p, sum q and the products of two widened floats, <= 3 for |p|^2, |q|^2 and products of doubles,
<= 8 for the plane terms).  Hence

    tol_s = 2 (n + 16) 2^-53 A_s                      (the 2: second-order terms and the one rounding of the reference)

and, where the rows travel in the compact format (icp_kernels.h, NN_CROW: the pass's tag replaces the low 16 mantissa bits of
compact slots 0 / 4 / 8 / 12 = ERR, SQ.x, SQP[1], SQP[5], once per row), 2^-36 A_s more for those four slots.  For ERR the
majorant is the sum itself: every term is a square.  These bounds are derived, not measured; a one-point defect (a point
dropped, counted twice, a padding lane added) is 8 to 10 orders of magnitude above them -- test_ref_moments.py shows that for
the very clouds the GPU tests use (clouds.py).
"""
from fractions import Fraction

import numpy as np

NMOM = 32
ERR, CNT, SP, SQ, SQP, SPP, SQQ, MC, MB = 0, 1, 2, 5, 8, 17, 18, 2, 23
P2P_SLOTS = tuple(range(SP, SQQ + 1))                 # beside ERR and CNT
P2P_COMPACT_SLOTS = tuple(range(SP, SPP))             # the compact rows carry neither SPP nor SQQ
PLANE_SLOTS = tuple(range(MC, MB + 6))
COMPACT_TAGGED = (ERR, SQ, SQP + 1, SQP + 5)          # compact slots 0, 4, 8, 12
U = 2.0 ** -53


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------
def _exact_ints(arrays):
    """float arrays (fp32 / fp64) -> (object arrays of Python ints, e) with array == ints * 2**e EXACTLY, one e for all"""
    parts = []
    for a in arrays:
        a = np.asarray(a)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        m, ex = np.frexp(a.astype(np.float64))                    # a = m 2^ex, 0.5 <= |m| < 1 (widening a float is exact)
        mant = np.ldexp(m, 53).astype(np.int64)                   # an integer below 2^53 in magnitude: exact
        parts.append((mant, ex.astype(np.int64) - 53))
    lows = [int(ex[mant != 0].min()) for mant, ex in parts if (mant != 0).any()]
    e = min(lows) if lows else 0
    out = []
    for mant, ex in parts:
        shift = np.where(mant != 0, ex - e, 0)
        out.append(mant.astype(object) << shift.astype(object))
    return out, e


def _round_once(total, e):
    """the integer `total` on the scale 2**e, as the nearest double"""
    return float(Fraction(int(total)) * Fraction(2) ** e)


def _osum(a):
    return int(sum(a.tolist(), 0))


def _cols(a):
    return a[:, 0], a[:, 1], a[:, 2]


def sq_error(P_new, Q, idx_prev):
    """sum |P_new[i] - Q[idx_prev[i]]|^2, exact and rounded once (0 where there was no transform)"""
    if P_new is None or idx_prev is None:
        return 0.0
    (p, q), e = _exact_ints([P_new, np.asarray(Q)[np.asarray(idx_prev)]])
    d = q - p
    return _round_once(_osum((d * d).reshape(-1)), 2 * e)


def p2p(P, Q, idx, P_new=None, idx_prev=None):
    """(moments[32], majorants[32]) of a point-to-point pass over P (n x 3) matched to Q[idx]; ERR from (P_new, idx_prev)"""
    P, Q, idx = np.asarray(P), np.asarray(Q), np.asarray(idx)
    assert P.dtype == Q.dtype and P.ndim == 2 and P.shape[1] == 3 and idx.shape == (P.shape[0],)
    n = P.shape[0]
    G = Q[idx]
    (p, q), e = _exact_ints([P, G])
    mom, maj = np.zeros(NMOM), np.zeros(NMOM)
    mom[ERR] = sq_error(P_new, Q, idx_prev)
    maj[ERR] = mom[ERR]
    mom[CNT] = maj[CNT] = float(n)
    aP, aG = np.abs(P.astype(np.float64)), np.abs(G.astype(np.float64))
    for a in range(3):
        mom[SP + a] = _round_once(_osum(p[:, a]), e)
        mom[SQ + a] = _round_once(_osum(q[:, a]), e)
        maj[SP + a] = aP[:, a].sum()
        maj[SQ + a] = aG[:, a].sum()
        for b in range(3):
            mom[SQP + 3 * a + b] = _round_once(_osum(q[:, a] * p[:, b]), 2 * e)
            maj[SQP + 3 * a + b] = (aG[:, a] * aP[:, b]).sum()
    mom[SPP] = _round_once(_osum((p * p).reshape(-1)), 2 * e)
    mom[SQQ] = _round_once(_osum((q * q).reshape(-1)), 2 * e)
    maj[SPP], maj[SQQ] = (aP * aP).sum(), (aG * aG).sum()
    return mom, maj


def plane_terms_abs(P, G, N):
    """per point: (|cn| (n x 6), |bi| (n,)) with every operand replaced by its absolute value and every subtraction by an addition"""
    (px, py, pz), (qx, qy, qz), (nx, ny, nz) = (_cols(np.abs(np.asarray(a, dtype=np.float64))) for a in (P, G, N))
    cn = np.stack([py * nz + pz * ny, pz * nx + px * nz, px * ny + py * nx, nx, ny, nz], axis=1)
    bi = (px + qx) * nx + (py + qy) * ny + (pz + qz) * nz
    return cn, bi


def plane(P, Q, Nrm, idx, P_new=None, idx_prev=None):
    """(moments[32], majorants[32]) of a point-to-plane pass: C (21, upper triangle row-major) and b (6), evaluated exactly
    from the kernels' statements cn = (p x n, n), bi = (p - q) . n, C += cn cn^T, b -= cn bi with q = Q[idx], n = Nrm[idx]"""
    P, Q, Nrm, idx = np.asarray(P), np.asarray(Q), np.asarray(Nrm), np.asarray(idx)
    assert P.dtype == Q.dtype == Nrm.dtype and idx.shape == (P.shape[0],)
    n = P.shape[0]
    G, N = Q[idx], Nrm[idx]
    (p, q, nr), e = _exact_ints([P, G, N])
    assert e <= 0
    one = 1 << (-e)                                    # the number 1 on the scale 2^e
    (px, py, pz), (qx, qy, qz), (nx, ny, nz) = _cols(p), _cols(q), _cols(nr)
    cn = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx * one, ny * one, nz * one]   # scale 2^2e
    bi = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz                                            # scale 2^2e
    acn, abi = plane_terms_abs(P, G, N)
    mom, maj = np.zeros(NMOM), np.zeros(NMOM)
    mom[ERR] = sq_error(P_new, Q, idx_prev)
    maj[ERR] = mom[ERR]
    mom[CNT] = maj[CNT] = float(n)
    o = MC
    for a in range(6):
        for c in range(a, 6):
            mom[o] = _round_once(_osum(cn[a] * cn[c]), 4 * e)
            maj[o] = (acn[:, a] * acn[:, c]).sum()
            o += 1
    for a in range(6):
        mom[MB + a] = _round_once(-_osum(cn[a] * bi), 4 * e)
        maj[MB + a] = (acn[:, a] * abi).sum()
    return mom, maj


def tolerance(maj, n, compact=False):
    """tol_s = 2 (n + 16) 2^-53 A_s, and 2^-36 A_s more for the four tagged slots of compact rows (module docstring)"""
    tol = 2.0 * (n + 16) * U * np.asarray(maj, dtype=np.float64)
    if compact:
        for s in COMPACT_TAGGED:
            tol[s] += 2.0 ** -36 * maj[s]
    return tol


# ---- per-point terms (what one dropped or doubled point changes a slot by) ---------------------------------------------------
def p2p_point_terms(P, Q, idx, idx_prev=None):
    """(n x 32) the term every point adds to each slot, in double (a one-point defect moves the slot by exactly that much)"""
    P, G = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)[np.asarray(idx)]
    t = np.zeros((P.shape[0], NMOM))
    if idx_prev is not None:
        t[:, ERR] = ((np.asarray(Q, dtype=np.float64)[np.asarray(idx_prev)] - P) ** 2).sum(axis=1)
    t[:, CNT] = 1.0
    t[:, SP:SP + 3], t[:, SQ:SQ + 3] = P, G
    for a in range(3):
        for b in range(3):
            t[:, SQP + 3 * a + b] = G[:, a] * P[:, b]
    t[:, SPP], t[:, SQQ] = (P * P).sum(axis=1), (G * G).sum(axis=1)
    return t


def plane_point_terms(P, Q, Nrm, idx, idx_prev=None):
    P64, Q64, N64 = (np.asarray(a, dtype=np.float64) for a in (P, Q, Nrm))
    G, N = Q64[np.asarray(idx)], N64[np.asarray(idx)]
    cn = np.concatenate([np.cross(P64, N), N], axis=1)
    bi = ((P64 - G) * N).sum(axis=1)
    t = np.zeros((P64.shape[0], NMOM))
    if idx_prev is not None:
        t[:, ERR] = ((Q64[np.asarray(idx_prev)] - P64) ** 2).sum(axis=1)
    t[:, CNT] = 1.0
    o = MC
    for a in range(6):
        for c in range(a, 6):
            t[:, o] = cn[:, a] * cn[:, c]
            o += 1
    for a in range(6):
        t[:, MB + a] = -cn[:, a] * bi
    return t


# ---- the transform front end, operation by operation -------------------------------------------------------------------------
def apply_rt(P, R, t):
    """((r0 x + r1 y) + r2 z) + t with every product and sum rounded in P's precision (apply_rt of icp_device.h; R, t are cast to
    that precision first, as the launchers and the mailbox do)"""
    P = np.asarray(P)
    F = P.dtype.type
    R = np.asarray(R, dtype=np.float64).reshape(3, 3).astype(P.dtype)
    t = np.asarray(t, dtype=np.float64).reshape(3).astype(P.dtype)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.empty_like(P)
    for a in range(3):
        c = (R[a, 0] * x).astype(P.dtype)
        c = (c + (R[a, 1] * y).astype(P.dtype)).astype(P.dtype)
        c = (c + (R[a, 2] * z).astype(P.dtype)).astype(P.dtype)
        out[:, a] = (c + F(t[a])).astype(P.dtype)
    return out
