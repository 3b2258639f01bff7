"""Exact reference of the evaluation vector of icp_batch_evaluate (include/icp_mi355x_diag.h, ICP_EVAL_*), in ref_moments' manner,
and the assembly of the call's outputs from a vector, in plain Python floats.  numpy only; nothing here touches a device.

    both metrics     SD = sum |q - p|^2    CNT                         p = P[i], q = M[idx[i]], over the kept points only
    point-to-point   SQ(3) = sum q         SQQ(6) = sum q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z, q_z q_z
    point-to-plane   C(21) at MC .. MC + 20: ref_moments.plane's C, cn = (p x n, n)

Every sum is formed exactly -- Python integers on one common scale (ref_moments._exact_ints) -- and rounded once.  Beside each value
comes its majorant A_s: sum |q_a| for SQ, sum |q_a| |q_b| for SQQ, ref_moments.plane's for C, and the sum itself for SD (every term
is a square, as check_front_end takes it for ERR).  The device forms every term in double from the widened coordinates and adds
the terms in some fixed order, so ref_moments' bound holds slot by slot:

    tol_s = 2 (n + 16) 2^-53 A_s,   n = the pair's point count (kept or not: the upper bound of the terms added)

The bounds are derived, not measured; test_batch_eval_ref.py shows that a one-point defect is orders of magnitude above them.
"""
import math

import numpy as np

import ref_moments as rm

NMOM = rm.NMOM
SD, CNT, SQ, SQQ, MC = 0, 1, 2, 5, rm.MC
SQQ_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
POINT_SLOTS = tuple(range(SQ, SQQ + 6))
PLANE_SLOTS = tuple(range(MC, MC + 21))


def exact(P, M, idx, mask, plane=False, nrm=None):
    """(vector[32], majorants[32]) of an evaluation of P (n x 3) matched to M[idx], over the points of `mask`; all zeros where the
    mask keeps nothing"""
    P, M, idx, mask = np.asarray(P), np.asarray(M), np.asarray(idx), np.asarray(mask, dtype=bool)
    assert P.dtype == M.dtype and idx.shape == mask.shape == (P.shape[0],)
    vec, maj = np.zeros(NMOM), np.zeros(NMOM)
    if not mask.any():
        return vec, maj
    Pk, ik = P[mask], idx[mask]
    vec[SD] = maj[SD] = rm.sq_error(Pk, M, ik)
    vec[CNT] = maj[CNT] = float(mask.sum())
    if plane:
        mom, mmaj = rm.plane(Pk, M, nrm, ik)
        for s in PLANE_SLOTS:
            vec[s], maj[s] = mom[s], mmaj[s]
        return vec, maj
    G = M[ik]
    (q,), e = rm._exact_ints([G])
    aG = np.abs(G.astype(np.float64))
    for a in range(3):
        vec[SQ + a] = rm._round_once(rm._osum(q[:, a]), e)
        maj[SQ + a] = aG[:, a].sum()
    for k, (a, b) in enumerate(SQQ_PAIRS):
        vec[SQQ + k] = rm._round_once(rm._osum(q[:, a] * q[:, b]), 2 * e)
        maj[SQQ + k] = (aG[:, a] * aG[:, b]).sum()
    return vec, maj


def tolerance(maj, n):
    """tol_s = 2 (n + 16) 2^-53 A_s for the pair's n points"""
    return rm.tolerance(maj, n)


def point_terms(M, idx):
    """(n x 32) the term every point adds to the point-to-point slots behind SD, in double (what a one-point defect moves a slot by)"""
    G = np.asarray(M, dtype=np.float64)[np.asarray(idx)]
    t = np.zeros((G.shape[0], NMOM))
    t[:, CNT] = 1.0
    t[:, SQ:SQ + 3] = G
    for k, (a, b) in enumerate(SQQ_PAIRS):
        t[:, SQQ + k] = G[:, a] * G[:, b]
    return t


def assemble(vec, n, plane=False):
    """dict(inliers, fitness, rmse, information) from an evaluation vector alone, in Python floats: the header's formulas, each
    entry of the information matrix at most one addition of two slots"""
    v = [float(x) for x in vec]
    cnt = v[CNT]
    I = [[0.0] * 6 for _ in range(6)]

    def sym(r, s, val):
        I[r][s] = I[s][r] = val

    if plane:
        o = MC
        for r in range(6):
            for s in range(r, 6):
                sym(r, s, v[o])
                o += 1
    else:
        sx, sy, sz = v[SQ], v[SQ + 1], v[SQ + 2]
        xx, xy, xz, yy, yz, zz = v[SQQ:SQQ + 6]
        sym(0, 0, yy + zz), sym(1, 1, xx + zz), sym(2, 2, xx + yy)
        sym(0, 1, -xy), sym(0, 2, -xz), sym(1, 2, -yz)
        sym(0, 4, -sz), sym(0, 5, sy)
        sym(1, 3, sz), sym(1, 5, -sx)
        sym(2, 3, -sy), sym(2, 4, sx)
        sym(3, 3, cnt), sym(4, 4, cnt), sym(5, 5, cnt)
    return dict(inliers=int(cnt), fitness=cnt / float(n), rmse=math.sqrt(v[SD] / cnt) if cnt > 0.0 else 0.0,
                information=np.array(I, dtype=np.float64))


def info_direct(Q):
    """sum over the rows q = (x, y, z) of Q of G^T G, G = [g1; g2; g3] = [-[q]x | I], formed directly in float64"""
    Q = np.asarray(Q, dtype=np.float64)
    out = np.zeros((6, 6))
    for x, y, z in Q:
        G = np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]])
        out += G.T @ G
    return out


def info_tolerance(maj, n):
    """the bound of every entry of a point-to-point information matrix assembled from a vector within `tolerance` of the exact one:
    the assembly of the slots' bounds (an entry is a slot or the sum of two), plus one rounding of the addition"""
    t = tolerance(maj, n)
    m = assemble(maj, n)["information"]
    return np.abs(assemble(t, n)["information"]) + rm.U * np.abs(m)
