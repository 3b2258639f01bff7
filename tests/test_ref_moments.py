"""The exact moment reference (ref_moments.py) checked on its own, without a device: it agrees with a plain extended-precision
evaluation, and its tolerance sees a single dropped or doubled point in every cloud tests/test_gpu_moments.py uses."""
import math

import numpy as np
import pytest

import clouds as cl
import ref_moments as rm


def _normals(orc, M):
    return orc.normals(M, orc.knn4(M))[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_p2p_reference_against_longdouble(orc, dtype):
    D, M = cl.case_pair(23, 17, dtype)
    assert D.dtype == M.dtype == dtype
    if dtype == np.float64:   # (mantissas that fp32 cannot hold)
        assert not np.array_equal(D, D.astype(np.float32))
    idx = orc.nn(D, M)
    prev = np.roll(idx, 1)
    mom, maj = rm.p2p(D, M, idx, P_new=D, idx_prev=prev)
    L = np.longdouble
    P, G = D.astype(L), M.astype(L)[idx]
    want = np.zeros(rm.NMOM, dtype=L)
    want[rm.ERR] = ((M.astype(L)[prev] - P) ** 2).sum()
    want[rm.CNT] = len(D)
    want[rm.SP:rm.SP + 3], want[rm.SQ:rm.SQ + 3] = P.sum(axis=0), G.sum(axis=0)
    want[rm.SQP:rm.SQP + 9] = (G.T @ P).reshape(9)
    want[rm.SPP], want[rm.SQQ] = (P * P).sum(), (G * G).sum()
    ld_eps = float(np.finfo(L).eps)
    for s in (rm.ERR, rm.CNT) + rm.P2P_SLOTS:
        bound = 4 * len(D) * ld_eps * max(maj[s], 1e-300) + 2.0 ** -52 * abs(mom[s])
        assert abs(float(L(mom[s]) - want[s])) <= bound, s
    assert (maj * (1 + 1e-12) >= np.abs(mom)).all()   # (the majorant itself is an ordinary double sum)
    if dtype == np.float32:   # products of two widened floats are exact in double: math.fsum over them is the same number
        P64, G64 = D.astype(np.float64), M.astype(np.float64)[idx]
        assert mom[rm.SP] == math.fsum(P64[:, 0]) and mom[rm.SQP + 5] == math.fsum(G64[:, 1] * P64[:, 2])
        assert mom[rm.SPP] == math.fsum((P64 * P64).reshape(-1))


def test_plane_reference_against_longdouble(orc):
    D, M = cl.case_pair(23, 17)
    Nrm = _normals(orc, M)
    idx = orc.nn(D, M)
    mom, maj = rm.plane(D, M, Nrm, idx, P_new=D, idx_prev=idx)
    L = np.longdouble
    P, G, N = D.astype(L), M.astype(L)[idx], Nrm.astype(L)[idx]
    cn = np.concatenate([np.cross(P, N), N], axis=1)
    bi = ((P - G) * N).sum(axis=1)
    Cm = cn.T @ cn
    want = np.zeros(rm.NMOM, dtype=L)
    want[rm.ERR], want[rm.CNT] = ((G - P) ** 2).sum(), len(D)
    want[rm.MC:rm.MC + 21] = [Cm[a, c] for a in range(6) for c in range(a, 6)]
    want[rm.MB:rm.MB + 6] = -(cn * bi[:, None]).sum(axis=0)
    ld_eps = float(np.finfo(L).eps)
    for s in (rm.ERR, rm.CNT) + rm.PLANE_SLOTS:
        assert abs(float(L(mom[s]) - want[s])) <= 16 * len(D) * ld_eps * maj[s] + 2.0 ** -52 * abs(mom[s]), s
    assert (maj * (1 + 1e-12) >= np.abs(mom)).all()   # (the majorant itself is an ordinary double sum)


def test_apply_rt_rounds_every_operation():
    P = np.array([[1.0000001, 3.0, -7.0]], dtype=np.float32)
    R = np.array([[1 / 3, 1e-8, 0.1], [0, 1, 0], [0, 0, 1]])
    t = np.array([1e-3, 0, 0])
    f = np.float32
    want = f(f(f(f(f(R[0, 0]) * P[0, 0]) + f(f(R[0, 1]) * P[0, 1])) + f(f(R[0, 2]) * P[0, 2])) + f(t[0]))
    got = rm.apply_rt(P, R, t)
    assert got.dtype == np.float32 and got[0, 0] == want and got[0, 1] == f(3.0) and got[0, 2] == f(-7.0)
    assert rm.apply_rt(P.astype(np.float64), R, t).dtype == np.float64


P2P_CLOUDS = sorted({(n, m) for n in cl.ROW64_N + cl.ROW128_N + cl.FIN_N + cl.BATCH_N for m in cl.MODEL_M} | {(cl.CAP_N, 17), (cl.TWO_STAGE_N, 17)})
PLANE_CLOUDS = sorted({(n, m) for n in cl.ROW64_N + cl.ROW128_N + cl.FIN_N for m in cl.MODEL_M})


def _seen_fraction(terms, tol, slots):
    """share of the points whose removal (or doubling) moves EVERY one of `slots` by more than that slot's tolerance"""
    return float((np.abs(terms[:, slots]) > tol[slots]).all(axis=1).mean())


@pytest.mark.parametrize("n,m", P2P_CLOUDS)
def test_tolerance_sees_one_point_p2p(orc, n, m):
    for dtype in (np.float32, np.float64) if n <= 1200 else (np.float32,):
        D, M = cl.case_pair(n, m, dtype)
        idx = orc.nn(D, M)
        _, maj = rm.p2p(D, M, idx, P_new=D, idx_prev=idx)
        terms = rm.p2p_point_terms(D, M, idx, idx_prev=idx)
        full = list((rm.ERR, rm.CNT) + rm.P2P_SLOTS)
        assert _seen_fraction(terms, rm.tolerance(maj, n), full) >= 0.99
        if dtype == np.float32:   # the compact rows: wider bounds on their four tagged slots, no SPP / SQQ
            compact = list((rm.ERR, rm.CNT) + rm.P2P_COMPACT_SLOTS)
            assert _seen_fraction(terms, rm.tolerance(maj, n, compact=True), compact) >= 0.99


@pytest.mark.parametrize("n,m", PLANE_CLOUDS)
def test_tolerance_sees_one_point_plane(orc, n, m):
    # float64: the clouds of test_full_rows_fp64_point_to_plane and the float64 batch (rows of 64), with the fp32 model's normals cast
    for dtype in (np.float32, np.float64) if n in cl.ROW64_N + cl.BATCH_N else (np.float32,):
        D, M = cl.case_pair(n, m, dtype)
        Nrm = _normals(orc, cl.case_pair(n, m)[1]).astype(dtype)
        idx = orc.nn(D, M)
        _, maj = rm.plane(D, M, Nrm, idx, P_new=D, idx_prev=idx)
        terms = rm.plane_point_terms(D, M, Nrm, idx, idx_prev=idx)
        assert _seen_fraction(terms, rm.tolerance(maj, n), list((rm.ERR, rm.CNT) + rm.PLANE_SLOTS)) >= 0.99
