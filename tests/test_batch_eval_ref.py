"""CPU: the exact evaluation reference (batch_eval_ref.py) checked on its own, on the clouds the GPU test uses (batch_ref.gate_case):
the point-to-point information matrix assembled from the exact vector is sum G^T G, symmetric and positive semi-definite, and the
tolerance the GPU test grants sees a single dropped or doubled point."""
import numpy as np
import pytest

import batch_eval_ref as er
from batch_ref import CASES, gate_case, gate_mask

MD = 0.05


def _case(orc, c, dtype):
    A, M, _ = gate_case(*c, dtype=dtype)
    idx = orc.nn(A, M)
    return A, M, idx, gate_mask(A, M, idx, MD)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("c", CASES, ids=[str(c) for c in CASES])
def test_point_information_is_sum_gtg(orc, c, dtype):
    A, M, idx, gated = _case(orc, c, dtype)
    for what, mask in (("gated", gated), ("all", np.ones(len(A), dtype=bool))):
        assert mask.any()
        n = len(A)
        vec, maj = er.exact(A, M, idx, mask)
        out = er.assemble(vec, n)
        I = out["information"]
        want = er.info_direct(M[idx[mask]])
        tol = er.info_tolerance(maj, n)
        dev = np.abs(I - want)
        print(f"{c} {np.dtype(dtype).name} {what}: kept {int(mask.sum())}, largest |assembled - direct| / tol = {np.max(dev / np.maximum(tol, 1e-300)):.4f}")
        assert (dev <= tol).all(), (what, dev, tol)
        assert np.array_equal(I, I.T)
        assert I[0, 3] == I[1, 4] == I[2, 5] == 0.0 and I[3, 4] == I[3, 5] == I[4, 5] == 0.0
        assert I[3, 3] == I[4, 4] == I[5, 5] == float(mask.sum()) == out["inliers"]
        w = np.linalg.eigvalsh(I)
        assert w.min() >= -64 * np.finfo(np.float64).eps * w.max(), w   # positive semi-definite up to the eigen-solver's rounding
        assert out["fitness"] == mask.sum() / float(n)
        d = M[idx[mask]].astype(np.float64) - A[mask].astype(np.float64)
        assert abs(out["rmse"] - np.sqrt((d ** 2).sum() / mask.sum())) <= 1e-12 * out["rmse"]
    zero = er.assemble(er.exact(A, M, idx, np.zeros(len(A), dtype=bool))[0], len(A))
    assert zero["inliers"] == 0 and zero["fitness"] == 0.0 and zero["rmse"] == 0.0 and not zero["information"].any()


def test_plane_assembly_mirrors_c(orc):
    A, M, idx, mask = _case(orc, CASES[0], np.float32)
    nrm = orc.normals(M, orc.knn4(M))[0]
    vec, maj = er.exact(A, M, idx, mask, plane=True, nrm=nrm)
    assert not vec[er.MC + 21:].any() and vec[er.CNT] == mask.sum()
    I = er.assemble(vec, len(A), plane=True)["information"]
    assert np.array_equal(I, I.T)
    assert [I[a, c] for a in range(6) for c in range(a, 6)] == vec[er.MC:er.MC + 21].tolist()
    P64, N64 = A[mask].astype(np.float64), nrm[idx[mask]].astype(np.float64)
    cn = np.concatenate([np.cross(P64, N64), N64], axis=1)
    assert np.abs(I - cn.T @ cn).max() <= 1e-12 * np.abs(I).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("c", CASES, ids=[str(c) for c in CASES])
def test_tolerance_sees_one_point(orc, c, dtype):
    """dropping or doubling one kept point moves some slot by orders of magnitude more than that slot's tolerance"""
    A, M, idx, _ = _case(orc, c, dtype)
    mask = np.ones(len(A), dtype=bool)
    _, maj = er.exact(A, M, idx, mask)
    tol = er.tolerance(maj, len(A))
    terms = er.point_terms(M, idx)
    d = M[idx].astype(np.float64) - A.astype(np.float64)
    terms[:, er.SD] = (d ** 2).sum(axis=1)
    slots = [er.SD] + list(er.POINT_SLOTS)   # (without CNT, which moves by exactly 1: the sums themselves must tell)
    ratio = np.abs(terms[:, slots]) / np.where(tol[slots] > 0, tol[slots], np.inf)
    per_point = ratio.max(axis=1)
    print(f"{c} {np.dtype(dtype).name}: a one-point defect moves its most telling slot by {per_point.min():.3e} .. {per_point.max():.3e} tolerances")
    assert per_point.min() >= 1e6
    assert (terms[:, er.CNT] == 1.0).all()
