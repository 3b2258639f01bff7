"""CPU: the reference the GPU tests of robust kernels lean on (tests/batch_robust_ref.py), pinned with the figures it gives on the
clouds of batch_ref.gate_case -- numpy and the oracle only, no device.  The same figures for both dtypes (the fp64 clouds are the
fp32 ones, widened).

    loop (no gate, no trim, max_iter 40, tol 1e-6)     iterations per case     final RMS of the true inliers
    point-to-point, plain                              18, 17, 20, 5           0.72 .. 1.40
    point-to-point, Tukey  k = 0.5                     2, 3, 2, 2              1.67e-3 .. 1.77e-3   every outlier weight exactly 0
    point-to-point, Cauchy k = 0.05                    3, 3, 3, 2              1.69e-3 .. 1.78e-3
    point-to-point, Huber  k = 0.05                    3, 9, 4, 3              4.7e-3 .. 3.1e-2     (outliers still pull: weight about 0.01)
    point-to-plane, plain                              40, 40, 40, 30          0.31 .. 1.42
    point-to-plane, Tukey  k = 0.2                     2, 3, 3, 2              1.71e-3 .. 1.85e-3   every outlier weight exactly 0
    point-to-plane, Cauchy k = 0.02                    3, 4, 3, 2              1.71e-3 .. 1.91e-3

The plane loops use the normals of ref_numpy.knn4 + normals_longdouble (batch_robust_ref.robust_normals).  All four cases stay
under the 2e-3 of test_gpu_batch_reciprocal.test_reciprocal_end_to_end, the 17-point model of the fourth case included: none is
left out of the plane end-to-end run.  Point-to-plane Huber does not recover from these outliers and is not run end to end."""
import numpy as np
import pytest

import batch_robust_ref as br
import ref_moments as rm
from batch_ref import CASES, gate_case

ITER_PLAIN = {False: [18, 17, 20, 5], True: [40, 40, 40, 30]}
RUNS = {   # (plane, kernel): (k, iterations per case)
    (False, "tukey"): (0.5, [2, 3, 2, 2]),
    (False, "cauchy"): (0.05, [3, 3, 3, 2]),
    (True, "tukey"): (0.2, [2, 3, 3, 2]),
    (True, "cauchy"): (0.02, [3, 4, 3, 2]),
}
HUBER_P2P = (0.05, [3, 9, 4, 3])
RMS_BOUND = 2e-3
PLAIN_BOUND = 0.3


def test_weight_functions():
    k = 0.5
    r = np.array([0.0, 0.25, 0.5, 1.0, 1e200, np.inf])
    with np.errstate(over="ignore"):
        r2 = r * r                                                                           # (1e200 squared overflows: +inf)
    assert np.array_equal(br.weight(br.NONE, r2, k), np.ones(6))
    assert np.array_equal(br.weight(br.HUBER, r2, k), [1.0, 1.0, 1.0, 0.5, 0.0, 0.0])       # (r2 = +inf: 0, never a NaN)
    assert np.array_equal(br.weight(br.CAUCHY, r2, k), [1.0, 0.8, 0.5, 0.2, 0.0, 0.0])
    assert np.array_equal(br.weight(br.TUKEY, r2, k), [1.0, 0.5625, 0.0, 0.0, 0.0, 0.0])
    # continuous at r = k, and |dw/dr| <= 2 / k everywhere (the constant of the weight bound): a fine grid of slopes
    rr = np.linspace(0.0, 4.0 * k, 200001)
    for kind, slope in ((br.HUBER, 1.0), (br.CAUCHY, 0.65), (br.TUKEY, 1.54)):
        w = br.weight(kind, rr * rr, k)
        assert (w >= 0).all() and (w <= 1).all() and (np.diff(w) <= 0).all()
        worst = np.abs(np.diff(w) / np.diff(rr)).max() * k
        assert slope - 0.02 <= worst <= slope + 1e-3, (kind, worst)


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_plain_loop_does_not_recover(orc, dtype, plane):
    its = []
    for c in CASES:
        A, M, is_out = gate_case(*c, dtype=dtype)
        w = br.robust_loop(orc, A, M, br.NONE, 1.0, 40, 1e-6, br.robust_normals(M) if plane else None)
        rms = br.inlier_rms(w["moved"], M, w["idx"], is_out)
        print(f"{c}: plain loop, iterations {w['iterations']}, inlier RMS {rms:.3e}")
        assert rms > PLAIN_BOUND
        assert all((x == 1.0).all() for x in w["weights"])
        its.append(w["iterations"])
    assert its == ITER_PLAIN[plane]


@pytest.mark.parametrize("run", sorted(RUNS), ids=lambda r: f"{'plane' if r[0] else 'p2p'}-{r[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_robust_loop_figures(orc, dtype, run):
    plane, name = run
    k, want_its = RUNS[run]
    its = []
    for c in CASES:
        A, M, is_out = gate_case(*c, dtype=dtype)
        w = br.robust_loop(orc, A, M, br.KINDS[name], k, 40, 1e-6, br.robust_normals(M) if plane else None)
        rms = br.inlier_rms(w["moved"], M, w["idx"], is_out)
        print(f"{c}: {name} k = {k}, iterations {w['iterations']}, inlier RMS {rms:.3e}")
        assert rms < RMS_BOUND
        last = w["weights"][-1]
        assert last.shape == (A.shape[0],) and (last >= 0).all() and (last <= 1).all()
        if name == "tukey":
            assert (last[is_out] == 0.0).all() and (last[~is_out] > 0.9).all()
        else:
            print('   largest outlier weight', last[is_out].max())
            assert (last[is_out] > 0.0).all() and last[is_out].max() < 1e-3
        its.append(w["iterations"])
    assert its == want_its


def test_huber_point_to_point_is_pulled_by_the_outliers(orc):
    k, want_its = HUBER_P2P
    its, rms = [], []
    for c in CASES:
        A, M, is_out = gate_case(*c)
        w = br.robust_loop(orc, A, M, br.HUBER, k, 40, 1e-6)
        its.append(w["iterations"])
        rms.append(br.inlier_rms(w["moved"], M, w["idx"], is_out))
        assert 0.003 < w["weights"][-1][is_out].min() and w["weights"][-1][is_out].max() < 0.02
    assert its == want_its
    assert 4.5e-3 < min(rms) < 5e-3 and 3.0e-2 < max(rms) < 3.2e-2, rms


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_exact_weighted_sums_against_longdouble(orc, dtype, plane):
    """the integer arithmetic of batch_robust_ref.weighted against a longdouble evaluation: within n 2^-63 A_s + one double
    rounding; W = sum w and CNT = n; with all weights 1 the sums are ref_moments' own"""
    for c, (name, k) in zip(CASES, (("tukey", 0.5), ("cauchy", 0.05), ("huber", 0.05), ("cauchy", 0.02))):
        A, M, _ = gate_case(*c, dtype=dtype)
        nrm = br.robust_normals(M) if plane else None
        idx = orc.nn(A, M)
        w = br.weight(br.KINDS[name], br.residual_sq(plane, A, M, idx, nrm), k)
        assert 0 < w.min() < 0.5 or name == "tukey"
        mom, maj = br.weighted(plane, A, M, nrm, idx, w)
        ld = br.weighted_longdouble(plane, A, M, nrm, idx, w)
        n = A.shape[0]
        assert mom[rm.CNT] == n and mom[rm.ERR] == 0.0
        for s in br.slots(plane):
            bound = (n + 8) * 2.0 ** -63 * maj[s] + 2.0 ** -53 * abs(mom[s])
            assert abs(float(np.longdouble(mom[s]) - ld[s])) <= bound, (c, s, mom[s], ld[s])
        ones = np.ones(n)
        m1, j1 = br.weighted(plane, A, M, nrm, idx, ones)
        m0, j0 = (rm.plane(A, M, nrm, idx) if plane else rm.p2p(A, M, idx))
        assert m1[br.MOM_W] == n
        m1[br.MOM_W] = j1[br.MOM_W] = 0.0
        assert np.array_equal(m1, m0) and np.allclose(j1, j0, rtol=1e-15, atol=0)
        # the residual formed exactly is the double one within its own rounding, far inside the weight bound's budget
        r2x, A_r = br.residual_sq_exact(plane, A, M, idx, nrm)
        r2d = br.residual_sq(plane, A, M, idx, nrm)
        assert (np.abs(np.sqrt(r2x) - np.sqrt(r2d)) <= 8 * br.U * A_r).all()
        assert (A_r >= np.sqrt(r2x)).all()
        assert np.array_equal(br.tolerance(maj, n), 2.0 * (n + 17) * br.U * maj)


def test_reference_constants_are_the_librarys(pkg):
    """the kinds and the slot this reference uses are the ones the header and the Python mirror define"""
    cap = pkg.capi
    assert (cap.ICP_ROBUST_NONE, cap.ICP_ROBUST_HUBER, cap.ICP_ROBUST_CAUCHY, cap.ICP_ROBUST_TUKEY) == (br.NONE, br.HUBER, br.CAUCHY, br.TUKEY)
    assert cap.ICP_MOM_W == br.MOM_W and br.MOM_W < cap.ICP_NMOM - 1 and br.MOM_W > rm.MB + 5 and br.MOM_W > rm.SQQ
    assert {name: pkg.engine._ROBUST_KINDS[name] for name in br.KINDS} == br.KINDS
