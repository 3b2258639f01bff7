"""CPU: the reference the GPU tests of reciprocal matches lean on (tests/batch_mutual_ref.py), pinned with the figures it gives on the
fp32 clouds of batch_ref.gate_case -- numpy and the oracle only, no device.

    rule                          passes        kept per case (of 270 / 194 / 1155 / 68 moving points)
    mutual alone                  0             148, 122, 426, 17
    mutual alone                  1 and 2       149, 123, 441, 17
    mutual + gate at MD = 0.05    0             21, 16, 55, 2
    mutual + trim 0.5             0             102, 91, 246, 9

None of the 70 / 64 / 130 / 5 planted outliers is kept in any of these passes; no distance was chosen to get that.  The loop of
the mutual rule alone ends in 4 / 3 / 5 / 4 iterations at an RMS between 9.6e-4 and 1.7e-3.  orc.nn and ref_numpy.nn agree in both
directions.  On the integer clouds (batch_mutual_ref.tie_clouds) 181 moving points have a tied forward minimum, 40 of the 61
distinct matched model points a tied reverse minimum, the rule keeps 42, and breaking the reverse ties towards the highest index
changes the mask at 52 points: a reverse search with another tie order cannot pass the GPU test on these clouds."""
import numpy as np

from batch_mutual_ref import (all_sq_dist, combined_mask, keep_mutual, mutual_loop, mutual_mask, mutual_mask_numpy, nn_highest,
                              tie_clouds)
from batch_ref import CASES, gate_case, rank, sq_dist, tau_ref, threshold

MD = 0.05
RHO = 0.5
SIZES = [270, 194, 1155, 68]
KEPT_PASS0 = [148, 122, 426, 17]
KEPT_LATER = [149, 123, 441, 17]
KEPT_GATE_PASS0 = [21, 16, 55, 2]
KEPT_TRIM_PASS0 = [102, 91, 246, 9]


def test_mutual_rule_on_the_gate_cases(orc):
    cases = [gate_case(*c) for c in CASES]
    assert [A.shape[0] for A, _, _ in cases] == SIZES
    assert [int(o.sum()) for _, _, o in cases] == [70, 64, 130, 5]
    for k, (A, M, is_out) in enumerate(cases):
        idx, rev, mask = mutual_mask(orc, A, M)
        assert idx.dtype == np.int32 and rev.shape == (M.shape[0],) and mask.dtype == bool
        assert mask.sum() == KEPT_PASS0[k], (k, int(mask.sum()))
        assert not (mask & is_out).any()
        # the lowest i that attains the pair's smallest distance is mutual: the rule alone never keeps nothing
        d = sq_dist(A, M, idx)
        assert mask[int(np.argmin(d))]
        # the reverse distance of (j, i) is the forward distance of (i, j), bit for bit
        D = all_sq_dist(A, M)
        assert np.array_equal(D.min(axis=1), d) and np.array_equal(np.argmin(D, axis=1), idx) and np.array_equal(np.argmin(D, axis=0), rev)
        # with a gate, with a trim: three independent tests; tau ranks all n distances
        gate, _, tau = combined_mask(A, M, idx, rev, md=MD)
        assert gate.sum() == KEPT_GATE_PASS0[k] and np.isinf(tau) and np.array_equal(gate, mask & (d <= threshold(MD, A.dtype)))
        trim, _, tau = combined_mask(A, M, idx, rev, rho=RHO)
        K = rank(RHO, A.shape[0])
        assert tau == tau_ref(d, K) and (d <= tau).sum() == K
        assert trim.sum() == KEPT_TRIM_PASS0[k] and trim.sum() < K
        assert not (gate & is_out).any() and not (trim & is_out).any()


def test_oracle_and_numpy_agree_in_both_directions(orc):
    for c in CASES:
        A, M, _ = gate_case(*c)
        for got, want in zip(mutual_mask(orc, A, M), mutual_mask_numpy(A, M)):
            assert np.array_equal(got, want), c
    A, M = tie_clouds(np.float32)
    for got, want in zip(mutual_mask(orc, A, M), mutual_mask_numpy(A, M)):
        assert np.array_equal(got, want)


def test_mutual_loop_figures(orc):
    its, rms = [], []
    for k, c in enumerate(CASES):
        A, M, is_out = gate_case(*c)
        w = mutual_loop(orc, A, M, keep_mutual(orc), 40, 1e-6)
        print(f"{c}: kept {w['kept']}, iterations {w['iterations']}, final RMS {w['err'][-1]:.3e}")
        assert w["kept"][0] == KEPT_PASS0[k]
        assert all(v == KEPT_LATER[k] for v in w["kept"][1:]) and len(w["kept"]) >= 3
        assert not any((m & is_out).any() for m in w["masks"])
        its.append(w["iterations"])
        rms.append(w["err"][-1])
    assert its == [4, 3, 5, 4]
    assert 9.55e-4 <= min(rms) < 9.65e-4 and 1.65e-3 <= max(rms) < 1.75e-3, rms   # 9.6e-4 and 1.7e-3, to two digits


def test_mutual_rule_on_tied_minima(orc):
    for dtype in (np.float32, np.float64):
        A, M = tie_clouds(dtype)
        idx, rev, mask = mutual_mask(orc, A, M)
        D = all_sq_dist(A, M)
        assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 20       # small integers: every comparison is exact
        tied_fwd = (D == D.min(axis=1, keepdims=True)).sum(axis=1) > 1
        assert tied_fwd.sum() == 181
        matched = np.unique(idx)
        tied_rev = (D[:, matched] == D[:, matched].min(axis=0, keepdims=True)).sum(axis=0) > 1
        assert matched.size == 61 and tied_rev.sum() == 40
        assert mask.sum() == 42
        other = nn_highest(M, A)[idx] == np.arange(A.shape[0])              # reverse ties towards the highest index instead
        assert (other != mask).sum() == 52
