"""CPU: what makes the clouds of tests/test_gpu_f64_matching.py tests of nn_match_row64_f64 -- conditions on the inputs, shown with
numpy and the oracle alone (no device): the ties are there and straddle the first round's end, the extreme scales leave the oracle
no choice but point 0, the fuzz's fixed seeds reach every kind, every scale and ragged chunk counts, the twins sit where the
docstring says, and a far pair's cold bound admits the whole model."""
import numpy as np
import pytest

import clouds as cl


def _d2(P, Q):
    """(dx*dx + dy*dy) + dz*dz, every operation rounded in float64: [len(P), len(Q)]"""
    d = P[:, None, :] - Q[None, :, :]
    d = d * d
    return (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]


def test_tie_pair_has_eight_tied_minima_that_straddle_the_first_round(orc):
    P, M = cl.straddling_tie_pair()
    assert P.shape == (700, 3) and M.shape == (40425, 3) and P.dtype == M.dtype == np.float64
    assert np.unique(M, axis=0).shape[0] == 40425 and np.unique(P, axis=0).shape[0] == 700
    assert M.shape[0] > cl.ROUND_POINTS and M.shape[0] + 16 < cl.SPARSE_M_PAD_BELOW          # two rounds, and still the sparse form's model
    want = orc.nn(P, M)
    straddle, first = 0, []
    for lo in range(0, 700, 100):
        d = _d2(P[lo:lo + 100], M)
        assert (d.min(axis=1) == 0.75).all()
        tie = d == 0.75
        assert (tie.sum(axis=1) == 8).all()
        for row in tie:
            j = np.flatnonzero(row)
            straddle += int(j[0] < cl.ROUND_POINTS <= j[-1])
            first.append(j[0])
    assert np.array_equal(np.array(first), want)                  # the oracle's answer is the lowest tied index
    assert straddle / 700 >= 0.5, straddle
    assert set(int(j) % 8 for j in first) == set(range(8))       # the winner sits at every place of a chunk of 8


def test_tie_pair_with_replacement_fills_more_rows_than_a_device_has_cus():
    P, M = cl.straddling_tie_pair(n=cl.EIGHT_WAVE_N, replace=True)
    assert P.shape == (cl.EIGHT_WAVE_N, 3) and np.array_equal(M, cl.straddling_tie_pair()[1])
    assert -(-cl.EIGHT_WAVE_N // 1024) * 1024 // 64 == 272         # padded to 17 408 points: 272 rows of 64, an MI355X has 256 CUs
    assert cl.EIGHT_WAVE_N <= 2 * 256 * 64                         # ... and at most two rows per CU: still the sparse form
    assert np.unique(P, axis=0).shape[0] > 4000


@pytest.mark.parametrize("scale,value", [(cl.UNDERFLOW_SCALE, 0.0), (cl.OVERFLOW_SCALE, np.inf)])
def test_extreme_scales_leave_the_oracle_point_zero(orc, scale, value):
    P, M = cl.straddling_tie_pair(scale=scale)
    assert np.isfinite(P).all() and np.isfinite(M).all() and np.unique(M, axis=0).shape[0] == M.shape[0]
    with np.errstate(over="ignore", under="ignore"):
        for lo in range(0, 700, 100):
            assert (_d2(P[lo:lo + 100], M) == value).all()
    assert (orc.nn(P, M) == 0).all()


@pytest.mark.parametrize("sparse", sorted(cl.F64_FUZZ_SEEDS))
def test_fuzz_seeds_reach_every_kind_scale_and_ragged_chunk(sparse):
    cases = list(cl.f64_matching_cases(cl.F64_FUZZ_SEEDS[sparse], 40))
    assert len(cases) == 40
    for kinds in ([c[2] for c in cases], [c[3] for c in cases]):
        assert set(kinds) == set(cl.FUZZ_KINDS)
    assert set(c[4] for c in cases) == set(cl.FUZZ_SCALES)
    assert {0, 1, 7} <= set(c[1] % 8 for c in cases)                 # models that end on, just past and just short of a chunk of 8
    assert any(c[1] < 8 for c in cases) or any(c[0] < 8 for c in cases) or min(c[1] for c in cases) < 64
    full, dup, lattice, line, neg0 = False, False, False, False, False
    for n, m, kp, km, scale, P, Q in cases:
        assert P.shape == (n, 3) and Q.shape == (m, 3) and P.dtype == Q.dtype == np.float64
        assert 1 <= n < 700 and 1 <= m < 900
        if km == "uniform":
            full |= bool((Q != Q.astype(np.float32)).any())          # mantissas float32 cannot hold
        if km == "clustered" and m > 20:
            dup |= np.unique(Q, axis=0).shape[0] < m
        if km == "lattice":
            lattice |= bool((Q == np.round(Q / scale) * scale).all()) and np.unique(Q, axis=0).shape[0] <= 343
        if km == "line":
            line |= bool((Q[:, 1:] == 0.0).all()) and np.unique(Q[:, 0]).shape[0] > 1 or m == 1
        neg0 |= bool((np.signbit(Q) & (Q == 0.0)).any()) and bool((~np.signbit(Q) & (Q == 0.0)).any())
    assert full and dup and lattice and line and neg0


def test_float32_fuzz_clouds_are_the_float64_ones_rounded_once():
    for kind in cl.FUZZ_KINDS:
        a = cl.fuzz_cloud(np.random.default_rng(5), 200, kind, 1e3)
        b = cl.fuzz_cloud(np.random.default_rng(5), 200, kind, 1e3, np.float64)
        assert a.dtype == np.float32 and b.dtype == np.float64 and np.array_equal(a, b.astype(np.float32))


def test_twin_model_has_its_twins_where_it_says(orc):
    P, M, want = cl.twin_model()
    assert np.array_equal(orc.nn(P, M), want)
    same_chunk = other_chunk = other_round = second_round = zeros = 0
    for k in range(0, len(P), 2):
        a = int(want[k])
        twins = np.flatnonzero((M == M[a]).all(axis=1))              # (== takes -0.0 for 0.0)
        assert len(twins) == 3 and twins[0] == a and np.array_equal(P[k], M[twins[1]]) and np.array_equal(P[k + 1], M[twins[2]])
        b, c = int(twins[1]), int(twins[2])
        same_chunk += a // 8 == c // 8
        other_chunk += a // 8 != b // 8 and c < cl.ROUND_POINTS
        other_round += a < cl.ROUND_POINTS <= c
        second_round += a >= cl.ROUND_POINTS
        zeros += bool((np.signbit(M[c]) != np.signbit(M[a])).any())
    assert min(same_chunk, other_chunk, other_round, second_round) >= 10 and zeros >= 20


def test_far_pair_admits_nearly_every_chunk_in_both_rounds(orc):
    P, M = cl.far_pair()
    assert M.shape == (40000, 3) and P.shape == (700, 3)
    idx = orc.nn(P, M)
    d = P - M[idx]
    nn = ((d * d)[:, 0] + (d * d)[:, 1]) + (d * d)[:, 2]
    lo, hi = M.reshape(5000, 8, 3).min(axis=1), M.reshape(5000, 8, 3).max(axis=1)     # the chunks' boxes
    for r in range(0, 700, 64):                                                        # a row of 64 points: one block
        glo, ghi = P[r:r + 64].min(axis=0), P[r:r + 64].max(axis=0)
        g = np.maximum(np.maximum(lo - ghi, glo - hi), 0.0)
        L = (g * g).sum(axis=1)
        for chunks in (slice(0, 4096), slice(4096, 5000)):
            # (a block admits a chunk under its points' LARGEST bound, and a cold bound is no tighter than the true minimum)
            assert (L[chunks] < nn[r:r + 64].max()).mean() > 0.95
