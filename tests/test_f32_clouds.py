"""CPU: what makes the clouds of tests/test_gpu_f32_matching.py tests of the float32 matching kernels -- conditions on the inputs,
shown with numpy and the oracle alone (no device): what every scale of cl.F32_TIE_SCALES does to the squared distances of the tie
pair (ties kept, subnormal non-zero minima, all-zero and all-inf tables with the oracle at point 0), ties that straddle the end of
the first 32 768-point super box, the twins where the docstring puts them after the rounding to float32, a far pair whose cold
bound admits both super boxes, fuzz seeds that reach every kind, every scale twice, both signs of zero and ragged chunks, and a
mixed cloud whose five outliers have no finite distance while everybody else has one."""
import numpy as np
import pytest

import clouds as cl

TINY = float(np.finfo(np.float32).tiny)          # the smallest normal float32


def _d2(P, Q):
    """(dx*dx + dy*dy) + dz*dz, every operation rounded in float32: [len(P), len(Q)]"""
    assert P.dtype == Q.dtype == np.float32
    with np.errstate(over="ignore", under="ignore"):
        d = P[:, None, :] - Q[None, :, :]
        d = d * d
        out = (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]
    assert out.dtype == np.float32
    return out


def _tie_table(orc, scale):
    """per centre of the tie pair at `scale`: (minimum, number of tied minima, first tied index, last tied index), the shares of
    +inf and of 0 among all squared distances, and the oracle's answer"""
    P, M = cl.straddling_tie_pair(scale=scale, dtype=np.float32)
    assert P.shape == (700, 3) and M.shape == (40425, 3) and P.dtype == M.dtype == np.float32
    assert np.isfinite(P).all() and np.isfinite(M).all()
    assert np.unique(M, axis=0).shape[0] == 40425 and np.unique(P, axis=0).shape[0] == 700      # distinct after the cast
    mn, ties, first, last, ninf, nzero = [], [], [], [], 0, 0
    for lo in range(0, 700, 100):
        d = _d2(P[lo:lo + 100], M)
        m = d.min(axis=1)
        tie = d == m[:, None]
        mn.append(m)
        ties.append(tie.sum(axis=1))
        first.append(tie.argmax(axis=1))
        last.append(M.shape[0] - 1 - tie[:, ::-1].argmax(axis=1))
        ninf += int(np.isinf(d).sum())
        nzero += int((d == 0).sum())
    total = 700 * M.shape[0]
    return (np.concatenate(mn), np.concatenate(ties), np.concatenate(first), np.concatenate(last), ninf / total, nzero / total, orc.nn(P, M))


def test_scales_are_the_issue_s():
    assert cl.F32_TIE_SCALES == (1.0, 1e-20, 3e-22, 1e-25, 1e19, 1e20)
    assert cl.F32_FUZZ_SCALES == (1e-25, 3e-22, 1e-20, 1e-3, 1.0, 1e3, 1e15, 1e19, 1e20)
    assert set(cl.F32_TIE_SCALES) == {1.0, cl.F32_ZERO_SCALE, cl.F32_PART_INF_SCALE, cl.F32_INF_SCALE} | set(cl.F32_SUBNORMAL_SCALES)


def test_tie_pair_float64_form_is_unchanged():
    """the dtype argument leaves the float64 pair, and so tests/test_gpu_f64_matching.py's inputs, as they were"""
    P, M = cl.straddling_tie_pair()
    assert P.dtype == M.dtype == np.float64 and P.flags.c_contiguous and M.flags.c_contiguous
    P32, M32 = cl.straddling_tie_pair(dtype=np.float32)
    assert np.array_equal(P32, P.astype(np.float32)) and np.array_equal(M32, M.astype(np.float32))
    assert np.array_equal(P32.astype(np.float64), P) and np.array_equal(M32.astype(np.float64), M)     # (small half-integers: exact)


def test_tie_pair_at_scale_one_straddles_the_first_super_box(orc):
    mn, ties, first, last, inf_share, zero_share, want = _tie_table(orc, 1.0)
    assert (mn == np.float32(0.75)).all() and (ties == 8).all() and inf_share == 0.0 and zero_share == 0.0
    assert np.array_equal(first, want)                                   # the oracle's answer is the lowest tied index
    assert ((first < cl.SUPER_BOX_POINTS) & (last >= cl.SUPER_BOX_POINTS)).mean() >= 0.5
    assert set(int(j) % 8 for j in first) == set(range(8))               # the winner sits at every place of a chunk of 8
    m_pad = -(-40425 // 16) * 16
    assert m_pad > cl.SUPER_BOX_POINTS and m_pad < cl.SPARSE_M_PAD_BELOW   # past the sample probe's m_pad <= 32768, flat search by default


@pytest.mark.parametrize("scale,lo,hi", [(1e-20, 7.4e-41, 7.6e-41), (3e-22, 6.6e-44, 6.8e-44)])
def test_subnormal_scales_keep_all_eight_ties(orc, scale, lo, hi):
    """every minimum is a subnormal that is not zero, and the eight ties of scale 1 are all still there"""
    mn, ties, first, last, inf_share, zero_share, want = _tie_table(orc, scale)
    assert (mn > 0).all() and (mn < TINY).all() and lo < float(mn.min()) and float(mn.max()) < hi, (mn.min(), mn.max())
    assert (ties == 8).all(), (int(ties.min()), int(ties.max()))
    assert inf_share == 0.0
    assert np.array_equal(first, want)
    assert np.array_equal(want, _tie_table(orc, 1.0)[6])                 # ... the very ties of scale 1: the same winners
    assert ((first < cl.SUPER_BOX_POINTS) & (last >= cl.SUPER_BOX_POINTS)).mean() >= 0.5


@pytest.mark.parametrize("scale,value", [(cl.F32_ZERO_SCALE, 0.0), (cl.F32_INF_SCALE, np.inf)])
def test_extreme_scales_leave_the_oracle_point_zero(orc, scale, value):
    mn, ties, first, last, inf_share, zero_share, want = _tie_table(orc, scale)
    assert (mn == value).all() and (ties == 40425).all()                 # the whole table is one value
    assert (inf_share, zero_share) == ((1.0, 0.0) if value else (0.0, 1.0))
    assert (want == 0).all()


def test_partly_overflowing_scale_has_finite_minima_among_infinities(orc):
    mn, ties, first, last, inf_share, zero_share, want = _tie_table(orc, cl.F32_PART_INF_SCALE)
    assert inf_share > 0.99 and inf_share < 1.0, inf_share
    assert np.isfinite(mn).all() and 7.4e37 < float(mn.min()) and float(mn.max()) < 7.6e37, (mn.min(), mn.max())
    assert int(ties.min()) == 1 and int(ties.max()) == 8                 # the coordinates' rounding thins the ties out
    assert np.array_equal(first, want)


def test_tie_pair_with_replacement_fills_more_rows_than_a_device_has_cus():
    P, M = cl.straddling_tie_pair(n=cl.EIGHT_WAVE_N, replace=True, dtype=np.float32)
    assert P.shape == (cl.EIGHT_WAVE_N, 3) and np.array_equal(M, cl.straddling_tie_pair(dtype=np.float32)[1])
    n_pad = -(-cl.EIGHT_WAVE_N // 1024) * 1024
    assert n_pad // 64 == 272 and n_pad // 128 == 136                    # rows of 64: more than 256 CUs; rows of 128: one segment (>= half the CUs)
    assert np.unique(P, axis=0).shape[0] > 4000


def test_twin_model_has_its_twins_where_it_says(orc):
    P, M, want = cl.twin_model(dtype=np.float32)
    P64, M64, want64 = cl.twin_model()
    assert P.dtype == M.dtype == np.float32 and np.array_equal(want, want64)
    assert np.array_equal(P, P64.astype(np.float32)) and np.array_equal(M, M64.astype(np.float32))
    assert np.array_equal(orc.nn(P, M), want)
    same_chunk = other_chunk = other_box = second_box = zeros = 0
    for k in range(0, len(P), 2):
        a = int(want[k])
        twins = np.flatnonzero((M == M[a]).all(axis=1))              # (== takes -0.0 for 0.0): nobody else fell onto the point
        assert len(twins) == 3 and twins[0] == a and np.array_equal(P[k], M[twins[1]]) and np.array_equal(P[k + 1], M[twins[2]])
        b, c = int(twins[1]), int(twins[2])
        same_chunk += a // 8 == c // 8
        other_chunk += a // 8 != b // 8 and c < cl.SUPER_BOX_POINTS
        other_box += a < cl.SUPER_BOX_POINTS <= c
        second_box += a >= cl.SUPER_BOX_POINTS
        zeros += bool((np.signbit(M[c]) != np.signbit(M[a])).any())
    assert min(same_chunk, other_chunk, other_box, second_box) >= 10 and zeros >= 20


def test_far_pair_admits_nearly_every_chunk_of_both_super_boxes(orc):
    P, M = cl.far_pair(dtype=np.float32)
    assert M.shape == (40000, 3) and P.shape == (700, 3) and P.dtype == M.dtype == np.float32
    idx = orc.nn(P, M)
    d = P - M[idx]
    nn = ((d * d)[:, 0] + (d * d)[:, 1]) + (d * d)[:, 2]
    assert nn.min() > 12.0                                                              # wider than the model: its diagonal squared is 12
    lo, hi = M.reshape(5000, 8, 3).min(axis=1), M.reshape(5000, 8, 3).max(axis=1)     # the chunks' boxes
    for rows in (64, 128):
        for r in range(0, 700, rows):                                                   # a row of points: one block
            glo, ghi = P[r:r + rows].min(axis=0), P[r:r + rows].max(axis=0)
            g = np.maximum(np.maximum(lo - ghi, glo - hi), np.float32(0.0))
            L = ((g * g)[:, 0] + (g * g)[:, 1]) + (g * g)[:, 2]
            for chunks in (slice(0, 4096), slice(4096, 5000)):
                # (a block admits a chunk under its points' LARGEST bound, and a cold bound is no tighter than the true minimum)
                assert (L[chunks] < nn[r:r + rows].max()).mean() > 0.95


def test_mixed_cloud_has_five_points_without_a_finite_distance(orc):
    P, M = cl.mixed_overflow_pair()
    assert P.shape == (705, 3) and P.dtype == M.dtype == np.float32 and np.isfinite(P).all() and np.isfinite(M).all()
    assert np.abs(M).max() <= 1.0
    assert cl.MIXED_OUTLIERS == (0, 63, 127, 128, 704)          # lanes 0 and 63 of a row of 64, both sides of a row-of-128 border, the last
    d = _d2(P, M)
    out = np.zeros(705, dtype=bool)
    out[list(cl.MIXED_OUTLIERS)] = True
    assert np.isinf(d[out]).all() and np.isfinite(d[~out].min(axis=1)).all() and np.isfinite(d[~out]).all()
    assert 1.9e19 < np.abs(P[out]).min() and np.abs(P[out]).max() < 5e19 and np.abs(P[~out]).max() < 1.1
    want = orc.nn(P, M)
    assert (want[out] == 0).all() and np.array_equal(want, np.where(out, 0, d.argmin(axis=1)))
    assert (want[~out] != 0).mean() > 0.99                      # (point 0 is not everybody's answer)


def test_float32_signed_zeros_come_after_every_other_draw():
    """signed_zeros=True is legal in float32, changes signs of zeros only, and a cloud without it has the bytes it always had"""
    for kind in cl.FUZZ_KINDS:
        a = cl.fuzz_cloud(np.random.default_rng(5), 200, kind, 1e3)
        b = cl.fuzz_cloud(np.random.default_rng(5), 200, kind, 1e3, np.float32, signed_zeros=True)
        assert b.dtype == np.float32 and np.array_equal(a, b)                   # (== takes -0.0 for 0.0)
        flipped = np.signbit(b) & (b == 0)
        assert flipped.any() == bool((a == 0).any()) and not (np.signbit(a) & (a == 0)).any()
        c = cl.fuzz_cloud(np.random.default_rng(5), 200, kind, 1e3, np.float64, signed_zeros=True)
        assert np.array_equal(np.signbit(c), np.signbit(b))                    # the float64 form's very draws


@pytest.mark.parametrize("sort", sorted(cl.F32_FUZZ_SEEDS))
def test_fuzz_seeds_reach_every_kind_scale_and_ragged_chunk(orc, sort):
    cases = list(cl.f32_matching_cases(cl.F32_FUZZ_SEEDS[sort], cl.F32_FUZZ_CASES))
    assert len(cases) == 36
    for kinds in ([c[2] for c in cases], [c[3] for c in cases]):
        assert set(kinds) == set(cl.FUZZ_KINDS)
    scales = [c[4] for c in cases]
    assert all(scales.count(s) >= 2 for s in cl.F32_FUZZ_SCALES) and set(scales) == set(cl.F32_FUZZ_SCALES)
    assert {0, 1, 7} <= set(c[1] % 8 for c in cases)                 # models that end on, just past and just short of a chunk of 8
    dup = lattice = line = neg0 = pos0 = False
    none_found = some_found = 0
    for n, m, kp, km, scale, P, Q in cases:
        assert P.shape == (n, 3) and Q.shape == (m, 3) and P.dtype == Q.dtype == np.float32
        assert 1 <= n < 700 and 1 <= m < 900 and np.isfinite(P).all() and np.isfinite(Q).all()
        if km == "clustered" and m > 20:
            dup |= np.unique(Q, axis=0).shape[0] < m
        if km == "lattice":
            lattice |= np.unique(Q, axis=0).shape[0] <= 343
        if km == "line":
            line |= bool((Q[:, 1:] == 0.0).all()) and np.unique(Q[:, 0]).shape[0] > 1 or m == 1
        for X in (P, Q):
            neg0 |= bool((np.signbit(X) & (X == 0.0)).any())
            pos0 |= bool((~np.signbit(X) & (X == 0.0)).any())
        d = _d2(P, Q).min(axis=1)
        want = orc.nn(P, Q)
        if scale == cl.F32_INF_SCALE or scale == cl.F32_PART_INF_SCALE:
            assert (want[np.isinf(d)] == 0).all()                    # no finite distance: point 0
            none_found += int(np.isinf(d).sum())
            some_found += int(np.isfinite(d).sum())
        if scale == cl.F32_ZERO_SCALE:
            assert (d == 0).all() and (want == 0).all()
        if scale in cl.F32_SUBNORMAL_SCALES:
            assert (d < TINY).all()
    assert dup and lattice and line and neg0 and pos0
    assert none_found > 100 and some_found > 100                     # points with no finite neighbour and points with one
