"""CPU: the numpy restatement of icp_batch_remove_outliers (tests/batch_outlier_ref.py) on hand cases, in fp32 and fp64: the
lattice whose deviation is exactly zero, a sheet with planted far points (what each rule removes is recorded here as the
reference gives it), coincident points, a cloud of k + 1 points, radius counts decided on the threshold, and the order of the
sums.  test_gpu_batch_outlier.py compares the device with this reference byte for byte."""
import numpy as np
import pytest

import batch_outlier_ref as ro

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@DTYPES
def test_lattice_has_no_deviation(dtype):
    L = ro.lattice(dtype)
    Y, m, score, st = ro.remove(L, ("statistical", 3, 0.0))
    assert st.tolist() == [0.5, 0.0, 0.5, 512.0]            # every point has three neighbours at exactly 0.5: a point on the threshold is kept
    assert (score == 0.5).all() and Y.tobytes() == L.tobytes() and np.array_equal(m, np.arange(512))
    Y, m, score, st = ro.remove(L, ("statistical", 6, 0.0))
    interior = ((L > 0) & (L < 3.5)).all(axis=1)
    assert st[3] == 216 and np.array_equal(m >= 0, interior)   # the 6 x 6 x 6 interior points: six neighbours at 0.5
    assert (score[interior] == 0.5).all() and (score[~interior] > st[0]).all() and st[2] == st[0]
    assert Y.tobytes() == L[interior].tobytes()


# per seed: (planted removed, sheet points removed) by statistical k=16 a=1, statistical k=8 a=2, radius 0.25 min 4
SHEET = {0: [(30, 0), (27, 0), (30, 0)], 1: [(29, 0), (25, 0), (30, 0)], 2: [(30, 0), (27, 0), (30, 0)], 3: [(30, 0), (28, 0), (30, 2)]}


@DTYPES
@pytest.mark.parametrize("seed", sorted(SHEET))
def test_sheet_with_planted_points(dtype, seed):
    X, planted = ro.sheet(seed, dtype)
    assert X.shape == (606, 3) and planted.sum() == 30
    got = []
    for rule in (("statistical", 16, 1.0), ("statistical", 8, 2.0), ("radius", 0.25, 4)):
        Y, m, score, st = ro.remove(X, rule)
        gone = m < 0
        got.append((int((gone & planted).sum()), int((gone & ~planted).sum())))
        assert Y.shape[0] == st[3] == 606 - gone.sum() and Y.tobytes() == X[~gone].tobytes()
        assert np.array_equal(m[~gone], np.arange(Y.shape[0]))
    assert got == SHEET[seed]
    # k = 16, a = 1 removes every planted point and no sheet point for three seeds of four; k = 8, a = 2 leaves planted points in
    # (the planted points inflate std: that is the algorithm); the radius rule removes all 30 and at most 2 sheet points
    assert (got[0] == (30, 0)) == (seed != 1) and 2 <= 30 - got[1][0] <= 5 and got[2][0] == 30 and got[2][1] <= 2


@DTYPES
def test_coincident_points_count_at_distance_zero(dtype):
    Z = ro.coincident(dtype)
    Y, m, score, st = ro.remove(Z, ("statistical", 8, 1.0))
    assert (score == 0.0).sum() == 40 and st[3] == 257       # 40 points coincide: each has 39 others at distance 0
    c, thr2 = ro.counts(Z, 1e-3)
    assert (c == 39).sum() == 40 and (c == 0).sum() == 260
    Y, m, score, st = ro.remove(Z, ("radius", 1e-3, 39))
    assert st[3] == 40 and (Y == Y[0]).all() and st[2] == float(dtype(1e-3 * 1e-3))


@DTYPES
def test_cloud_of_k_plus_one_points(dtype):
    X = ro.normal(9, 5, dtype)
    Y, m, score, st = ro.remove(X, ("statistical", 8, 0.5))
    d = np.sqrt(((X[:, None, :].astype(np.float64) - X[None, :, :].astype(np.float64)) ** 2).sum(-1))
    assert np.allclose(score, d.sum(axis=1) / 8.0, rtol=1e-6) and st[3] == 6   # every other point is a neighbour
    X2 = ro.normal(2, 6, dtype)
    Y, m, score, st = ro.remove(X2, ("statistical", 1, 0.0))
    assert score[0] == score[1] and st[1] == 0.0 and st[3] == 2
    with pytest.raises(AssertionError):
        ro.dbar(X, 9)


@DTYPES
def test_radius_counts_on_the_threshold(dtype):
    T = ro.threshold_cloud(dtype)   # the integer lattice 5 x 5 x 5: d2 is 1, 2, 3, ... exactly
    c, thr2 = ro.counts(T, 1.0)
    assert thr2 == 1.0 and np.bincount(c).tolist() == [0, 0, 0, 8, 36, 54, 27]           # d2 == thr2 counts
    c, thr2 = ro.counts(T, np.sqrt(2.0))
    assert thr2 == (2.0 if dtype == np.float32 else 2.0000000000000004) and c.max() == 18   # the face diagonals are in, in both
    c, thr2 = ro.counts(T, np.sqrt(3.0))
    # r * r in double is 2.9999999999999996: fp32 rounds it to 3.0 and the space diagonals are in, fp64 keeps them out
    assert (thr2, int(c.max())) == ((3.0, 26) if dtype == np.float32 else (2.9999999999999996, 18))
    c, thr2 = ro.counts(T, float(np.float32(np.sqrt(2.0))))   # sqrt(2) rounded down to fp32: the product stays below 2
    assert thr2 < 2.0 and c.max() == 6


def test_the_order_of_the_sums():
    x = ro.order_sensitive()
    by_rule = ro.ordered_sum(x) / 130
    assert by_rule == 0.004615384615384615
    assert float(np.sum(x)) / 130 != by_rule and sum(x.tolist()) / 130 != by_rule and ro.ordered_sum(x, granule=32) / 130 != by_rule
    mean, std, thr, keep = ro.statistic(np.abs(x), 1.0)
    assert mean == ro.ordered_sum(np.abs(x)) / 130 and thr == mean + 1.0 * std and keep.sum() == 128


def test_copy_and_pairs():
    X = ro.normal(70, 1, np.float32)
    X[3, 1] = -0.0
    Y, m, score, st = ro.remove(X, None)
    assert Y.tobytes() == X.tobytes() and np.array_equal(m, np.arange(70)) and (score == 0).all() and st.tolist() == [0, 0, 0, 70]
    ref = ro.remove_pairs([(X, X[:40])], ("statistical", 5, 1.0), [None])
    assert ref["stats"].shape == (2, 4) and ref["stats"][1].tolist() == [0, 0, 0, 40] and ref["clouds"][0][1].tobytes() == X[:40].tobytes()
    kept = ref["moving_map"][0] >= 0
    assert np.signbit(ref["clouds"][0][0][ref["moving_map"][0][3], 1]) if kept[3] else True
