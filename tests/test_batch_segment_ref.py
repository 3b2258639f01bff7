"""CPU: the numpy restatement of icp_batch_segment_plane (tests/batch_segment_ref.py) on hand cases -- a planted plane is found, the
refit's normal agrees with numpy.linalg.eigh on the inliers' covariance, the zero heap of a lidar behaves as the rule says, the
hall scan gives up its wall -- and the two host functions of the library (icp_plane_from_points, icp_plane_from_moments) equal it
bit for bit."""
import numpy as np
import pytest

import batch_segment_ref as sr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _angle(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), abs(float(a @ b))))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_plane_is_found(dtype):
    nv = np.array([1.0, 2.0, -2.0]) / 3.0
    X = sr.planted(600, 0.5, dtype, seed=3, normal=nv, offset=0.25, noise=0.002)
    r = sr.segment(X, sr.rule(sr.REMOVE, 0.004, 200), seed=11)
    assert r["status"] == sr.OK and r["winner"] >= 0
    assert r["inliers"] >= 300 and r["inliers"] == int(r["mask"].sum())
    assert _angle(r["plane"][:3], nv) < 2e-3 and abs(abs(r["plane"][3]) - 0.25) < 4e-3
    keep = r["mask"] == 0
    assert np.array_equal(r["cloud"], X[keep]) and np.array_equal(r["map"][keep], np.arange(int(keep.sum())))
    assert (r["map"][~keep] == -1).all()
    k = sr.segment(X, sr.rule(sr.KEEP, 0.004, 200), seed=11)
    assert np.array_equal(k["mask"], r["mask"]) and np.array_equal(k["cloud"], X[~keep])
    d = sr.segment(X, sr.rule(sr.DETECT, 0.004, 200), seed=11)
    assert np.array_equal(d["cloud"], X) and np.array_equal(d["map"], np.arange(600)) and np.array_equal(_bits(d["plane"]), _bits(r["plane"]))


def test_refit_normal_against_eigh():
    """the refit's normal is within 1e-9 rad of numpy.linalg.eigh's eigenvector on the covariance of the same inliers (the bound of
    the range tests)"""
    X = sr.planted(900, 0.6, np.float64, seed=5, normal=(0.3, -0.2, 0.9), offset=-0.1, noise=0.003)
    r = sr.segment(X, sr.rule(sr.DETECT, 0.006, 300), seed=2)
    win = r["planes"][r["winner"]]
    inl = sr.on_plane(X, win, 0.006)
    c, cov, k = sr.moments(X, inl)
    assert k == int(r["counts"][r["winner"]]) >= 500
    fit, ok = sr.plane_from_moments(c, cov)
    assert ok and np.array_equal(_bits(r["plane"]), _bits(fit if r["refit"] else win))
    r = dict(plane=fit)
    C = np.array([[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]])
    assert np.allclose(C, np.cov(X[inl].T, bias=True), rtol=1e-10, atol=1e-15) and np.allclose(c, X[inl].mean(0), rtol=1e-12)
    w, V = np.linalg.eigh(C)
    assert _angle(r["plane"][:3], V[:, 0]) < 1e-9
    assert abs(r["plane"][3] + float(r["plane"][:3] @ c)) < 1e-15


POINT_CASES = {
    "axes": [[0, 0, 0], [1, 0, 0], [0, 1, 0]],
    "flipped": [[0, 0, 0], [0, 1, 0], [1, 0, 0]],
    "general": [[0.3, -1.25, 2.0], [1.5, 0.75, -0.5], [-2.0, 0.125, 0.875]],
    "far": [[1e6 + 0.5, -3e5, 2.5e5], [1e6 - 1.0, -3e5 + 2.0, 2.5e5], [1e6, -3e5, 2.5e5 + 3.0]],
    "collinear": [[0, 0, 0], [1, 1, 1], [3, 3, 3]],
    "coincident": [[1.5, 2.5, -3.5]] * 3,
    "two coincide": [[1, 2, 3], [1, 2, 3], [4, 5, 6]],
    "tie xy +": [[0, 0, 0], [1, -1, 0], [0, 0, 1]],        # w = (-1, -1, 0): equal magnitudes, the lowest index decides -> negated
    "tie xy -": [[0, 0, 0], [0, 0, 1], [1, 1, 0]],         # w = (-1, 1, 0): x decides, negated to (1, -1, 0)
    "tie yz": [[0, 0, 0], [1, 0, 0], [0, 1, -1]],          # w = (0, 1, 1)
    "tie xyz": [[0, 0, 0], [1, -1, 0], [0, 1, -1]],        # w = (1, 1, 1)
    "tie xyz -": [[0, 0, 0], [0, 1, -1], [1, -1, 0]],      # w = (-1, -1, -1)
    "tie mixed": [[0, 0, 0], [1, 1, 0], [0, 1, 1]],        # w = (1, -1, 1): x positive decides, kept
    "huge": [[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0]],     # l overflows: invalid
    "tiny": [[0, 0, 0], [1e-200, 0, 0], [0, 1e-200, 0]],   # l underflows to 0: invalid
    "large ok": [[0, 0, 0], [2.0 ** 200, 0, 0], [0, 2.0 ** 200, 2.0 ** 199]],
    "small ok": [[0, 0, 0], [2.0 ** -200, 0, 0], [0, 2.0 ** -200, 2.0 ** -201]],
}


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_plane_from_points_equals_numpy(pkg, name):
    abc = np.array(POINT_CASES[name], dtype=np.float64)
    want, ok = sr.plane_from_points(abc[0], abc[1], abc[2])
    got = pkg.plane_from_points(abc)
    assert ok == (name not in ("collinear", "coincident", "two coincide", "huge", "tiny"))
    if not ok:
        assert got is None and not want.any()
        return
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    big = int(np.argmax(np.abs(want[:3])))                       # (argmax: the first of equal magnitudes)
    assert want[big] > 0 and abs(float(want[:3] @ want[:3]) - 1.0) < 1e-15


def test_plane_from_points_sign_ties():
    assert np.array_equal(sr.plane_from_points(*np.array(POINT_CASES["tie xy +"], dtype=np.float64))[0][:3] > 0, [True, True, False])
    assert np.array_equal(np.sign(sr.plane_from_points(*np.array(POINT_CASES["tie xy -"], dtype=np.float64))[0][:3]), [1.0, -1.0, 0.0])
    assert np.array_equal(np.sign(sr.plane_from_points(*np.array(POINT_CASES["tie xyz -"], dtype=np.float64))[0][:3]), [1.0, 1.0, 1.0])
    assert np.array_equal(np.sign(sr.plane_from_points(*np.array(POINT_CASES["tie mixed"], dtype=np.float64))[0][:3]), [1.0, -1.0, 1.0])


MOMENT_CASES = {
    "flat z": ([0.5, -0.25, 2.0], [1.0, 0.0, 0.0, 2.0, 0.0, 0.0]),
    "flat x": ([1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 1.0, 0.25, 3.0]),
    "general": ([0.1, 0.2, 0.3], [2.0, 0.3, -0.4, 1.5, 0.2, 0.7]),
    "zero matrix": ([1.0, 1.0, 1.0], [0.0] * 6),                 # the Jacobi leaves v = I: column 0 = (1, 0, 0)
    "isotropic": ([0.0, 0.0, 5.0], [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]),
    "large": ([3.0, 4.0, 5.0], [2.0 ** 500, 2.0 ** 498, 0.0, 2.0 ** 499, 2.0 ** 497, 2.0 ** 480]),
    "nan diagonal": ([0.0, 0.0, 0.0], [np.nan, 0.0, 0.0, 1.0, 0.0, 1.0]),   # off == 0 ends the Jacobi at once: v = I, a finite vector
    "nan": ([0.0, 0.0, 0.0], [1.0, np.nan, 0.0, 1.0, 0.0, 1.0]),             # the rotations spread the NaN: dropped
    "negative first": ([0.0, 1.0, 0.0], [1.0, 0.9, 0.0, 1.0, 0.0, 5.0]),   # the eigenvector (1, -1, 0) / sqrt 2 up to sign
}


@pytest.mark.parametrize("name", list(MOMENT_CASES))
def test_plane_from_moments_equals_numpy(pkg, name):
    c, cov = MOMENT_CASES[name]
    want, ok = sr.plane_from_moments(c, cov)
    got = pkg.plane_from_moments(c, cov)
    assert ok == (name != "nan")
    if not ok:
        assert got is None
        return
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert want[int(np.argmax(np.abs(want[:3])))] > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_heap(dtype):
    """40 % of the points are copies of the origin, as the zero returns of a lidar: no triple out of the heap is valid, and a plane
    through the origin counts every point of the heap -- the rule's stated answer; dropping them is the caller's job"""
    rng = np.random.default_rng(8)
    X = rng.uniform(-1.0, 1.0, (500, 3))
    X[:150, 2] = 0.5 + rng.uniform(-0.001, 0.001, 150)         # the true plane z = 0.5: 30 % of the cloud
    X[300:] = 0.0                                              # the heap: 40 %
    X = np.ascontiguousarray(X.astype(dtype))
    rl = sr.rule(sr.DETECT, 0.002, 400)
    r = sr.segment(X, rl, seed=4)
    heap = np.arange(300, 500)
    in_heap = np.isin(r["triples"], heap)
    assert (in_heap.sum(axis=1) == 3).any()                                    # such triples are drawn ...
    assert not r["valid"][in_heap.sum(axis=1) == 3].any()                      # ... and none of them is valid
    assert not r["valid"][in_heap.sum(axis=1) == 2].any()                      # (two coincident picks: collinear)
    through = r["valid"].astype(bool) & (in_heap.sum(axis=1) == 1)             # a plane through the origin ...
    assert through.any() and (r["counts"][through] >= 200).all()               # ... counts the whole heap
    assert r["mask"][heap].all() and r["inliers"] >= 200 and abs(r["plane"][3]) <= 0.002   # and such a plane wins: the trap
    dropped = sr.segment(X[:300], rl, seed=4)                                  # the caller's answer: drop them first
    assert dropped["inliers"] >= 150 and abs(dropped["plane"][2]) > 0.999 and abs(dropped["plane"][3] + 0.5) < 0.002


def test_collinear_cloud_has_no_plane():
    X = np.outer(np.arange(40, dtype=np.float64), [1.0, 2.0, -0.5])
    for kind in (sr.DETECT, sr.REMOVE):
        r = sr.segment(X, sr.rule(kind, 0.1, 33), seed=1)
        assert r["status"] == sr.ERR_EMPTY and not r["valid"].any() and (r["counts"] == -1).all()
        assert not r["plane"].any() and r["inliers"] == 0 and not r["mask"].any() and np.array_equal(r["cloud"], X)


def test_axis_picks_the_floor():
    rng = np.random.default_rng(2)
    wall = np.column_stack([np.zeros(300), rng.uniform(0, 2, 300), rng.uniform(0, 2, 300)])     # x = 0: the larger patch
    floor = np.column_stack([rng.uniform(0, 2, 120), rng.uniform(0, 2, 120), np.zeros(120)])    # z = 0
    X = np.ascontiguousarray(np.vstack([wall, floor, rng.uniform(0, 2, (60, 3))])[rng.permutation(480)])
    free = sr.segment(X, sr.rule(sr.DETECT, 0.01, 300), seed=9)
    held = sr.segment(X, sr.rule(sr.DETECT, 0.01, 300, axis=(0, 0, 2.0), min_cos=0.9), seed=9)
    assert abs(free["plane"][0]) > 0.999 and free["inliers"] >= 300
    assert abs(held["plane"][2]) > 0.999 and 120 <= held["inliers"] < 300
    assert np.array_equal(free["triples"], held["triples"]) and held["valid"].sum() < free["valid"].sum()


def test_hall_wall():
    """The hall pair, converted on the CPU from the golden ranges with the zero returns dropped (12 023 points each), under the
    hall rule: 1 000 hypotheses, distance 0.02, no axis.  Measured on this numpy reference before the condition was fixed: the
    moving cloud gives 2 675 inliers (22.2 %) and the model 2 665 (22.2 %) at the test's seed, 2024 -- the wall x = -2.29 -- and the
    moving cloud 21.3 % to 22.2 % over the seeds 1 .. 7.  The condition is that floor less a margin for the seed: >= 15 %."""
    P, Q = sr.hall()
    assert P.shape == (12023, 3) and Q.shape == P.shape and P.dtype == np.float32
    for X, r in zip((P, Q), sr.hall_reference()):
        share = r["inliers"] / X.shape[0]
        print(f"hall: {r['inliers']} of {X.shape[0]} = {share:.4f}, plane {r['plane']}, refit {r['refit']}")
        assert r["status"] == sr.OK and share >= 0.15
        assert abs(r["plane"][0]) > 0.98 and abs(abs(r["plane"][3]) - 2.29) < 0.05
        assert r["cloud"].shape[0] == X.shape[0] - r["inliers"]
