"""CPU: the numpy restatement of batched global registration (tests/batch_feature_ref.py) against itself and against plain
properties -- the descriptor of a cloud equals that of its rigidly moved copy with moved normals, the diamond angle is monotone
in atan2, every sub-histogram sums to 100 or is all zero, the generator's draws match values computed independently (a C program
with uint64_t arithmetic), and the driver recovers a planted pose."""
import numpy as np

import batch_feature_ref as fr


def test_descriptor_is_invariant_under_a_rigid_motion():
    X, N = fr.blob(3, 240, np.float64)
    k = 10
    R, t = fr.rodrigues((0.3, -1.0, 0.7), 77.0), np.array([0.4, -1.1, 2.5])
    Y, NY = np.ascontiguousarray(X @ R.T + t), np.ascontiguousarray(N @ R.T)
    hx, hy = fr.neighbourhood(X, k), fr.neighbourhood(Y, k)
    assert np.array_equal(hx[2], hy[2])   # a generic cloud: no decision of the neighbourhood sits on a rounding
    Sx, Sy = fr.spfh(X, N, k, hx)[0], fr.spfh(Y, NY, k, hy)[0]
    # away from bin edges: a point whose own SPFH and whose neighbours' SPFH fell into the same bins in both poses
    same = (Sx == Sy).all(axis=1)
    away = same & ~(hx[2] & ~same[None, :]).any(axis=1)
    assert away.mean() > 0.9, away.mean()
    Fx, Fy = fr.fpfh(X, N, k), fr.fpfh(Y, NY, k)
    assert np.abs(Fx - Fy)[away].max() < 1e-9
    assert np.abs(Fx).max() > 10.0   # (not a comparison of zeros)


def test_diamond_angle_is_monotone_in_atan2():
    a = np.linspace(-np.pi, np.pi, 20001)[1:-1]
    x, y = np.cos(a), np.sin(a)
    t = fr.diamond(x, y)
    assert (np.diff(t) > 0).all() and t.min() > -2.0 and t.max() < 2.0
    assert fr.diamond(1.0, 0.0) == 0.0 and fr.diamond(0.0, 1.0) == 1.0 and fr.diamond(-1.0, 0.0) == 2.0 and fr.diamond(0.0, -1.0) == -1.0
    assert fr.diamond(0.0, 0.0) == 0.0
    assert abs(fr.diamond(-1.0, -1e-300) + 2.0) < 1e-12
    b = fr.bin_of(t, -2.0, 4.0)
    assert b.min() == 0 and b.max() == 10 and (np.diff(b) >= 0).all()
    assert fr.bin_of(np.array([-1.0, 1.0, 0.999999, np.nan, 5.0, -5.0]), -1.0, 2.0).tolist() == [0, 10, 10, 0, 10, 0]


def test_every_sub_histogram_sums_to_100_or_is_zero():
    X, N = fr.blob(5, 150, np.float32)
    F = fr.fpfh(X, N, 8)
    s = F.reshape(-1, 3, 11).sum(axis=2)
    assert np.abs(s - 100.0).max() < 1e-9 and (F >= 0).all()
    S, c = fr.spfh(X, N, 8)
    assert (c >= 8).all() and np.abs(S.reshape(-1, 3, 11).sum(axis=2) - 100.0).max() < 1e-9
    # a collinear cloud whose normals lie along the line: every pair has v = d x n1 = 0 and is skipped
    L = np.zeros((20, 3), dtype=np.float32)
    L[:, 0] = np.arange(20)
    NL = np.tile(np.array([1.0, 0.0, 0.0]), (20, 1))
    S, c = fr.spfh(L, NL, 3)
    assert (c == 0).all() and (S == 0).all() and (fr.fpfh(L, NL, 3) == 0).all()


def test_generator_matches_independent_values():
    assert fr.mix(0) == 16294208416658607535          # splitmix64's first output for the state 0
    assert fr.draw(0, 0, 0, 391) == 348
    assert fr.draw(1, 7, 2, 3) == 1
    assert fr.draw(0xDEADBEEFCAFEF00D, 1999, 15, 65536) == 33665
    s = fr.triple(5, 11, 391)
    assert len(set(s)) == 3 and s == [fr.draw(5, 11, r, 391) for r in range(3)]
    assert fr.triple(5, 11, 2)[2] == -1               # two candidates can never fill three slots


def test_matching_rule_lowest_index_wins_both_ways():
    rng = np.random.default_rng(2)
    F = rng.uniform(0, 100, (9, 33))
    G = np.concatenate([F[[4, 4, 2]], rng.uniform(0, 100, (3, 33))])
    fwd, rev, kept = fr.match(F, G, True)
    assert fwd[4] == 0 and fwd[2] == 2 and rev[0] == 4 and rev[1] == 4 and kept[4] == 1 and kept[2] == 1
    assert fr.match(F, G, False)[2].all()
    ci, cj = fr.correspondences(fwd, kept)
    assert (np.diff(ci) > 0).all() and np.array_equal(cj, fwd[ci])


def test_driver_recovers_a_planted_pose():
    rng = np.random.default_rng(8)
    P = rng.standard_normal((60, 3)).astype(np.float32)
    R, t = fr.rodrigues((1.0, -2.0, 0.5), 131.0), np.array([0.3, 0.2, -0.7])
    Q = (P.astype(np.float64) @ R.T + t).astype(np.float32)
    ci = np.arange(60, dtype=np.int32)
    cj = ci.copy()
    cj[::3] = rng.integers(0, 60, 20)                 # a third of the matches are wrong
    r = fr.ransac(P, Q, ci, cj, 7, 64, 0.01, 0.9)
    assert r["status"] == 0 and r["inliers"] >= 40 and r["counts"][r["winner"]] == r["counts"][r["valid"] > 0].max()
    assert (r["counts"][:r["winner"]] < r["counts"][r["winner"]]).all()
    assert fr.angle_deg(r["T"][:3, :3] @ R.T) < 0.01 and np.abs(r["T"][:3, 3] - t).max() < 1e-4
    assert abs(np.linalg.det(r["T"][:3, :3]) - 1.0) < 1e-12
    assert fr.ransac(P, Q, ci[:2], cj[:2], 7, 8, 0.01, 0.9)["status"] == "empty"
