"""CPU: the numpy restatement of batched Fast Global Registration (tests/batch_fgr_ref.py) against planted pairs and plain
properties -- the driver recovers the planted pose within the RANSAC test's bounds, right matches end with a weight near 1 and
wrong ones near 0, the objective does not rise while mu stays, a three-point list reproduces its pose, the schedule never goes below
delta^2, the used list of the tuple test is sorted and free of repeats, and the restated solve agrees with numpy's."""
import numpy as np
import pytest

import batch_feature_ref as fr
import batch_fgr_ref as gr
import ref_moments as rm

ROWS = [(31, 130, 3), (32, 65, 2), (33, 64, 3)]      # seed, points, every wrong-th match is wrong
_RUN = {}


def planted(seed, n, wrong, dtype):
    key = (seed, n, wrong, np.dtype(dtype).str)
    if key not in _RUN:
        P, Q, F, G, T = gr.planted_pair(seed, n, dtype, wrong)
        fwd, _, kept = fr.match(F, G, False)
        ci, cj = fr.correspondences(fwd, kept)
        _RUN[key] = (P, Q, ci, cj, T, gr.fgr(P, Q, ci, cj, 0.02))
    return _RUN[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("seed,n,wrong", ROWS)
def test_driver_recovers_the_planted_pose(seed, n, wrong, dtype):
    P, Q, ci, cj, T, r = planted(seed, n, wrong, dtype)
    assert r["status"] == gr.OK and r["used"].size == n
    rot, tr = fr.angle_deg(r["T"][:3, :3] @ T[:3, :3].T), np.abs(r["T"][:3, 3] - T[:3, 3]).max()
    right = cj == ci
    print(f"seed {seed}: rot {rot:.2e} deg trans {tr:.2e} l right >= {r['weights'][right].min():.6f} l wrong <= {r['weights'][~right].max():.6f}")
    assert rot < 0.1 and tr < 1e-3
    assert (r["weights"][right] > 0.99).all() and (r["weights"][~right] < 0.5).all()
    assert abs(np.linalg.det(r["T"][:3, :3]) - 1.0) < 1e-12
    # the objective does not rise between two iterations that share one mu
    mu, obj = r["mu_hist"], r["mom_hist"][:, rm.ERR]
    same = mu[1:] == mu[:-1]
    assert same.sum() >= 40 and (obj[1:][same] <= obj[:-1][same] * (1.0 + 1e-12)).all()
    assert r["objective"] == obj[-1] and np.array_equal(r["T_hist"][0], np.eye(4))


def test_a_three_point_list_reproduces_the_pose():
    P, Q, ci, cj, T, _ = planted(31, 130, 3, np.float64)
    right = np.flatnonzero(cj == ci)[:3]
    r = gr.fgr(P, Q, ci[right], cj[right], 0.02)
    assert r["status"] == gr.OK and r["used"].size == 3
    assert fr.angle_deg(r["T"][:3, :3] @ T[:3, :3].T) < 1e-6
    assert (r["weights"][ci[right]] > 0.999999).all() and np.count_nonzero(r["weights"]) == 3
    assert gr.fgr(P, Q, ci[right][:2], cj[right][:2], 0.02)["status"] == gr.EMPTY


def test_schedule():
    mu = gr.schedule(12.0, 0.02, 64, 1.4, 4)
    assert mu[0] == 12.0 / 1.4 and (mu[:4] == mu[0]).all() and mu[4] == mu[0] / 1.4 and len(set(mu.tolist())) == 16
    low = gr.schedule(1e-3, 0.02, 64, 1.4, 1)
    assert low[-1] == 0.02 * 0.02 and (low >= 0.02 * 0.02).all() and (np.diff(low) <= 0).all()
    assert (gr.schedule(1e-5, 0.02, 8, 1.4, 1) == 1e-5).all()      # already below delta^2: never raised, never lowered


def test_used_list_of_the_tuple_test():
    P, Q, ci, cj, _, _ = planted(31, 130, 3, np.float32)
    u = gr.used_list(P, Q, ci, cj, 5, 96, 0.9)
    tr, valid = fr.hypotheses(P, Q, ci, cj, 5, 96, 0.9)
    assert (np.diff(u) > 0).all() and set(u.tolist()) == set(tr[valid > 0].reshape(-1).tolist()) and 3 <= u.size < 130
    every = gr.used_list(P, Q, ci, cj, 5, 96, 0.0)
    assert np.array_equal(every, gr.drawn(5, 96, len(ci))) and set(u.tolist()) <= set(every.tolist())
    assert np.array_equal(gr.used_list(P, Q, ci, cj, 5, 0, 0.9), np.arange(130))
    r = gr.fgr(P, Q, ci, cj, 0.02, tuples=96, tuple_similarity=0.9, seed=5)
    assert r["status"] == gr.OK and np.count_nonzero(r["weights"]) <= u.size and (r["weights"][np.setdiff1d(np.arange(130), ci[u])] == 0).all()


def test_restated_solve_agrees_with_numpy():
    import batch_gicp_ref as gic
    P, Q, ci, cj, _, _ = planted(32, 65, 2, np.float64)
    t, _, ok = gr.terms(P[ci], Q[cj], np.eye(4), 3.0)
    mom, maj = gr.exact_sums(t, ok)
    assert ok.all() and mom[rm.CNT] == 65 and (mom[30:] == 0).all() and (maj >= np.abs(mom)).all()
    R, tv = gr.solve(mom)
    R2, t2 = gic.solve(mom)
    assert np.abs(R - R2).max() < 1e-9 and np.abs(tv - t2).max() < 1e-9
    zero = mom.copy()
    zero[rm.MC] = 0.0
    assert gr.solve(zero) is None


def test_collinear_pair_is_singular_at_the_identity():
    for dtype in (np.float32, np.float64):
        P, Q, F, G = gr.collinear_pair(dtype)
        fwd, _, kept = fr.match(F, G, False)
        ci, cj = fr.correspondences(fwd, kept)
        assert np.array_equal(cj, np.arange(3))
        r = gr.fgr(P, Q, ci, cj, 0.02)
        assert r["status"] == gr.SINGULAR and np.array_equal(r["T"], np.eye(4)) and r["mom_hist"][0, rm.MC] == 0.0
        assert (r["mu_hist"][1:] == 0).all() and (r["weights"] > 0).all()
