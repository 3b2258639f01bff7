"""GPU: batched Fast Global Registration (icp_batch_fgr, icp_diag_batch_fgr; Batch.fgr, Batch.diag_fgr,
Context.register_batch_global(method="fgr")) against the numpy restatement tests/batch_fgr_ref.py.

    1  terms and sums of every iteration: lists of 130, 65 and 2 correspondences (a work item plus two entries, plus one, less than
       a triple; every third match is wrong; the seeds are those of the every-third rows of tests/test_batch_fgr_ref.py, 31 and
       33 -- the numpy restatement alone puts seed 32 with every third match wrong 1.27e-3 off in translation, outside the
       planted bound, so that draw serves the other tests with every second match wrong, as in its row) -- mu bit for bit, CNT, every slot within ref_moments.tolerance of math.fsum of the numpy terms at the device's own
       pose, the next pose against numpy's solve of the device's own vector (1e-9), the planted pose, the weights
    2  a list of exactly 64 entries (one full work item, no tail) and a list of 3
    3  a pair's bytes do not depend on the batch; a second call gives the same bytes
    4  the tuple test: the used list equals numpy's, similarity 0 uses every drawn position, a NULL seed is refused
    5  a collinear pair ends ICP_ERR_SINGULAR at the identity beside a healthy pair that does not notice
    6  the bunny pair end to end, see test_bunny_end_to_end
    7  refusals; 8  a loop under way does not notice

The weights: the header's rule is one IEEE double operation per statement and the kernel is compiled without contraction, so the
device's l and numpy's are the same bits -- bits_equal is asserted, not the 4 ulp the looser reading would allow."""
import ctypes as C

import numpy as np
import pytest

import batch_feature_ref as fr
import batch_fgr_ref as gr
import batch_gicp_ref as gic
import ref_moments as rm
from batch_ref import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
DELTA = 0.02
_PAIR = {}


def pair(seed, n, dtype, wrong=3):
    """(P, Q, F, G, T, ci, cj): batch_fgr_ref.planted_pair and its correspondence list without the mutual test, made once"""
    key = (seed, n, np.dtype(dtype).str, wrong)
    if key not in _PAIR:
        P, Q, F, G, T = gr.planted_pair(seed, n, dtype, wrong)
        fwd, _, kept = fr.match(F, G, False)
        _PAIR[key] = (P, Q, F, G, T) + fr.correspondences(fwd, kept)
    return _PAIR[key]


def cut(X, keep):
    """the pair X reduced to the points `keep`, matched one to one"""
    P, Q = np.ascontiguousarray(X[0][keep]), np.ascontiguousarray(X[1][keep])
    G = np.zeros((len(keep), 33))
    G[np.arange(len(keep)), np.arange(len(keep))] = 50.0
    ci = np.arange(len(keep), dtype=np.int32)
    return P, Q, G.copy(), G, X[4], ci, ci.copy()


def planted(bt, pairs):
    bt.diag_set_features([X[2] for X in pairs], [X[3] for X in pairs])
    fwd, _, kept = bt.match_features(mutual=False)
    for b, X in enumerate(pairs):
        assert np.array_equal(fwd[b], X[6]) and kept[b].all()


def check_history(bt, b, X, res, iterations=64, division_factor=1.4, decrease_every=4, tuples=0, similarity=0.95, seed=0):
    """every iteration of pair b against the numpy terms at the device's own poses; returns the largest |device - exact| / tol"""
    P, Q, ci, cj = X[0], X[1], X[5], X[6]
    dg = bt.diag_fgr(b)
    used = gr.used_list(P, Q, ci, cj, seed, tuples, similarity)
    assert np.array_equal(dg["used_pos"], used) and res["used"] == used.size and used.size >= 3
    U = used.size
    Pu, Qu = P[ci[used]].astype(np.float64), Q[cj[used]].astype(np.float64)
    mus = gr.schedule(gr.scale(Pu, Qu)[0], DELTA, iterations, division_factor, decrease_every)
    assert bits_equal(dg["mu_hist"], mus)
    assert bits_equal(dg["T_hist"][0], np.eye(4)) and res["status"] == 0
    worst = 0.0
    for it in range(iterations):
        T, mom = dg["T_hist"][it], dg["mom_hist"][it]
        t, _, ok = gr.terms(Pu, Qu, T, mus[it])
        assert ok.all()
        want, maj = gr.exact_sums(t, ok)
        tol = gr.tolerance(maj, U)
        assert mom[rm.CNT] == float(U), (b, it, mom[rm.CNT])
        for s in gr.FGR_SLOTS:
            dev = abs(mom[s] - want[s])
            assert dev <= tol[s], f"pair {b} iteration {it} slot {s}: device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
            if tol[s] > 0:
                worst = max(worst, dev / tol[s])
        assert mom[30] == 0.0 and mom[31] == 0.0
        R, tv = gic.solve(mom)                                   # numpy's solve of the device's own vector
        nxt = dg["T_hist"][it + 1] if it + 1 < iterations else res["T"]
        assert np.abs(nxt - gr.compose(R, tv, T)).max() < 1e-9, (b, it)
    assert res["objective"] == dg["mom_hist"][-1][rm.ERR]
    _, l, ok = gr.terms(Pu, Qu, res["T"], mus[-1])
    w = np.zeros(P.shape[0])
    w[ci[used]] = np.where(ok, l, 0.0)
    assert bits_equal(res["weights"], w), np.abs(res["weights"] - w).max()
    return worst


def check_pose(X, res):
    T, ci, cj = X[4], X[5], X[6]
    assert fr.angle_deg(res["T"][:3, :3] @ T[:3, :3].T) < 0.1 and np.abs(res["T"][:3, 3] - T[:3, 3]).max() < 1e-3
    right = cj == ci
    assert (res["weights"][ci[right]] > 0.99).all() and (res["weights"][ci[~right]] < 0.5).all()
    assert abs(np.linalg.det(res["T"][:3, :3]) - 1.0) < 1e-12


def same_bytes(a, b):
    return all(bits_equal(np.asarray(a[f]), np.asarray(b[f])) for f in a) and set(a) == set(b)


# 1 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_terms_and_sums_every_iteration(ctx, pkg, dtype):
    X, Y = pair(31, 130, dtype), pair(33, 65, dtype)
    tiny = cut(X, np.arange(2))
    with ctx.batch([(X[0], X[1]), (Y[0], Y[1]), (tiny[0], tiny[1])]) as bt:
        planted(bt, [X, Y, tiny])
        res = bt.fgr(DELTA)
        worst = max(check_history(bt, 0, X, res[0]), check_history(bt, 1, Y, res[1]))
        print(f"largest |device - exact| / tolerance over every slot and iteration: {worst:.3f}")
        check_pose(X, res[0])
        check_pose(Y, res[1])
        # less than a triple: empty, the identity, no weight, no history
        assert res[2]["status"] == pkg.capi.ICP_ERR_EMPTY and res[2]["used"] == 2 and res[2]["objective"] == 0.0
        assert bits_equal(res[2]["T"], np.eye(4)) and (res[2]["weights"] == 0.0).all()
        dg = bt.diag_fgr(2)
        assert np.array_equal(dg["used_pos"], [0, 1]) and not dg["mu_hist"].any() and not dg["mom_hist"].any() and not dg["T_hist"].any()
        tm = bt.diag_fgr_times()
        assert tm["iterations"] == 64 and min(tm["enqueue_s"], tm["wait_s"], tm["solve_s"]) > 0.0


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_full_work_item_and_a_triple(ctx, pkg, dtype):
    X = pair(33, 64, dtype)
    three = cut(X, np.flatnonzero(X[6] == X[5])[:3])
    with ctx.batch([(X[0], X[1]), (three[0], three[1])]) as bt:
        planted(bt, [X, three])
        res = bt.fgr(DELTA)
        check_history(bt, 0, X, res[0])
        check_history(bt, 1, three, res[1])
        check_pose(X, res[0])
        check_pose(three, res[1])
        assert res[0]["used"] == 64 and res[1]["used"] == 3 and fr.angle_deg(res[1]["T"][:3, :3] @ X[4][:3, :3].T) < 1e-4


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_pairs_bits_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X, Y = pair(31, 130, dtype), pair(32, 65, dtype, wrong=2)

    def run(pairs, twice=False):
        with ctx.batch([(Z[0], Z[1]) for Z in pairs]) as bt:
            planted(bt, pairs)
            res = bt.fgr(DELTA)
            dg = [bt.diag_fgr(b) for b in range(len(pairs))]
            if twice:
                again = bt.fgr(DELTA)
                assert all(same_bytes(again[b], res[b]) and same_bytes(bt.diag_fgr(b), dg[b]) for b in range(len(pairs)))
            return res, dg

    both, swapped = run([X, Y], twice=True), run([Y, X])
    ax, ay = run([X]), run([Y])
    for (res, dg) in ((swapped[0][1], swapped[1][1]), (ax[0][0], ax[1][0])):
        assert same_bytes(res, both[0][0]) and same_bytes(dg, both[1][0])
    for (res, dg) in ((swapped[0][0], swapped[1][0]), (ay[0][0], ay[1][0])):
        assert same_bytes(res, both[0][1]) and same_bytes(dg, both[1][1])
    assert both[0][0]["status"] == 0 and both[0][0]["weights"].max() > 0.99


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_tuple_test(ctx, pkg, dtype):
    X, Y = pair(31, 130, dtype), pair(32, 65, dtype, wrong=2)
    with ctx.batch([(X[0], X[1]), (Y[0], Y[1])]) as bt:
        planted(bt, [X, Y])
        res = bt.fgr(DELTA, tuples=96, tuple_similarity=0.9, seed=[5, 6])
        check_history(bt, 0, X, res[0], tuples=96, similarity=0.9, seed=5)
        check_history(bt, 1, Y, res[1], tuples=96, similarity=0.9, seed=6)
        assert 3 <= res[0]["used"] < 130 and np.count_nonzero(res[0]["weights"]) <= res[0]["used"]
        dg = [bt.diag_fgr(b) for b in range(2)]
        again = bt.fgr(DELTA, tuples=96, tuple_similarity=0.9, seed=[5, 6])
        assert all(same_bytes(again[b], res[b]) and same_bytes(bt.diag_fgr(b), dg[b]) for b in range(2))
        other = bt.fgr(DELTA, tuples=96, tuple_similarity=0.9, seed=[7, 6])
        assert not np.array_equal(bt.diag_fgr(0)["used_pos"], dg[0]["used_pos"]) and same_bytes(other[1], res[1])
        # the edge check off: every position that was drawn
        every = bt.fgr(DELTA, tuples=96, tuple_similarity=0.0, seed=[5, 6])
        for b, (Z, seed) in enumerate(((X, 5), (Y, 6))):
            assert np.array_equal(bt.diag_fgr(b)["used_pos"], gr.drawn(seed, 96, len(Z[5]))) and every[b]["used"] > res[b]["used"]
        # a NULL seed: fine without tuples, refused with them
        prm = pkg.capi.icp_fgr_params(64, DELTA, 1.4, 4, 96, 0.9)
        assert bt._lib.icp_batch_fgr(bt._h, C.byref(prm), None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID
        assert bt.diag_fgr(0)["used_pos"].size == every[0]["used"]        # a refused call leaves the earlier result readable
        prm.tuples = 0
        assert bt._lib.icp_batch_fgr(bt._h, C.byref(prm), None, None, None, None, None, None) == 0


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_singular_pair(ctx, pkg, dtype):
    """three points on the x axis: at the identity row rx of C is exactly zero, the first pivot is 0 whatever the order of the sums.
    batch_fgr_ref.fgr on this pair ends SINGULAR at the identity (tests/test_batch_fgr_ref.py): that status is asserted here."""
    Pl, Ql, Fl, Gl = gr.collinear_pair(dtype)
    line = (Pl, Ql, Fl, Gl, np.eye(4), np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32))
    X = pair(31, 130, dtype)
    want = gr.fgr(Pl, Ql, line[5], line[6], DELTA)
    assert want["status"] == gr.SINGULAR == pkg.capi.ICP_ERR_SINGULAR
    with ctx.batch([(X[0], X[1])]) as bt:
        planted(bt, [X])
        alone, dga = bt.fgr(DELTA)[0], bt.diag_fgr(0)
    with ctx.batch([(Pl, Ql), (X[0], X[1])]) as bt:
        planted(bt, [line, X])
        res = bt.fgr(DELTA)
        assert res[0]["status"] == pkg.capi.ICP_ERR_SINGULAR and res[0]["used"] == 3
        assert np.isfinite(res[0]["T"]).all() and bits_equal(res[0]["T"], want["T"]) and np.isfinite(res[0]["weights"]).all()
        assert bits_equal(res[0]["weights"], want["weights"]) and res[0]["objective"] == want["objective"]
        dg = bt.diag_fgr(0)
        assert dg["mom_hist"][0][rm.CNT] == 3.0 and dg["mom_hist"][0][rm.MC] == 0.0 and not dg["mu_hist"][1:].any()
        assert same_bytes(res[1], alone) and same_bytes(bt.diag_fgr(1), dga) and res[1]["status"] == 0


# 6 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_bunny_end_to_end(ctx, pkg, golden, dtype):
    """The bunny pair of batch_feature_ref.bunny_pair, set up as test_gpu_batch_feature.test_bunny_end_to_end sets it up (k = 24,
    normals facing the centroids, mutual matches: 391 correspondences, about 30 % of them right).  Conditions: fgr(7.5 mm) with
    every correspondence ends with status 0 within 5 degrees and 1 cm of the truth (the numpy restatement: 0.94 degrees, 2.7 mm); a
    point-to-point batch gated at 1 cm and started from that pose ends within 2 degrees, from the identity more than 30 degrees
    away; with the tuple test (2 000 tuples, 0.95, seed 1) the pose is within 10 degrees and 1 cm."""
    A, M, Tt = fr.bunny_pair(golden)
    A, M = A.astype(dtype), M.astype(dtype)
    K, MD, GATE = 24, 0.0075, 0.01
    err = lambda T: (fr.angle_deg(T[:3, :3] @ Tt[:3, :3].T), float(np.linalg.norm(T[:3, 3] - Tt[:3, 3])))
    with ctx.batch([(A, M)]) as bt:
        cm, cq = bt.estimate_covariances(K, None, regularisation="none", want=True)
        NA = pkg.oriented_normals(A, cm[0], A.astype(np.float64).mean(0))
        NM = pkg.oriented_normals(M, cq[0], M.astype(np.float64).mean(0))
        bt.compute_features(K, ([NA], [NM]))
        fwd, rev, kept = bt.match_features(mutual=True)
        start = bt.fgr(MD)[0]
        tup = bt.fgr(MD, tuples=2000, tuple_similarity=0.95, seed=1)[0]
    print(f"used {start['used']} rot {err(start['T'])[0]:.3f} deg trans {err(start['T'])[1] * 1e3:.2f} mm objective {start['objective']:.4e}; "
          f"tuple test: used {tup['used']} rot {err(tup['T'])[0]:.3f} deg trans {err(tup['T'])[1] * 1e3:.2f} mm")
    assert start["status"] == 0 and start["used"] == 391 == int(kept[0].sum())
    assert err(start["T"])[0] < 5.0 and err(start["T"])[1] < 0.01
    assert np.count_nonzero(start["weights"]) == 391 and (start["weights"][kept[0] == 0] == 0.0).all()
    assert tup["status"] == 0 and 3 <= tup["used"] < 391 and err(tup["T"])[0] < 10.0 and err(tup["T"])[1] < 0.01
    fine_ = ctx.register_batch([(A, M)], max_distance=GATE, init=start["T"][None])[0]
    cold = ctx.register_batch([(A, M)], max_distance=GATE)[0]
    print(f"refined {err(fine_.T)[0]:.3f} deg, from the identity {err(cold.T)[0]:.3f} deg")
    assert err(fine_.T)[0] < 2.0
    assert err(cold.T)[0] > 30.0
    # the one-call entry runs the same sequence; the default method is RANSAC, byte for byte
    res = ctx.register_batch_global([(A, M)], 0.0, K, 0, MD, method="fgr", gate=GATE)[0]
    assert same_bytes(res.extra["global"], start) and bits_equal(res.T, fine_.T)
    plain = ctx.register_batch_global([(A, M)], 0.0, K, 2000, MD, seed=1, gate=GATE)[0]
    named = ctx.register_batch_global([(A, M)], 0.0, K, 2000, MD, seed=1, gate=GATE, method="ransac")[0]
    assert bits_equal(plain.extra["global"]["T"], named.extra["global"]["T"]) and plain.extra["global"]["inliers"] == named.extra["global"]["inliers"]
    assert bits_equal(plain.T, named.T) and set(plain.extra["global"]) == {"T", "inliers", "correspondences", "status"}
    with pytest.raises(ValueError):
        ctx.register_batch_global([(A, M)], 0.0, K, 0, MD, method="teaser")


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, pkg):
    E, S = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    X = pair(32, 65, np.float32, wrong=2)

    def code(fn):
        with pytest.raises(pkg.IcpError) as err:
            fn()
        return err.value.code

    with ctx.batch([(X[0], X[1])]) as bt:
        assert code(lambda: bt.fgr(DELTA)) == S                        # no matches
        assert code(lambda: bt.diag_fgr(0)) == S and code(bt.diag_fgr_times) == S
        planted(bt, [X])
        good = bt.fgr(DELTA)[0]
        dg = bt.diag_fgr(0)
        for kw in (dict(iterations=0), dict(iterations=1025), dict(max_distance=0.0), dict(max_distance=np.inf), dict(max_distance=np.nan),
                   dict(division_factor=1.0), dict(division_factor=np.inf), dict(decrease_every=0), dict(tuples=-1), dict(tuples=65537),
                   dict(tuples=8, tuple_similarity=1.0), dict(tuples=8, tuple_similarity=-0.1), dict(tuples=8, tuple_similarity=np.nan)):
            args = dict(max_distance=DELTA)
            args.update(kw)
            assert code(lambda: bt.fgr(**args)) == E, kw
        assert same_bytes(bt.diag_fgr(0), dg)                          # a refused call leaves the earlier result readable
        assert same_bytes(bt.fgr(DELTA, iterations=1024, decrease_every=1 << 20, tuples=0, tuple_similarity=7.0)[0], bt.fgr(DELTA, iterations=1024, decrease_every=1024)[0])
        assert good["status"] == 0
        bt.diag_set_features([X[2]], [X[3]])                           # new descriptors discard the matches
        assert code(lambda: bt.fgr(DELTA)) == S


# 8 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_loop_under_way_does_not_notice(ctx, pkg, dtype):
    A, NA = fr.blob(51, 200, dtype)
    M, NM = fr.blob(52, 150, dtype)
    A = np.ascontiguousarray((A.astype(np.float64) @ fr.rodrigues((0, 0, 1), 4.0).T + 0.02).astype(dtype))

    def run(disturb):
        with ctx.batch([(A, M)]) as bt:
            bt.begin(max_iter=12, tol=1e-9)
            bt.run(3)
            if disturb:
                bt.compute_features(9, ([NA], [NM]))
                bt.match_features()
                r = bt.fgr(0.05)[0]
                bt.fgr(0.05, tuples=40, tuple_similarity=0.5, seed=3)
                bt.diag_fgr(0)
                assert r["status"] in (0, pkg.capi.ICP_ERR_SINGULAR, pkg.capi.ICP_ERR_EMPTY) and np.isfinite(r["T"]).all()
            while bt.run(1 << 20)[1] > 0:
                pass
            return bt.state(0), bt.get_moving()[0], bt.loop_indices()[0], bt.diag_moments(0)

    a, b = run(False), run(True)
    assert a[0]["iterations"] == b[0]["iterations"] and a[0]["status"] == b[0]["status"]
    assert bits_equal(a[0]["T"], b[0]["T"]) and bits_equal(np.asarray(a[0]["err"]), np.asarray(b[0]["err"]))
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and bits_equal(np.asarray(a[3]), np.asarray(b[3]))
