"""GPU: the per-pair reciprocal (mutual nearest neighbour) matches of a batch (icp_batch_set_reciprocal, icp_diag_batch_reverse;
Batch.set_reciprocal, Batch.diag_reverse, Context.register_batch(reciprocal=...)).

A reciprocal pair keeps, in every matching pass, the matches i -> idx[i] with rev[idx[i]] == i, rev[j] being the lowest i that
minimises dist2(p_i, q_j) on the cloud the pass matched on: the deferred route with the reverse search -- matching without a
decision, nn_match_batch_rev, [batch_trim_select,] batch_trim_moments<MUTUAL>.

    1  the reverse search alone, at its granules: the quarters of the MOVING cloud are what nn_match_batch_rev tiles, so n runs
       over batch_ref.KNN_M (three empty quarters, ragged quarters, one sub-tile per quarter and a second) and 1, while m cycles
       through a single model point and a ragged, an exact and a one-over model work item; and 40 coincident points against
       themselves: only the lowest of them may be kept
    2  ties: integer clouds with tied minima in both directions (test_batch_mutual_ref.py: another reverse tie order changes the
       mask at 52 points)
    3  every pass exactly (the structure of test_gpu_batch_trim.test_trim_every_pass_exactly): mutual alone, with a gate, with a
       trim, with both
    4  end to end against a numpy loop, through Context.register_batch
    5  bits: off means off, a pair with flag 0 in a reciprocal batch, independence of the other pairs, refusals and state,
       initial transforms

The clouds of 3 - 5 are those of test_gpu_batch_gate.py (batch_ref.gate_case); what the rule keeps on them is pinned on the CPU in
test_batch_mutual_ref.py.  Every condition on the clouds is asserted on the reference alone before the device is consulted.

Bounds: rev, idx, every mask, tau and moved cloud bit for bit -- both searches compare the same numbers (dist2 squares its
differences), so no decision of the mutual rule is a rounding; the sums at ref_moments.tolerance (derived there); T and err of the
end-to-end run at the project's 1e-5 (test_gpu_batch.py).  The end-to-end masks are not compared: the numpy loop moves its cloud
with its own solve, the reference's closest reverse decision has a relative gap of 1.7e-5 in fp32 (the 1025 x 513 case), and a
1e-7 difference in a moved fp32 coordinate can cross that; test 3 is where masks are exact."""
import ctypes as C

import numpy as np
import pytest

import ref_moments as rm
from batch_mutual_ref import combined_mask, keep_mutual, mutual_loop, mutual_mask, tie_clouds
from batch_ref import (CASES, KNN_M, assert_same_run, bits_equal, check_front_end, check_sums, compose, final, gate_case, hom, knn_models,
                       normals_for, rank, rel, rot, run_to_end, same_pair_bytes, step_together, tau_bits_equal)

pytestmark = pytest.mark.gpu

MD = 0.05
RHO = 0.5
PASSES = 4
KEPT_PASS0 = {"mutual": [148, 122, 426, 17], "mutual+gate": [21, 16, 55, 2], "mutual+trim": [102, 91, 246, 9]}
REV_N = (1,) + KNN_M
REV_M = (1, 63, 64, 65, 130)


# 1 ------------------------------------------------------------------------------------------------------------------------
def reverse_pairs(dtype):
    """one pair per n of REV_N: the moving clouds are batch_ref.knn_models' (their last, 300 points of which 40 coincide, is
    matched against itself), the models standard-normal clouds of REV_M points in turn"""
    clouds = knn_models(dtype)
    Z = clouds[-1]
    movers = [np.random.default_rng(77).standard_normal((1, 3)).astype(dtype)] + clouds[:-1]
    assert tuple(A.shape[0] for A in movers) == REV_N
    pairs = []
    for k, A in enumerate(movers):
        m = REV_M[k % len(REV_M)]
        pairs.append((A, np.random.default_rng(500 + k).standard_normal((m, 3)).astype(dtype)))
    pairs.append((Z, Z.copy()))
    return pairs


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reverse_search_at_its_granules(ctx, pkg, orc, dtype):
    pairs = reverse_pairs(dtype)
    want = [mutual_mask(orc, A, M) for A, M in pairs]
    # the reference alone: every model size of REV_M meets several quarter shapes, and the coincident points keep their lowest
    assert {M.shape[0] for _, M in pairs[:-1]} == set(REV_M)
    idx, rev, mask = want[-1]
    assert np.array_equal(idx[100:140], np.full(40, 100)) and rev[100] == 100 and mask[100] and not mask[101:140].any()
    assert mask.sum() == 261
    assert all(m.any() for _, _, m in want)
    with ctx.batch(pairs) as bt:
        bt.set_reciprocal(True)
        bt.begin(max_iter=2, tol=0.0, fixed_iterations=True)
        assert bt.run(1)[0] == 1
        got_rev, got_idx, inl = bt.diag_reverse(), bt.get_indices(), bt.get_inliers()
        for b, ((A, M), (idx, rev, mask)) in enumerate(zip(pairs, want)):
            what = f"pair {b}: n {A.shape[0]} m {M.shape[0]}"
            assert got_rev[b].dtype == np.int32 and got_rev[b].shape == (M.shape[0],), what
            assert np.array_equal(got_rev[b], rev), f"{what}: rev differs at {np.flatnonzero(got_rev[b] != rev)[:8]}"
            assert np.array_equal(got_idx[b], idx), what
            assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
            assert bt.diag_moments(b)[rm.CNT] == float(mask.sum()), what


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_ties_go_to_the_lowest_index_both_ways(ctx, pkg, orc, dtype):
    A, M = tie_clouds(dtype)
    idx, rev, mask = mutual_mask(orc, A, M)
    assert mask.sum() == 42   # (what makes these clouds a test of the tie order: test_batch_mutual_ref.py)
    with ctx.batch([(A, M)]) as bt:
        bt.set_reciprocal([True])
        bt.begin(max_iter=2, tol=0.0, fixed_iterations=True)
        assert bt.run(1)[0] == 1
        assert np.array_equal(bt.get_indices()[0], idx)
        assert np.array_equal(bt.diag_reverse()[0], rev)
        assert np.array_equal(bt.get_inliers()[0], mask)
        assert bt.diag_moments(0)[rm.CNT] == 42.0


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mutual", "mutual+gate", "mutual+trim", "mutual+gate+trim"])
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_every_pass_exactly(ctx, pkg, orc, dtype, plane, mode):
    gated, trimmed = "gate" in mode, "trim" in mode
    md, rho = (MD if gated else None), (RHO if trimmed else None)
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    Ks = [rank(RHO, A.shape[0]) for A, _ in pairs]
    # the reference alone: what pass 0 keeps (the fp64 clouds are the fp32 ones, widened: the same decisions)
    for b, (A, M) in enumerate(pairs):
        idx0, rev0, _ = mutual_mask(orc, A, M)
        m0 = combined_mask(A, M, idx0, rev0, md, rho)[0]
        assert m0.any()
        if mode in KEPT_PASS0:
            assert m0.sum() == KEPT_PASS0[mode][b], (mode, b, int(m0.sum()))
        else:
            assert m0.sum() <= min(KEPT_PASS0["mutual+gate"][b], KEPT_PASS0["mutual+trim"][b])
    checked, worst, kept_log = [0] * len(pairs), 0.0, [[] for _ in pairs]
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        if gated:
            bt.set_max_distance(MD)
        if trimmed:
            bt.set_trim(RHO)
        bt.set_reciprocal(True)
        bt.begin(max_iter=PASSES, tol=0.0, fixed_iterations=True, metric=metric)
        prev = [None] * len(pairs)
        for k in range(PASSES + 1):
            running = ~bt.done()
            took, _ = bt.run(1)
            assert took == (1 if running.any() else 0)
            if not took:
                break
            moving, idx, inl, revs = bt.get_moving(), bt.get_indices(), bt.get_inliers(), bt.diag_reverse()
            for b in np.flatnonzero(running):
                P, M = moving[b], pairs[b][1]
                what = f"{mode} pair {b} {CASES[b]} pass {k}"
                mom = bt.diag_moments(b)
                st = bt.state(b)
                check_front_end(pkg, plane, P, M, mom, st["err"][k], prev[b], what)
                if k == PASSES:   # the error-only pass matches nothing: rev stays that of the last matching pass
                    assert np.array_equal(revs[b], prev[b]["rev"]), what
                    checked[b] += 1
                    continue
                # the reference, from the cloud the pass matched on (bit for bit the device's: check_front_end)
                want_idx, want_rev, _ = mutual_mask(orc, P, M)
                mask, d, tau_want = combined_mask(P, M, want_idx, want_rev, md, rho)
                kept_log[b].append(int(mask.sum()))
                if k == 0 and mode in KEPT_PASS0:
                    assert mask.sum() == KEPT_PASS0[mode][b], what
                # the device
                assert np.array_equal(idx[b], want_idx), what
                assert np.array_equal(revs[b], want_rev), f"{what}: rev differs at {np.flatnonzero(revs[b] != want_rev)[:8]}"
                tau, kk = bt.diag_trim(b)
                if trimmed:
                    assert kk == Ks[b] and tau_bits_equal(tau, tau_want), f"{what}: tau {tau!r}, reference {float(tau_want)!r}"
                else:
                    assert (tau, kk) == (np.inf, P.shape[0]), what
                assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}"
                worst = max(worst, check_sums(plane, P, M, nrm[b] if plane else None, want_idx, mask, mom, what))
                prev[b] = dict(P=P, idx=want_idx, mask=mask, mom=mom, rev=want_rev)
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            assert checked[b] == PASSES + 1 or bt.state(b)["status"] != pkg.capi.ICP_OK, (b, checked[b])
        if not gated:   # (the mutual rule and the trim always keep a point; under the gate a pair may end early with its status)
            assert min(checked[:3]) == PASSES + 1
        assert max(checked) == PASSES + 1
    print(f"[reciprocal moments] {mode}/{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}: kept {kept_log}, "
          f"largest |device - exact| / tol = {worst:.4f}")


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_end_to_end(ctx, pkg, orc, dtype):
    tol = 1e-6
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    wants = [mutual_loop(orc, A, M, keep_mutual(orc), 40, tol) for A, M, _ in cases]
    for c, w, (A, M, is_out) in zip(CASES, wants, cases):   # the reference alone
        print(f"{c}: reference keeps {w['kept']}, iterations {w['iterations']}, final RMS {w['err'][-1]:.3e}")
        assert not any((m & is_out).any() for m in w["masks"])
        assert w["err"][-1] < 2e-3
    assert [w["iterations"] for w in wants] == [4, 3, 5, 4]
    pairs = [(A, M) for A, M, _ in cases]
    res = ctx.register_batch(pairs, max_iter=40, tol=tol, reciprocal=True)
    for c, r, w, (A, M, is_out) in zip(CASES, res, wants, cases):
        assert r.extra["status"] == pkg.capi.ICP_OK
        print(f"{c}: iterations {r.iterations} (reference {w['iterations']}), rel T {rel(r.T, w['T']):.3e}, err {r.err}")
        assert_same_run(r.iterations, r.err, r.T, w, tol, dtype == np.float32)   # err at TOL_E, T at TOL_T
        inl = r.extra["inliers"]
        assert inl.dtype == bool and inl.any() and not (inl & is_out).any()
        assert r.extra["fitness"] == inl.sum() / A.shape[0]
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_off_means_off(ctx, pkg, orc, dtype, plane):
    """(a) set_reciprocal(None) and all flags 0 give, step by step, the bytes of a batch that was never told"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    for off in (None, False, [0, 0, 0, 0], "after"):
        with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
            for bt in (X, Y):
                if plane:
                    bt.set_model_normals(nrm)
            if off == "after":   # switched on, run, and switched off again
                Y.set_reciprocal(True)
                assert not all(f["linl"].all() for f in run_to_end(Y, metric, max_iter=12))
                Y.set_reciprocal(None)
            else:
                Y.set_reciprocal(off)
            for bt in (X, Y):
                bt.begin(max_iter=12, tol=1e-6, metric=metric)
            counts = step_together(X, Y, f"off = {off!r}")
            for b, (A, _) in enumerate(pairs):
                assert counts[b] and set(counts[b]) == {A.shape[0]}, (off, b)
                same_pair_bytes(final(X)[b], final(Y)[b], f"off = {off!r}, pair {b}")
            assert all((r == -1).all() for r in Y.diag_reverse())


@pytest.mark.parametrize("gated", [False, True], ids=["no gate", "gate"])
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_flag_zero_pair_keeps_its_bits(ctx, pkg, orc, dtype, plane, gated):
    """(b) with flags 1, 0, 1, 0 pairs 1 and 3 have, after every step and to the end, the bytes they have in a plain batch: the
    deferred route adds their rows in the fused pass's order, and their rev rows stay -1"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            if plane:
                bt.set_model_normals(nrm)
            if gated:
                bt.set_max_distance(MD)
        X.set_reciprocal([1, 0, 1, 0])
        for bt in (X, Y):
            bt.begin(max_iter=12, tol=1e-6, metric=metric)
        step = 0
        while True:
            kx, ky = X.run(1), Y.run(1)   # (the reciprocal pairs may end on another pass than their plain twins: either batch may idle)
            if not kx[0] and not ky[0]:
                break
            fx, fy, revs = final(X), final(Y), X.diag_reverse()
            for b in (1, 3):
                what = f"step {step} pair {b}"
                same_pair_bytes(fx[b], fy[b], what)
                assert bits_equal(X.diag_moments(b), Y.diag_moments(b)), what
                assert (revs[b] == -1).all(), what
            for b in (0, 2):
                assert revs[b].min() >= 0 and revs[b].max() < pairs[b][0].shape[0], (step, b)
                if step == 0:
                    assert not bits_equal(fx[b]["inl"], fy[b]["inl"]), (step, b)   # (reciprocity does something)
            step += 1
            assert step <= 14
        assert step >= 3 and X.done().all() and Y.done().all()


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_pairs_are_independent(ctx, pkg, orc, dtype, plane):
    """(c) a reciprocal pair's bytes are those of that pair in a batch of its own, in either order of the pairs, whatever the
    others' flags, shares and gates; the one-call entry runs the same thing"""
    order = [0, 1, 2, 3, 0, 1]
    flags = np.array([1, 1, 0, 1, 1, 0], dtype=bool)
    rho = np.array([1.0, RHO, RHO, 1.0, 0.7, 1.0])
    md = np.array([np.inf, np.inf, MD, MD, MD, np.inf])
    cases = [gate_case(*CASES[c], dtype=dtype) for c in order]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT

    def run(sel):
        with ctx.batch([pairs[i] for i in sel]) as bt:
            if plane:
                bt.set_model_normals([nrm[i] for i in sel])
            bt.set_max_distance(md[sel])
            bt.set_trim(rho[sel])
            bt.set_reciprocal(flags[sel])
            return run_to_end(bt, metric, max_iter=12)

    everything = list(range(len(pairs)))
    fwd, rev = run(everything), run(everything[::-1])[::-1]
    for i in everything:
        alone = run([i])[0]
        same_pair_bytes(alone, fwd[i], f"pair {i}, forward")
        same_pair_bytes(alone, rev[i], f"pair {i}, reversed")
    res = ctx.register_batch(pairs, metric=metric, normals=nrm, max_iter=12, max_distance=md, trim=rho, reciprocal=flags)
    for i, r in enumerate(res):
        assert r.extra["status"] == fwd[i]["st"]["status"] and r.iterations == fwd[i]["st"]["iterations"] and r.passes == fwd[i]["st"]["passes"]
        assert bits_equal(r.T, fwd[i]["st"]["T"]) and bits_equal(r.err, fwd[i]["st"]["err"]) and bits_equal(r.idx, fwd[i]["idx"])
        assert bits_equal(r.moved, fwd[i]["moved"]) and bits_equal(r.extra["inliers"], fwd[i]["linl"])
    assert not bits_equal(fwd[0]["st"]["T"], fwd[4]["st"]["T"])   # the same clouds, a share and a gate beside the flag


def test_reciprocal_register_batch_defaults(ctx, pkg, orc):
    """the one-call entry without options is the plain batch: max_iter None means 40 (point-to-point) and 50 (point-to-plane)"""
    cases = [gate_case(*c) for c in CASES[:2]]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs]
    for got, want in zip(ctx.register_batch(pairs), ctx.point_to_point_batch(pairs)):
        assert bits_equal(got.T, want.T) and bits_equal(got.err, want.err) and bits_equal(got.idx, want.idx) and bits_equal(got.moved, want.moved)
        assert got.extra["inliers"].all() and got.extra["fitness"] == 1.0 and got.extra["status"] == want.extra["status"]
    for got, want in zip(ctx.register_batch(pairs, metric=pkg.ICP_POINT_TO_PLANE, normals=nrm), ctx.point_to_plane_batch(pairs, normals=nrm)):
        assert bits_equal(got.T, want.T) and bits_equal(got.err, want.err) and bits_equal(got.idx, want.idx) and bits_equal(got.moved, want.moved)


def test_reciprocal_refusals_and_state(ctx, pkg, orc):
    """(d) a set during a loop discards it; diag_reverse before the first step is ICP_ERR_STATE; a pair with flag 0, and a pair
    that has not matched since begin, get -1 rows; a wrong number of flags is refused in Python and leaves the batch alone"""
    lib = pkg.load()
    cases = [gate_case(*c) for c in CASES[:3]]
    pairs = [(A, M) for A, M, _ in cases]
    P2P = pkg.ICP_POINT_TO_POINT
    total_m = sum(M.shape[0] for _, M in pairs)
    buf = np.full(total_m, 7, dtype=np.int32)
    p32 = C.POINTER(C.c_int32)
    with ctx.batch(pairs) as bt:
        assert lib.icp_diag_batch_reverse(bt._h, buf.ctypes.data_as(p32)) == pkg.capi.ICP_ERR_STATE   # no loop
        assert lib.icp_diag_batch_reverse(bt._h, None) == pkg.capi.ICP_ERR_INVALID
        bt.set_reciprocal([1, 0, 1])
        with pytest.raises(pkg.IcpError) as e:   # run before begin after a set
            bt.run(1)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        bt.begin(max_iter=12)
        assert lib.icp_diag_batch_reverse(bt._h, buf.ctypes.data_as(p32)) == pkg.capi.ICP_ERR_STATE   # no step yet
        assert (buf == 7).all()
        want = run_to_end(bt, P2P, max_iter=12)
        revs = bt.diag_reverse()
        assert (revs[1] == -1).all() and revs[0].min() >= 0 and revs[2].min() >= 0
        assert not want[0]["linl"].all() and want[1]["linl"].all() and not want[2]["linl"].all()
        with pytest.raises(ValueError):
            bt.set_reciprocal([1, 0])
        assert bt.run(1) == (0, 0)   # a refused call leaves the batch alone: its loop is still the finished one
        got = run_to_end(bt, P2P, max_iter=12)   # ... and the flags are those set before
        for b in range(3):
            same_pair_bytes(want[b], got[b], f"pair {b}")
        # a set during a loop discards it
        for v in ([1, 0, 1], None, False, True):
            bt.begin(max_iter=12)
            assert bt.run(1)[0] == 1
            bt.set_reciprocal(v)
            with pytest.raises(pkg.IcpError) as e:
                bt.run(1)
            assert e.value.code == pkg.capi.ICP_ERR_STATE
            with pytest.raises(pkg.IcpError) as e:
                bt.diag_reverse()
            assert e.value.code == pkg.capi.ICP_ERR_STATE
        # the last set switched every pair on: the rows of the loop before are not shown for a pair that has not matched yet
        bt.begin(max_iter=12)
        assert bt.run(1)[0] == 1
        assert all(r.min() >= 0 for r in bt.diag_reverse())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reciprocal_with_initial_transforms(ctx, pkg, orc, dtype):
    """(f) reciprocity on a batch that holds initial transforms is reciprocity on a batch created from the pre-moved clouds: both
    searches run on the start cloud"""
    G = hom(rot("z", np.deg2rad(40.0)), (3.0, -2.0, 1.0))
    T_back = hom(G[:3, :3].T, -G[:3, :3].T @ G[:3, 3])
    T0F = np.eye(4)
    T0F[:3, :] = T_back[:3, :].astype(dtype).astype(np.float64)
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    far = [(rm.apply_rt(A, G[:3, :3], G[:3, 3]), M) for A, M, _ in cases]
    moved = [(rm.apply_rt(A, T_back[:3, :3], T_back[:3, 3]), M) for A, M in far]
    with ctx.batch(far) as X, ctx.batch(moved) as Y:
        X.set_initial_transforms(T_back)
        for bt in (X, Y):
            bt.set_reciprocal(True)
        fx, fy = run_to_end(X, pkg.ICP_POINT_TO_POINT, max_iter=12), run_to_end(Y, pkg.ICP_POINT_TO_POINT, max_iter=12)
        rx, ry = X.diag_reverse(), Y.diag_reverse()
        for b in range(len(far)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}", T=compose(fy[b]["st"]["T"], T0F))
            assert np.array_equal(rx[b], ry[b]) and rx[b].min() >= 0
            assert fy[b]["st"]["passes"] >= 1 and not fy[b]["linl"].all()
