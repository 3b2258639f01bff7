"""GPU: the per-pair initial transforms of a batch (icp_batch_set_initial_transforms; Batch.set_initial_transforms,
Context.point_to_point_batch(init=...), Context.point_to_plane_batch_gated(init=...)).

The clouds are those of test_gpu_batch_gate.py (clouds.ragged_pair with a run of far outliers spliced in at point 64), carried
to a far pose G -- 40 degrees about z, shifted by (3, -2, 1) -- from where a gate of 0.03 keeps no point at pass 0 and an
ungated loop runs into a wrong minimum.  ragged_pair's picks d of a model point m satisfy m = R d + c (+ noise of 1e-3) with its
own R and c = (0.02, -0.01, 0.03), so

    T_back = G^-1                      undoes the pose: the start cloud is the gate test's cloud, up to rounding
    T_good = [Rp|tp] [R|c] G^-1        a roughly right guess: the aligning motion, off by Rp = Rz(.004) Ry(-.003) Rx(.002),
                                       tp = (.003, -.002, .0025) -- within the 0.03 gate for every non-outlier

Bounds: start clouds, indices, masks, moment vectors, err series, moved clouds and T are compared bit for bit against
ref_moments.apply_rt (the front end's arithmetic, operation by operation), against a batch without initial transforms created
from the pre-moved clouds, and against `compose` (the stated product, in Python floats).  Only the end-to-end test compares with
numpy: T and err at the project's 1e-5 (test_gpu_batch.py)."""
import ctypes as C

import numpy as np
import pytest

from batch_ref import (CASES, TOL_E, TOL_T, apply, bits_equal, compose, final, gate_case, hom, inv_rigid, keep_within, normals_for,
                       reference_loop, rel, rot, run_to_end, same_pair_bytes, step_together, t0f)
from clouds import BATCH_N, case_pair

pytestmark = pytest.mark.gpu

MD = 0.05          # the gate of the equivalence tests
MD_FINE = 0.03     # keeps nothing at pass 0 from the far pose, exactly the non-outliers from T_good


# ---- constructions -------------------------------------------------------------------------------------------------------------
G = hom(rot("z", np.deg2rad(40.0)), (3.0, -2.0, 1.0))
RAGGED = hom(rot("z", 0.04) @ rot("y", -0.03) @ rot("x", 0.05), (0.02, -0.01, 0.03))   # m = R d + c (clouds.ragged_pair)
PERTURB = hom(rot("z", 0.004) @ rot("y", -0.003) @ rot("x", 0.002), (0.003, -0.002, 0.0025))
T_BACK = inv_rigid(G)
T_GOOD = PERTURB @ RAGGED @ inv_rigid(G)


def far_case(c, dtype):
    """(A_far, M, is_out): the gate case carried to the far pose"""
    A, M, is_out = gate_case(*c, dtype=dtype)
    return apply(A, G), M, is_out


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_start_cloud_bit_for_bit(ctx, pkg, dtype):
    pairs = [case_pair(n, 17, dtype) for n in BATCH_N]
    ident = 2
    pairs[ident][0][5, 1] = -0.0
    pairs[ident][0][9, 2] = 0.0
    rng = np.random.default_rng(41)
    Ts = []
    for b in range(len(pairs)):   # a different transform per pair, with values neither precision holds exactly
        ang = rng.uniform(-np.pi, np.pi, 3)
        Ts.append(hom(rot("z", ang[0]) @ rot("y", ang[1]) @ rot("x", ang[2]) * (1.0 + 0.1 * b), rng.uniform(-5.0, 5.0, 3)))
    Ts[ident] = np.eye(4)
    Ts = np.array(Ts)
    with ctx.batch(pairs) as bt:
        bt.set_initial_transforms(Ts)
        bt.begin(max_iter=3)
        start = bt.get_moving()
        for b, (A, _) in enumerate(pairs):
            want = A if b == ident else apply(A, Ts[b])
            assert bits_equal(start[b], want), f"pair {b} (n = {A.shape[0]})"
            if b != ident:
                assert not bits_equal(start[b], A)
            T = bt.state(b)["T"]
            assert bits_equal(T, np.eye(4) if b == ident else compose(np.eye(4), t0f(Ts[b], dtype))), b
            if b != ident and dtype == np.float32:
                assert not bits_equal(T, Ts[b])   # the rounded matrix, not the caller's doubles
            st = bt.state(b)
            assert st["status"] == pkg.capi.ICP_OK and st["passes"] == 0 and st["err"].tolist() == [0.0]
        assert np.signbit(start[ident][5, 1]) and not np.signbit(start[ident][9, 2])
        assert not bt.done().any()
    with ctx.batch(pairs) as bt:   # no transforms: the bytes of the upload
        bt.set_initial_transforms(None)
        bt.begin(max_iter=3)
        for b, got in enumerate(bt.get_moving()):
            assert bits_equal(got, pairs[b][0]), b
            assert bits_equal(bt.state(b)["T"], np.eye(4))
        with pytest.raises(ValueError):
            bt.set_initial_transforms(np.eye(3))
        with pytest.raises(ValueError):
            bt.set_initial_transforms(np.zeros((len(pairs) + 1, 4, 4)))


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_is_a_plain_batch_on_the_moved_clouds(ctx, pkg, orc, dtype, plane, gated):
    cases = [far_case(c, dtype) for c in CASES]
    far = [(A, M) for A, M, _ in cases]
    moved = [(apply(A, T_BACK), M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in far] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    what = f"{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}/{'gated' if gated else 'ungated'}"
    with ctx.batch(far) as X, ctx.batch(moved) as Y:
        for bt in (X, Y):
            if plane:
                bt.set_model_normals(nrm)
            if gated:
                bt.set_max_distance(MD)
        X.set_initial_transforms(T_BACK)
        for bt in (X, Y):
            bt.begin(max_iter=12, tol=1e-6, metric=metric)
        for b, got in enumerate(X.get_moving()):
            assert bits_equal(got, moved[b][0]), (what, b)
        counts = step_together(X, Y, what)
        fx, fy = final(X), final(Y)
        for b in range(len(far)):
            same_pair_bytes(fx[b], fy[b], f"{what} pair {b}", T=compose(fy[b]["st"]["T"], t0f(T_BACK, dtype)))
            assert not bits_equal(fx[b]["st"]["T"], fy[b]["st"]["T"])
        print(f"[init equivalence] {what}: passes {[f['st']['passes'] for f in fy]}, kept per pass {counts}")
        if gated and not plane:   # on the plain batch alone: the gate is at work, the kept set changes from pass to pass
            for b in range(3):
                assert fy[b]["st"]["passes"] >= 3, (what, b, fy[b]["st"]["passes"])
                assert len(set(counts[b])) > 1, (what, b, counts[b])


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_end_to_end_from_the_far_pose(ctx, pkg, orc, dtype):
    tol = 1e-6
    cases = [far_case(c, dtype) for c in CASES]
    wants = []
    for c, (A, M, is_out) in zip(CASES, cases):   # the reference alone, before the device is looked at
        w = reference_loop(orc, apply(A, T_GOOD), M, keep_within(MD_FINE), 40, tol)
        print(f"{c}: reference keeps {w['kept']}, margin {w['margin']:.3e}, iterations {w['iterations']}, err {w['err']}")
        assert all(np.array_equal(m, ~is_out) for m in w["masks"]), c   # exactly the non-outliers, in every pass
        assert w["margin"] >= 1e-3, (c, w["margin"])
        assert reference_loop(orc, A, M, keep_within(MD_FINE), 40, tol)["kept"] == [0], c   # without the initial transform: nothing
        wants.append(w)
    pairs = [(A, M) for A, M, _ in cases]
    with ctx.batch(pairs) as bt:   # the kept count of every pass
        bt.set_max_distance(MD_FINE)
        bt.set_initial_transforms(T_GOOD)
        bt.begin(max_iter=40, tol=tol)
        counts = [[] for _ in pairs]
        while True:
            running = ~bt.done()
            if not bt.run(1)[0]:
                break
            inl = bt.get_inliers()
            for b in np.flatnonzero(running):
                counts[b].append(int(inl[b].sum()))
        for b, w in enumerate(wants):   # (the device matches once more than the reference, on the pass that stops it)
            k = len(w["kept"])
            assert len(counts[b]) >= k and counts[b][:k] == w["kept"], (CASES[b], counts[b], w["kept"])
        bt.set_initial_transforms(None)   # the same batch without them: every pair ends empty at pass 0
        for f in run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=40, tol=tol):
            assert f["st"]["status"] == pkg.capi.ICP_ERR_EMPTY and f["st"]["passes"] == 0 and not f["inl"].any()
    res = ctx.point_to_point_batch(pairs, max_iter=40, tol=tol, max_distance=MD_FINE, init=T_GOOD)
    for c, r, w, (A, M, is_out) in zip(CASES, res, wants, cases):
        want_T = w["T"] @ t0f(T_GOOD, dtype)
        print(f"{c}: iterations {r.iterations} (reference {w['iterations']}), rel T {rel(r.T, want_T):.3e}, "
              f"err {np.abs(r.err[:len(w['err'])] - w['err'][:len(r.err)]).max():.3e}")
        assert r.extra["status"] == pkg.capi.ICP_OK
        assert r.iterations == w["iterations"], (c, r.iterations, w["iterations"])
        n = min(len(r.err), len(w["err"]))
        assert n == len(w["err"]) and np.abs(r.err[:n] - w["err"][:n]).max() < TOL_E
        assert rel(r.T, want_T) < TOL_T
        assert r.extra["inliers"].dtype == bool and np.array_equal(r.extra["inliers"], ~is_out)
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_pairs_are_independent(ctx, pkg, dtype):
    cases = [far_case(c, dtype) for c in (CASES[0], CASES[1], CASES[3])]
    pairs = [(A, M) for A, M, _ in cases]
    Ts = np.array([T_BACK, T_GOOD, hom(rot("y", 0.01), (0.004, 0.0, -0.003)) @ T_BACK])

    def run(sel):
        with ctx.batch([pairs[i] for i in sel]) as bt:
            bt.set_max_distance(MD)
            bt.set_initial_transforms(Ts[sel])
            return run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)

    fwd, rev = run([0, 1, 2]), run([2, 1, 0])[::-1]
    for i in range(3):
        alone = run([i])[0]
        same_pair_bytes(alone, fwd[i], f"pair {i}, forward")
        same_pair_bytes(alone, rev[i], f"pair {i}, reversed")
        assert alone["st"]["status"] == pkg.capi.ICP_OK and alone["st"]["passes"] >= 1, i
    assert not bits_equal(fwd[0]["st"]["T"][:3], fwd[1]["st"]["T"][:3])


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_init_state_and_refusals(ctx, pkg):
    lib = pkg.load()
    cases = [far_case(c, np.float32) for c in (CASES[3], CASES[0], CASES[3])]
    pairs = [(A, M) for A, M, _ in cases]
    pd = C.POINTER(C.c_double)
    T_a = np.array([T_BACK, T_GOOD, T_GOOD])
    T_b = np.array([T_GOOD, T_BACK, hom(rot("x", 0.3), (1.0, 2.0, 3.0))])
    P2P = pkg.ICP_POINT_TO_POINT
    with ctx.batch(pairs) as bt:
        fresh = run_to_end(bt, P2P, max_iter=12)
        bt.set_initial_transforms(T_a)
        want = run_to_end(bt, P2P, max_iter=12)
        assert not bits_equal(want[0]["moved"], fresh[0]["moved"])
        bads = []
        # a NaN, an inf, bottom rows 0 0 0 2 and 1e-30 0 0 1 (and 0 0 -1 1, 0 0 0 NaN), a double that is infinite as a float
        for k, v in ((5, np.nan), (3, np.inf), (10, -np.inf), (15, 2.0), (12, 1e-30), (14, -1.0), (15, np.nan), (0, 1e39)):
            bad = T_b.copy()
            bad.reshape(3, 16)[2, k] = v
            bads.append(bad)
        for bad in bads:
            assert lib.icp_batch_set_initial_transforms(bt._h, bad.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
            assert "pair 2" in lib.icp_last_error().decode(), lib.icp_last_error().decode()
            with pytest.raises(pkg.IcpError) as e:
                bt.set_initial_transforms(bad)
            assert e.value.code == pkg.capi.ICP_ERR_INVALID
        first = T_b.copy()   # the message names the FIRST offending pair
        first[1, 0, 0], first[2, 3, 3] = np.nan, 2.0
        assert lib.icp_batch_set_initial_transforms(bt._h, first.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
        assert "pair 1" in lib.icp_last_error().decode()
        assert bt.run(1) == (0, 0)   # a refused call leaves the batch alone: its loop is still the finished one
        got = run_to_end(bt, P2P, max_iter=12)    # ... and the transforms are those set before
        for b in range(3):
            same_pair_bytes(want[b], got[b], f"after the refusals, pair {b}")
        # a set during a loop discards it
        for T in (T_b, None, T_a):
            bt.begin(max_iter=12)
            assert bt.run(1)[0] == 1
            bt.set_initial_transforms(T)
            for _ in range(2):
                with pytest.raises(pkg.IcpError) as e:
                    bt.run(1)
                assert e.value.code == pkg.capi.ICP_ERR_STATE
        # transforms do not compound: T_a, begin, run; T_b, begin -- the start cloud is apply(A, T_b)
        run_to_end(bt, P2P, max_iter=12)
        bt.set_initial_transforms(T_b)
        for _ in range(2):   # (nor over repeated begins)
            bt.begin(max_iter=12)
            for b, got_b in enumerate(bt.get_moving()):
                assert bits_equal(got_b, apply(pairs[b][0], T_b[b])), b
                assert not bits_equal(got_b, apply(apply(pairs[b][0], T_a[b]), T_b[b]))
            bt.run(2)
        # NULL restores the bytes of a fresh batch
        bt.set_initial_transforms(None)
        again = run_to_end(bt, P2P, max_iter=12)
        for b in range(3):
            same_pair_bytes(fresh[b], again[b], f"None, pair {b}")
    with ctx.batch(pairs[:1]) as bt:   # a batch that never held transforms keeps none after a refused call
        with pytest.raises(pkg.IcpError):
            bt.set_initial_transforms(np.full((4, 4), np.nan))
        same_pair_bytes(fresh[0], run_to_end(bt, P2P, max_iter=12)[0], "refused on a fresh batch")


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_overflow_ends_that_pair_only(ctx, pkg, dtype):
    cases = [far_case(c, dtype) for c in (CASES[0], CASES[3], CASES[1])]
    pairs = [(A, M) for A, M, _ in cases]
    big = np.eye(4)
    big[:3, :3] *= 3e38 if dtype == np.float32 else 1.5e308
    assert np.isfinite(big).all() and np.isfinite(big.astype(dtype)).all()
    with np.errstate(over="ignore", invalid="ignore"):
        gone = apply(pairs[1][0], big)
    assert not np.isfinite(gone).all()   # a finite transform, a finite cloud, a start cloud that is neither
    Ts = np.array([T_BACK, big, T_GOOD])
    with ctx.batch(pairs) as bt:
        bt.set_max_distance(MD)
        bt.set_initial_transforms(Ts)
        bt.begin(max_iter=12)   # (returns ICP_OK: anything else raises)
        st = bt.state(1)
        assert st["status"] == pkg.capi.ICP_ERR_INVALID and st["passes"] == 0 and st["iterations"] == 0
        assert st["err"].tolist() == [0.0] and np.array_equal(st["T"], t0f(big, dtype))
        assert bt.done().tolist() == [False, True, False]
        while bt.run(1 << 20)[1]:
            pass
        got = final(bt)
        st = bt.state(1)
        assert st["status"] == pkg.capi.ICP_ERR_INVALID and st["passes"] == 0 and st["iterations"] == 0
    with ctx.batch([pairs[0], pairs[2]]) as bt:
        bt.set_max_distance(MD)
        bt.set_initial_transforms(Ts[[0, 2]])
        want = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)
    same_pair_bytes(got[0], want[0], "pair 0 beside the overflowing pair")
    same_pair_bytes(got[2], want[1], "pair 2 beside the overflowing pair")
    assert want[0]["st"]["status"] == pkg.capi.ICP_OK and want[0]["st"]["passes"] >= 1


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_init_coarse_to_fine_on_one_batch(ctx, pkg, dtype):
    """gated at 0.05 from T_back to the end, then from that result gated at 0.03, without another upload: the bytes of a plain
    batch created from the clouds moved by the first result, for all four pairs; the three large pairs end with exactly their
    non-outliers.  (The 63-point pair on its 17-point model keeps 7 points at 0.05 from T_back and settles on those -- in the
    numpy loop as well: reference_loop keeps [7, 7] -- so its final mask is not the non-outliers, whatever the start.)"""
    cases = [far_case(c, dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    with ctx.batch(pairs) as bt:
        bt.set_max_distance(MD)
        bt.set_initial_transforms(T_BACK)
        coarse = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=40)
        T1 = np.array([f["st"]["T"] for f in coarse])
        bt.set_initial_transforms(T1)
        bt.set_max_distance(MD_FINE)
        fine = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=40)
    with ctx.batch([(apply(A, T1[b]), M) for b, (A, M) in enumerate(pairs)]) as bt:
        bt.set_max_distance(MD_FINE)
        plain = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=40)
    for b, (_, _, is_out) in enumerate(cases):
        same_pair_bytes(fine[b], plain[b], f"pair {b}", T=compose(plain[b]["st"]["T"], t0f(T1[b], dtype)))
        assert fine[b]["st"]["status"] == pkg.capi.ICP_OK
        if b < 3:
            assert np.array_equal(fine[b]["linl"], ~is_out) and np.array_equal(fine[b]["inl"], ~is_out), b
