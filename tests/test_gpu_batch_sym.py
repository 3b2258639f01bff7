"""GPU: the symmetric metric of a batch (icp_batch_begin with ICP_SYMMETRIC on the point normals of icp_batch_set_point_normals /
icp_batch_estimate_point_normals; Batch.*, Context.register_batch_symmetric).

    1  one step and a second on batch_ref.CASES and on moving clouds of 63, 64, 65 points and of one (a ragged work item, a full
       one, one point over, a single lane): idx and masks are those of a point-to-point batch on the device's own moved cloud, byte
       for byte, with a gate, a trim, reciprocity and an initial transform; diag_rotation is the rotation of the composed motions
       and the 3 x 3 of the reported T; the front end moved the cloud by the host solve (icp_solve_symmetric) of the previous
       vector; every slot of the vector agrees with the exact sum (math.fsum) of the numpy terms within ref_moments.tolerance -- a
       derived bound, 2 (n + 16) u sum |term|.  The point normals are random unit vectors (so about half the matches take the
       difference of the two normals), a few of them exact zeros
    2  a pair's vectors and finished run are the same bytes alone, first, last and in the middle of a batch
    3  the loop against batch_sym_ref.reference_loop on the scene at a quarter of its size and on a CASES pair; the scene is
       registered where the plane metric is still degrees away; register_batch_symmetric with device normals
    4  refusals and state
    5  a batch that holds point normals runs the four other metrics with the bytes of one that holds none"""
import ctypes as C
import types

import numpy as np
import pytest

import batch_gicp_ref as gr
import batch_sym_ref as sr
from batch_ref import (CASES, assert_same_run, bits_equal, check_front_end, compose, final, gate_case, hom, keep_closest, keep_within, rel,
                       rot, run_to_end, same_pair_bytes, t0f)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
MD, RHO = 0.05, 0.5


def unit_normals(seed, n, zero_every=0):
    """(n, 3) float64 random unit vectors; zero_every > 0: every zero_every-th is exactly (0, 0, 0), the stored fallback"""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    if zero_every:
        v[zero_every - 1::zero_every] = 0.0
    return np.ascontiguousarray(v)


# 1 ------------------------------------------------------------------------------------------------------------------------
def step_pairs(dtype):
    """batch_ref.CASES, moving clouds of 63, 64 and 65 points, and one of a single point (its loop may end after its first pass: one
    match cannot fix six unknowns)"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES] + [gate_case(60, 150, 3, dtype), gate_case(61, 90, 3, dtype), gate_case(62, 120, 3, dtype)]
    pairs = [(A, M) for A, M, _ in cases]
    assert [A.shape[0] for A, _ in pairs[-3:]] == [63, 64, 65]
    rng = np.random.default_rng(41)
    pairs.append((rng.standard_normal((1, 3)).astype(dtype) * 0.1, rng.standard_normal((40, 3)).astype(dtype)))
    return pairs


def set_options(bt, mode, count, T0=None):
    if "gate" in mode:
        bt.set_max_distance([MD] * (count - 1) + [np.inf])
    if "trim" in mode:
        bt.set_trim([RHO] * (count - 1) + [1.0])
    if "mutual" in mode:
        bt.set_reciprocal([True] * (count - 1) + [False])
    if T0 is not None:
        bt.set_initial_transforms(T0)


@pytest.mark.parametrize("mode", ["plain", "gate", "trim", "mutual", "init", "gate+trim+mutual+init"])
@DTYPES
def test_steps_decide_as_point_to_point_and_sum_the_terms(ctx, pkg, dtype, mode):
    pairs = step_pairs(dtype)
    count = len(pairs)
    Np = [unit_normals(500 + b, A.shape[0], 17) for b, (A, _) in enumerate(pairs)]
    Nq = [unit_normals(600 + b, M.shape[0], 13) for b, (_, M) in enumerate(pairs)]
    # (the pair of one point: parallel axis normals, so that v2 == v3 == 0 and its one match's system has an exact zero pivot)
    Np[-1], Nq[-1] = np.array([[0.0, 0.0, 1.0]]), np.tile([0.0, 0.0, 1.0], (pairs[-1][1].shape[0], 1))
    sym_solve = types.SimpleNamespace(solve_point_to_plane=pkg.solve_symmetric)   # check_front_end's host solve of a plane vector
    T0 = None
    if "init" in mode:
        T0 = np.stack([hom(rot("z", 0.004 * (b + 1)) @ rot("x", -0.003 * b), np.array([0.002 * b, -0.003, 0.001])) for b in range(count)])
        T0[1] = T0[count - 1] = np.eye(4)
    worst, flips, zeros = 0.0, 0, 0
    with ctx.batch(pairs) as bt:
        bt.set_point_normals(Np, Nq)
        set_options(bt, mode, count, T0)
        bt.begin(max_iter=3, tol=0.0, fixed_iterations=True, metric=pkg.ICP_SYMMETRIC)
        prev = [None] * count
        for step in (1, 2):
            live = np.flatnonzero(~bt.done())
            assert step == 2 or live.size == count
            for b in set(range(count - 1)) - set(live.tolist()):   # a pair ends early only where its pass kept fewer matches than unknowns
                assert prev[b]["mask"].sum() < 6 and bt.state(b)["status"] in (pkg.capi.ICP_ERR_SINGULAR, pkg.capi.ICP_ERR_EMPTY), (mode, step, b)
            assert {0, 1, 2} <= set(live.tolist()), (mode, step)   # (the larger clouds keep enough under every option)
            assert bt.run(1)[0] == 1, (mode, step)
            moved, idx, inl = bt.get_moving(), bt.get_indices(), bt.get_inliers()
            # the decision is the point-to-point batch's, on the cloud the device matched on
            with ctx.batch([(moved[b], pairs[b][1]) for b in range(count)]) as pp:
                set_options(pp, mode.replace("init", ""), count)
                pp.begin(max_iter=3, tol=0.0, fixed_iterations=True)
                assert pp.run(1)[0] == 1
                pidx, pinl = pp.get_indices(), pp.get_inliers()
            for b in live:
                A, M = pairs[b]
                what = f"{mode} step {step} pair {b}"
                assert bits_equal(idx[b], pidx[b]) and bits_equal(inl[b], pinl[b]), what
                st, mom, R = bt.state(b), bt.diag_moments(b), bt.diag_rotation(b)
                copied = T0 is None or b in (1, count - 1)   # (an identity is not composed: the pair's T is the loop's)
                Tinit = np.eye(4) if copied else t0f(T0[b], dtype)
                assert bits_equal(R, np.ascontiguousarray(st["T"][:3, :3])), what
                if step == 1:
                    assert bits_equal(R, np.ascontiguousarray(Tinit[:3, :3])), what
                else:
                    Rs, ts = pkg.solve_symmetric(prev[b]["mom"])[:2]
                    Tk = hom(Rs.astype(dtype).astype(np.float64), ts.astype(dtype).astype(np.float64))
                    Tl = compose(Tk, np.eye(4))
                    want_T = Tl if copied else compose(Tl, Tinit)
                    assert bits_equal(R, np.ascontiguousarray(want_T[:3, :3])), what
                check_front_end(sym_solve, True, moved[b], M, mom, st["err"][step - 1] if step > 1 else 0.0, prev[b], what)
                worst = max(worst, sr.check_sums(moved[b], M, Np[b], Nq[b], idx[b], inl[b], R, mom, what))
                n, _, _ = sr.residual(moved[b], M, Np[b], Nq[b], idx[b], R)
                s = (np.asarray(Np[b]) @ R.T * Nq[b][idx[b]]).sum(axis=1)
                flips += int((s[inl[b]] < 0).sum())
                zeros += int(((n[0] == 0) & (n[1] == 0) & (n[2] == 0))[inl[b]].sum())
                prev[b] = dict(P=moved[b], idx=idx[b], mask=inl[b], mom=mom)
            if "gate" in mode or "trim" in mode or "mutual" in mode:
                assert any((~inl[b]).any() for b in range(count - 1)), (mode, step)   # the options reject something
    assert flips > 20   # the sign rule decided both ways
    print(f"[sym steps] {mode}/{np.dtype(dtype).name}: largest |device - exact| / tol = {worst:.4f}; {flips} kept matches took the "
          f"difference of the normals, {zeros} had n == 0")


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_pairs_bytes_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X, Y, Z = ((A, M) for A, M, _ in (gate_case(*c, dtype=dtype) for c in (CASES[0], CASES[3], CASES[1])))
    nrm = {id(p): (unit_normals(70 + k, p[0].shape[0], 17), unit_normals(80 + k, p[1].shape[0], 13)) for k, p in enumerate((X, Y, Z))}

    def run(pairs):
        with ctx.batch(pairs) as bt:
            bt.set_point_normals([nrm[id(p)][0] for p in pairs], [nrm[id(p)][1] for p in pairs])
            bt.set_max_distance(0.3)
            bt.set_trim(0.9)
            bt.set_reciprocal([id(p) == id(X) for p in pairs])
            bt.begin(max_iter=6, tol=1e-7, metric=pkg.ICP_SYMMETRIC)
            assert bt.run(1)[0] == 1
            first = [bt.diag_moments(b).copy() for b in range(bt.count)]
            while bt.run(1 << 20)[1]:
                pass
            return first, final(bt)

    alone, first, last, mid = run([X]), run([X, Y, Z]), run([Z, Y, X]), run([Y, X, Z])
    for other, k, what in ((first, 0, "first"), (last, 2, "last"), (mid, 1, "in the middle")):
        assert bits_equal(alone[0][0], other[0][k]), what
        same_pair_bytes(alone[1][0], other[1][k], what)
    assert bits_equal(first[0][2], last[0][0]) and bits_equal(first[0][1], last[0][1])
    same_pair_bytes(first[1][2], last[1][0], "Z")
    assert alone[1][0]["st"]["passes"] >= 2


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_loop_against_the_reference_loop(ctx, pkg, orc, dtype):
    f32 = dtype == np.float32
    sc = sr.scene(dtype, model=20, moving=17)
    A2, M2, _ = gate_case(*CASES[0], dtype=dtype)
    Nq2 = unit_normals(91, M2.shape[0])
    Np2 = np.ascontiguousarray(Nq2[orc.nn(A2, M2)])           # the normal of the model point each moving point starts nearest to
    pairs = [(sc["A"], sc["M"]), (A2, M2)]
    max_iter, tol = 12, 1e-6
    with ctx.batch(pairs) as bt:
        bt.set_point_normals([sc["Np"], Np2], [sc["Nq"], Nq2])
        bt.set_max_distance([np.inf, 0.3])
        res = run_to_end(bt, pkg.ICP_SYMMETRIC, max_iter, tol)
        bt.set_model_normals([sc["Nq"].astype(dtype), Nq2.astype(dtype)])
        plane = run_to_end(bt, pkg.ICP_POINT_TO_PLANE, 2, 0.0, fixed=True)
        two = run_to_end(bt, pkg.ICP_SYMMETRIC, 2, 0.0, fixed=True)
    wants = [sr.reference_loop(orc, sc["A"], sc["M"], sc["Np"], sc["Nq"], max_iter, tol, truth=sc["R"]),
             sr.reference_loop(orc, A2, M2, Np2, Nq2, max_iter, tol, keep=keep_within(0.3))]
    for b, want in enumerate(wants):
        st = res[b]["st"]
        n = min(len(st["err"]), len(want["err"]))
        print(f"[sym loop] {np.dtype(dtype).name} pair {b}: iterations {st['iterations']} / {want['iterations']}, passes {st['passes']}, "
              f"rel T {rel(st['T'], want['T']):.3e}, max |dE| {np.abs(st['err'][:n] - want['err'][:n]).max():.3e}")
        assert st["status"] == pkg.capi.ICP_OK and not want["empty"] and not want["singular"], b
        assert_same_run(st["iterations"], st["err"], st["T"], want, tol, fp32=f32)
        if st["iterations"] == want["iterations"]:
            assert st["passes"] == len(want["err"]) - 1, b
    # the scene is registered: 40 degrees about z and SHIFT; after two passes the plane metric is still degrees away
    end = sr.angle_deg(res[0]["st"]["T"][:3, :3], sc["R"])
    a_sym, a_plane = sr.angle_deg(two[0]["st"]["T"][:3, :3], sc["R"]), sr.angle_deg(plane[0]["st"]["T"][:3, :3], sc["R"])
    print(f"[sym loop] {np.dtype(dtype).name} scene: rotation error {end:.3e} degrees at the end (numpy {wants[0]['ang'][-1]:.3e}); after two passes "
          f"symmetric {a_sym:.4g}, plane {a_plane:.4g}")
    assert abs(end - wants[0]["ang"][-1]) < 1e-3 and np.abs(res[0]["st"]["T"][:3, 3] - sr.SHIFT).max() < 0.02
    assert two[0]["st"]["passes"] == plane[0]["st"]["passes"] == 2 and a_sym < a_plane


def test_register_batch_symmetric(ctx, pkg, orc):
    sc = sr.scene(np.float32, deg=20.0, model=20, moving=17)
    pairs = [(sc["A"], sc["M"])]
    res = ctx.register_batch_symmetric(pairs, normals=([sc["Np"]], [sc["Nq"]]), max_iter=12, tol=1e-6)
    want = sr.reference_loop(orc, sc["A"], sc["M"], sc["Np"], sc["Nq"], 12, 1e-6)
    assert res[0].extra["status"] == pkg.capi.ICP_OK and res[0].extra["fitness"] == 1.0
    assert_same_run(res[0].iterations, res[0].err, res[0].T, want, 1e-6, fp32=True)
    # device normals: covariances from k neighbours, the eigenvector of the smallest eigenvalue, unoriented -- the sign rule's case
    with ctx.batch(pairs) as bt:
        bt.estimate_covariances(10)
        Np, Nq = bt.estimate_point_normals("none", want=True)
    raw = ctx.register_batch_symmetric(pairs, k=10, orient="none", max_iter=12, tol=1e-6, trim=0.95)
    want = sr.reference_loop(orc, sc["A"], sc["M"], Np[0], Nq[0], 12, 1e-6, keep=keep_closest(0.95))
    assert raw[0].extra["status"] == pkg.capi.ICP_OK
    assert_same_run(raw[0].iterations, raw[0].err, raw[0].T, want, 1e-6, fp32=True)
    res = ctx.register_batch_symmetric(pairs, k=10, max_iter=12, tol=1e-6, trim=0.95)
    assert res[0].extra["status"] == pkg.capi.ICP_OK and rel(res[0].T, raw[0].T) < 1e-4   # the orientation of the normals does not matter
    with pytest.raises(TypeError):
        ctx.register_batch_symmetric(pairs, kernel="huber")


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(ctx, pkg):
    lib = pkg.load()
    INV, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    SYM = pkg.ICP_SYMMETRIC
    pi = C.POINTER(C.c_int)
    pairs = [(gr.blob(1, 70, np.float32), gr.blob(2, 90, np.float32)), (gr.blob(3, 66, np.float32), gr.blob(4, 77, np.float32))]
    Np, Nq = [unit_normals(1, 70), unit_normals(2, 66)], [unit_normals(3, 90), unit_normals(4, 77)]
    last = lambda: lib.icp_last_error().decode()

    def code(call):
        try:
            call()
        except pkg.IcpError as e:
            return e.code
        return 0

    begin_code = lambda bt, metric=SYM: code(lambda: bt.begin(max_iter=5, metric=metric))

    with ctx.batch(pairs) as bt:
        assert begin_code(bt) == INV and "moving clouds" in last()
        assert "icp_batch_estimate_point_normals" in last() and "icp_batch_set_point_normals" in last()
        bt.set_point_normals(moving=Np)
        assert begin_code(bt) == INV and "models" in last() and "icp_batch_set_point_normals" in last()
        with ctx.batch(pairs) as other:
            other.set_point_normals(model=Nq)
            assert begin_code(other) == INV and "moving clouds" in last()
        bt.set_point_normals(model=Nq)
        bt.set_robust("huber", 0.1)
        assert begin_code(bt) == INV and "robust" in last()
        bt.set_robust(None)
        assert begin_code(bt) == 0
        with pytest.raises(pkg.IcpError) as e:
            bt.begin(max_iter=5, metric=5)
        assert e.value.code == INV
        st = np.zeros(2, dtype=np.intc)
        assert lib.icp_batch_evaluate(bt._h, SYM, None, st.ctypes.data_as(pi), None, None, None, None, None, None) == INV
        # a point-normal call during a symmetric loop discards it
        bt.estimate_covariances(8)
        for change in (lambda: bt.set_point_normals(moving=Np), lambda: bt.set_point_normals(model=Nq), lambda: bt.estimate_point_normals("centroid"),
                       lambda: bt.estimate_point_normals("none")):
            assert begin_code(bt) == 0 and bt.run(1)[0] == 1
            bt.diag_rotation(0)
            change()
            assert code(lambda: bt.run(1)) == STATE
            assert code(lambda: bt.diag_rotation(0)) == STATE
        # a refused call leaves the loop running
        assert begin_code(bt) == 0 and bt.run(1)[0] == 1
        bad = [Np[0].copy(), Np[1]]
        bad[0][3, 1] = np.nan
        assert code(lambda: bt.set_point_normals(moving=bad)) == INV
        assert code(lambda: bt.estimate_point_normals(7)) == INV
        assert bt.run(1)[0] == 1
    # under a point-to-point loop the calls leave the loop running, with its bytes
    with ctx.batch(pairs) as plain, ctx.batch(pairs) as held:
        held.estimate_covariances(8)   # (before the loop: new covariances discard any loop, as they always did)
        for bt in (plain, held):
            bt.begin(max_iter=8, tol=1e-7)
            assert bt.run(2)[0] == 2
        held.set_point_normals(Np, Nq)
        held.estimate_point_normals("centroid")
        assert code(lambda: held.diag_rotation(0)) == STATE
        for bt in (plain, held):
            while bt.run(1 << 20)[1]:
                pass
        for p, (a, b) in enumerate(zip(final(plain), final(held))):
            same_pair_bytes(a, b, f"pair {p}")
        # ... and after a symmetric loop has ended and a point-to-point loop has begun
        run_to_end(held, SYM, 3)
        held.begin(max_iter=8, tol=1e-7)
        assert held.run(2)[0] == 2
        held.set_point_normals(Np, Nq)
        while held.run(1 << 20)[1]:
            pass
        for p, (a, b) in enumerate(zip(final(plain), final(held))):
            same_pair_bytes(a, b, f"pair {p}, after a symmetric loop")
    # the entries that take a metric elsewhere refuse the value as they refuse any unknown one
    A, M = pairs[0]
    with pytest.raises(pkg.IcpError) as e:
        ctx._run_batch(SYM, pairs, None, 5, 1e-6, False)
    assert e.value.code == INV
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with pytest.raises(pkg.IcpError) as e:
            c.loop_begin(metric=SYM, max_iter=5)
        assert e.value.code == INV


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_point_normals_do_not_touch_the_other_metrics(ctx, pkg, dtype):
    pairs = [(A, M) for A, M, _ in (gate_case(*c, dtype=dtype) for c in CASES[:3])]
    inten = lambda seed, n: np.random.default_rng(seed).uniform(0.0, 1.0, n)
    for metric in (pkg.ICP_POINT_TO_POINT, pkg.ICP_POINT_TO_PLANE, pkg.ICP_GENERALIZED, pkg.ICP_COLORED):
        with ctx.batch(pairs) as plain, ctx.batch(pairs) as held:
            for bt in (plain, held):
                bt.estimate_normals()
                bt.estimate_covariances(10)
                bt.set_max_distance(MD)
                bt.set_intensities([inten(b, A.shape[0]) for b, (A, _) in enumerate(pairs)], [inten(9 + b, M.shape[0]) for b, (_, M) in enumerate(pairs)])
                bt.estimate_intensity_gradients(8)
            held.estimate_point_normals("centroid")
            a, b = run_to_end(plain, metric, 20), run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}")
            # ... also after a symmetric loop ran on the same batch
            run_to_end(held, pkg.ICP_SYMMETRIC, 5)
            b = run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}, after a symmetric loop")
