"""GPU: the generalized (plane-to-plane) metric of a batch (icp_batch_set_covariances, icp_batch_estimate_covariances,
icp_batch_get_covariances, icp_batch_begin with ICP_GENERALIZED; Batch.*, Context.register_batch_generalized).

    1  covariances byte for byte against numpy (batch_gicp_ref.covariances): clouds of k + 1, 63, 64, 65, 130, 257, 513 and 1025
       points (a single lane, ragged and full work items, the LDS tile edges of 256 and 512 points per wave), k at the edges of
       the three list capacities, a lattice (ties at the k-th: a neighbourhood larger than k + 1), duplicated points (tau = 0,
       f = 0), a far cloud, both regularisations, both dtypes; and a pair's result alone and at either end of a batch whose other
       pairs use another k (another capacity of the launch)
    2  one step and a second: idx and masks are those of a point-to-point batch on the device's own moved cloud, byte for byte,
       with a gate, a trim, reciprocity and an initial transform; diag_rotation is the rotation of the composed motions; the
       front end moved the cloud by the host solve of the previous vector; every slot of the vector agrees with the exact sum
       (math.fsum) of the numpy terms within ref_moments.tolerance -- a derived bound, 2 (n + 16) u sum |term|
    3  the loop against the numpy reference loop on batch_ref.fp64_pairs / fp32_pairs: status, iterations where assert_same_run
       demands them, T and err at the project's TOL_T / TOL_E; a run from covariances_from_normals; a pair with the raw
       covariances of a planar cloud on both sides (every det == 0) ends ICP_ERR_EMPTY while the others finish
    4  refusals and state; a batch that holds covariances runs the other metrics with the bytes of one that holds none"""
import ctypes as C

import numpy as np
import pytest

import batch_gicp_ref as gr
import batch_outlier_ref as orf
from batch_ref import (CASES, assert_same_run, bits_equal, check_front_end, compose, fp32_pairs, fp64_pairs, gate_case,
                       hom, rel, rot, run_to_end, same_pair_bytes, t0f)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = (63, 64, 65, 130, 257, 513, 1025)
K_MODEL = {3: 8, 8: 3, 9: 16, 16: 9, 17: 32, 32: 17}   # the models' k: the other edge of the same list capacity
MD, RHO = 0.05, 0.5
_REF = {}


def ref_cov(X, k, reg, lam):
    """batch_gicp_ref.covariances, computed once per (cloud, k, regularisation)"""
    key = (X.dtype.str, X.shape[0], X.tobytes(), k, reg, lam)
    if key not in _REF:
        _REF[key] = gr.covariances(X, k, reg, lam)
    return _REF[key]


def fine(X, seed):
    """fp64 clouds get mantissas fp32 cannot hold"""
    if X.dtype == np.float64:
        X = X + 1e-9 * np.random.default_rng(seed).standard_normal(X.shape)
    return np.ascontiguousarray(X)


def special_models(dtype):
    """a lattice (ties at every rank), 300 points of which 40 coincide, a cloud 1e4 from the origin, a small blob"""
    return [orf.lattice(dtype, side=6, step=0.5), orf.coincident(dtype), orf.far(dtype)[:200].copy(), fine(gr.blob(31, 40, dtype), 32)]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", ["frobenius", "none"])
@pytest.mark.parametrize("k", sorted(K_MODEL))
@DTYPES
def test_covariances_bit_for_bit(ctx, pkg, dtype, k, reg):
    lam = 1e-3
    movers = [fine(gr.blob(100 + n, n, dtype), n) for n in (k + 1,) + SIZES]
    models = special_models(dtype)
    models = [models[i % len(models)] for i in range(len(movers))]
    kq = K_MODEL[k]
    regc = gr.COV_FROBENIUS if reg == "frobenius" else gr.COV_NONE
    with ctx.batch(list(zip(movers, models))) as bt:
        cm, cq = bt.estimate_covariances(k, kq, regularisation=reg, lam=lam, want=True)
        gm, gq = bt.get_covariances()
        larger = 0
        for b, (A, M) in enumerate(zip(movers, models)):
            wm, cnt_m = ref_cov(A, k, regc, lam)
            wq, cnt_q = ref_cov(M, kq, regc, lam)
            larger += int((cnt_q > kq + 1).any())
            for got, want, what in ((cm[b], wm, "moving"), (cq[b], wq, "model")):
                assert got.dtype == np.float64 and got.shape == want.shape
                bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
                assert bad.size == 0, f"pair {b} {what} k {k}/{kq}: {bad.size} points differ, first {bad[0]}: {got[bad[0]]!r} / {want[bad[0]]!r}"
            assert bits_equal(gm[b], cm[b]) and bits_equal(gq[b], cq[b])
        assert larger >= 2   # the lattice and the duplicates: neighbourhoods larger than k + 1
        # one side alone replaces that side only
        bt.estimate_covariances(None, k, regularisation=reg, lam=lam)
        gm2, gq2 = bt.get_covariances()
        for b, M in enumerate(models):
            assert bits_equal(gm2[b], cm[b]) and bits_equal(gq2[b], ref_cov(M, k, regc, lam)[0])


@DTYPES
def test_covariances_over_sub_tiles(ctx, pkg, dtype):
    """2100 points -- more than one LDS sub-tile per wave in either precision (the sizes above reach a second one in fp64 alone), a
    last chunk that is padded, work items that straddle the quarters -- beside k + 1 points, at both edges of a list capacity"""
    lam = 1e-3
    movers = [fine(gr.blob(51, 2100, dtype), 52), fine(gr.blob(53, 10, dtype), 54)]
    models = [fine(gr.blob(55, 17, dtype), 56), fine(gr.blob(57, 2100, dtype), 58)]
    ks = [16, 9]
    with ctx.batch(list(zip(movers, models))) as bt:
        cm, cq = bt.estimate_covariances(ks, ks, regularisation="frobenius", lam=lam, want=True)
        for b in range(2):
            for got, X, what in ((cm[b], movers[b], "moving"), (cq[b], models[b], "model")):
                want = ref_cov(X, ks[b], gr.COV_FROBENIUS, lam)[0]
                bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
                assert bad.size == 0, f"pair {b} {what} k {ks[b]}: {bad.size} points differ, first {bad[0]}: {got[bad[0]]!r} / {want[bad[0]]!r}"


def test_duplicates_give_lambda_identity_on_the_device(ctx, pkg):
    X = orf.coincident(np.float32)
    with ctx.batch([(X, X.copy())]) as bt:
        cm, _ = bt.estimate_covariances(8, None, regularisation="frobenius", lam=0.25, want=True)
        assert (cm[0][100:140] == np.array([0.25, 0, 0, 0.25, 0, 0.25])).all() and not np.signbit(cm[0][100:140]).any()
        cm, _ = bt.estimate_covariances(8, None, regularisation="none", want=True)
        assert (cm[0][100:140] == 0.0).all()


@DTYPES
def test_a_pairs_covariances_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X = (fine(gr.blob(7, 300, dtype), 8), orf.lattice(dtype, side=5, step=0.25))
    Y = (fine(gr.blob(9, 130, dtype), 10), fine(gr.blob(11, 65, dtype), 12))
    Z = (fine(gr.blob(13, 70, dtype), 14), fine(gr.blob(15, 513, dtype), 16))
    with ctx.batch([X]) as bt:
        alone = bt.estimate_covariances(5, 7, want=True)   # a launch of capacity 8
    with ctx.batch([X, Y, Z]) as bt:
        first = bt.estimate_covariances([5, 20, 32], [7, 12, 9], want=True)   # capacity 32
    with ctx.batch([Z, Y, X]) as bt:
        last = bt.estimate_covariances([32, 20, 5], [9, 12, 7], want=True)
    for side in range(2):
        assert bits_equal(alone[side][0], first[side][0]) and bits_equal(alone[side][0], last[side][2])
        assert bits_equal(first[side][2], last[side][0]) and bits_equal(first[side][1], last[side][1])


# 2 ------------------------------------------------------------------------------------------------------------------------
def spd(seed, n):
    """n random symmetric positive definite matrices as (n, 6), eigenvalues in [1e-3, 1]"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, 3, 3))
    S = np.einsum("nab,ncb->nac", A, A) / 3.0 + 1e-3 * np.eye(3)
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))


def step_pairs(dtype):
    """batch_ref.CASES and a moving cloud of one point (a single lane; its pass is checked like any other, and its loop then ends
    with ICP_ERR_SINGULAR: one match cannot fix six unknowns)"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
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
    Cp = [spd(500 + b, A.shape[0]) for b, (A, _) in enumerate(pairs)]
    T0 = None
    if "init" in mode:
        T0 = np.stack([hom(rot("z", 0.004 * (b + 1)) @ rot("x", -0.003 * b), np.array([0.002 * b, -0.003, 0.001])) for b in range(count)])
        T0[1] = np.eye(4)
    worst = 0.0
    with ctx.batch(pairs) as bt:
        bt.set_covariances(moving=Cp)
        _, Cq = bt.estimate_covariances(None, 10, want=True)
        set_options(bt, mode, count, T0)
        bt.begin(max_iter=3, tol=0.0, fixed_iterations=True, metric=pkg.ICP_GENERALIZED)
        prev = [None] * count
        for step in (1, 2):
            # (the pair of one point takes part in step 1 alone: one match gives a 6 x 6 system of rank 3, which the solve refuses)
            live = range(count) if step == 1 else range(count - 1)
            assert bt.run(1) == (1, count - 1), (mode, step)
            assert bt.state(count - 1)["status"] == pkg.capi.ICP_ERR_SINGULAR
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
                assert bits_equal(R, np.ascontiguousarray(st["T"][:3, :3])), what
                Tinit = np.eye(4) if (T0 is None or b == 1) else t0f(T0[b], dtype)
                if step == 1:
                    assert bits_equal(R, np.ascontiguousarray(Tinit[:3, :3])), what
                else:
                    Rs, ts = pkg.solve_point_to_plane(prev[b]["mom"])[:2]
                    Tk = hom(Rs.astype(dtype).astype(np.float64), ts.astype(dtype).astype(np.float64))
                    Tl = compose(Tk, np.eye(4))
                    want_T = Tl if (T0 is None or b == 1) else compose(Tl, Tinit)
                    assert bits_equal(R, np.ascontiguousarray(want_T[:3, :3])), what
                check_front_end(pkg, True, moved[b], M, mom, st["err"][step - 1] if step > 1 else 0.0, prev[b], what)
                worst = max(worst, gr.check_sums(moved[b], M, idx[b], inl[b], Cp[b], Cq[b], R, mom, what))
                prev[b] = dict(P=moved[b], idx=idx[b], mask=inl[b], mom=mom)
            if "gate" in mode or "trim" in mode or "mutual" in mode:
                assert any((~inl[b]).any() for b in range(count - 1)), (mode, step)   # the options reject something
    print(f"[gicp steps] {mode}/{np.dtype(dtype).name}: largest |device - exact| / tol = {worst:.4f}")


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_loop_against_the_reference_loop(ctx, pkg, orc, golden, dtype):
    f32 = dtype == np.float32
    pairs = fp32_pairs(pkg, golden) if f32 else fp64_pairs(pkg, orc)
    max_iter, tol = (40, 1e-6) if f32 else (200, 1e-5)
    with ctx.batch(pairs) as bt:
        Cp, Cq = bt.estimate_covariances(12, want=True)
        res = run_to_end(bt, pkg.ICP_GENERALIZED, max_iter, tol)
    for b, (A, M) in enumerate(pairs):
        want = gr.gicp_loop(orc, A, M, Cp[b], Cq[b], max_iter, tol)
        st = res[b]["st"]
        print(f"[gicp loop] {np.dtype(dtype).name} pair {b}: iterations {st['iterations']} / {want['iterations']}, "
              f"rel T {rel(st['T'], want['T']):.3e}, max |dE| {np.abs(st['err'][:len(want['err'])] - want['err'][:len(st['err'])]).max():.3e}")
        assert st["status"] == pkg.capi.ICP_OK and not want["empty"], b
        assert_same_run(st["iterations"], st["err"], st["T"], want, tol, fp32=f32)


def test_loop_from_normals_and_one_call(ctx, pkg, orc):
    A = gr.surface(9, 400, np.float32)
    T = hom(rot("z", 0.04) @ rot("x", -0.03), np.array([0.03, -0.02, 0.025]))
    M = np.ascontiguousarray((A.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    nrm = np.stack([-0.6 * np.cos(2 * A[:, 0]) - 0.1 * A[:, 1], 0.6 * np.sin(3 * A[:, 1]) - 0.1 * A[:, 0], np.ones(400)], -1).astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    Cp, Cq = pkg.covariances_from_normals(nrm), pkg.covariances_from_normals(nrm @ T[:3, :3].T)
    B = gr.surface(10, 300, np.float32)
    pairs = [(A, M), (B, np.ascontiguousarray((B.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)))]
    res = ctx.register_batch_generalized(pairs[:1], covariances=([Cp], [Cq]), max_iter=50, tol=1e-7)
    want = gr.gicp_loop(orc, A, M, Cp, Cq, 50, 1e-7)
    assert res[0].extra["status"] == pkg.capi.ICP_OK
    assert_same_run(res[0].iterations, res[0].err, res[0].T, want, 1e-7, fp32=True)
    assert rel(res[0].T, T) < 1e-4 and res[0].extra["fitness"] == 1.0
    # estimated on the device, through the one-call entry
    res = ctx.register_batch_generalized(pairs, k=(12, 10), max_iter=50, tol=1e-7)
    for r in res:
        assert r.extra["status"] == pkg.capi.ICP_OK and rel(r.T, T) < 1e-4
    with pytest.raises(TypeError):
        ctx.register_batch_generalized(pairs, kernel="huber")


def test_multiscale_passes_the_metric_through(ctx, pkg):
    """coarse-to-fine with the generalized metric: every level estimates the covariances of its own (thinned) clouds"""
    A = gr.surface(21, 600, np.float32)
    T = hom(rot("z", 0.05) @ rot("y", 0.02), np.array([0.04, -0.03, 0.02]))
    M = np.ascontiguousarray((A.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    res = ctx.register_batch_multiscale([(A, M)], [0.2, 0.0], metric=pkg.ICP_GENERALIZED, k=8, max_iter=50, tol=1e-7)
    assert res[0].extra["status"] == pkg.capi.ICP_OK and rel(res[0].T, T) < 1e-4
    assert [lv["n"] for lv in res[0].extra["levels"]][1] == 600 and res[0].extra["levels"][0]["n"] < 600


def test_a_pair_whose_sums_are_singular_ends_empty(ctx, pkg, orc):
    """raw covariances of a planar grid on both sides and no rotation about an in-plane axis: S has an exact zero row, every det
    is 0, nothing is kept -- ICP_ERR_EMPTY for that pair; the others finish"""
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([g, np.zeros((64, 1))], 1).astype(np.float32)
    A = gr.surface(3, 200, np.float32)
    T = hom(rot("y", 0.03), np.array([0.01, 0.02, -0.01]))
    pairs = [(A, np.ascontiguousarray((A.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))), (P, P.copy()), (A[:70].copy(), A.copy())]
    with ctx.batch(pairs) as bt:
        cm, cq = bt.estimate_covariances(8, regularisation="none", want=True)
        assert (cm[1][:, [2, 4, 5]] == 0.0).all()
        fm, fq = bt.estimate_covariances([8, 8, 8], regularisation="frobenius", lam=1e-3, want=True)
        bt.set_covariances([fm[0], cm[1], fm[2]], [fq[0], cq[1], fq[2]])
        res = run_to_end(bt, pkg.ICP_GENERALIZED, 30, 1e-7)
        assert [r["st"]["status"] for r in res] == [pkg.capi.ICP_OK, pkg.capi.ICP_ERR_EMPTY, pkg.capi.ICP_OK]
        assert not res[1]["inl"].any() and res[1]["st"]["passes"] == 0
        assert rel(res[0]["st"]["T"], T) < 1e-4 and res[0]["inl"].all()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(ctx, pkg):
    lib = pkg.load()
    INV, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    GEN = pkg.ICP_GENERALIZED
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    pairs = [(gr.blob(1, 70, np.float32), gr.blob(2, 90, np.float32)), (gr.blob(3, 6, np.float32), gr.blob(4, 130, np.float32))]

    def begin_code(bt, metric=GEN):
        try:
            bt.begin(max_iter=5, metric=metric)
        except pkg.IcpError as e:
            return e.code
        return 0

    with ctx.batch(pairs) as bt:
        assert begin_code(bt) == INV and "covariances" in lib.icp_last_error().decode()        # none
        bt.estimate_covariances(None, 5)
        assert begin_code(bt) == INV and "moving" in lib.icp_last_error().decode()             # one side only
        with pytest.raises(pkg.IcpError) as e:
            bt.get_covariances()
        assert e.value.code == STATE
        for k, names in (([5, 2], "pair 1, moving cloud"), ([33, 5], "pair 0, moving cloud"), ([5, 6], "pair 1, moving cloud")):   # range; 6 points < k + 1
            ka = np.asarray(k, dtype=np.intc)
            assert lib.icp_batch_estimate_covariances(bt._h, ka.ctypes.data_as(pi), None, 1, 1e-3, None, None) == INV, k
            assert names in lib.icp_last_error().decode(), (k, lib.icp_last_error().decode())
        ka = np.asarray([5, 131], dtype=np.intc)
        assert lib.icp_batch_estimate_covariances(bt._h, None, ka.ctypes.data_as(pi), 1, 1e-3, None, None) == INV
        assert "pair 1, model" in lib.icp_last_error().decode()
        ka = np.asarray([5, 5], dtype=np.intc)
        assert lib.icp_batch_estimate_covariances(bt._h, None, None, 1, 1e-3, None, None) == INV
        assert lib.icp_batch_estimate_covariances(bt._h, ka.ctypes.data_as(pi), None, 2, 1e-3, None, None) == INV      # unknown regularisation
        for lam in (0.0, -1.0, np.nan, np.inf):
            assert lib.icp_batch_estimate_covariances(bt._h, ka.ctypes.data_as(pi), None, 1, lam, None, None) == INV, lam
        assert lib.icp_batch_set_covariances(bt._h, None, None) == INV
        bad = np.ones((76, 6))
        bad[72, 3] = np.nan
        assert lib.icp_batch_set_covariances(bt._h, bad.ctypes.data_as(pd), None) == INV
        assert "pair 1, moving cloud" in lib.icp_last_error().decode()
        assert begin_code(bt) == INV                                                                 # every refusal left the batch as it was
        bt.estimate_covariances([5, 5], None, regularisation="none", lam=float("nan"))               # NONE: lambda is not read
        bt.set_robust("huber", 0.1)
        assert begin_code(bt) == INV and "robust" in lib.icp_last_error().decode()
        bt.set_robust(None)
        assert begin_code(bt) == 0
        st = np.zeros(2, dtype=np.intc)
        assert lib.icp_batch_evaluate(bt._h, GEN, None, st.ctypes.data_as(pi), None, None, None, None, None, None) == INV
        # setting or estimating during a loop discards it
        want = bt.get_covariances()
        for change in (lambda: bt.set_covariances(model=want[1]), lambda: bt.estimate_covariances(None, 4)):
            assert begin_code(bt) == 0 and bt.run(1)[0] == 1
            change()
            with pytest.raises(pkg.IcpError) as e:
                bt.run(1)
            assert e.value.code == STATE
    # the entries that take a metric elsewhere refuse the value as they refuse any unknown one
    A, M = pairs[0]
    with pytest.raises(pkg.IcpError) as e:
        ctx._run_batch(GEN, pairs, None, 5, 1e-6, False)
    assert e.value.code == INV
    # a context with a pending pass
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with pytest.raises(pkg.IcpError) as e:
            c.loop_begin(metric=GEN, max_iter=5)
        assert e.value.code == INV
        with c.batch(pairs) as bt:
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            for call in (lambda: bt.estimate_covariances(5), lambda: bt.set_covariances(model=[np.ones((90, 6)), np.ones((130, 6))]), bt.get_covariances):
                with pytest.raises(pkg.IcpError) as e:
                    call()
                assert e.value.code == STATE
            c.loop_complete()
            bt.estimate_covariances(5)
            assert begin_code(bt) == 0


@DTYPES
def test_covariances_do_not_touch_the_other_metrics(ctx, pkg, dtype):
    cases = [gate_case(*c, dtype=dtype) for c in CASES[:3]]
    pairs = [(A, M) for A, M, _ in cases]
    for metric in (pkg.ICP_POINT_TO_POINT, pkg.ICP_POINT_TO_PLANE):
        with ctx.batch(pairs) as plain, ctx.batch(pairs) as held:
            held.estimate_covariances(10)
            for bt in (plain, held):
                bt.estimate_normals()
                bt.set_max_distance(MD)
            a, b = run_to_end(plain, metric, 20), run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}")
            # ... also after a generalized loop ran on the same batch
            held.set_max_distance(None)
            run_to_end(held, pkg.ICP_GENERALIZED, 5)
            held.set_max_distance(MD)
            b = run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}, after a generalized loop")
