"""GPU: the colored metric of a batch (icp_batch_set_intensities, icp_batch_estimate_intensity_gradients,
icp_batch_set_intensity_gradients, icp_batch_get_intensity_gradients, icp_batch_set_color_weight, icp_batch_begin with ICP_COLORED;
Batch.*, Context.register_batch_colored).

    1  gradients byte for byte against numpy (batch_color_ref.gradients): models of k + 1, 63, 64, 65, 130, 257, 513 and 1025
       points (a single lane, ragged and full work items, the LDS tile edges of 256 and 512 points per wave), k at the edges of
       the three list capacities, a lattice (ties at the k-th: a neighbourhood larger than k), duplicated points (tau = 0, the
       fallback), a far cloud, both dtypes; and a pair's result alone and at either end of a batch whose other pairs use another
       k (another capacity of the launch)
    2  one step and a second: idx and masks are those of a point-to-point batch on the device's own moved cloud, byte for byte,
       with a gate, a trim, reciprocity and an initial transform; the front end moved the cloud by the host solve of the previous
       vector; every slot of the vector agrees with the exact sum (math.fsum) of the numpy terms within ref_moments.tolerance -- a
       derived bound, 2 (n + 16) u sum |term|; lambda differs per pair
    3  lambda = 1 throughout: the vectors and the finished runs of a gated point-to-plane batch
    4  the loop against the numpy reference loop on the flat and the curved textured pair: the plane metric ends the flat pair
       ICP_ERR_SINGULAR, the colored metric registers it; register_batch_colored from RGB
    5  refusals and state
    6  a batch that holds intensities and gradients runs the other metrics with the bytes of one that holds none"""
import ctypes as C

import numpy as np
import pytest

import batch_color_ref as cr
import batch_gicp_ref as gr
import batch_outlier_ref as orf
import ref_moments as rm
from batch_ref import (CASES, TOL_E, TOL_T, assert_same_run, bits_equal, check_front_end, gate_case, hom, keep_within, rel, rot,
                       run_to_end, same_pair_bytes)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = (63, 64, 65, 130, 257, 513, 1025)
K_EDGES = (3, 8, 9, 16, 17, 32)
MD, RHO = 0.05, 0.5
_REF = {}


def unit_normals(seed, n, dtype):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return np.ascontiguousarray((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype))


def intensities(seed, n):
    return np.random.default_rng(seed).uniform(0.0, 1.0, n)


def ref_grad(X, N, I, k):
    """batch_color_ref.gradients, computed once per (cloud, k)"""
    key = (X.dtype.str, X.tobytes(), N.tobytes(), I.tobytes(), k)
    if key not in _REF:
        _REF[key] = cr.gradients(X, N, I, k)
    return _REF[key]


def fine(X, seed):
    """fp64 clouds get mantissas fp32 cannot hold"""
    if X.dtype == np.float64:
        X = X + 1e-9 * np.random.default_rng(seed).standard_normal(X.shape)
    return np.ascontiguousarray(X)


def gradient_models(dtype, k):
    """blobs of k + 1 to 1025 points, a lattice (ties at every rank), 300 points of which 40 coincide, a cloud 1e4 from the origin"""
    models = [fine(gr.blob(100 + n, n, dtype), n) for n in (k + 1,) + SIZES]
    return models + [orf.lattice(dtype, side=6, step=0.5), orf.coincident(dtype), orf.far(dtype)[:200].copy()]


def tiny_movers(count, dtype):
    return [gr.blob(900 + b, 3, dtype) for b in range(count)]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_EDGES)
@DTYPES
def test_gradients_bit_for_bit(ctx, pkg, dtype, k):
    models = gradient_models(dtype, k)
    count = len(models)
    Ns = [unit_normals(200 + b, M.shape[0], dtype) for b, M in enumerate(models)]
    Is = [intensities(300 + b, M.shape[0]) for b, M in enumerate(models)]
    with ctx.batch(list(zip(tiny_movers(count, dtype), models))) as bt:
        bt.set_model_normals(Ns)
        bt.set_intensities(model=Is)
        got = bt.estimate_intensity_gradients(k, want=True)
        held = bt.get_intensity_gradients()
        larger = 0
        for b, M in enumerate(models):
            want, cnt = ref_grad(M, Ns[b], Is[b], k)
            larger += int((cnt > k).any())
            assert got[b].dtype == np.float64 and got[b].shape == want.shape
            bad = np.flatnonzero((got[b].view(np.uint64) != want.view(np.uint64)).any(axis=1))
            assert bad.size == 0, f"pair {b} k {k}: {bad.size} of {M.shape[0]} points differ, first {bad[0]}: {got[b][bad[0]]!r} / {want[bad[0]]!r}"
            assert bits_equal(held[b], got[b])
        assert larger >= 2   # the lattice and the duplicates: neighbourhoods larger than k
        assert (got[count - 2][100:140] == 0.0).all()   # the duplicates: the fallback
        # the caller's own gradients come back as given
        mine = [np.random.default_rng(40 + b).standard_normal(g.shape) for b, g in enumerate(got)]
        bt.set_intensity_gradients(mine)
        for a, b_ in zip(bt.get_intensity_gradients(), mine):
            assert bits_equal(a, b_)


@DTYPES
def test_gradients_over_sub_tiles(ctx, pkg, dtype):
    """2100 points -- more than one LDS sub-tile per wave in either precision (the sizes above reach a second one in fp64 alone), a
    last chunk that is padded, work items that straddle the quarters -- beside k + 1 points, at both edges of a list capacity"""
    models = [fine(gr.blob(61, 2100, dtype), 62), fine(gr.blob(63, 17, dtype), 64), fine(gr.blob(65, 10, dtype), 66)]
    ks = [9, 16, 9]
    Ns = [unit_normals(220 + b, M.shape[0], dtype) for b, M in enumerate(models)]
    Is = [intensities(320 + b, M.shape[0]) for b, M in enumerate(models)]
    with ctx.batch(list(zip(tiny_movers(len(models), dtype), models))) as bt:
        bt.set_model_normals(Ns)
        bt.set_intensities(model=Is)
        got = bt.estimate_intensity_gradients(ks, want=True)
        for b, M in enumerate(models):
            want = ref_grad(M, Ns[b], Is[b], ks[b])[0]
            bad = np.flatnonzero((got[b].view(np.uint64) != want.view(np.uint64)).any(axis=1))
            assert bad.size == 0, f"pair {b} k {ks[b]}: {bad.size} of {M.shape[0]} points differ, first {bad[0]}: {got[b][bad[0]]!r} / {want[bad[0]]!r}"


@DTYPES
def test_a_pairs_gradients_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X, Y, Z = fine(gr.blob(7, 300, dtype), 8), orf.lattice(dtype, side=5, step=0.25), fine(gr.blob(15, 513, dtype), 16)
    N = {id(M): unit_normals(60 + b, M.shape[0], dtype) for b, M in enumerate((X, Y, Z))}
    I = {id(M): intensities(70 + b, M.shape[0]) for b, M in enumerate((X, Y, Z))}

    def run(models, ks):
        with ctx.batch(list(zip(tiny_movers(len(models), dtype), models))) as bt:
            bt.set_model_normals([N[id(M)] for M in models])
            bt.set_intensities(model=[I[id(M)] for M in models])
            return bt.estimate_intensity_gradients(ks, want=True)

    alone = run([X], 5)                       # a launch of capacity 8
    first = run([X, Y, Z], [5, 20, 32])       # capacity 32
    last = run([Z, Y, X], [32, 20, 5])
    mid = run([Y, X, Z], [20, 5, 12])         # capacity 32, another neighbour
    assert bits_equal(alone[0], first[0]) and bits_equal(alone[0], last[2]) and bits_equal(alone[0], mid[1])
    assert bits_equal(first[2], last[0]) and bits_equal(first[1], last[1])
    assert bits_equal(alone[0], ref_grad(X, N[id(X)], I[id(X)], 5)[0])


# 2 ------------------------------------------------------------------------------------------------------------------------
def step_pairs(dtype):
    """batch_ref.CASES and a moving cloud of one point (a single lane; its pass is checked like any other)"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    rng = np.random.default_rng(41)
    pairs.append((rng.standard_normal((1, 3)).astype(dtype) * 0.1, rng.standard_normal((40, 3)).astype(dtype)))
    return pairs


LAMBDAS = [0.0, 1.0, cr.LAMBDA_DEFAULT, 0.5, 0.3]


def set_options(bt, mode, count, T0=None):
    if "gate" in mode:
        bt.set_max_distance([MD] * (count - 1) + [np.inf])
    if "trim" in mode:
        bt.set_trim([RHO] * (count - 1) + [1.0])
    if "mutual" in mode:
        bt.set_reciprocal([True] * (count - 1) + [False])
    if T0 is not None:
        bt.set_initial_transforms(T0)


def dress(bt, pairs, lam):
    """normals from the device, random intensities, device gradients, the weights: (normals, Ip, Iq, D)"""
    Nq = bt.estimate_normals()
    Ip = [intensities(600 + b, A.shape[0]) for b, (A, _) in enumerate(pairs)]
    Iq = [intensities(700 + b, M.shape[0]) for b, (_, M) in enumerate(pairs)]
    bt.set_intensities(Ip, Iq)
    D = bt.estimate_intensity_gradients(8, want=True)
    bt.set_color_weight(lam)
    return Nq, Ip, Iq, D


@pytest.mark.parametrize("mode", ["plain", "gate", "trim", "mutual", "init", "gate+trim+mutual+init"])
@DTYPES
def test_steps_decide_as_point_to_point_and_sum_the_terms(ctx, pkg, dtype, mode):
    pairs = step_pairs(dtype)
    count = len(pairs)
    assert count == len(LAMBDAS)
    T0 = None
    if "init" in mode:
        T0 = np.stack([hom(rot("z", 0.004 * (b + 1)) @ rot("x", -0.003 * b), np.array([0.002 * b, -0.003, 0.001])) for b in range(count)])
        T0[1] = np.eye(4)
    worst = 0.0
    with ctx.batch(pairs) as bt:
        Nq, Ip, Iq, D = dress(bt, pairs, LAMBDAS)
        set_options(bt, mode, count, T0)
        bt.begin(max_iter=3, tol=0.0, fixed_iterations=True, metric=pkg.ICP_COLORED)
        prev = [None] * count
        for step in (1, 2):
            live = np.flatnonzero(~bt.done())
            assert step == 2 or live.size == count
            assert set(range(count - 1)) <= set(live.tolist()), (mode, step)   # (one match cannot fix six unknowns: the pair of one point may end)
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
                st, mom = bt.state(b), bt.diag_moments(b)
                check_front_end(pkg, True, moved[b], M, mom, st["err"][step - 1] if step > 1 else 0.0, prev[b], what)
                worst = max(worst, cr.check_sums(moved[b], M, Nq[b], idx[b], inl[b], Ip[b], Iq[b], D[b], LAMBDAS[b], mom, what))
                prev[b] = dict(P=moved[b], idx=idx[b], mask=inl[b], mom=mom)
            if "gate" in mode or "trim" in mode or "mutual" in mode:
                assert any((~inl[b]).any() for b in range(count - 1)), (mode, step)   # the options reject something
    print(f"[color steps] {mode}/{np.dtype(dtype).name}: largest |device - exact| / tol = {worst:.4f}")


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_lambda_one_is_the_gated_plane_batch(ctx, pkg, dtype):
    pairs = [(A, M) for A, M, _ in (gate_case(*c, dtype=dtype) for c in CASES[:3])]
    count = len(pairs)
    with ctx.batch(pairs) as col, ctx.batch(pairs) as pl:
        Nq, Ip, Iq, D = dress(col, pairs, 1.0)
        pl.set_model_normals(Nq)
        for bt in (col, pl):
            bt.set_max_distance(MD)
        col.begin(max_iter=30, tol=1e-6, metric=pkg.ICP_COLORED)
        pl.begin(max_iter=30, tol=1e-6, metric=pkg.ICP_POINT_TO_PLANE)
        assert col.run(1)[0] == 1 and pl.run(1)[0] == 1
        idx, inl, pidx, pinl = col.get_indices(), col.get_inliers(), pl.get_indices(), pl.get_inliers()
        for b, (A, M) in enumerate(pairs):
            assert bits_equal(idx[b], pidx[b]) and bits_equal(inl[b], pinl[b]) and not inl[b].all() and inl[b].any()
            mc, mp = col.diag_moments(b), pl.diag_moments(b)
            _, maj = rm.plane(A[inl[b]], M, Nq[b], idx[b][inl[b]])
            tol = rm.tolerance(maj, A.shape[0])
            assert mc[rm.CNT] == mp[rm.CNT] == float(inl[b].sum())
            for s in rm.PLANE_SLOTS:
                assert abs(mc[s] - mp[s]) <= tol[s], f"pair {b} slot {s}: colored {mc[s]!r} plane {mp[s]!r} tol {tol[s]:.3e}"
        a, p = run_to_end(col, pkg.ICP_COLORED, 30), run_to_end(pl, pkg.ICP_POINT_TO_PLANE, 30)
        for b in range(count):
            sa, sp = a[b]["st"], p[b]["st"]
            print(f"[color lambda 1] {np.dtype(dtype).name} pair {b}: iterations {sa['iterations']} / {sp['iterations']}, rel T {rel(sa['T'], sp['T']):.3e}")
            assert sa["status"] == sp["status"] == pkg.capi.ICP_OK
            assert_same_run(sa["iterations"], sa["err"], sa["T"], dict(iterations=sp["iterations"], err=sp["err"], T=sp["T"]), 1e-6,
                            fp32=dtype == np.float32)
            assert rel(sa["T"], sp["T"]) < TOL_T and np.abs(sa["err"][:len(sp["err"])] - sp["err"][:len(sa["err"])]).max() < TOL_E


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_loop_registers_what_the_plane_metric_cannot(ctx, pkg, orc, dtype):
    tex = [cr.textured(0.0, dtype), cr.textured(0.05, dtype)]
    pairs = [(t["A"], t["M"]) for t in tex]
    lam = [cr.LAMBDA_DEFAULT, 0.5]
    with ctx.batch(pairs) as bt:
        bt.set_model_normals([t["N"] for t in tex])
        bt.set_max_distance(cr.GATE_TEX)
        plane = run_to_end(bt, pkg.ICP_POINT_TO_PLANE, cr.ITER_TEX, 0.0, fixed=True)
        assert plane[0]["st"]["status"] == pkg.capi.ICP_ERR_SINGULAR and plane[1]["st"]["status"] == pkg.capi.ICP_OK
        bt.set_intensities([t["Ip"] for t in tex], [t["Iq"] for t in tex])
        D = bt.estimate_intensity_gradients(cr.K_TEX, want=True)
        bt.set_color_weight(lam)
        res = run_to_end(bt, pkg.ICP_COLORED, cr.ITER_TEX, 0.0, fixed=True)
    for b, t in enumerate(tex):
        assert bits_equal(D[b], ref_grad(t["M"], t["N"], t["Iq"], cr.K_TEX)[0])
        want = cr.color_loop(orc, t["A"], t["M"], t["N"], t["Ip"], t["Iq"], D[b], lam[b], cr.ITER_TEX, 0.0, keep=keep_within(cr.GATE_TEX))
        st = res[b]["st"]
        start, end = cr.pose_error(np.eye(4), t), cr.pose_error(st["T"], t)
        print(f"[color loop] {np.dtype(dtype).name} pair {b}: iterations {st['iterations']} / {want['iterations']}, rel T {rel(st['T'], want['T']):.3e}, "
              f"max |dE| {np.abs(st['err'][:len(want['err'])] - want['err'][:len(st['err'])]).max():.3e}, pose error {start:.3e} -> {end:.3e}")
        assert st["status"] == pkg.capi.ICP_OK and not want["empty"] and not want["singular"], b
        assert_same_run(st["iterations"], st["err"], st["T"], want, 0.0, fp32=dtype == np.float32)
        assert end < 0.1 * start, (b, start, end)
    e_plane = cr.pose_error(plane[1]["st"]["T"], tex[1])
    print(f"[color loop] {np.dtype(dtype).name} curved: plane metric's pose error {e_plane:.3e}")
    assert cr.pose_error(res[1]["st"]["T"], tex[1]) < 0.2 * e_plane


def test_register_batch_colored_from_rgb(ctx, pkg):
    tex = [cr.textured(0.0, np.float32), cr.textured(0.05, np.float32, seed=3)]
    pairs = [(t["A"], t["M"]) for t in tex]
    tint = np.array([0.9, 1.0, 1.1])   # a colour whose channel mean is the texture
    Ip = [pkg.intensity_from_rgb(t["Ip"][:, None] * tint) for t in tex]
    Iq = [pkg.intensity_from_rgb(t["Iq"][:, None] * tint) for t in tex]
    res = ctx.register_batch_colored(pairs, (Ip, Iq), k=cr.K_TEX, normals=[t["N"] for t in tex], max_distance=cr.GATE_TEX, max_iter=cr.ITER_TEX)
    for r, t in zip(res, tex):
        assert r.extra["status"] == pkg.capi.ICP_OK and r.extra["fitness"] > 0.9
        assert cr.pose_error(r.T, t) < 0.1 * cr.pose_error(np.eye(4), t)
    # normals estimated on the device, lambda per pair, an option passed through
    res = ctx.register_batch_colored(pairs[1:], (Ip[1:], Iq[1:]), k=[10], lam=[0.9], max_distance=cr.GATE_TEX, trim=0.95, max_iter=cr.ITER_TEX)
    assert res[0].extra["status"] == pkg.capi.ICP_OK and cr.pose_error(res[0].T, tex[1]) < 0.1 * cr.pose_error(np.eye(4), tex[1])
    with pytest.raises(TypeError):
        ctx.register_batch_colored(pairs, (Ip, Iq), kernel="huber")


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(ctx, pkg):
    lib = pkg.load()
    INV, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    COL = pkg.ICP_COLORED
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    pairs = [(gr.blob(1, 70, np.float32), gr.blob(2, 90, np.float32)), (gr.blob(3, 6, np.float32), gr.blob(4, 7, np.float32))]
    Ip, Iq = [intensities(1, 70), intensities(2, 6)], [intensities(3, 90), intensities(4, 7)]
    last = lambda: lib.icp_last_error().decode()

    def begin_code(bt, metric=COL):
        try:
            bt.begin(max_iter=5, metric=metric)
        except pkg.IcpError as e:
            return e.code
        return 0

    def code(call):
        try:
            call()
        except pkg.IcpError as e:
            return e.code
        return 0

    with ctx.batch(pairs) as bt:
        assert begin_code(bt) == INV and "normals" in last()
        assert code(lambda: bt.estimate_intensity_gradients(5)) == STATE and "intensities" in last()
        bt.set_intensities(model=Iq)
        assert code(lambda: bt.estimate_intensity_gradients(5)) == STATE and "normals" in last()
        bt.estimate_normals()
        assert begin_code(bt) == INV and "moving clouds" in last()
        bt.set_intensities(moving=Ip)
        assert begin_code(bt) == INV and "gradients" in last()
        assert code(bt.get_intensity_gradients) == STATE
        for k, names in (([5, 2], "pair 1"), ([33, 5], "pair 0"), ([5, 7], "pair 1")):   # range; 7 points < k + 1
            ka = np.asarray(k, dtype=np.intc)
            assert lib.icp_batch_estimate_intensity_gradients(bt._h, ka.ctypes.data_as(pi), None) == INV, k
            assert names in last(), (k, last())
        assert lib.icp_batch_estimate_intensity_gradients(bt._h, None, None) == INV
        assert lib.icp_batch_set_intensities(bt._h, None, None) == INV
        bad = np.concatenate(Ip)
        bad[72] = np.nan
        assert lib.icp_batch_set_intensities(bt._h, bad.ctypes.data_as(pd), None) == INV and "pair 1, moving cloud" in last()
        bad = np.concatenate(Iq)
        bad[3] = np.inf
        assert lib.icp_batch_set_intensities(bt._h, None, bad.ctypes.data_as(pd)) == INV and "pair 0, model" in last()
        g = np.zeros((97, 3))
        g[95, 1] = np.nan
        assert lib.icp_batch_set_intensity_gradients(bt._h, g.ctypes.data_as(pd)) == INV and "pair 1" in last()
        assert lib.icp_batch_set_intensity_gradients(bt._h, None) == INV
        for lam in ([0.5, 1.5], [-0.1, 0.5], [0.5, np.nan]):
            la = np.asarray(lam)
            assert lib.icp_batch_set_color_weight(bt._h, la.ctypes.data_as(pd)) == INV and "pair" in last()
        assert begin_code(bt) == INV and "gradients" in last()                                      # every refusal left the batch as it was
        bt.estimate_intensity_gradients([5, 6])
        bt.set_robust("huber", 0.1)
        assert begin_code(bt) == INV and "robust" in last()
        bt.set_robust(None)
        assert begin_code(bt) == 0
        st = np.zeros(2, dtype=np.intc)
        assert lib.icp_batch_evaluate(bt._h, COL, None, st.ctypes.data_as(pi), None, None, None, None, None, None) == INV
        # a change during a loop discards it
        grads = bt.get_intensity_gradients()
        for change in (lambda: bt.set_intensities(moving=Ip), lambda: bt.set_intensity_gradients(grads), lambda: bt.estimate_intensity_gradients(4),
                       lambda: bt.set_color_weight(0.5), lambda: bt.set_color_weight(None)):
            assert begin_code(bt) == 0 and bt.run(1)[0] == 1
            change()
            assert code(lambda: bt.run(1)) == STATE
        # new model intensities and new normals discard the gradients
        assert begin_code(bt) == 0
        bt.set_intensities(model=Iq)
        assert begin_code(bt) == INV and "gradients" in last() and code(bt.get_intensity_gradients) == STATE
        bt.set_intensity_gradients(grads)
        assert begin_code(bt) == 0
        bt.estimate_normals()
        assert begin_code(bt) == INV and "gradients" in last()
        bt.set_intensity_gradients(grads)
        bt.set_model_normals([unit_normals(5, 90, np.float32), unit_normals(6, 7, np.float32)])
        assert begin_code(bt) == INV and "gradients" in last()
        bt.set_intensities(moving=Ip)                                                               # the moving side discards nothing
        bt.estimate_intensity_gradients(3)
        assert begin_code(bt) == 0
    # the entries that take a metric elsewhere refuse the value as they refuse any unknown one
    A, M = pairs[0]
    with pytest.raises(pkg.IcpError) as e:
        ctx._run_batch(COL, pairs, None, 5, 1e-6, False)
    assert e.value.code == INV
    # a context with a pending pass
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with pytest.raises(pkg.IcpError) as e:
            c.loop_begin(metric=COL, max_iter=5)
        assert e.value.code == INV
        with c.batch(pairs) as bt:
            bt.estimate_normals()
            bt.set_intensities(Ip, Iq)
            bt.estimate_intensity_gradients(5)
            grads = bt.get_intensity_gradients()
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            for call in (lambda: bt.set_intensities(Ip, Iq), lambda: bt.estimate_intensity_gradients(5), lambda: bt.set_intensity_gradients(grads),
                         bt.get_intensity_gradients, lambda: bt.set_color_weight(0.5)):
                assert code(call) == STATE
            c.loop_complete()
            assert begin_code(bt) == 0


# 6 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_intensities_do_not_touch_the_other_metrics(ctx, pkg, dtype):
    pairs = [(A, M) for A, M, _ in (gate_case(*c, dtype=dtype) for c in CASES[:3])]
    for metric in (pkg.ICP_POINT_TO_POINT, pkg.ICP_POINT_TO_PLANE, pkg.ICP_GENERALIZED):
        with ctx.batch(pairs) as plain, ctx.batch(pairs) as held:
            for bt in (plain, held):
                bt.estimate_normals()
                bt.estimate_covariances(10)
                bt.set_max_distance(MD)
            held.set_intensities([intensities(b, A.shape[0]) for b, (A, _) in enumerate(pairs)], [intensities(9 + b, M.shape[0]) for b, (_, M) in enumerate(pairs)])
            held.estimate_intensity_gradients(8)
            a, b = run_to_end(plain, metric, 20), run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}")
            # ... also after a colored loop ran on the same batch
            run_to_end(held, pkg.ICP_COLORED, 5)
            b = run_to_end(held, metric, 20)
            for p in range(len(pairs)):
                same_pair_bytes(a[p], b[p], f"metric {metric} pair {p}, after a colored loop")
