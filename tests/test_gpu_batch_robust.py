"""GPU: the per-pair robust kernels of a batch (icp_batch_set_robust, icp_batch_get_weights; Batch.set_robust, Batch.get_weights,
Context.register_batch_robust).

Every kept match of a robust pair enters the sums of its pass with a Huber, Cauchy or Tukey weight of its residual; the step runs
deferred with batch_robust_moments in batch_trim_moments' place, and the pair's host loop solves on the vector with CNT <- W.

    1  the weights at the kernel's granules: one step over moving clouds of 1 and batch_ref.KNN_M points (a single lane, ragged
       and exact work items, up to 65 of them), each kernel, both dtypes, both metrics
    2  every pass exactly (the structure of test_gpu_batch_reciprocal.test_reciprocal_every_pass_exactly): robust alone, with a
       gate, a trim, the mutual rule, and all of them; the four pairs carry Tukey, Cauchy, Huber and no kernel
    3  end to end against the numpy IRLS loop, through Context.register_batch_robust
    4  bits: off means off, a pair without a kernel in a robust batch, independence of the other pairs and their order
    5  ending and state: a pair whose weights add up to 0, refusals, a pending pass, a set during a loop, initial transforms,
       an evaluation between steps

The clouds of 2 - 5 are those of test_gpu_batch_gate.py (batch_ref.gate_case); what the reference gives on them is pinned on the
CPU in test_batch_robust_ref.py.  Bounds (derived in batch_robust_ref.py, not measured): a weight against the formula of an
exactly formed r2 within 8u + (2 / k) 8u A_r; every slot against the exact sum with the device's own weights within 2 (n + 17) u
A_s; idx, masks, tau, rev and the moved cloud bit for bit; T and err of the end-to-end run at the project's 1e-5."""
import ctypes as C

import numpy as np
import pytest

import batch_robust_ref as br
import ref_moments as rm
from batch_mutual_ref import combined_mask
from batch_ref import (CASES, KNN_M, assert_same_run, bits_equal, check_front_end, compose, final, gate_case, hom, knn_models, rank, rel,
                       rot, run_to_end, same_pair_bytes, step_together, tau_bits_equal)

pytestmark = pytest.mark.gpu

MD = 0.05
RHO = 0.5
PASSES = 4
GRAN_N = (1,) + KNN_M
GRAN_M = (1, 63, 64, 65, 130)
KERNELS = ("huber", "cauchy", "tukey")
MIXED = ["tukey", "cauchy", "huber", None]          # the kernels of the four gate cases in tests 2, 4 and 5
MIXED_K = {False: [0.5, 0.05, 0.05, 1.0], True: [0.2, 0.02, 0.02, 1.0]}
END_RUNS = {(False, "tukey"): (0.5, [2, 3, 2, 2]), (False, "cauchy"): (0.05, [3, 3, 3, 2]),      # test_batch_robust_ref.RUNS
            (True, "tukey"): (0.2, [2, 3, 3, 2]), (True, "cauchy"): (0.02, [3, 4, 3, 2])}
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
PLANE = pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])


def metric_of(pkg, plane):
    return pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT


def gate_pairs(dtype, plane, order=range(4)):
    cases = [gate_case(*CASES[c], dtype=dtype) for c in order]
    pairs = [(A, M) for A, M, _ in cases]
    return cases, pairs, ([br.robust_normals(M) for _, M in pairs] if plane else None)


def check_weights(plane, kind, k, P, M, nrm, idx, mask, w, what):
    """the device's weights of one pair: 0.0 where rejected, exactly 1.0 without a kernel, else within the weight bound of the
    formula applied to an exactly formed r2.  Returns the largest |w_dev - w_ref| / bound"""
    assert w.dtype == np.float64 and w.shape == (P.shape[0],), what
    assert (w[~mask] == 0.0).all(), what
    if kind is None:
        assert (w[mask] == 1.0).all(), what
        return 0.0
    if not mask.any():
        return 0.0
    r2, A_r = br.residual_sq_exact(plane, P[mask], M, idx[mask], nrm)
    want = br.weight(br.KINDS[kind], r2, k)
    tol = br.weight_tolerance(k, A_r)
    dev = np.abs(w[mask] - want)
    i = int(np.argmax(dev / tol))
    assert (dev <= tol).all(), f"{what}: weight {w[mask][i]!r} formula {want[i]!r} |diff| {dev[i]:.3e} bound {tol[i]:.3e}"
    assert (w >= 0.0).all() and (w <= 1.0).all(), what
    return float((dev / tol).max())


# 1 ------------------------------------------------------------------------------------------------------------------------
def granule_pairs(dtype):
    """one pair per n of GRAN_N: the moving clouds of batch_ref.knn_models (and one point), against standard-normal models of
    GRAN_M points in turn with random unit normals"""
    movers = [np.random.default_rng(77).standard_normal((1, 3)).astype(dtype)] + knn_models(dtype)[:-1]
    assert tuple(A.shape[0] for A in movers) == GRAN_N
    pairs, nrm = [], []
    for i, A in enumerate(movers):
        m = GRAN_M[i % len(GRAN_M)]
        rng = np.random.default_rng(600 + i)
        pairs.append((A, rng.standard_normal((m, 3)).astype(dtype)))
        v = rng.standard_normal((m, 3))
        nrm.append((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype))
    return pairs, nrm


@pytest.mark.parametrize("kernel", KERNELS)
@PLANE
@DTYPES
def test_weights_at_the_granules(ctx, pkg, orc, dtype, plane, kernel):
    pairs, nrm = granule_pairs(dtype)
    if not plane:
        nrm = [None] * len(pairs)
    # the reference alone: a scale per pair at the median residual, so that both branches of Huber and Tukey are taken
    idxs = [orc.nn(A, M) for A, M in pairs]
    ks, both = [], 0
    for (A, M), idx, N in zip(pairs, idxs, nrm):
        r2 = br.residual_sq_exact(plane, A, M, idx, N)[0]
        ks.append(float(np.sqrt(np.median(r2))))
        assert ks[-1] > 0
        both += int((r2 <= ks[-1] ** 2).any() and (r2 > ks[-1] ** 2).any())
    assert both >= len(pairs) - 2   # (all but the one-point pair and at most one more)
    worst_w = worst_s = 0.0
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        bt.set_robust(kernel, ks)
        bt.begin(max_iter=2, tol=0.0, fixed_iterations=True, metric=metric_of(pkg, plane))
        assert bt.run(1)[0] == 1
        got_idx, inl, wts = bt.get_indices(), bt.get_inliers(), bt.get_weights()
        for b, ((A, M), idx, N) in enumerate(zip(pairs, idxs, nrm)):
            what = f"{kernel} pair {b}: n {A.shape[0]} m {M.shape[0]}"
            mom = bt.diag_moments(b)
            assert np.array_equal(got_idx[b], idx), what
            assert inl[b].dtype == bool and inl[b].all(), what
            assert mom[rm.CNT] == float(A.shape[0]) and mom[rm.ERR] == 0.0, what
            worst_w = max(worst_w, check_weights(plane, kernel, ks[b], A, M, N, idx, inl[b], wts[b], what))
            worst_s = max(worst_s, br.check_weighted_sums(plane, A, M, N, idx, inl[b], wts[b], mom, what))
    print(f"[robust granules] {kernel}/{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}: largest |w - formula| / bound = {worst_w:.4f}, "
          f"largest |device - exact| / tol = {worst_s:.4f}")


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["robust", "robust+gate", "robust+trim", "robust+mutual", "robust+gate+trim+mutual"])
@PLANE
@DTYPES
def test_robust_every_pass_exactly(ctx, pkg, orc, dtype, plane, mode):
    gated, trimmed, mutual = "gate" in mode, "trim" in mode, "mutual" in mode
    md, rho = (MD if gated else None), (RHO if trimmed else None)
    cases, pairs, nrm = gate_pairs(dtype, plane)
    ks = MIXED_K[plane]
    Ks = [rank(RHO, A.shape[0]) for A, _ in pairs]
    checked, worst, worst_w, kept_log = [0] * len(pairs), 0.0, 0.0, [[] for _ in pairs]
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        if gated:
            bt.set_max_distance(MD)
        if trimmed:
            bt.set_trim(RHO)
        if mutual:
            bt.set_reciprocal(True)
        bt.set_robust(MIXED, ks)
        bt.begin(max_iter=PASSES, tol=0.0, fixed_iterations=True, metric=metric_of(pkg, plane))
        prev = [None] * len(pairs)
        for k in range(PASSES + 1):
            running = ~bt.done()
            took, _ = bt.run(1)
            assert took == (1 if running.any() else 0)
            if not took:
                break
            moving, idx, inl, wts = bt.get_moving(), bt.get_indices(), bt.get_inliers(), bt.get_weights()
            revs = bt.diag_reverse() if mutual else None
            for b in np.flatnonzero(running):
                P, M = moving[b], pairs[b][1]
                N = nrm[b] if plane else None
                what = f"{mode} pair {b} {CASES[b]} {MIXED[b]} pass {k}"
                mom = bt.diag_moments(b)
                st = bt.state(b)
                # (the host solved pass k-1 on its vector with CNT <- W: the moved cloud is that solve's, bit for bit)
                check_front_end(pkg, plane, P, M, mom, st["err"][k], prev[b], what)
                if k == PASSES:   # the error-only pass matches nothing: the weights stay those of the last matching pass
                    assert bits_equal(wts[b], prev[b]["w"]), what
                    assert mom[br.MOM_W] == 0.0 and mom[rm.CNT] == 0.0, what
                    checked[b] += 1
                    continue
                # the reference, from the cloud the pass matched on (bit for bit the device's: check_front_end)
                want_idx = orc.nn(P, M)
                want_rev = orc.nn(M, P) if mutual else None
                mask, d, tau_want = combined_mask(P, M, want_idx, want_rev, md, rho, mutual=mutual)
                kept_log[b].append(int(mask.sum()))
                # the device
                assert np.array_equal(idx[b], want_idx), what
                if mutual:
                    assert np.array_equal(revs[b], want_rev), f"{what}: rev differs at {np.flatnonzero(revs[b] != want_rev)[:8]}"
                tau, kk = bt.diag_trim(b)
                if trimmed:
                    assert kk == Ks[b] and tau_bits_equal(tau, tau_want), f"{what}: tau {tau!r}, reference {float(tau_want)!r}"
                else:
                    assert (tau, kk) == (np.inf, P.shape[0]), what
                assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                worst_w = max(worst_w, check_weights(plane, MIXED[b], ks[b], P, M, N, want_idx, mask, wts[b], what))
                worst = max(worst, br.check_weighted_sums(plane, P, M, N, want_idx, mask, wts[b], mom, what))
                if MIXED[b] is None:
                    assert mom[br.MOM_W] == mom[rm.CNT], what
                prev[b] = dict(P=P, idx=want_idx, mask=mask, mom=br.with_cnt_from_w(mom), w=wts[b])
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            assert checked[b] == PASSES + 1 or bt.state(b)["status"] != pkg.capi.ICP_OK, (b, checked[b])
        if not gated:   # (no rule but the gate can empty a pass here; under the gate a pair may end early with its status)
            assert min(checked[:3]) == PASSES + 1
        assert max(checked) == PASSES + 1
    print(f"[robust moments] {mode}/{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}: kept {kept_log}, "
          f"largest |device - exact| / tol = {worst:.4f}, largest |w - formula| / bound = {worst_w:.4f}")


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", sorted(END_RUNS), ids=lambda r: f"{'plane' if r[0] else 'p2p'}-{r[1]}")
@DTYPES
def test_robust_end_to_end(ctx, pkg, orc, dtype, run):
    """all four gate cases, for both metrics: the numpy loop stays under 2e-3 on the 17-point model too (test_batch_robust_ref.py)"""
    plane, kernel = run
    k, want_its = END_RUNS[run]
    tol = 1e-6
    cases, pairs, nrm = gate_pairs(dtype, plane)
    wants = [br.robust_loop(orc, A, M, br.KINDS[kernel], k, 40, tol, nrm[b] if plane else None) for b, (A, M) in enumerate(pairs)]
    for c, w, (A, M, is_out) in zip(CASES, wants, cases):   # the reference alone
        assert br.inlier_rms(w["moved"], M, w["idx"], is_out) < 2e-3
    assert [w["iterations"] for w in wants] == want_its
    res = ctx.register_batch_robust(pairs, kernel, k, metric=metric_of(pkg, plane), normals=nrm, max_iter=40, tol=tol)
    plain = ctx.register_batch(pairs, metric=metric_of(pkg, plane), normals=nrm, max_iter=40, tol=tol)
    for c, r, p, w, (A, M, is_out) in zip(CASES, res, plain, wants, cases):
        assert r.extra["status"] == pkg.capi.ICP_OK
        rms, rms_plain = br.inlier_rms(r.moved, M, r.idx, is_out), br.inlier_rms(p.moved, M, p.idx, is_out)
        print(f"{c}: iterations {r.iterations} (reference {w['iterations']}), rel T {rel(r.T, w['T']):.3e}, inlier RMS {rms:.3e}, plain {rms_plain:.3e}")
        assert_same_run(r.iterations, r.err, r.T, w, tol, dtype == np.float32)   # err at TOL_E, T at TOL_T
        assert rms < 2e-3
        assert rms_plain > 0.3 and "weights" not in p.extra
        wt = r.extra["weights"]
        assert wt.dtype == np.float64 and wt.shape == (A.shape[0],) and (wt >= 0).all() and (wt <= 1).all()
        assert r.extra["inliers"].all() and r.extra["fitness"] == 1.0   # weights change no mask
        if kernel == "tukey":
            assert (wt[is_out] == 0.0).all() and (wt[~is_out] > 0.9).all()
        else:
            assert (wt[is_out] > 0.0).all() and wt[is_out].max() < 1e-3
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]


# 4 ------------------------------------------------------------------------------------------------------------------------
@PLANE
@DTYPES
def test_robust_off_means_off(ctx, pkg, orc, dtype, plane):
    """(a) set_robust(None) and all kinds NONE give, step by step, the bytes of a batch that was never told"""
    cases, pairs, nrm = gate_pairs(dtype, plane)
    metric = metric_of(pkg, plane)
    for off in ("null", "none", "zeros", "after"):
        with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
            for bt in (X, Y):
                if plane:
                    bt.set_model_normals(nrm)
            if off == "after":   # switched on, run, and switched off again
                Y.set_robust(MIXED, MIXED_K[plane])
                assert all(f["linl"].all() for f in run_to_end(Y, metric, max_iter=12))
                assert not all((w == 1.0).all() for w in Y.get_weights())
                Y.set_robust(None)
            elif off == "null":
                Y.set_robust(None)
            elif off == "none":
                Y.set_robust([None] * 4)          # (no scale at all: allowed where every kind is NONE)
            else:
                Y.set_robust([0, 0, 0, 0], [np.nan, -1.0, 0.0, np.inf])   # (the scale of a NONE pair is not read)
            for bt in (X, Y):
                bt.begin(max_iter=12, tol=1e-6, metric=metric)
            counts = step_together(X, Y, f"off = {off!r}")
            for b, (A, _) in enumerate(pairs):
                assert counts[b] and set(counts[b]) == {A.shape[0]}, (off, b)
                same_pair_bytes(final(X)[b], final(Y)[b], f"off = {off!r}, pair {b}")
            for wx, wy, (A, _) in zip(X.get_weights(), Y.get_weights(), pairs):   # without kernels: the kept mask as 1.0 / 0.0
                assert bits_equal(wx, wy) and bits_equal(wy, np.ones(A.shape[0]))


@pytest.mark.parametrize("gated", [False, True], ids=["no gate", "gate"])
@PLANE
@DTYPES
def test_robust_pair_without_a_kernel_keeps_its_bits(ctx, pkg, orc, dtype, plane, gated):
    """(b) with kernels Tukey, none, Cauchy, none pairs 1 and 3 have, after every step and to the end, the bytes they have in the
    same batch without kernels: w = 1.0 multiplies exactly and the rows are added in the same order.  Their vectors differ in the
    one slot the plain batch leaves 0: W, which equals CNT"""
    cases, pairs, nrm = gate_pairs(dtype, plane)
    metric = metric_of(pkg, plane)
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            if plane:
                bt.set_model_normals(nrm)
            if gated:
                bt.set_max_distance(MD)
        X.set_robust(["tukey", None, "cauchy", None], MIXED_K[plane])
        for bt in (X, Y):
            bt.begin(max_iter=12, tol=1e-6, metric=metric)
        step = 0
        while True:
            kx, ky = X.run(1), Y.run(1)   # (the robust pairs end on another pass than their plain twins: either batch may idle)
            if not kx[0] and not ky[0]:
                break
            fx, fy, wx = final(X), final(Y), X.get_weights()
            for b in (1, 3):
                what = f"step {step} pair {b}"
                same_pair_bytes(fx[b], fy[b], what)
                mx, my = X.diag_moments(b), Y.diag_moments(b)
                if fx[b]["st"]["status"] == pkg.capi.ICP_OK:
                    matched = not (mx[rm.CNT] == 0.0)   # (the error-only last pass carries neither a count nor a weight sum)
                    assert mx[br.MOM_W] == (mx[rm.CNT] if matched else 0.0) and my[br.MOM_W] == 0.0, what
                mx[br.MOM_W] = 0.0
                assert bits_equal(mx, my), what
                assert bits_equal(wx[b], fx[b]["inl"].astype(np.float64)), what
            if step == 0:
                for b in (0, 2):
                    assert not bits_equal(X.diag_moments(b), Y.diag_moments(b)), (step, b)   # (the kernels do something)
            step += 1
            assert step <= 14
        assert step >= 3 and X.done().all() and Y.done().all()


@PLANE
@DTYPES
def test_robust_pairs_are_independent(ctx, pkg, orc, dtype, plane):
    """(c) a robust pair's bytes are those of that pair in a batch of its own, in either order of the pairs, whatever the others'
    kernels, scales, flags, shares and gates; the one-call entry runs the same thing"""
    order = [0, 1, 2, 3, 0, 1]
    kinds = ["tukey", "cauchy", None, "huber", "cauchy", "tukey"]
    kk = MIXED_K[plane]
    ks = np.array([kk[0], kk[1], 1.0, kk[2], 2 * kk[1], kk[0]])
    flags = np.array([0, 1, 0, 1, 1, 0], dtype=bool)
    rho = np.array([1.0, RHO, RHO, 1.0, 0.7, 1.0])
    md = np.array([np.inf, np.inf, MD, 1.0, 1.0, np.inf])
    cases, pairs, nrm = gate_pairs(dtype, plane, order)
    metric = metric_of(pkg, plane)

    def run(sel):
        with ctx.batch([pairs[i] for i in sel]) as bt:
            if plane:
                bt.set_model_normals([nrm[i] for i in sel])
            bt.set_max_distance(md[sel])
            bt.set_trim(rho[sel])
            bt.set_reciprocal(flags[sel])
            bt.set_robust([kinds[i] for i in sel], ks[sel])
            out = run_to_end(bt, metric, max_iter=12)
            for f, w in zip(out, bt.get_weights()):
                f["w"] = w
            return out

    everything = list(range(len(pairs)))
    fwd, rev = run(everything), run(everything[::-1])[::-1]
    for i in everything:
        alone = run([i])[0]
        for other, what in ((fwd[i], "forward"), (rev[i], "reversed")):
            same_pair_bytes(alone, other, f"pair {i}, {what}")
            assert bits_equal(alone["w"], other["w"]), (i, what)
    res = ctx.register_batch_robust(pairs, kinds, ks, metric=metric, normals=nrm, max_iter=12, max_distance=md, trim=rho, reciprocal=flags)
    for i, r in enumerate(res):
        assert r.extra["status"] == fwd[i]["st"]["status"] and r.iterations == fwd[i]["st"]["iterations"] and r.passes == fwd[i]["st"]["passes"]
        assert bits_equal(r.T, fwd[i]["st"]["T"]) and bits_equal(r.err, fwd[i]["st"]["err"]) and bits_equal(r.idx, fwd[i]["idx"])
        assert bits_equal(r.moved, fwd[i]["moved"]) and bits_equal(r.extra["inliers"], fwd[i]["linl"]) and bits_equal(r.extra["weights"], fwd[i]["w"])
    assert not bits_equal(fwd[1]["st"]["T"], fwd[5]["st"]["T"])   # the same clouds, another kernel and other options


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_robust_weight_sum_zero_ends_the_pair(ctx, pkg, orc):
    """Tukey at k = 1e-3 on a pair shifted by 1: every match is kept, every weight is 0, and the pair ends with ICP_ERR_EMPTY,
    passes 0, while the others finish"""
    cases, pairs, _ = gate_pairs(np.float32, False)
    A, M = pairs[1]
    far = (A + np.float32(1.0)).astype(np.float32)
    idx = orc.nn(far, M)
    assert np.sqrt(br.residual_sq(False, far, M, idx).min()) > 2e-3   # the reference alone: nobody is within k = 1e-3
    pairs = [pairs[0], (far, M), pairs[2]]
    with ctx.batch(pairs) as bt:
        bt.set_robust(["tukey", "tukey", "cauchy"], [0.5, 1e-3, 0.05])
        out = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=40)
        wts = bt.get_weights()
        assert out[1]["st"]["status"] == pkg.capi.ICP_ERR_EMPTY and out[1]["st"]["passes"] == 0 and out[1]["st"]["iterations"] == 0
        assert out[1]["inl"].all() and (wts[1] == 0.0).all()          # kept, with weight 0
        assert bits_equal(out[1]["moved"], far)
        mom = bt.diag_moments(1)
        assert mom[rm.CNT] == float(far.shape[0]) and mom[br.MOM_W] == 0.0
        for b in (0, 2):
            assert out[b]["st"]["status"] == pkg.capi.ICP_OK and out[b]["st"]["passes"] >= 2
            assert br.inlier_rms(out[b]["moved"], pairs[b][1], out[b]["idx"], cases[b][2]) < 2e-3


def test_robust_refusals_and_state(ctx, pkg, orc):
    """refusals leave the batch as it was; a pending pass of the context is ICP_ERR_STATE; a set during a loop discards it;
    get_weights follows get_indices' errors"""
    lib = pkg.load()
    cases, pairs, _ = gate_pairs(np.float32, False)
    pairs = pairs[:3]
    P2P = pkg.ICP_POINT_TO_POINT
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    INV, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    total = sum(A.shape[0] for A, _ in pairs)
    buf = np.full(total, 7.0)

    def raw(bt, kind, scale):
        kind = np.asarray(kind, dtype=np.intc)
        scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        return lib.icp_batch_set_robust(bt._h, kind.ctypes.data_as(pi), None if scale is None else scale.ctypes.data_as(pd))

    with ctx.batch(pairs) as bt:
        assert lib.icp_batch_get_weights(bt._h, buf.ctypes.data_as(pd)) == STATE   # no loop
        assert lib.icp_batch_get_weights(bt._h, None) == INV
        bt.set_robust(["tukey", None, "cauchy"], [0.5, -1.0, 0.05])
        with pytest.raises(pkg.IcpError) as e:   # run before begin after a set
            bt.run(1)
        assert e.value.code == STATE
        bt.begin(max_iter=12)
        assert lib.icp_batch_get_weights(bt._h, buf.ctypes.data_as(pd)) == STATE   # no step yet
        assert (buf == 7.0).all()
        want = run_to_end(bt, P2P, max_iter=12)
        want_w = bt.get_weights()
        assert (want_w[1] == 1.0).all() and want_w[0].min() == 0.0 and 0.0 < want_w[2].min() < 1e-3
        bad = [([1, 7, 2], [0.5, 0.5, 0.5], "pair 1"), ([-1, 0, 0], [0.5, 0.5, 0.5], "pair 0"),
               ([1, 0, 2], [0.5, 0.5, 0.0], "pair 2"), ([1, 0, 2], [-0.5, 0.5, 0.5], "pair 0"),
               ([0, 3, 0], [0.5, np.nan, 0.5], "pair 1"), ([0, 0, 3], [0.5, 0.5, np.inf], "pair 2"),
               ([1, 1, 1], [0.5, 1e200, 1e-200], "pair 1"), ([1, 1, 1], [0.5, 0.5, 1e-200], "pair 2"),
               ([0, 2, 0], None, "pair 1")]
        for kind, scale, names in bad:
            assert raw(bt, kind, scale) == INV, (kind, scale)
            assert names in lib.icp_last_error().decode(), (kind, scale, lib.icp_last_error().decode())
            assert bt.run(1) == (0, 0)   # a refused call leaves the batch alone: its loop is still the finished one
        with pytest.raises(ValueError):
            bt.set_robust(["tukey", None])
        got = run_to_end(bt, P2P, max_iter=12)   # ... and the kernels are those set before
        for b in range(3):
            same_pair_bytes(want[b], got[b], f"pair {b}")
            assert bits_equal(bt.get_weights()[b], want_w[b])
        # a set during a loop discards it
        for v in ((MIXED[:3], MIXED_K[False][:3]), (None, None), ([None] * 3, None), ("cauchy", 0.05)):
            bt.begin(max_iter=12)
            assert bt.run(1)[0] == 1
            bt.set_robust(*v)
            for call in (lambda: bt.run(1), bt.get_weights):
                with pytest.raises(pkg.IcpError) as e:
                    call()
                assert e.value.code == STATE
    # a context with a pending pass
    A, M = pairs[0]
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with c.batch(pairs[:2]) as bt:
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            with pytest.raises(pkg.IcpError) as e:
                bt.set_robust("tukey", 0.5)
            assert e.value.code == STATE
            assert lib.icp_batch_get_weights(bt._h, buf.ctypes.data_as(pd)) == STATE
            c.loop_complete()
            bt.set_robust("tukey", 0.5)
            bt.begin(max_iter=10, tol=1e-5)
            assert bt.run(1)[0] == 1 and bt.get_weights()[0].min() == 0.0


@PLANE
@DTYPES
def test_robust_with_initial_transforms(ctx, pkg, orc, dtype, plane):
    """the robust loop from T0 is the robust loop of a batch created from the start cloud, byte for byte: weights act on residuals
    measured after the transform"""
    G = hom(rot("z", np.deg2rad(40.0)), (3.0, -2.0, 1.0))
    T_back = hom(G[:3, :3].T, -G[:3, :3].T @ G[:3, 3])
    T0F = np.eye(4)
    T0F[:3, :] = T_back[:3, :].astype(dtype).astype(np.float64)
    cases, pairs, nrm = gate_pairs(dtype, plane)
    far = [(rm.apply_rt(A, G[:3, :3], G[:3, 3]), M) for A, M in pairs]
    moved = [(rm.apply_rt(A, T_back[:3, :3], T_back[:3, 3]), M) for A, M in far]
    metric = metric_of(pkg, plane)
    with ctx.batch(far) as X, ctx.batch(moved) as Y:
        X.set_initial_transforms(T_back)
        for bt in (X, Y):
            if plane:
                bt.set_model_normals(nrm)
            bt.set_robust(MIXED, MIXED_K[plane])
        fx, fy = run_to_end(X, metric, max_iter=12), run_to_end(Y, metric, max_iter=12)
        wx, wy = X.get_weights(), Y.get_weights()
        for b in range(len(far)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}", T=compose(fy[b]["st"]["T"], T0F))
            assert bits_equal(wx[b], wy[b])
            assert fy[b]["st"]["passes"] >= 1
        assert (wx[0][cases[0][2]] == 0.0).all()   # Tukey: the outliers of the first case end with weight 0


@DTYPES
def test_robust_evaluate_between_steps_changes_nothing(ctx, pkg, orc, dtype):
    cases, pairs, nrm = gate_pairs(dtype, True)
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            bt.set_model_normals(nrm)
            bt.set_robust(MIXED, MIXED_K[True])
            bt.begin(max_iter=12, tol=1e-6, metric=pkg.ICP_POINT_TO_PLANE)
        steps = 0
        while True:
            ev = X.evaluate(max_distance=MD, metric=pkg.ICP_POINT_TO_POINT if steps & 1 else pkg.ICP_POINT_TO_PLANE, want_matches=True)
            assert len(ev) == len(pairs)
            kx, ky = X.run(1), Y.run(1)
            assert kx == ky, (steps, kx, ky)
            if not ky[0]:
                break
            fx, fy, wx, wy = final(X), final(Y), X.get_weights(), Y.get_weights()
            for b in range(len(pairs)):
                same_pair_bytes(fx[b], fy[b], f"step {steps} pair {b}")
                assert bits_equal(X.diag_moments(b), Y.diag_moments(b)) and bits_equal(wx[b], wy[b]), (steps, b)
            steps += 1
        assert steps >= 3 and X.done().all()
