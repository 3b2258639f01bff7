"""GPU: the evaluation of a batch at the pose it stands at (icp_batch_evaluate, icp_diag_batch_eval_moments; Batch.evaluate,
Batch.diag_eval_moments): per-pair fitness, inlier RMSE and information matrix.

The clouds are batch_ref.CASES through gate_case -- (200, 300, 70) a ragged last item, (130, 1000, 64) a work item rejected whole,
(1025, 513, 130) 19 items and model quarters that are no tile multiple, (63, 17, 5) one short item -- plus a pair of one point
and one model point.  At the uploaded pose a distance of 0.05 keeps 29, 16, 121 and 7 of their points and 0.03 keeps none, and no
squared distance of a gated pair comes closer to its threshold than 3e-4 relative (batch_ref, test_gpu_batch_gate.py): both are
asserted on the reference before the device is looked at, so a flipped mask is never rounding.

Bounds: indices, masks, counts and every output formed on the host (information, fitness, rmse against batch_eval_ref.assemble of
the device's own vector) are compared bit for bit; the vector's slots against exact sums at batch_eval_ref.tolerance = 2 (n + 16)
2^-53 A_s (derived there, from ref_moments); everything "the loop does not notice" and "a pair's bits are its own" byte for byte.

Measured on the MI355X, largest |device - exact| / tol over all slots, pairs and variants: 0.0094 at begin, 0.0084 after a
registration (each test prints its own figure, [eval ...])."""
import ctypes as C

import numpy as np
import pytest

import batch_eval_ref as er
from batch_ref import (CASES, apply, bits_equal, final, gate_case, gate_margin, gate_mask, hom, inv_rigid, keep_within, normals_for,
                       reference_loop, rot, run_to_end, same_pair_bytes, sq_dist)

pytestmark = pytest.mark.gpu

MD = 0.05
MD_EMPTY = 0.03
MD_ONE = 0.02                                   # the 1 x 1 pair: its only distance is 0.01
BEGIN_MD = (MD, MD, np.inf, MD_EMPTY, MD_ONE)   # per pair, at begin
KEPT_AT_BEGIN = (29, 16, None, 0, 1)            # on the reference; the third pair is not gated there
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
METRICS = pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
_CACHE = {}


def five_pairs(orc, dtype):
    """([(A, M)], [normals], [is_out]) of the four gate cases and the 1 x 1 pair; computed once per dtype and never changed"""
    key = np.dtype(dtype).name
    if key not in _CACHE:
        cases = [gate_case(*c, dtype=dtype) for c in CASES]
        pairs = [(A, M) for A, M, _ in cases]
        nrm = [normals_for(orc, M) for _, M in pairs]
        pairs.append((np.array([[0.1, 0.2, 0.3]], dtype=dtype), np.array([[0.11, 0.2, 0.3]], dtype=dtype)))
        nrm.append(np.array([[0.0, 0.0, 1.0]], dtype=dtype))   # (a model of one point has no neighbours to estimate a normal from)
        _CACHE[key] = (pairs, nrm, [o for _, _, o in cases] + [np.zeros(1, dtype=bool)])
    return _CACHE[key]


def metric_of(pkg, plane):
    return pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT


def reference_matches(orc, P, M, md):
    """(idx, mask, margin) on the reference alone: the oracle's neighbours, the gate as numpy states it (None: everything)"""
    idx = orc.nn(P, M)
    if md is None or np.isinf(md):
        return idx, np.ones(len(P), dtype=bool), np.inf
    d = sq_dist(P, M, idx)
    return idx, gate_mask(P, M, idx, md), gate_margin(d, md)


def check_pair(pkg, bt, b, res, P, M, nrm, plane, idx, mask, what):
    """one pair of one evaluation against the reference matches (idx, mask): matches bit for bit, the device's vector within the
    derived tolerance of the exact sums, every host-formed output the Python assembly of that vector bit for bit.  Returns the
    largest |device - exact| / tol"""
    n = len(P)
    r = res[b]
    assert r["status"] == pkg.capi.ICP_OK, what
    assert r["idx"].dtype == np.int32 and np.array_equal(r["idx"], idx), f"{what}: idx differs at {np.flatnonzero(r['idx'] != idx)[:8]}"
    assert r["inliers_mask"].dtype == bool and np.array_equal(r["inliers_mask"], mask), f"{what}: mask differs at {np.flatnonzero(r['inliers_mask'] != mask)[:8]}"
    assert r["inliers"] == int(mask.sum()), what
    vec = bt.diag_eval_moments(b)
    want, maj = er.exact(P, M, idx, mask, plane=plane, nrm=nrm)
    tol = er.tolerance(maj, n)
    slots = (er.SD, er.CNT) + (er.PLANE_SLOTS if plane else er.POINT_SLOTS)
    worst = 0.0
    for s in range(er.NMOM):
        if s not in slots:
            assert vec[s] == 0.0, f"{what}: slot {s} is {vec[s]!r}, not 0"
            continue
        dev = abs(vec[s] - want[s])
        assert dev <= tol[s], f"{what}: slot {s} device {vec[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
        if tol[s] > 0:
            worst = max(worst, dev / tol[s])
    assert vec[er.CNT] == float(mask.sum()), what
    asm = er.assemble(vec, n, plane=plane)
    assert r["inliers"] == asm["inliers"], what
    assert bits_equal(np.float64(r["fitness"]), np.float64(asm["fitness"])), (what, r["fitness"], asm["fitness"])
    assert bits_equal(np.float64(r["rmse"]), np.float64(asm["rmse"])), (what, r["rmse"], asm["rmse"])
    assert r["information"].shape == (6, 6) and r["information"].dtype == np.float64
    assert bits_equal(r["information"], asm["information"]), what
    assert bits_equal(r["information"], np.ascontiguousarray(r["information"].T)), what
    if not mask.any():
        assert not vec.any() and not r["information"].any() and r["rmse"] == 0.0 and r["fitness"] == 0.0, what
    return worst


def check_batch(pkg, orc, bt, pairs, nrm, plane, mds, what):
    """evaluate(want_matches) of the whole batch where its clouds stand, every pair through check_pair; mds: per pair, or None"""
    P = bt.get_moving()
    refs = [reference_matches(orc, P[b], M, None if mds is None else mds[b]) for b, (_, M) in enumerate(pairs)]
    for b, (_, _, margin) in enumerate(refs):   # the reference alone: no decision sits on its threshold
        assert margin >= 3e-4, (what, b, margin)
    res = bt.evaluate(max_distance=None if mds is None else np.array(mds, dtype=np.float64), metric=metric_of(pkg, plane), want_matches=True)
    assert len(res) == len(pairs)
    worst = 0.0
    for b, (_, M) in enumerate(pairs):
        idx, mask, _ = refs[b]
        worst = max(worst, check_pair(pkg, bt, b, res, P[b], M, nrm[b] if plane else None, plane, idx, mask, f"{what} pair {b}"))
    return res, refs, worst


# 1 ------------------------------------------------------------------------------------------------------------------------
@METRICS
@DTYPES
def test_eval_at_begin_against_exact_sums(ctx, pkg, orc, dtype, plane):
    pairs, nrm, _ = five_pairs(orc, dtype)
    what = f"{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}"
    for b, (A, M) in enumerate(pairs):   # the reference alone, at the uploaded pose: what the module's docstring quotes
        _, mask, margin = reference_matches(orc, A, M, BEGIN_MD[b])
        assert margin >= 3e-4, (b, margin)
        if KEPT_AT_BEGIN[b] is not None:
            assert int(mask.sum()) == KEPT_AT_BEGIN[b], (b, int(mask.sum()))
    assert not reference_matches(orc, *pairs[3], MD_EMPTY)[1].any()   # 0.03 keeps nothing at pass 0
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        bt.begin(max_iter=5, metric=metric_of(pkg, plane))
        for b, got in enumerate(bt.get_moving()):
            assert bits_equal(got, pairs[b][0]), b
        res, _, w_gated = check_batch(pkg, orc, bt, pairs, nrm, plane, BEGIN_MD, f"{what} gated")
        assert [r["inliers"] for r in res][:2] == list(KEPT_AT_BEGIN[:2]) and res[2]["inliers"] == len(pairs[2][0])
        assert res[3]["inliers"] == 0 and res[3]["status"] == pkg.capi.ICP_OK and res[3]["rmse"] == 0.0
        assert res[4]["inliers"] == 1 and res[4]["fitness"] == 1.0
        res, _, w_all = check_batch(pkg, orc, bt, pairs, nrm, plane, None, f"{what} NULL")
        assert [r["inliers"] for r in res] == [len(A) for A, _ in pairs]
        assert all(r["fitness"] == 1.0 for r in res)
        plain = bt.evaluate(metric=metric_of(pkg, plane))   # without the matches: the same numbers, no idx and no mask
        for r, q in zip(res, plain):
            assert set(q) == {"status", "inliers", "fitness", "rmse", "information"}
            assert q["inliers"] == r["inliers"] and q["rmse"] == r["rmse"] and bits_equal(q["information"], r["information"])
        st = bt.state(0)
        assert st["passes"] == 0 and st["err"].tolist() == [0.0] and not bt.done().any()   # nothing ran
    print(f"[eval at begin] {what}: largest |device - exact| / tol = {max(w_gated, w_all):.4f}")


# 2 ------------------------------------------------------------------------------------------------------------------------
@METRICS
@DTYPES
def test_eval_after_a_registration(ctx, pkg, orc, dtype, plane):
    pairs, nrm, is_out = five_pairs(orc, dtype)
    what = f"{'plane' if plane else 'p2p'}/{np.dtype(dtype).name}"
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        bt.set_max_distance(MD)
        fin = run_to_end(bt, metric_of(pkg, plane), max_iter=40, tol=1e-6)
        assert bt.done().all()
        print(f"[eval after run] {what}: status {[f['st']['status'] for f in fin]}, passes {[f['st']['passes'] for f in fin]}")
        P = bt.get_moving()
        for b in range(len(pairs)):
            assert bits_equal(P[b], fin[b]["moved"]), b
        for b in range(3):   # the reference alone, at the final pose: exactly the non-outliers are within the distance
            _, mask, _ = reference_matches(orc, P[b], pairs[b][1], MD)
            assert np.array_equal(mask, ~is_out[b]), (what, b, int(mask.sum()), int((~is_out[b]).sum()))
        res, _, worst = check_batch(pkg, orc, bt, pairs, nrm, plane, [MD] * len(pairs), what)
        for b, (n, _, n_out) in enumerate(CASES[:3]):
            assert res[b]["inliers"] == n
            assert bits_equal(np.float64(res[b]["fitness"]), np.float64(n) / np.float64(n + n_out)), (what, b)
            assert 0.0 < res[b]["rmse"] < 0.01
        after = final(bt)   # the ended loop answers as before the evaluation
        for b in range(len(pairs)):
            same_pair_bytes(after[b], fin[b], f"{what} pair {b} after the evaluation")
    print(f"[eval after run] {what}: largest |device - exact| / tol = {worst:.4f}")


# 3 ------------------------------------------------------------------------------------------------------------------------
def loop_snapshot(pkg, bt):
    """everything a caller can read of the loop between two steps, as bytes (or the error code that refuses it)"""
    out = []
    for name, fn in (("indices", bt.get_indices), ("inliers", bt.get_inliers), ("moving", bt.get_moving), ("done", bt.done)):
        try:
            v = fn()
            out.append((name, [np.ascontiguousarray(a).tobytes() for a in v] if isinstance(v, list) else v.tobytes()))
        except pkg.IcpError as e:
            out.append((name, e.code))
    for b in range(bt.count):
        for name, fn in (("moments", bt.diag_moments), ("trim", bt.diag_trim)):
            try:
                v = fn(b)
                out.append((name, b, v.tobytes() if isinstance(v, np.ndarray) else (np.float64(v[0]).tobytes(), v[1])))
            except pkg.IcpError as e:
                out.append((name, b, e.code))
        st = bt.state(b)
        out.append(("state", b, st["status"], st["iterations"], st["passes"], st["err"].tobytes(), st["T"].tobytes()))
    return out


@DTYPES
def test_eval_the_loop_does_not_notice(ctx, pkg, orc, dtype):
    pairs, nrm, _ = five_pairs(orc, dtype)
    pairs, nrm = pairs[:4], nrm[:4]
    other_md = np.array([0.07, np.inf, 0.02, 0.2])
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            bt.set_model_normals(nrm)
            bt.set_max_distance(MD)
            bt.set_trim(0.8)
            bt.begin(max_iter=12, tol=1e-6, metric=pkg.ICP_POINT_TO_PLANE)
        steps = 0
        while True:
            X.evaluate(max_distance=other_md, metric=pkg.ICP_POINT_TO_POINT, want_matches=bool(steps & 1))   # the other metric, another distance
            X.evaluate(metric=pkg.ICP_POINT_TO_PLANE)
            sx, sy = loop_snapshot(pkg, X), loop_snapshot(pkg, Y)
            assert sx == sy, (steps, [a[:2] for a, c in zip(sx, sy) if a != c])
            kx, ky = X.run(1), Y.run(1)
            assert kx == ky, (steps, kx, ky)
            if not ky[0]:
                break
            steps += 1
        assert steps >= 3 and X.done().all()
        fx, fy = final(X), final(Y)
        for b in range(len(pairs)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}")
        assert loop_snapshot(pkg, X) == loop_snapshot(pkg, Y)
    print(f"[eval unnoticed] {np.dtype(dtype).name}: {steps} steps, evaluated before each, passes {[f['st']['passes'] for f in fy]}")


# 4 ------------------------------------------------------------------------------------------------------------------------
def eval_bytes(bt, b, res):
    return (bt.diag_eval_moments(b).tobytes(), res[b]["idx"].tobytes(), res[b]["inliers_mask"].tobytes(), res[b]["information"].tobytes(),
            res[b]["inliers"], np.float64(res[b]["fitness"]).tobytes(), np.float64(res[b]["rmse"]).tobytes())


@METRICS
@DTYPES
def test_eval_a_pairs_bits_are_its_own(ctx, pkg, orc, dtype, plane):
    pairs, nrm, _ = five_pairs(orc, dtype)
    metric = metric_of(pkg, plane)
    order = list(range(len(pairs)))[::-1]

    def run(sel):
        with ctx.batch([pairs[i] for i in sel]) as bt:
            if plane:
                bt.set_model_normals([nrm[i] for i in sel])
            bt.begin(max_iter=5, metric=metric)
            res = bt.evaluate(max_distance=np.array([BEGIN_MD[i] for i in sel]), metric=metric, want_matches=True)
            return [eval_bytes(bt, k, res) for k in range(len(sel))]

    together = run(order)
    for k, i in enumerate(order):
        alone = run([i])[0]
        assert alone == together[k], f"pair {i}: alone and in the reversed batch of five differ in {[j for j, (a, c) in enumerate(zip(alone, together[k])) if a != c]}"
    assert together[0][0] != together[1][0]


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_eval_scores_hypotheses_without_iterations(ctx, pkg, orc):
    dtype = np.float32
    A, M, _ = gate_case(*CASES[0], dtype=dtype)
    good = reference_loop(orc, A, M, keep_within(MD), 40, 1e-6)["T"]
    Ts = np.array([np.eye(4), good, hom(rot("z", 0.5), (1.0, 0.0, 0.0)), hom(rot("x", -0.3), (0.0, 0.5, -0.5))])
    moved = [A if k == 0 else apply(A, T) for k, T in enumerate(Ts)]
    kept = [int(reference_matches(orc, P, M, MD)[1].sum()) for P in moved]   # the reference alone
    print(f"[eval hypotheses] the reference keeps {kept} of {len(A)} at identity, the good pose and two wrong poses")
    assert kept[1] > max(kept[0], kept[2], kept[3])
    with ctx.batch([(A, M)] * 4) as X, ctx.batch([(P, M) for P in moved]) as Y:
        X.set_initial_transforms(Ts)
        for bt in (X, Y):
            bt.begin(max_iter=5)
        rx, ry = (bt.evaluate(max_distance=MD, want_matches=True) for bt in (X, Y))
        for k in range(4):
            assert eval_bytes(X, k, rx) == eval_bytes(Y, k, ry), k
            assert rx[k]["inliers"] == kept[k] and rx[k]["status"] == pkg.capi.ICP_OK
            assert X.state(k)["passes"] == 0
        assert int(np.argmax([r["fitness"] for r in rx])) == 1


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_eval_refusals_and_edges(ctx, pkg, orc):
    dtype = np.float32
    pairs, nrm, _ = five_pairs(orc, dtype)
    pairs = pairs[:2]
    lib, pd, cap = pkg.capi.load(), C.POINTER(C.c_double), pkg.capi

    def refused(bt, code, **kw):
        with pytest.raises(pkg.IcpError) as e:
            bt.evaluate(**kw)
        assert e.value.code == code, (e.value.code, code, kw)
        return str(e.value)

    with ctx.batch(pairs) as bt:
        refused(bt, cap.ICP_ERR_STATE)                               # before begin
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_eval_moments(0)                                  # before any evaluation
        assert e.value.code == cap.ICP_ERR_STATE
        bt.begin(max_iter=5)
        refused(bt, cap.ICP_ERR_INVALID, metric=cap.ICP_POINT_TO_PLANE)   # no normals
        refused(bt, cap.ICP_ERR_INVALID, metric=7)
        with pytest.raises(pkg.IcpError):
            bt.diag_eval_moments(0)                                  # a refused call is no evaluation
        first = bt.evaluate(max_distance=MD)
        before = [bt.diag_eval_moments(b) for b in range(2)]
        assert first[0]["inliers"] == KEPT_AT_BEGIN[0] and first[1]["inliers"] == KEPT_AT_BEGIN[1]
        for bad, who in (([MD, np.nan], "pair 1"), ([0.0, MD], "pair 0"), ([MD, -np.inf], "pair 1"), ([-1.0, np.nan], "pair 0")):
            assert who in refused(bt, cap.ICP_ERR_INVALID, max_distance=bad), (bad, who)
            for b in range(2):
                assert bits_equal(bt.diag_eval_moments(b), before[b]), (bad, b)
        with pytest.raises(ValueError):
            bt.evaluate(max_distance=[MD, MD, MD])
        # every output pointer NULL
        assert lib.icp_batch_evaluate(bt._h, cap.ICP_POINT_TO_POINT, None, None, None, None, None, None, None, None) == cap.ICP_OK
        assert bt.diag_eval_moments(0)[er.CNT] == len(pairs[0][0])
        md = np.array([MD, np.inf])
        assert lib.icp_batch_evaluate(bt._h, cap.ICP_POINT_TO_POINT, md.ctypes.data_as(pd), None, None, None, None, None, None, None) == cap.ICP_OK
        assert bits_equal(bt.diag_eval_moments(0), before[0])
        assert bt.run(1)[0] == 1                                     # the loop is still there
        bt.evaluate(max_distance=MD)
        bt.set_max_distance(MD)                                      # discards the loop
        refused(bt, cap.ICP_ERR_STATE, max_distance=MD)
        bt.begin(max_iter=5)
        assert bt.evaluate(max_distance=MD)[0]["inliers"] == KEPT_AT_BEGIN[0]
        bt.set_model_normals(nrm[:2])                                # so does this
        refused(bt, cap.ICP_ERR_STATE, metric=cap.ICP_POINT_TO_PLANE)
        bt.begin(max_iter=5)                                         # a point-to-point loop of a batch that holds normals: either metric
        assert bt.evaluate(metric=cap.ICP_POINT_TO_PLANE)[1]["inliers"] == len(pairs[1][0])
    # a pair pushed out of fp32 range by its initial transform is not evaluated; the other pair of the batch is
    big = np.eye(4)
    big[:3, :3] *= 3e38
    with np.errstate(over="ignore", invalid="ignore"):
        assert not np.isfinite(apply(pairs[1][0], big)).all()
    T_back = inv_rigid(hom(rot("z", np.deg2rad(40.0)), (3.0, -2.0, 1.0)))
    with ctx.batch(pairs) as bt, ctx.batch(pairs[:1]) as alone:
        bt.set_initial_transforms(np.array([T_back, big]))
        alone.set_initial_transforms(T_back)
        for x in (bt, alone):
            x.begin(max_iter=5)
        assert bt.state(1)["status"] == cap.ICP_ERR_INVALID
        res, want = bt.evaluate(max_distance=np.inf, want_matches=True), alone.evaluate(max_distance=np.inf, want_matches=True)
        assert res[1]["status"] == cap.ICP_ERR_INVALID and res[1]["inliers"] == 0 and res[1]["fitness"] == 0.0 and res[1]["rmse"] == 0.0
        assert not res[1]["information"].any() and not res[1]["idx"].any() and not res[1]["inliers_mask"].any()
        assert not bt.diag_eval_moments(1).any()
        assert res[0]["status"] == cap.ICP_OK and res[0]["inliers"] == len(pairs[0][0])
        assert eval_bytes(bt, 0, res) == eval_bytes(alone, 0, want)
