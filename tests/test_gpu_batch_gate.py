"""GPU: the per-pair maximum correspondence distance of a batch (icp_batch_set_max_distance, icp_batch_get_inliers,
icp_batch_loop_inliers; Batch.set_max_distance, Context.point_to_*_batch(max_distance=...)).

The clouds are clouds.ragged_pair with a run of far outliers spliced in at point 64, so that a whole 64-point work item can be
rejected and the kept set changes from pass to pass:

    (200, 300, 70)     ragged last item
    (130, 1000, 64)    the second work item is rejected whole (its row of partials is all zeros)
    (1025, 513, 130)   19 items; model quarters that are no multiple of the tile
    (63, 17, 5)        a single short item

Gated at 0.05 a numpy restatement of the loop keeps 29 -> 200 -> 200, 16 -> 120 -> 130 -> 130 and 121 -> 1025 -> 1025 points
per pass on the first three (fp32 and fp64) and ends with exactly the non-outliers; no squared distance comes closer to the
threshold than 3e-4 relative, so a flipped mask is never rounding.  test_gate_end_to_end re-derives both from its own reference,
and asserts the margin on the reference alone, before it looks at the device.  At 0.03 all three keep nothing at pass 0.

Bounds: every mask, index and moved cloud is compared bit for bit; the sums at ref_moments.tolerance (derived there); T and err
at the project's 1e-5 (test_gpu_batch.py)."""
import ctypes as C

import numpy as np
import pytest

import ref_moments as rm
from batch_ref import (CASES, TOL_E, TOL_T, bits_equal, check_front_end, check_sums, gate_case, gate_mask, keep_within, normals_for,
                       reference_loop, rel, run_to_end, same_pair_bytes, sq_dist)

pytestmark = pytest.mark.gpu

MD = 0.05          # keeps the true picks once the clouds are roughly aligned
MD_EMPTY = 0.03    # keeps nothing at pass 0
KEPT = {(200, 300, 70): [29, 200, 200], (130, 1000, 64): [16, 120, 130, 130], (1025, 513, 130): [121, 1025, 1025]}
PASSES = 4         # matching passes of the fixed-length loops of test 1; pass PASSES is the error-only one


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gate_every_pass_exactly(ctx, pkg, orc, dtype, plane):
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    checked, worst = [0] * len(pairs), 0.0
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        bt.set_max_distance(MD)
        bt.begin(max_iter=PASSES, tol=0.0, fixed_iterations=True, metric=metric)
        prev = [None] * len(pairs)
        for k in range(PASSES + 1):
            running = ~bt.done()
            took, _ = bt.run(1)
            assert took == (1 if running.any() else 0)
            if not took:
                break
            moving, idx, inl = bt.get_moving(), bt.get_indices(), bt.get_inliers()
            for b in np.flatnonzero(running):
                P, M = moving[b], pairs[b][1]
                n = P.shape[0]
                what = f"pair {b} {CASES[b]} pass {k}"
                mom = bt.diag_moments(b)
                st = bt.state(b)
                check_front_end(pkg, plane, P, M, mom, st["err"][k], prev[b], what)
                if k == PASSES:   # the error-only pass matches nothing
                    checked[b] += 1
                    continue
                assert np.array_equal(idx[b], orc.nn(P, M)), what
                mask = gate_mask(P, M, idx[b], MD)
                assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                print(f"{what}: kept {int(mask.sum())} of {n}")
                assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}"
                worst = max(worst, check_sums(plane, P, M, nrm[b] if plane else None, idx[b], mask, mom, what))
                if not mask.any():
                    assert st["status"] == pkg.capi.ICP_ERR_EMPTY, what
                prev[b] = dict(P=P, idx=idx[b], mask=mask, mom=mom)
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            assert checked[b] == PASSES + 1 or bt.state(b)["status"] != pkg.capi.ICP_OK, (b, checked[b])
        assert max(checked[:3]) == PASSES + 1   # the gate did not end the three large pairs
    print(f"[gate moments] {'plane' if plane else 'p2p'}/{np.dtype(dtype).name}: largest |device - exact| / tol = {worst:.4f}")


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gate_end_to_end(ctx, pkg, orc, dtype):
    tol = 1e-6
    cases = [gate_case(*c, dtype=dtype) for c in CASES[:3]]
    wants = [reference_loop(orc, A, M, keep_within(MD), 40, tol) for A, M, _ in cases]
    for c, w, (A, M, is_out) in zip(CASES, wants, cases):   # the reference alone: the figures the module's docstring quotes
        print(f"{c}: reference keeps {w['kept']}, margin {w['margin']:.3e}, iterations {w['iterations']}")
        assert w["margin"] >= 1e-4
        k = min(len(w["kept"]), len(KEPT[c]))   # (the device matches once more than the reference, on the pass that stops it)
        assert k >= 3 and w["kept"][:k] == KEPT[c][:k] and set(w["kept"][k:]) <= {KEPT[c][-1]}
        assert w["kept"][0] < w["kept"][-1]     # the kept set changes between passes
        assert np.array_equal(w["mask"], ~is_out)
        assert reference_loop(orc, A, M, keep_within(MD_EMPTY), 40, tol)["kept"] == [0]
    pairs = [(A, M) for A, M, _ in cases]
    with ctx.batch(pairs) as bt:   # the kept count of every pass
        bt.set_max_distance(MD)
        bt.begin(max_iter=40, tol=tol)
        counts = [[] for _ in pairs]
        while True:
            running = ~bt.done()
            if not bt.run(1)[0]:
                break
            inl = bt.get_inliers()
            for b in np.flatnonzero(running):
                counts[b].append(int(inl[b].sum()))
        for b, w in enumerate(wants):
            st = bt.state(b)
            k = min(len(counts[b]), len(w["kept"]), st["passes"])
            assert k >= len(KEPT[CASES[b]]) - 1 and counts[b][:k] == w["kept"][:k], (CASES[b], counts[b], w["kept"])
    res = ctx.point_to_point_batch(pairs, max_iter=40, tol=tol, max_distance=MD)
    for c, r, w, (A, M, is_out) in zip(CASES, res, wants, cases):
        assert r.extra["status"] == pkg.capi.ICP_OK
        print(f"{c}: iterations {r.iterations} (reference {w['iterations']}), rel T {rel(r.T, w['T']):.3e}")
        n = min(len(r.err), len(w["err"]))
        assert np.abs(r.err[:n] - w["err"][:n]).max() < TOL_E
        if r.iterations != w["iterations"]:   # (test_gpu_batch.assert_same_run)
            assert dtype == np.float32 and abs(r.iterations - w["iterations"]) == 1, (r.iterations, w["iterations"])
            kk = min(r.iterations, w["iterations"]) + 1
            dE = abs(w["err"][kk] - w["err"][kk - 1])
            assert abs(dE - tol) < 5e-7 or abs(w["err"][kk] - tol) < 5e-7, f"stop rule disagreed away from the threshold: dE={dE}"
        assert rel(r.T, w["T"]) < TOL_T
        assert r.extra["inliers"].dtype == bool and np.array_equal(r.extra["inliers"], ~is_out)
        assert r.extra["fitness"] == (A.shape[0] - is_out.sum()) / A.shape[0]
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]


# 3, 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gate_off_means_off(ctx, pkg, orc, dtype, plane):
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        plain = run_to_end(bt, metric, max_iter=12)
        bt.set_max_distance(np.inf)
        inf = run_to_end(bt, metric, max_iter=12)
        bt.set_max_distance(MD)
        gated = run_to_end(bt, metric, max_iter=12)
        bt.set_max_distance(None)
        again = run_to_end(bt, metric, max_iter=12)
    for b in range(len(pairs)):
        assert plain[b]["inl"].all() and plain[b]["linl"].all() and inf[b]["inl"].all() and inf[b]["linl"].all()
        same_pair_bytes(plain[b], inf[b], f"+inf, pair {b}")
        same_pair_bytes(plain[b], again[b], f"None after a gated run, pair {b}")
        assert plain[b]["idx"].min() >= 0 and gated[b]["idx"].max() < pairs[b][1].shape[0] and gated[b]["idx"].min() >= 0
    assert any(not bits_equal(plain[b]["st"]["T"], gated[b]["st"]["T"]) for b in range(3))   # (the gate does something)
    if not plane:   # the one-call function has no gate: the ungated bits are its bits
        one = ctx.point_to_point_batch(pairs, max_iter=12)
        for b, r in enumerate(one):
            assert bits_equal(r.T, plain[b]["st"]["T"]) and bits_equal(r.err, plain[b]["st"]["err"]) and bits_equal(r.idx, plain[b]["idx"])


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gate_mixed_batch_and_empty_pair(ctx, pkg, orc, dtype, plane):
    """some pairs gated at 0.05, some at +inf, one at 0.03: per pair the bytes of that pair in a batch of its own, in either order;
    the pair gated at 0.03 ends empty at pass 0 and the others finish"""
    order = [0, 1, 2, 3, 0, 1]
    md = np.array([MD, np.inf, MD, MD, MD_EMPTY, MD])
    cases = [gate_case(*CASES[c], dtype=dtype) for c in order]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT

    def run(sel):
        with ctx.batch([pairs[i] for i in sel]) as bt:
            if plane:
                bt.set_model_normals([nrm[i] for i in sel])
            bt.set_max_distance(md[sel])
            return run_to_end(bt, metric, max_iter=12)

    everything = list(range(len(pairs)))
    fwd, rev = run(everything), run(everything[::-1])[::-1]
    for i in everything:
        alone = run([i])[0]
        same_pair_bytes(alone, fwd[i], f"pair {i}, forward")
        same_pair_bytes(alone, rev[i], f"pair {i}, reversed")
    # the one-call mirror runs the same thing: Result.extra carries the last contributing pass's mask and its share
    res = (ctx.point_to_plane_batch_gated(pairs, md, normals=nrm, max_iter=12) if plane else ctx.point_to_point_batch(pairs, max_iter=12, max_distance=md))
    for i, r in enumerate(res):
        assert r.extra["status"] == fwd[i]["st"]["status"] and r.iterations == fwd[i]["st"]["iterations"] and r.passes == fwd[i]["st"]["passes"]
        assert bits_equal(r.T, fwd[i]["st"]["T"]) and bits_equal(r.err, fwd[i]["st"]["err"]) and bits_equal(r.idx, fwd[i]["idx"])
        assert bits_equal(r.moved, fwd[i]["moved"]) and bits_equal(r.extra["inliers"], fwd[i]["linl"])
        assert r.extra["fitness"] == fwd[i]["linl"].sum() / fwd[i]["linl"].size
    e = fwd[4]
    assert e["st"]["status"] == pkg.capi.ICP_ERR_EMPTY
    assert e["st"]["iterations"] == 0 and e["st"]["passes"] == 0
    assert np.array_equal(e["st"]["T"], np.eye(4)) and e["st"]["err"].tolist() == [0.0]
    assert bits_equal(e["moved"], pairs[4][0])
    assert not e["inl"].any() and not e["linl"].any()
    assert np.array_equal(e["idx"], orc.nn(*pairs[4]))   # idx is the nearest neighbour, kept or not
    for i in (0, 1, 2, 5):
        assert fwd[i]["st"]["status"] == pkg.capi.ICP_OK, i
    assert fwd[1]["inl"].all()
    if not plane:
        assert np.array_equal(fwd[0]["linl"], ~cases[0][2]) and np.array_equal(fwd[2]["linl"], ~cases[2][2])


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gate_on_the_threshold(ctx, pkg, orc, dtype):
    A, M, _ = gate_case(*CASES[0], dtype=dtype)
    F = np.dtype(dtype).type
    idx = orc.nn(A, M)
    d = sq_dist(A, M, idx)
    found = None
    for i in np.argsort(d):   # a point whose own d, and F's next value below it, are both some (F)(md * md) (in fp64 not every d is)
        md = float(np.sqrt(np.float64(d[i])))
        root = float(np.sqrt(np.float64(np.nextafter(d[i], F(0)))))
        lower = [b for b in (root, float(np.nextafter(root, 0.0)), float(np.nextafter(root, np.inf))) if F(b * b) == np.nextafter(d[i], F(0))]
        if md > 0 and F(md * md) == d[i] and lower:
            found = (int(i), md, lower[0])
            break
    assert found is not None
    i, md, below = found
    assert F(md * md) == d[i]
    assert F(below * below) == np.nextafter(d[i], F(0)) < d[i]
    with ctx.batch([(A, M), (A, M)]) as bt:
        bt.set_max_distance([md, below])
        bt.begin(max_iter=3, tol=0.0, fixed_iterations=True)
        assert bt.run(1)[0] == 1
        on, under = bt.get_inliers()
        got = bt.get_indices()
    assert np.array_equal(got[0], idx) and np.array_equal(got[1], idx)
    assert on[i] and not under[i]
    assert np.array_equal(on, d <= d[i]) and np.array_equal(under, d < d[i])


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_gate_refusals(ctx, pkg, orc):
    lib = pkg.load()
    cases = [gate_case(*c) for c in CASES[:2]]
    pairs = [(A, M) for A, M, _ in cases]
    pd, pu8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    total = sum(A.shape[0] for A, _ in pairs)
    buf = np.zeros(total, dtype=np.uint8)
    with ctx.batch(pairs) as bt:
        for fn in (lib.icp_batch_get_inliers, lib.icp_batch_loop_inliers):   # nothing to read before the first pass
            assert fn(bt._h, buf.ctypes.data_as(pu8)) == pkg.capi.ICP_ERR_STATE
        bt.set_max_distance([MD, np.inf])
        bt.begin(max_iter=12)
        for fn in (lib.icp_batch_get_inliers, lib.icp_batch_loop_inliers):
            assert fn(bt._h, buf.ctypes.data_as(pu8)) == pkg.capi.ICP_ERR_STATE
        bt.run(1)
        assert lib.icp_batch_get_inliers(bt._h, None) == pkg.capi.ICP_ERR_INVALID
        assert lib.icp_batch_loop_inliers(bt._h, None) == pkg.capi.ICP_ERR_INVALID
        want = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)
        for bad in (np.nan, 0.0, -0.05, -np.inf):
            for where in (0, 1):
                v = np.array([MD, np.inf])
                v[where] = bad
                assert lib.icp_batch_set_max_distance(bt._h, v.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
                assert f"pair {where}" in lib.icp_last_error().decode()
        assert bt.run(1) == (0, 0)   # a refused call leaves the batch alone: its loop is still the finished one
        got = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)   # ... and the thresholds are those set before
        for b in range(2):
            same_pair_bytes(want[b], got[b], f"pair {b}")
        assert not got[0]["linl"].all() and got[1]["linl"].all()
        # a set during a loop discards it
        bt.begin(max_iter=12)
        assert bt.run(1)[0] == 1
        bt.set_max_distance([MD, MD])
        with pytest.raises(pkg.IcpError) as e:
            bt.run(1)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        bt.begin(max_iter=12)
        assert bt.run(1)[0] == 1
        bt.set_max_distance(None)
        with pytest.raises(pkg.IcpError) as e:
            bt.run(1)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        with pytest.raises(ValueError):
            bt.set_max_distance([MD, MD, MD])
    with ctx.batch(pairs[:1]) as bt:   # a batch that never held thresholds keeps none after a refused call
        plain = run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)
        with pytest.raises(pkg.IcpError) as e:
            bt.set_max_distance(-1.0)
        assert e.value.code == pkg.capi.ICP_ERR_INVALID
        same_pair_bytes(plain[0], run_to_end(bt, pkg.ICP_POINT_TO_POINT, max_iter=12)[0])
