"""GPU: the per-pair trimmed rejection of a batch (icp_batch_set_trim, icp_diag_batch_trim; Batch.set_trim, Batch.diag_trim,
Context.point_to_point_batch(trim=...), Context.point_to_plane_batch_gated(trim=...)).

A trimmed pair keeps, in every matching pass, the matches whose winning squared distance d is <= tau, the K-th smallest of the
pair's n distances, K = ceil(rho n): the deferred route -- matching without a decision, batch_trim_select, batch_trim_moments.

    1  the selection alone: clouds whose d spans 0 .. ~70 over 13 (fp32) and 25 (fp64) decades, so that every byte of the key
       below the top one takes (nearly) all 256 values, at cloud sizes around the block's granules, for ranks 1, 2, n/2, n-1, n
    2  ties: integer clouds whose d is 0, 1, 2 or 3 exactly, with the rank inside the group d = 1
    3  every pass exactly (the structure of test_gpu_batch_gate.test_gate_every_pass_exactly), trim alone and trim with a gate
    4  end to end against a numpy loop
    5  bits: untrimmed means untrimmed, an untrimmed pair in a batch that trims, independence of the other pairs, refusals, state,
       initial transforms

The clouds of 3 - 5 are those of test_gpu_batch_gate.py (batch_ref.gate_case).  Keeping the closest half a
numpy restatement of the loop keeps 135, 97, 578 and 34 points in every pass, ends with no outlier kept and an RMS of about
1.2e-3 in 5, 4, 5, 4 iterations; the relative gap between the K-th and the (K+1)-th smallest d never falls below 1e-4, so a
flipped mask is never rounding -- every such condition is asserted on the reference alone before the device is consulted.

Bounds: tau, every mask, index and moved cloud bit for bit; the sums at ref_moments.tolerance (derived there); T and err of the
end-to-end run at the project's 1e-5 (test_gpu_batch.py)."""
import ctypes as C

import numpy as np
import pytest

import ref_moments as rm
from batch_ref import (CASES, TOL_E, TOL_T, bits_equal, check_front_end, check_sums, compose, final, gate_case, gate_margin, hom,
                       keep_closest, kth_gap, normals_for, rank, reference_loop, rel, rho_for, rot, run_to_end, same_pair_bytes, sq_dist,
                       tau_bits_equal, tau_ref, threshold)

pytestmark = pytest.mark.gpu

MD = 0.05
RHO = 0.5
KEPT_TRIM = [135, 97, 578, 34]          # ceil(0.5 n), no ties at the K-th
KEPT_GATE_PASS0 = [29, 16, 121, 7]      # the gate decides at pass 0 ...
KEPT_GATE_LATER = [135, 97, 578, 7]     # ... the trim from pass 1 on (point-to-point, a numpy loop)
PASSES = 4
SELECT_N = [1, 63, 64, 65, 255, 256, 257, 1025, 4097, 65536]


# 1 ------------------------------------------------------------------------------------------------------------------------
def select_clouds(dtype):
    """(M, [A_n for n in SELECT_N]): A = M[pick] + v 10^u, v a unit vector, u uniform on [-6, 1] (fp32) or [-12, 1] (fp64); the
    first three points of every cloud sit exactly on model points"""
    rng = np.random.default_rng(11)
    M = rng.standard_normal((300, 3)).astype(dtype)
    lo = -6.0 if dtype == np.float32 else -12.0
    out = []
    for n in SELECT_N:
        pick = rng.integers(0, M.shape[0], n)
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        u = rng.uniform(lo, 1.0, n)
        A = (M[pick].astype(np.float64) + v * (10.0 ** u)[:, None]).astype(dtype)
        A[:min(3, n)] = M[pick[:min(3, n)]]
        out.append(A)
    return M, out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_selection_every_digit_and_granule(ctx, pkg, orc, dtype):
    M, clouds = select_clouds(dtype)
    idx = [orc.nn(A, M) for A in clouds]
    d = [sq_dist(A, M, i) for A, i in zip(clouds, idx)]
    # the reference alone: the distances exercise every round of the selection
    U = np.uint32 if dtype == np.float32 else np.uint64
    nbytes = np.dtype(U).itemsize
    for n, dn in zip(SELECT_N, d):
        assert np.isfinite(dn).all() and (dn >= 0).all() and (dn[:min(3, n)] == 0).all()
        if n < 4097:
            continue
        keys = dn.view(U)
        pos = dn[dn > 0]
        span = float(np.log10(pos.max() / pos.min()))
        per_byte = [int(np.unique((keys >> U(8 * k)) & U(255)).size) for k in range(nbytes)]
        print(f"n {n} {np.dtype(dtype).name}: d from 0 through {pos.min():.2e} to {pos.max():.2e}, values per key byte (low first) {per_byte}")
        assert dn.min() == 0 and pos.max() > 10.0
        assert span >= (12.0 if dtype == np.float32 else 24.0), span   # u spans 7 (13) decades, d twice as many
        assert min(per_byte[:-1]) >= 200, per_byte
        assert per_byte[-1] >= (20 if dtype == np.float32 else 8), per_byte
    pairs = [(A, M) for A in clouds]
    with ctx.batch(pairs) as bt:
        for which in range(5):
            Ks = [min(max([1, 2, n // 2, n - 1, n][which], 1), n) for n in SELECT_N]
            bt.set_trim([rho_for(K, n) for K, n in zip(Ks, SELECT_N)])
            bt.begin(max_iter=2, tol=0.0, fixed_iterations=True)
            assert bt.run(1)[0] == 1
            got_idx, inl = bt.get_indices(), bt.get_inliers()
            for b, (n, K) in enumerate(zip(SELECT_N, Ks)):
                what = f"n {n} K {K}"
                assert np.array_equal(got_idx[b], idx[b]), what
                tau, k = bt.diag_trim(b)
                want = tau_ref(d[b], K)
                assert k == K, (what, k)
                assert tau_bits_equal(tau, want), f"{what}: tau {tau!r}, reference {float(want)!r}"
                mask = d[b] <= want
                assert mask.sum() >= K
                assert np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                assert bt.diag_moments(b)[rm.CNT] == float(mask.sum()), what


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_keeps_every_point_tied_with_the_kth(ctx, pkg, orc, dtype):
    A = np.random.default_rng(5).integers(0, 8, (200, 3)).astype(dtype)
    g = np.arange(5) * 2
    M = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(dtype)
    idx = orc.nn(A, M)
    d = sq_dist(A, M, idx)
    # the reference alone: d is the number of odd coordinates, and rank 60 falls inside the group d = 1
    assert M.shape == (125, 3)
    assert [int((d == v).sum()) for v in (0, 1, 2, 3)] == [19, 83, 71, 27]
    K = rank(0.3, 200)
    assert K == 60 and tau_ref(d, K) == 1.0 and int((d < 1).sum()) < K < int((d <= 1).sum()) == 102
    with ctx.batch([(A, M)]) as bt:
        bt.set_trim(0.3)
        bt.begin(max_iter=2, tol=0.0, fixed_iterations=True)
        assert bt.run(1)[0] == 1
        tau, k = bt.diag_trim(0)
        assert k == 60 and tau_bits_equal(tau, dtype(1.0))
        assert np.array_equal(bt.get_indices()[0], idx)
        assert np.array_equal(bt.get_inliers()[0], d <= 1.0)
        assert bt.diag_moments(0)[rm.CNT] == 102.0


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["trim", "trim+gate"])
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_every_pass_exactly(ctx, pkg, orc, dtype, plane, gated):
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    Ks = [rank(RHO, A.shape[0]) for A, _ in pairs]
    assert Ks == KEPT_TRIM
    thr = threshold(MD, dtype)
    checked, worst, kept_log = [0] * len(pairs), 0.0, [[] for _ in pairs]
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        if gated:
            bt.set_max_distance(MD)
        bt.set_trim(RHO)
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
                want_idx = orc.nn(P, M)
                d = sq_dist(P, M, want_idx)
                # conditions on the reference alone (P is the reference's own cloud, bit for bit): no decision is a rounding
                gap = kth_gap(d, Ks[b])
                assert gap >= 1e-4, f"{what}: relative gap at the K-th distance {gap:.3e}"
                if gated:
                    margin = gate_margin(d, MD)
                    assert margin >= 1e-4, f"{what}: a distance within {margin:.3e} of the gate"
                tau_want = tau_ref(d, Ks[b])
                mask = (d <= tau_want) & ((d <= thr) if gated else True)
                kept_log[b].append(int(mask.sum()))
                if not gated:
                    assert mask.sum() == KEPT_TRIM[b], what
                elif k == 0:
                    assert mask.sum() == KEPT_GATE_PASS0[b], what
                elif not plane and b < 3:
                    # (the 63-point pair: a numpy loop stays at 7, but the 7 points kept at pass 0 make a near-degenerate 3x3
                    # system, ref_numpy.minimize and the library's solve part there, and this test follows the library's clouds)
                    assert mask.sum() == KEPT_GATE_LATER[b], what
                # the device
                assert np.array_equal(idx[b], want_idx), what
                tau, kk = bt.diag_trim(b)
                assert kk == Ks[b] and tau_bits_equal(tau, tau_want), f"{what}: tau {tau!r}, reference {float(tau_want)!r}"
                assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}"
                worst = max(worst, check_sums(plane, P, M, nrm[b] if plane else None, want_idx, mask, mom, what))
                prev[b] = dict(P=P, idx=want_idx, mask=mask, mom=mom)
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            assert checked[b] == PASSES + 1 or bt.state(b)["status"] != pkg.capi.ICP_OK, (b, checked[b])
        assert min(checked[:3]) == PASSES + 1   # the three large pairs ran every pass
    print(f"[trim moments] {'plane' if plane else 'p2p'}/{np.dtype(dtype).name}/{'gate' if gated else 'no gate'}: kept {kept_log}, "
          f"largest |device - exact| / tol = {worst:.4f}")


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_end_to_end(ctx, pkg, orc, dtype):
    tol = 1e-6
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    wants = [reference_loop(orc, A, M, keep_closest(RHO), 40, tol) for A, M, _ in cases]
    for c, w, (A, M, is_out), K in zip(CASES, wants, cases, KEPT_TRIM):   # the reference alone
        print(f"{c}: reference keeps {w['kept']}, smallest K-th gap {w['margin']:.3e}, iterations {w['iterations']}, final RMS {w['err'][-1]:.3e}")
        assert w["margin"] >= 1e-4
        assert set(w["kept"]) == {K}
        assert not (w["mask"] & is_out).any()
        assert w["err"][-1] < 2e-3
    assert [w["iterations"] for w in wants] == [5, 4, 5, 4]
    pairs = [(A, M) for A, M, _ in cases]
    res = ctx.point_to_point_batch(pairs, max_iter=40, tol=tol, trim=RHO)
    for c, r, w, (A, M, is_out), K in zip(CASES, res, wants, cases, KEPT_TRIM):
        assert r.extra["status"] == pkg.capi.ICP_OK
        print(f"{c}: iterations {r.iterations} (reference {w['iterations']}), rel T {rel(r.T, w['T']):.3e}, err {r.err}")
        assert r.iterations == w["iterations"]
        n = min(len(r.err), len(w["err"]))
        assert n == len(w["err"]) and np.abs(r.err[:n] - w["err"][:n]).max() < TOL_E
        assert rel(r.T, w["T"]) < TOL_T
        inl = r.extra["inliers"]
        assert inl.dtype == bool and inl.sum() == K and not (inl & is_out).any()
        assert r.extra["fitness"] == K / A.shape[0]
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_off_means_off(ctx, pkg, orc, dtype, plane):
    """(a) set_trim(None) and set_trim(1.0) give the bytes of a batch that never heard of trimming"""
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    pairs = [(A, M) for A, M, _ in cases]
    nrm = [normals_for(orc, M) for _, M in pairs] if plane else None
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    with ctx.batch(pairs) as bt:
        if plane:
            bt.set_model_normals(nrm)
        plain = run_to_end(bt, metric, max_iter=12)
        bt.set_trim(1.0)
        ones = run_to_end(bt, metric, max_iter=12)
        taus = [bt.diag_trim(b) for b in range(bt.count)]
        bt.set_trim(RHO)
        half = run_to_end(bt, metric, max_iter=12)
        bt.set_trim(None)
        again = run_to_end(bt, metric, max_iter=12)
    for b in range(len(pairs)):
        same_pair_bytes(plain[b], ones[b], f"1.0, pair {b}")
        same_pair_bytes(plain[b], again[b], f"None after a trimmed run, pair {b}")
        assert taus[b] == (np.inf, pairs[b][0].shape[0])
        assert plain[b]["inl"].all() and ones[b]["linl"].all() and not half[b]["linl"].all()
    assert any(not bits_equal(plain[b]["st"]["T"], half[b]["st"]["T"]) for b in range(3))   # (trimming does something)
    if not plane:   # the one-call mirror: trim=1.0 goes through the Batch object and still gives the plain bits
        for b, r in enumerate(ctx.point_to_point_batch(pairs, max_iter=12, trim=1.0)):
            assert bits_equal(r.T, plain[b]["st"]["T"]) and bits_equal(r.err, plain[b]["st"]["err"]) and bits_equal(r.idx, plain[b]["idx"])
            assert r.extra["inliers"].all() and r.extra["fitness"] == 1.0


@pytest.mark.parametrize("gated", [False, True], ids=["no gate", "gate"])
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_untrimmed_pair_keeps_its_bits(ctx, pkg, orc, dtype, plane, gated):
    """(b) in a batch [0.5, 1.0, 0.5, 1.0] pairs 1 and 3 have, after each of 3 steps, the bytes they have in a plain batch: the
    deferred route adds an untrimmed pair's rows in the fused pass's order"""
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
        X.set_trim([RHO, 1.0, RHO, 1.0])
        for bt in (X, Y):
            bt.begin(max_iter=12, tol=1e-6, metric=metric)
        for step in range(3):
            kx, ky = X.run(1), Y.run(1)
            assert kx[0] == ky[0] == 1
            fx, fy = final(X), final(Y)
            for b in (1, 3):
                what = f"step {step} pair {b}"
                same_pair_bytes(fx[b], fy[b], what)
                assert bits_equal(X.diag_moments(b), Y.diag_moments(b)), what
                assert X.diag_trim(b) == (np.inf, pairs[b][0].shape[0]), what
            for b in (0, 2):   # (the other two are trimmed; under the gate pass 0 keeps what the gate alone keeps)
                assert gated or not bits_equal(fx[b]["inl"], fy[b]["inl"]), (step, b)
                assert np.isfinite(X.diag_trim(b)[0])


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_pairs_are_independent(ctx, pkg, orc, dtype, plane):
    """(c) a trimmed pair's bytes are those of that pair in a batch of its own, in either order of the pairs"""
    order = [0, 1, 2, 3, 0, 1]
    rho = np.array([RHO, 1.0, RHO, 0.4, 0.7, RHO])
    md = np.array([np.inf, MD, MD, np.inf, MD, np.inf])
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
            return run_to_end(bt, metric, max_iter=12)

    everything = list(range(len(pairs)))
    fwd, rev = run(everything), run(everything[::-1])[::-1]
    for i in everything:
        alone = run([i])[0]
        same_pair_bytes(alone, fwd[i], f"pair {i}, forward")
        same_pair_bytes(alone, rev[i], f"pair {i}, reversed")
    # the one-call mirror runs the same thing
    res = (ctx.point_to_plane_batch_gated(pairs, md, normals=nrm, max_iter=12, trim=rho) if plane
           else ctx.point_to_point_batch(pairs, max_iter=12, max_distance=md, trim=rho))
    for i, r in enumerate(res):
        assert r.extra["status"] == fwd[i]["st"]["status"] and r.iterations == fwd[i]["st"]["iterations"] and r.passes == fwd[i]["st"]["passes"]
        assert bits_equal(r.T, fwd[i]["st"]["T"]) and bits_equal(r.err, fwd[i]["st"]["err"]) and bits_equal(r.idx, fwd[i]["idx"])
        assert bits_equal(r.moved, fwd[i]["moved"]) and bits_equal(r.extra["inliers"], fwd[i]["linl"])
    assert not bits_equal(fwd[0]["st"]["T"], fwd[4]["st"]["T"])   # the same clouds, another share and a gate


def test_trim_refusals_and_state(ctx, pkg, orc):
    """(d) a refused set_trim leaves the earlier shares in place; (e) a set_trim during a loop discards it"""
    lib = pkg.load()
    cases = [gate_case(*c) for c in CASES[:3]]
    pairs = [(A, M) for A, M, _ in cases]
    pd = C.POINTER(C.c_double)
    P2P = pkg.ICP_POINT_TO_POINT
    tau, k = C.c_double(0.0), C.c_int(0)
    with ctx.batch(pairs) as bt:
        assert lib.icp_diag_batch_trim(bt._h, 0, C.byref(tau), C.byref(k)) == pkg.capi.ICP_ERR_STATE   # no loop
        good = np.array([RHO, 1.0, 0.7])
        bt.set_trim(good)
        bt.begin(max_iter=12)
        assert lib.icp_diag_batch_trim(bt._h, 0, C.byref(tau), C.byref(k)) == pkg.capi.ICP_ERR_STATE   # no matching pass yet
        assert lib.icp_diag_batch_trim(bt._h, 3, C.byref(tau), C.byref(k)) == pkg.capi.ICP_ERR_INVALID
        want = run_to_end(bt, P2P, max_iter=12)
        assert [bt.diag_trim(b)[1] for b in range(3)] == [135, 194, rank(0.7, 1155)]
        for bad in (np.nan, 0.0, -0.5, 1.0 + 1e-12, np.inf, -np.inf):
            v = np.array([0.9, 0.9, bad])
            assert lib.icp_batch_set_trim(bt._h, v.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
            assert "pair 2" in lib.icp_last_error().decode(), lib.icp_last_error().decode()
            with pytest.raises(pkg.IcpError) as e:
                bt.set_trim(v)
            assert e.value.code == pkg.capi.ICP_ERR_INVALID
        first = np.array([0.9, 0.0, np.nan])   # the message names the FIRST offending pair
        assert lib.icp_batch_set_trim(bt._h, first.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
        assert "pair 1" in lib.icp_last_error().decode()
        assert bt.run(1) == (0, 0)   # a refused call leaves the batch alone: its loop is still the finished one
        got = run_to_end(bt, P2P, max_iter=12)    # ... and the shares are those set before
        for b in range(3):
            same_pair_bytes(want[b], got[b], f"pair {b}")
        assert not got[0]["linl"].all() and got[1]["linl"].all() and not got[2]["linl"].all()
        # a set during a loop discards it
        for v in (good, None, 1.0):
            bt.begin(max_iter=12)
            assert bt.run(1)[0] == 1
            bt.set_trim(v)
            with pytest.raises(pkg.IcpError) as e:
                bt.run(1)
            assert e.value.code == pkg.capi.ICP_ERR_STATE
            with pytest.raises(pkg.IcpError) as e:
                bt.diag_trim(0)
            assert e.value.code == pkg.capi.ICP_ERR_STATE
        bt.begin(max_iter=12)
        assert bt.run(1)[0] == 1
        with pytest.raises(ValueError):
            bt.set_trim([RHO, RHO])
    with ctx.batch(pairs[:1]) as bt:   # a batch that never held shares keeps none after a refused call
        plain = run_to_end(bt, P2P, max_iter=12)
        with pytest.raises(pkg.IcpError) as e:
            bt.set_trim(1.5)
        assert e.value.code == pkg.capi.ICP_ERR_INVALID
        same_pair_bytes(plain[0], run_to_end(bt, P2P, max_iter=12)[0])


@pytest.mark.parametrize("gated", [False, True], ids=["no gate", "gate"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_with_initial_transforms(ctx, pkg, orc, dtype, gated):
    """(f) trimming a batch that holds initial transforms is trimming a batch created from the pre-moved clouds: the distances are
    measured after the transform (the contract of icp_batch_set_initial_transforms)"""
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
            if gated:
                bt.set_max_distance(MD)
            bt.set_trim(RHO)
        fx, fy = run_to_end(X, pkg.ICP_POINT_TO_POINT, max_iter=12), run_to_end(Y, pkg.ICP_POINT_TO_POINT, max_iter=12)
        for b in range(len(far)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}", T=compose(fy[b]["st"]["T"], T0F))
            assert X.diag_trim(b) == Y.diag_trim(b)
            assert fy[b]["st"]["passes"] >= 1 and not fy[b]["linl"].all()
