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

The clouds of 3 - 5 are those of test_gpu_batch_gate.py (gate_case and sq_dist are copied from there).  Keeping the closest half a
numpy restatement of the loop keeps 135, 97, 578 and 34 points in every pass, ends with no outlier kept and an RMS of about
1.2e-3 in 5, 4, 5, 4 iterations; the relative gap between the K-th and the (K+1)-th smallest d never falls below 1e-4, so a
flipped mask is never rounding -- every such condition is asserted on the reference alone before the device is consulted.

Bounds: tau, every mask, index and moved cloud bit for bit; the sums at ref_moments.tolerance (derived there); T and err of the
end-to-end run at the project's 1e-5 (test_gpu_batch.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import ref_moments as rm
import ref_numpy
from clouds import ragged_pair

pytestmark = pytest.mark.gpu

TOL_T = 1e-5
TOL_E = 1e-5
MD = 0.05
RHO = 0.5
CASES = [(200, 300, 70), (130, 1000, 64), (1025, 513, 130), (63, 17, 5)]
KEPT_TRIM = [135, 97, 578, 34]          # ceil(0.5 n), no ties at the K-th
KEPT_GATE_PASS0 = [29, 16, 121, 7]      # the gate decides at pass 0 ...
KEPT_GATE_LATER = [135, 97, 578, 7]     # ... the trim from pass 1 on (point-to-point, a numpy loop)
PASSES = 4
SELECT_N = [1, 63, 64, 65, 255, 256, 257, 1025, 4097, 65536]


# ---- helpers (gate_case, sq_dist: copies of test_gpu_batch_gate.py's) ------------------------------------------------------
def gate_case(n, m, n_out, dtype=np.float32):
    """(A, M, is_out): ragged_pair(n, m) with n_out far points as one run starting at point 64 (or behind a shorter cloud)"""
    D, M = ragged_pair(n * 1000 + m, n, m)
    O = (np.random.default_rng(n * 1000 + m + 7).standard_normal((n_out, 3)) * 0.5 + np.array([6.0, -5.0, 4.0])).astype(np.float32)
    A = np.concatenate([D[:64], O, D[64:]])
    is_out = np.zeros(n + n_out, dtype=bool)
    is_out[min(64, n):min(64, n) + n_out] = True
    return A.astype(dtype), M.astype(dtype), is_out


def sq_dist(P, M, idx):
    """the winning squared distance as the matching holds it: (dx*dx + dy*dy) + dz*dz, every operation rounded in P's dtype"""
    G = M[idx]
    dx, dy, dz = P[:, 0] - G[:, 0], P[:, 1] - G[:, 1], P[:, 2] - G[:, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == P.dtype
    return d


def threshold(md, dtype):
    return np.dtype(dtype).type(float(md) * float(md))


def rank(rho, n):
    """K = ceil(rho * (double)n), clamped to [1, n]"""
    return min(max(int(math.ceil(float(rho) * float(n))), 1), n)


def rho_for(K, n):
    """a share that gives rank K: (K - 0.5) / n, or 1 - 1e-9 for K = n (1.0 itself would mean: not trimmed)"""
    r = 1.0 - 1e-9 if K == n else (K - 0.5) / n
    assert rank(r, n) == K and r < 1.0
    return r


def tau_ref(d, K):
    return np.partition(d, K - 1)[K - 1]


def kth_gap(d, K):
    """relative gap between the K-th and the (K+1)-th smallest d (inf where K = n)"""
    s = np.sort(d.astype(np.float64))
    return np.inf if K >= s.size else float((s[K] - s[K - 1]) / s[K])


def same_bits(dev_tau, want):
    """the device's tau, read back in double, is the value `want` of the batch's dtype bit for bit"""
    return np.float64(dev_tau).tobytes() == np.float64(want).tobytes()


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def normals_for(orc, M):
    M32 = np.asarray(M, dtype=np.float32)
    return orc.normals(M32, orc.knn4(M32))[0].astype(M.dtype)


def final(bt):
    idx, moved, inl, linl = bt.loop_indices(), bt.get_moving(), bt.get_inliers(), bt.loop_inliers()
    return [dict(st=bt.state(b), idx=idx[b], moved=moved[b], inl=inl[b], linl=linl[b]) for b in range(bt.count)]


def run_to_end(bt, metric, max_iter=12, tol=1e-6):
    bt.begin(max_iter=max_iter, tol=tol, metric=metric)
    while bt.run(1 << 20)[1]:
        pass
    return final(bt)


def same_pair_bytes(a, b, what="", T=None):
    for f in ("status", "iterations", "passes"):
        assert a["st"][f] == b["st"][f], (what, f, a["st"][f], b["st"][f])
    assert bits_equal(a["st"]["err"], b["st"]["err"]), (what, "err")
    assert bits_equal(a["st"]["T"], b["st"]["T"] if T is None else T), (what, "T")
    for f in ("idx", "moved", "inl", "linl"):
        assert bits_equal(a[f], b[f]), (what, f)


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
                assert same_bits(tau, want), f"{what}: tau {tau!r}, reference {float(want)!r}"
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
        assert k == 60 and same_bits(tau, dtype(1.0))
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
    ulp = np.finfo(np.float64).eps
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
                pv = prev[b]
                if pv is not None:   # the transform front end: P_k from P_{k-1} and the host solve of pass k-1's vector
                    R, t = (pkg.solve_point_to_plane(pv["mom"])[:2] if plane else pkg.solve_point_to_point(pv["mom"]))
                    assert bits_equal(P, rm.apply_rt(pv["P"], R, t)), what
                    want_err = rm.sq_error(P[pv["mask"]], M, pv["idx"][pv["mask"]])
                    tol_err = rm.tolerance(np.full(rm.NMOM, want_err), n)[rm.ERR]
                    assert abs(mom[rm.ERR] - want_err) <= tol_err, f"{what}: ERR {mom[rm.ERR]!r} exact {want_err!r} tol {tol_err:.3e}"
                    e = np.sqrt(mom[rm.ERR]) / np.sqrt(float(pv["mask"].sum()))
                    assert abs(st["err"][k] - e) <= 4 * ulp * e, what
                else:
                    assert mom[rm.ERR] == 0.0, what
                if k == PASSES:   # the error-only pass matches nothing
                    checked[b] += 1
                    continue
                want_idx = orc.nn(P, M)
                d = sq_dist(P, M, want_idx)
                # conditions on the reference alone (P is the reference's own cloud, bit for bit): no decision is a rounding
                gap = kth_gap(d, Ks[b])
                assert gap >= 1e-4, f"{what}: relative gap at the K-th distance {gap:.3e}"
                if gated:
                    margin = float(np.abs(d.astype(np.float64) - float(thr)).min() / float(thr))
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
                assert kk == Ks[b] and same_bits(tau, tau_want), f"{what}: tau {tau!r}, reference {float(tau_want)!r}"
                assert inl[b].dtype == bool and np.array_equal(inl[b], mask), f"{what}: mask differs at {np.flatnonzero(inl[b] != mask)[:8]}"
                assert mom[rm.CNT] == float(mask.sum()), f"{what}: CNT {mom[rm.CNT]!r}"
                want, maj = (rm.plane(P[mask], M, nrm[b], want_idx[mask]) if plane else rm.p2p(P[mask], M, want_idx[mask]))
                tol = rm.tolerance(maj, n)
                for s in (rm.PLANE_SLOTS if plane else rm.P2P_SLOTS):
                    dev = abs(mom[s] - want[s])
                    assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
                    if tol[s] > 0:
                        worst = max(worst, dev / tol[s])
                prev[b] = dict(P=P, idx=want_idx, mask=mask, mom=mom)
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            assert checked[b] == PASSES + 1 or bt.state(b)["status"] != pkg.capi.ICP_OK, (b, checked[b])
        assert min(checked[:3]) == PASSES + 1   # the three large pairs ran every pass
    print(f"[trim moments] {'plane' if plane else 'p2p'}/{np.dtype(dtype).name}/{'gate' if gated else 'no gate'}: kept {kept_log}, "
          f"largest |device - exact| / tol = {worst:.4f}")


# 4 ------------------------------------------------------------------------------------------------------------------------
def reference_loop(orc, A, M, rho, max_iter, tol):
    """orc.nn + the trim mask + ref_numpy.minimize on the kept points; the error over the kept points, divided by their count"""
    P = A.copy()
    K = rank(rho, A.shape[0])
    E, T, i, kept, gap, mask = [0.0], np.eye(4), 0, [], np.inf, None
    while True:
        idx = orc.nn(P, M)
        d = sq_dist(P, M, idx)
        mask = d <= tau_ref(d, K)
        gap = min(gap, kth_gap(d, K))
        kept.append(int(mask.sum()))
        R, t = ref_numpy.minimize(P[mask], M, idx[mask])
        P = (P.astype(np.float64) @ R.T + t).astype(A.dtype)
        Tk = np.eye(4)
        Tk[:3, :3], Tk[:3, 3] = R, t
        T = Tk @ T
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, mask=mask, gap=gap)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trim_end_to_end(ctx, pkg, orc, dtype):
    tol = 1e-6
    cases = [gate_case(*c, dtype=dtype) for c in CASES]
    wants = [reference_loop(orc, A, M, RHO, 40, tol) for A, M, _ in cases]
    for c, w, (A, M, is_out), K in zip(CASES, wants, cases, KEPT_TRIM):   # the reference alone
        print(f"{c}: reference keeps {w['kept']}, smallest K-th gap {w['gap']:.3e}, iterations {w['iterations']}, final RMS {w['err'][-1]:.3e}")
        assert w["gap"] >= 1e-4
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
        plain = run_to_end(bt, metric)
        bt.set_trim(1.0)
        ones = run_to_end(bt, metric)
        taus = [bt.diag_trim(b) for b in range(bt.count)]
        bt.set_trim(RHO)
        half = run_to_end(bt, metric)
        bt.set_trim(None)
        again = run_to_end(bt, metric)
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
            return run_to_end(bt, metric)

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
        want = run_to_end(bt, P2P)
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
        got = run_to_end(bt, P2P)    # ... and the shares are those set before
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
        plain = run_to_end(bt, P2P)
        with pytest.raises(pkg.IcpError) as e:
            bt.set_trim(1.5)
        assert e.value.code == pkg.capi.ICP_ERR_INVALID
        same_pair_bytes(plain[0], run_to_end(bt, P2P)[0])


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def hom(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def compose(Tl, T0):
    """T_loop . T0F in HostLoop::note_applied's order: s = 0; for k = 0..3: s += T_loop[a][k] * T0F[k][b], in Python floats"""
    out = np.zeros((4, 4))
    for a in range(4):
        for b in range(4):
            s = 0.0
            for k in range(4):
                s += float(Tl[a][k]) * float(T0[k][b])
            out[a][b] = s
    return out


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
        fx, fy = run_to_end(X, pkg.ICP_POINT_TO_POINT), run_to_end(Y, pkg.ICP_POINT_TO_POINT)
        for b in range(len(far)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}", T=compose(fy[b]["st"]["T"], T0F))
            assert X.diag_trim(b) == Y.diag_trim(b)
            assert fy[b]["st"]["passes"] >= 1 and not fy[b]["linl"].all()
