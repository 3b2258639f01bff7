"""What the batch tests share (tests/test_gpu_batch*.py, test_gpu_plane_f64.py, test_oracle.py, test_batch_ref.py): the pairs, the
clouds with outliers, the decisions of the gate and of the trim as numpy states them, one numpy loop for every keep rule, the two
per-pass checks, and the byte comparisons.  One definition of each; nothing here touches a device except through the Batch handle
a test passes in.  The docstrings that explain a test's clouds and bounds stay with that test.
"""
import math
import os

import numpy as np

import clouds as cl
import ref_moments as rm
import ref_numpy

TOL_T = 1e-5       # T and the moved cloud, relative (test_gpu_parity.py)
TOL_E = 1e-5       # the error series, absolute
# (n, m, n_out) of gate_case: a ragged last item; a second work item that is rejected whole; 19 items and model quarters that are
# no multiple of the tile; a single short item
CASES = [(200, 300, 70), (130, 1000, 64), (1025, 513, 130), (63, 17, 5)]
_NORMALS = {}      # oracle normals are computed once per model


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def tau_bits_equal(dev_tau, want):
    """the device's tau, read back in double, is the value `want` of the batch's dtype bit for bit"""
    return np.float64(dev_tau).tobytes() == np.float64(want).tobytes()


def same_result_bits(a, b):
    """two Results of the one-call functions: every output byte for byte"""
    assert a.iterations == b.iterations and a.passes == b.passes and a.extra["status"] == b.extra["status"]
    for f in ("T", "err", "idx", "moved"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


def assert_same_run(res_iterations, res_err, res_T, want, tol, fp32):
    """(test_gpu_parity.assert_same_run) fp64 stops at the oracle's iteration; fp32 may stop one pass apart, but only where
    the deciding |dE| sits on the threshold"""
    n = min(len(res_err), len(want["err"]))
    assert np.abs(np.asarray(res_err)[:n] - want["err"][:n]).max() < TOL_E
    if res_iterations != want["iterations"]:
        assert fp32 and abs(res_iterations - want["iterations"]) == 1, (res_iterations, want["iterations"])
        k = min(res_iterations, want["iterations"]) + 1
        dE = abs(want["err"][k] - want["err"][k - 1])
        assert abs(dE - tol) < 5e-7 or abs(want["err"][k] - tol) < 5e-7, f"stop rule disagreed away from the threshold: dE={dE}"
    assert rel(res_T, want["T"]) < TOL_T


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
def fp64_pairs(pkg, orc):
    """configs[0]-style pairs that stop at different iterations (25, 10, 56, 7, 1, 10 passes)"""
    pairs = [orc.synth_icp_cpu(W) for W in (16, 24, 32)]
    D = orc.synth_icp_cpu(20)[0]
    for ang, t in [((0.3, -0.2, 0.1), (0.2, 0.1, -0.1)), ((0.05, 0.02, -0.04), (0.05, -0.02, 0.01)), ((0.6, 0.1, -0.3), (0.5, -0.2, 0.3))]:
        pairs.append((D, pkg.datasets.make_model_cpu(D, ang, t)))
    return pairs


def fp32_pairs(pkg, golden):
    D = pkg.datasets.synthetic_grid(32, np.float32)
    B = np.fromfile(os.path.join(golden, "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    return [(D, pkg.datasets.make_model_gpu(D, *pkg.datasets.P2P_GPU)), (D, pkg.datasets.make_model_standard(D)),
            (B, pkg.datasets.make_model_gpu(B, *pkg.datasets.BUNNY))]


def five_pairs(pkg, golden):
    """the plane batch: four synthetic grids and Bunny_res; the oracle stops them after 2, 3, 3, 1 and 5 iterations"""
    ds = pkg.datasets
    grid = lambda W: ds.synthetic_grid(W, np.float32)
    B = np.fromfile(os.path.join(golden, "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    G20 = grid(20)
    return [(grid(12), ds.make_model_gpu(grid(12), *ds.P2P_GPU)), (grid(24), ds.make_model_gpu(grid(24), *ds.P2P_GPU)),
            (grid(40), ds.make_model_gpu(grid(40), *ds.P2P_GPU)), (G20, ds.make_model_gpu(G20, (0.05, 0.02, -0.04), (0.05, -0.02, 0.01))),
            (B, ds.make_model_gpu(B, *ds.BUNNY))]


def degenerate_pair():
    """an 8 x 8 planar grid registered on itself with parallel normals (test_point_to_plane_degenerate_is_reported): the third
    pivot of the 6 x 6 system is an exact zero"""
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([g, np.zeros((64, 1))], 1).astype(np.float32)
    return (P, P.copy()), np.tile(np.array([[0, 0, 1]], dtype=np.float32), (64, 1))


# model sizes around the batch kernels' granules: a work item of 64 query points; four quarters of wseg = ceil(ceil(m / 4) / 8) * 8 model
# points, cut in whole chunks of 8 (m = 5, 6: all points in the first quarter, three quarters empty; 32: four quarters of 8; 33:
# quarters of 16, 16, 1 and 0; 63 .. 65: the last quarter short or one point over an item); a sub-tile of 512 (fp32) or 256
# (fp64) model points per wave (2048 / 2049 and 1024 / 1025: one tile per quarter / a second one)
KNN_M = (5, 6, 32, 33, 63, 64, 65, 130, 257, 1000, 1024, 1025, 2048, 2049, 4097)


def knn_models(dtype, sizes=KNN_M):
    models = [cl.ragged_pair(s, 1, m)[1] for s, m in enumerate(sizes)]
    Z = np.random.default_rng(5).standard_normal((300, 3)).astype(np.float32)
    Z[100:140] = 0.0   # 40 coincident points: the order among equal distances
    models.append(Z)
    if np.dtype(dtype) == np.float64:   # mantissas that fp32 cannot hold (clouds.case_pair); the coincident points stay coincident
        out = []
        for k, M in enumerate(models):
            M64 = M.astype(np.float64) + 1e-9 * np.random.default_rng(1000 + k).standard_normal(M.shape)
            if k == len(models) - 1:
                M64[100:140] = 0.0
            out.append(M64)
        models = out
    return models


def oracle_normals(orc, M):
    M = np.ascontiguousarray(M, dtype=np.float32)
    key = (M.shape[0], M.tobytes())
    if key not in _NORMALS:
        _NORMALS[key] = orc.normals(M, orc.knn4(M))[0]
    return _NORMALS[key]


def normals_for(orc, M):
    M32 = np.asarray(M, dtype=np.float32)   # (the fp32 model's normals, cast: the oracle's kNN and normals follow the dtype they are given)
    return orc.normals(M32, orc.knn4(M32))[0].astype(M.dtype)


def gate_case(n, m, n_out, dtype=np.float32):
    """(A, M, is_out): ragged_pair(n, m) with n_out far points as one run starting at point 64 (or behind a shorter cloud)"""
    D, M = cl.ragged_pair(n * 1000 + m, n, m)
    O = (np.random.default_rng(n * 1000 + m + 7).standard_normal((n_out, 3)) * 0.5 + np.array([6.0, -5.0, 4.0])).astype(np.float32)
    A = np.concatenate([D[:64], O, D[64:]])
    is_out = np.zeros(n + n_out, dtype=bool)
    is_out[min(64, n):min(64, n) + n_out] = True
    return A.astype(dtype), M.astype(dtype), is_out


# ---- the decisions: the gate, the trim ---------------------------------------------------------------------------------------------
def sq_dist(P, M, idx):
    """the winning squared distance as the matching holds it: (dx*dx + dy*dy) + dz*dz, every operation rounded in P's dtype"""
    G = M[idx]
    dx, dy, dz = P[:, 0] - G[:, 0], P[:, 1] - G[:, 1], P[:, 2] - G[:, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == P.dtype
    return d


def threshold(md, dtype):
    """(F)(md * md): the product in double, rounded once"""
    return np.dtype(dtype).type(float(md) * float(md))


def gate_mask(P, M, idx, md):
    return sq_dist(P, M, idx) <= threshold(md, P.dtype)


def gate_margin(d, md):
    """how close, relative to the threshold, any squared distance comes to it"""
    thr = float(threshold(md, d.dtype))
    return float(np.abs(d.astype(np.float64) - thr).min() / thr)


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


def keep_within(md):
    """reference_loop's rule of a gate at md; its margin: gate_margin"""
    def keep(d):
        return d <= threshold(md, d.dtype)
    keep.margin = lambda d: gate_margin(d, md)
    return keep


def keep_closest(rho):
    """reference_loop's rule of a trim to the share rho (and every match tied with the K-th); its margin: kth_gap"""
    def keep(d):
        return d <= tau_ref(d, rank(rho, d.size))
    keep.margin = lambda d: kth_gap(d, rank(rho, d.size))
    return keep


def reference_loop(orc, A, M, keep, max_iter, tol):
    """orc.nn + keep(the winning squared distances) + ref_numpy.minimize on the kept points; the error over the kept points, divided
    by their count.  A pass that keeps nothing ends the loop.  kept: the count of every pass; masks: its mask (mask: the last);
    margin: the smallest keep.margin(d) of any pass -- how far, relatively, the rule's closest decision was from going the other
    way (inf for a rule that states none)"""
    P = A.copy()
    E, T, i, kept, masks, margin = [0.0], np.eye(4), 0, [], [], np.inf
    while True:
        idx = orc.nn(P, M)
        d = sq_dist(P, M, idx)
        mask = keep(d)
        if hasattr(keep, "margin"):
            margin = min(margin, keep.margin(d))
        kept.append(int(mask.sum()))
        masks.append(mask)
        if not mask.any():
            break
        R, t = ref_numpy.minimize(P[mask], M, idx[mask])
        P = (P.astype(np.float64) @ R.T + t).astype(A.dtype)
        T = hom(R, t) @ T
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, masks=masks, mask=masks[-1], margin=margin)


# ---- rigid motions ---------------------------------------------------------------------------------------------------------------
def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def hom(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def inv_rigid(T):
    return hom(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


def apply(P, T):
    """the start cloud: ref_moments.apply_rt with the upper 3x4 of T (rounded there to P's precision, once)"""
    T = np.asarray(T, dtype=np.float64)
    return rm.apply_rt(P, T[:3, :3], T[:3, 3])


def t0f(T, dtype):
    """T as the batch holds it: the 12 values rounded once to dtype, read back in double"""
    out = np.eye(4)
    out[:3, :] = np.asarray(T, dtype=np.float64)[:3, :].astype(dtype).astype(np.float64)
    return out


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


# ---- a Batch handle: run, read, compare ----------------------------------------------------------------------------------------------
def final(bt):
    idx, moved, inl, linl = bt.loop_indices(), bt.get_moving(), bt.get_inliers(), bt.loop_inliers()
    return [dict(st=bt.state(b), idx=idx[b], moved=moved[b], inl=inl[b], linl=linl[b]) for b in range(bt.count)]


def run_to_end(bt, metric, max_iter, tol=1e-6, fixed=False):
    bt.begin(max_iter=max_iter, tol=tol, fixed_iterations=fixed, metric=metric)
    while bt.run(1 << 20)[1]:
        pass
    return final(bt)


def same_pair_bytes(a, b, what="", T=None):
    """every output of pair a is that of pair b, bit for bit; with T, a's T is T instead of b's"""
    for f in ("status", "iterations", "passes"):
        assert a["st"][f] == b["st"][f], (what, f, a["st"][f], b["st"][f])
    assert bits_equal(a["st"]["err"], b["st"]["err"]), (what, "err")
    assert bits_equal(a["st"]["T"], b["st"]["T"] if T is None else T), (what, "T")
    for f in ("idx", "moved", "inl", "linl"):
        assert bits_equal(a[f], b[f]), (what, f)


def step_together(X, Y, what):
    """run(1) on both batches to the end; after every step the moment vectors, indices and masks of every pair that took part are
    byte-equal.  Returns the kept count of every pass of every pair of Y."""
    counts = [[] for _ in range(Y.count)]
    while True:
        running = ~Y.done()
        assert np.array_equal(running, ~X.done()), what
        kx, ky = X.run(1), Y.run(1)
        assert kx == ky, (what, kx, ky)
        if not ky[0]:
            break
        ix, iy, mx, my = X.get_indices(), Y.get_indices(), X.get_inliers(), Y.get_inliers()
        for b in np.flatnonzero(running):
            assert bits_equal(X.diag_moments(b), Y.diag_moments(b)), (what, b, "moments")
            assert bits_equal(ix[b], iy[b]) and bits_equal(mx[b], my[b]), (what, b)
            counts[b].append(int(my[b].sum()))
    return counts


# ---- one pass of a gated or trimmed batch against exact sums -------------------------------------------------------------------------
def check_front_end(pkg, plane, P, M, mom, err_k, pv, what):
    """the transform front end of a pass: P (the cloud the pass was matched on) is P_{k-1} moved by the host solve of pass k-1's
    vector, bit for bit; slot ERR is the exact error over the points pass k-1 kept, within ref_moments.tolerance; err_k, the loop's
    err[k], is that slot's RMS within 4 ulp.  pv: dict(P, idx, mask, mom) of the pair's previous pass, or None -- ERR is exactly 0"""
    if pv is None:
        assert mom[rm.ERR] == 0.0, what
        return
    R, t = (pkg.solve_point_to_plane(pv["mom"])[:2] if plane else pkg.solve_point_to_point(pv["mom"]))
    assert bits_equal(P, rm.apply_rt(pv["P"], R, t)), what
    want_err = rm.sq_error(P[pv["mask"]], M, pv["idx"][pv["mask"]])
    tol_err = rm.tolerance(np.full(rm.NMOM, want_err), P.shape[0])[rm.ERR]
    assert abs(mom[rm.ERR] - want_err) <= tol_err, f"{what}: ERR {mom[rm.ERR]!r} exact {want_err!r} tol {tol_err:.3e}"
    e = np.sqrt(mom[rm.ERR]) / np.sqrt(float(pv["mask"].sum()))
    print(f"{what}: err {err_k!r} from the vector {e!r}")
    assert abs(err_k - e) <= 4 * np.finfo(np.float64).eps * e, what


def check_sums(plane, P, M, nrm, idx, mask, mom, what):
    """the metric's slots of a pass's vector against the exact sums over the kept points (ref_moments.p2p / .plane; all zero where
    nothing is kept), slot by slot within ref_moments.tolerance for the pair's n points.  Returns the largest |device - exact| / tol"""
    if mask.any():
        want, maj = (rm.plane(P[mask], M, nrm, idx[mask]) if plane else rm.p2p(P[mask], M, idx[mask]))
    else:
        want, maj = np.zeros(rm.NMOM), np.zeros(rm.NMOM)
    tol = rm.tolerance(maj, P.shape[0])
    worst = 0.0
    for s in (rm.PLANE_SLOTS if plane else rm.P2P_SLOTS):
        dev = abs(mom[s] - want[s])
        assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
        if tol[s] > 0:
            worst = max(worst, dev / tol[s])
    return worst
