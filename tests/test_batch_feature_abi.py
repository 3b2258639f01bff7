"""CPU: the C ABI of batched global registration (icp_batch_compute_features, icp_batch_get_features, icp_batch_match_features,
icp_batch_score_transforms, icp_batch_ransac, icp_diag_batch_ransac, icp_solve_rigid, ICP_FEATURE_BINS, icp_ransac_params) is
declared, exported and bound with the exact ctypes signatures, the ABI version stays 2, a NULL batch is refused without a
device, the header states the rules, the Python mirror carries the additions, and icp_solve_rigid is icp_solve_point_to_point
with the determinant fix."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import batch_feature_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
_pd, _pi, _p32, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def test_feature_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(DIAG).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    prm = C.POINTER(pkg.capi.icp_ransac_params)
    want = {"icp_batch_compute_features": (C.c_int, [C.c_void_p, _pi, _pi, _pd, _pd, _pd, _pd]),
            "icp_batch_get_features": (C.c_int, [C.c_void_p, _pd, _pd]),
            "icp_batch_match_features": (C.c_int, [C.c_void_p, C.c_int, _p32, _p32, _pu8]),
            "icp_batch_score_transforms": (C.c_int, [C.c_void_p, C.c_int, _pd, _pd, _p32]),
            "icp_batch_ransac": (C.c_int, [C.c_void_p, prm, C.POINTER(C.c_uint64), _pd, _p32, _p32, _pi]),
            "icp_diag_batch_ransac": (C.c_int, [C.c_void_p, C.c_int, _p32, _pu8, _pd, _p32]),
            "icp_diag_batch_set_features": (C.c_int, [C.c_void_p, _pd, _pd]),
            "icp_solve_rigid": (C.c_int, [_pd, _pd, _pd])}
    for name, (res, args) in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name][0] is res and pkg.capi.SIGNATURES[name][1] == args, name
    assert re.search(r"#define\s+ICP_FEATURE_BINS\s+33\b", src) and pkg.capi.ICP_FEATURE_BINS == 33
    assert re.search(r"typedef struct icp_ransac_params \{ int hypotheses; double max_distance; double edge_similarity; \} icp_ransac_params;", src)
    assert [f[0] for f in pkg.capi.icp_ransac_params._fields_] == ["hypotheses", "max_distance", "edge_similarity"]
    assert C.sizeof(pkg.capi.icp_ransac_params) == 24
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rules():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("a 33-bin FPFH", "always double, whatever the batch's precision; both sides are required",
                   "Unit length and a consistent orientation of the normals are the caller's duty", "The batch does not keep the normals",
                   "never the moved cloud.  The loop does not notice: the call neither discards nor advances it",
                   "the only functions used are + - * / sqrt fabs floor", "tau_i is the k-th smallest over j != i by index",
                   "every j != i with d2(i, j) <= tau_i: all ties are in", "the pair is skipped if r2 == 0 or r2 is not finite",
                   "If fabs(a1) < fabs(a2) the roles swap: n1 = n_j, n2 = n_i, d = -d, f3 = -a2", "the pair is skipped if vv == 0 or vv is not finite",
                   "w = n1 x v; f2 = dot(v, n2); x = dot(n1, n2); y = dot(w, n2)", "a deliberate deviation from PCL",
                   "t = q if x >= 0, t = 2 - q if y >= 0, else t = -2 - q", "no bin decision hangs on a libm",
                   "bin(val, lo, width) = clamp((int)floor((11.0 * (val - lo)) / width), 0, 10)",
                   "S_i[b] = (100.0 * (double)cnt_b) / (double)c, or all zeros where c == 0",
                   "wgt = 1.0 / (double)d2(i, j); A[b] += S_j[b] * wgt", "F_i[b] = (A[b] * 100.0) / s, or 0.0 where s is not > 0 or not finite",
                   "fwd[i] is the lowest j that minimises D, rev[j] the lowest i", "kept[i] = !mutual || rev[fwd[i]] == i",
                   "((r0 x + r1 y) + r2 z) + t", "a moved point that is not finite is a miss",
                   "draw(h, r) = mix(mix(mix(seed_p) + h) + r) % C_p; the modulo bias is accepted", "at most 16 draws are used",
                   "iff la >= e*lb && lb >= e*la for all three", "Winner: the largest count, the lowest h among equals",
                   "the refit is returned if its count is at least the winner's, else the winner",
                   "status ICP_ERR_EMPTY where C_p < 3 or no hypothesis is valid", "the last column of U is flipped when det(U Vt) < 0"):
        assert clause in text, clause
    host_only = text[text.index("---- host-only pieces"):]
    assert "icp_solve_rigid" in host_only and "icp_solve_point_to_point" in host_only


def test_feature_null_batch_is_invalid(pkg):
    lib = pkg.load()
    d = np.full(99, -7.0)
    k = np.array([5, 5], dtype=np.intc)
    i32 = np.full(8, -3, dtype=np.int32)
    u8 = np.full(8, 9, dtype=np.uint8)
    seed = np.array([1], dtype=np.uint64)
    st = np.array([5], dtype=np.intc)
    prm = pkg.capi.icp_ransac_params(10, 0.1, 0.9)
    E = pkg.capi.ICP_ERR_INVALID
    pd, p32 = d.ctypes.data_as(_pd), i32.ctypes.data_as(_p32)
    assert lib.icp_batch_compute_features(None, k.ctypes.data_as(_pi), k.ctypes.data_as(_pi), pd, pd, pd, pd) == E
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_get_features(None, pd, pd) == E
    assert lib.icp_batch_match_features(None, 1, p32, p32, u8.ctypes.data_as(_pu8)) == E
    assert lib.icp_batch_score_transforms(None, 1, pd, pd, p32) == E
    assert lib.icp_batch_ransac(None, C.byref(prm), seed.ctypes.data_as(C.POINTER(C.c_uint64)), pd, p32, p32, st.ctypes.data_as(_pi)) == E
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_diag_batch_ransac(None, 0, p32, u8.ctypes.data_as(_pu8), pd, p32) == E
    assert lib.icp_diag_batch_set_features(None, pd, pd) == E
    assert (d == -7.0).all() and (i32 == -3).all() and (u8 == 9).all() and st[0] == 5


def test_feature_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.compute_features).parameters
    assert list(prm) == ["self", "k", "normals", "k_model", "want"] and prm["k_model"].default is None and prm["want"].default is False
    assert list(inspect.signature(B.get_features).parameters) == ["self"]
    prm = inspect.signature(B.match_features).parameters
    assert list(prm) == ["self", "mutual"] and prm["mutual"].default is True
    assert list(inspect.signature(B.score_transforms).parameters) == ["self", "T", "max_distance"]
    prm = inspect.signature(B.ransac).parameters
    assert list(prm) == ["self", "hypotheses", "max_distance", "edge_similarity", "seed"]
    assert prm["edge_similarity"].default == 0.9 and prm["seed"].default == 0
    prm = inspect.signature(Ctx.register_batch_global).parameters
    assert list(prm) == ["self", "pairs", "voxel", "k", "hypotheses", "max_distance", "options"] and prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(pkg.oriented_normals).parameters) == ["points", "covariances", "viewpoint"]
    assert list(inspect.signature(pkg.solve_rigid).parameters) == ["mom"]
    # what existed keeps its parameter list
    assert list(inspect.signature(B.estimate_covariances).parameters) == ["self", "k", "k_model", "regularisation", "lam", "want"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]


def test_oriented_normals(pkg):
    import batch_gicp_ref as gr
    X, _ = fr.blob(4, 120, np.float32)
    C6, _ = gr.covariances(X, 10, gr.COV_NONE)
    eye = np.array([0.0, 0.0, 0.0])
    N = pkg.oriented_normals(X, C6, eye)
    assert N.dtype == np.float64 and N.shape == (120, 3) and N.flags.c_contiguous
    assert N.tobytes() == fr.oriented_normals(X, C6, eye).tobytes()
    assert np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-12
    assert ((N * (eye - X.astype(np.float64))).sum(1) >= 0).all()                     # facing the viewpoint
    full = gr.full(C6)
    assert np.abs(np.einsum("na,nab,nb->n", N, full, N) - np.linalg.eigvalsh(full)[:, 0]).max() < 1e-12   # the smallest eigenvalue's direction


def _mom(P, Q):
    m = np.zeros(32)
    m[1] = len(P)
    m[2:5], m[5:8] = P.sum(0), Q.sum(0)
    m[8:17] = (Q.T @ P).reshape(9)
    m[17], m[18] = (P * P).sum(), (Q * Q).sum()
    return m


def test_solve_rigid_is_point_to_point_with_the_determinant_fix(pkg):
    rng = np.random.default_rng(21)
    P = rng.standard_normal((50, 3)) + 1.0
    R, t = fr.rodrigues((0.2, 0.5, -1.0), 63.0), np.array([0.5, -0.25, 2.0])
    Q = P @ R.T + t + 1e-3 * rng.standard_normal((50, 3))
    m = _mom(P, Q)
    R1, t1 = pkg.solve_point_to_point(m)
    R2, t2 = pkg.solve_rigid(m)
    assert np.linalg.det(R1) > 0 and R1.tobytes() == R2.tobytes() and t1.tobytes() == t2.tobytes()   # no fix needed: the same solve
    # three points (a rank-2 cross-covariance) on which the unfixed solve returns a reflection
    P3 = np.array([[0.35, 0.82, 0.33], [-1.3, 0.91, 0.45], [-0.54, 0.58, 0.36]])
    R, t = fr.rodrigues((1.0, 2.0, 3.0), 149.0), np.array([0.1, -0.2, 0.3])
    Q3 = P3 @ R.T + t
    m = _mom(P3, Q3)
    R1, _ = pkg.solve_point_to_point(m)
    assert np.linalg.det(R1) < 0
    R2, t2 = pkg.solve_rigid(m)
    assert abs(np.linalg.det(R2) - 1.0) < 1e-12 and np.abs(R2 @ R2.T - np.eye(3)).max() < 1e-12
    assert np.abs(R2 - R).max() < 1e-9 and np.abs(P3 @ R2.T + t2 - Q3).max() < 1e-9
    assert np.abs(R2 - fr.kabsch(P3, Q3)[:3, :3]).max() < 1e-9
    lib = pkg.load()
    m[1] = 0.0
    out = np.zeros(12)
    assert lib.icp_solve_rigid(m.ctypes.data_as(_pd), out.ctypes.data_as(_pd), out[9:].ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
    assert lib.icp_solve_rigid(None, out.ctypes.data_as(_pd), out[9:].ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
