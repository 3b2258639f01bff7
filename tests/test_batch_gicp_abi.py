"""CPU: the C ABI of the generalized metric (icp_batch_set_covariances, icp_batch_estimate_covariances,
icp_batch_get_covariances, icp_diag_batch_rotation, ICP_GENERALIZED, ICP_COV_*) is declared, exported and bound with the exact
ctypes signatures, the ABI version stays 2, a NULL batch is refused without a device, the Python mirror carries the additions
while what existed keeps its parameter lists, and the host loop accepts the metric and solves as for point-to-plane."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_gicp_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(DIAG).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    want = {"icp_batch_set_covariances": (C.c_int, [C.c_void_p, _pd, _pd]),
            "icp_batch_estimate_covariances": (C.c_int, [C.c_void_p, _pi, _pi, C.c_int, C.c_double, _pd, _pd]),
            "icp_batch_get_covariances": (C.c_int, [C.c_void_p, _pd, _pd]),
            "icp_diag_batch_rotation": (C.c_int, [C.c_void_p, C.c_int, _pd])}
    for name, (res, args) in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name][0] is res and pkg.capi.SIGNATURES[name][1] == args, name
    for macro, value in (("ICP_GENERALIZED", 2), ("ICP_COV_NONE", 0), ("ICP_COV_FROBENIUS", 1), ("ICP_COV_MIN_NEIGHBOURS", 3),
                         ("ICP_COV_MAX_NEIGHBOURS", 32)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src) and getattr(pkg.capi, macro) == value, macro
    assert pkg.ICP_GENERALIZED == 2
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())
    assert re.search(r"typedef enum \{ ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1 \} icp_metric;", src)   # the enum is as it was


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("6 doubles per point, xx, xy, xz, yy, yz, zz", "always double, whatever the batch's precision",
                   "A NULL array on one side leaves that side untouched", "is the caller's duty", "(dx*dx + dy*dy) + dz*dz",
                   "tau_i is the k-th smallest d2(i, j) over j != i by index", "all ties with the k-th are in", "c >= k + 1",
                   "in ascending j", "differences against the query", "C_ab = (S_ab - (s_a * s_b) / (double)c) / (double)c",
                   "f = sqrt(((xx*xx + yy*yy) + zz*zz) + 2.0 * ((xy*xy + xz*xz) + yz*yz))", "f == 0: C' = lambda I exactly",
                   "f and the quotients are formed on the matrix icp_eigh3's range rule leaves", "multiplies the six by 2^-600 first",
                   "f == 0 is left to the zero matrix alone", "Within 2^+-400 nothing is multiplied",
                   "weights on a Mahalanobis residual are a later change", "det = (S00*c00 + S01*c01) + S02*c02",
                   "A match whose det is not finite or not > 0 is rejected", "j0 = (0, -pz, py), j1 = (pz, 0, -px), j2 = (-py, px, 0)",
                   "Slot C(a, c) += j_a . u_c for a <= c; slot B(a) -= u_a . e", "Every dot product is (x*x' + y*y') + z*z'",
                   "With M = n n^T these are the plane pass's statements", "three launches, up to five, one download"):
        assert clause in text, clause


def test_gicp_null_batch_is_invalid(pkg):
    lib = pkg.load()
    cov = np.full(12, -7.0)
    k = np.array([5, 5], dtype=np.intc)
    assert lib.icp_batch_set_covariances(None, cov.ctypes.data_as(_pd), cov.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_estimate_covariances(None, k.ctypes.data_as(_pi), k.ctypes.data_as(_pi), 1, 1e-3, cov.ctypes.data_as(_pd),
                                              cov.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_get_covariances(None, cov.ctypes.data_as(_pd), cov.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
    assert lib.icp_diag_batch_rotation(None, 0, cov.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID
    assert (cov == -7.0).all() and (k == 5).all()


def test_gicp_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.set_covariances).parameters
    assert list(prm) == ["self", "moving", "model"] and prm["moving"].default is None and prm["model"].default is None
    prm = inspect.signature(B.estimate_covariances).parameters
    assert list(prm) == ["self", "k", "k_model", "regularisation", "lam", "want"]
    assert (prm["k"].default, prm["k_model"].default, prm["regularisation"].default, prm["lam"].default, prm["want"].default) == (20, None, "frobenius", 1e-3, False)
    assert list(inspect.signature(B.get_covariances).parameters) == ["self"]
    assert list(inspect.signature(B.diag_rotation).parameters) == ["self", "b"]
    prm = inspect.signature(Ctx.register_batch_generalized).parameters
    assert list(prm) == ["self", "pairs", "k", "regularisation", "lam", "covariances", "options"]
    assert (prm["k"].default, prm["regularisation"].default, prm["lam"].default, prm["covariances"].default) == (20, "frobenius", 1e-3, None)
    assert prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    prm = inspect.signature(pkg.covariances_from_normals).parameters
    assert list(prm) == ["normals", "eps"] and prm["eps"].default == 1e-3
    # what existed keeps its parameter list
    assert list(inspect.signature(B.__init__).parameters) == ["self", "ctx", "pairs"]
    assert list(inspect.signature(B.begin).parameters) == ["self", "max_iter", "tol", "fixed_iterations", "metric"]
    assert list(inspect.signature(B.set_model_normals).parameters) == ["self", "normals"]
    assert list(inspect.signature(B.estimate_normals).parameters) == ["self", "want_neighbours"]
    assert list(inspect.signature(B.evaluate).parameters) == ["self", "max_distance", "metric", "want_matches"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_robust).parameters) == ["self", "pairs", "kernel", "scale", "options"]
    assert list(inspect.signature(Ctx.register_batch_multiscale).parameters) == ["self", "pairs", "voxels", "options"]


def test_covariances_from_normals(pkg):
    import batch_gicp_ref as gr
    rng = np.random.default_rng(3)
    N = rng.standard_normal((50, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    C6 = pkg.covariances_from_normals(N.astype(np.float32), eps=1e-2)
    assert C6.dtype == np.float64 and C6.shape == (50, 6) and C6.flags.c_contiguous
    assert C6.tobytes() == gr.from_normals(N.astype(np.float32), 1e-2).tobytes()
    full = gr.full(C6)
    w = np.linalg.eigvalsh(full)
    assert np.abs(w[:, 0] - 1e-2).max() < 1e-6 and np.abs(w[:, 1:] - 1.0).max() < 1e-6   # eps along the normal, 1 across it
    assert np.abs(np.einsum("nab,nb->na", full, N.astype(np.float32).astype(np.float64)) - 1e-2 * N).max() < 1e-6


def test_host_loop_accepts_the_metric_and_solves_as_plane(pkg):
    lib = pkg.load()
    rng = np.random.default_rng(11)
    A = rng.standard_normal((40, 6))
    x = np.array([0.01, -0.02, 0.015, 0.1, -0.05, 0.02])
    Cm, b = A.T @ A, (A.T @ A) @ x
    mom = np.zeros(pkg.capi.ICP_NMOM)
    mom[pkg.capi.MOM_CNT] = 40.0
    o = pkg.capi.MOM_C
    for a in range(6):
        for c in range(a, 6):
            mom[o] = Cm[a, c]
            o += 1
    mom[pkg.capi.MOM_B:pkg.capi.MOM_B + 6] = b
    got = {}
    for metric in (pkg.capi.ICP_POINT_TO_PLANE, pkg.capi.ICP_GENERALIZED):
        prm = pkg.capi.icp_params(5, 1e-9, 0, pkg.capi.ICP_F64, metric)
        h = C.c_void_p()
        assert lib.icp_host_loop_create(C.byref(prm), C.byref(h)) == pkg.capi.ICP_OK
        done, R, t = C.c_int(0), np.zeros(9), np.zeros(3)
        assert lib.icp_host_loop_advance(h, mom.ctypes.data_as(_pd), C.byref(done), R.ctypes.data_as(_pd), t.ctypes.data_as(_pd)) == pkg.capi.ICP_OK
        assert done.value == 0
        got[metric] = (R.copy(), t.copy())
        lib.icp_host_loop_destroy(h)
    assert got[1][0].tobytes() == got[2][0].tobytes() and got[1][1].tobytes() == got[2][1].tobytes()
    assert np.abs(got[2][1] - x[3:]).max() < 1e-9 and np.abs(got[2][0].reshape(3, 3) - np.eye(3)).max() < 0.05
    prm = pkg.capi.icp_params(5, 1e-9, 0, pkg.capi.ICP_F64, 3)   # still an unknown metric
    h = C.c_void_p()
    assert lib.icp_host_loop_create(C.byref(prm), C.byref(h)) == pkg.capi.ICP_ERR_INVALID
