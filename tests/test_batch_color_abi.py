"""CPU: the C ABI of the colored metric (icp_batch_set_intensities, icp_batch_estimate_intensity_gradients,
icp_batch_set_intensity_gradients, icp_batch_get_intensity_gradients, icp_batch_set_color_weight, ICP_COLORED,
ICP_COLOR_LAMBDA_DEFAULT) is declared, exported and bound with the exact ctypes signatures, the ABI version stays 2, a NULL batch
is refused on every entry without a device, the Python mirror carries the additions while what existed keeps its parameter
lists, and the host loop still refuses the value."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_color_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    want = {"icp_batch_set_intensities": (C.c_int, [C.c_void_p, _pd, _pd]),
            "icp_batch_estimate_intensity_gradients": (C.c_int, [C.c_void_p, _pi, _pd]),
            "icp_batch_set_intensity_gradients": (C.c_int, [C.c_void_p, _pd]),
            "icp_batch_get_intensity_gradients": (C.c_int, [C.c_void_p, _pd]),
            "icp_batch_set_color_weight": (C.c_int, [C.c_void_p, _pd])}
    for name, (res, args) in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name][0] is res and pkg.capi.SIGNATURES[name][1] == args, name
    for decl in ("int icp_batch_set_intensities(icp_batch* b, const double* moving_I, const double* model_I);",
                 "int icp_batch_estimate_intensity_gradients(icp_batch* b, const int* k_model, double* grad_out);",
                 "int icp_batch_set_intensity_gradients(icp_batch* b, const double* grad);",
                 "int icp_batch_get_intensity_gradients(icp_batch* b, double* grad_out);",
                 "int icp_batch_set_color_weight(icp_batch* b, const double* lambda);"):
        assert decl in src, decl
    assert re.search(r"#define\s+ICP_COLORED\s+3\b", src) and pkg.capi.ICP_COLORED == 3 and pkg.ICP_COLORED == 3
    assert re.search(r"#define\s+ICP_COLOR_LAMBDA_DEFAULT\s+0\.968\b", src) and pkg.capi.ICP_COLOR_LAMBDA_DEFAULT == 0.968
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())
    assert re.search(r"typedef enum \{ ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1 \} icp_metric;", src)   # the enum is as it was


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("an intensity is one double per point, a gradient three doubles per model point", "always double, whatever the batch's precision",
                   "new model intensities and new model normals", "there is a host wait only when it is given",
                   "NULL means ICP_COLOR_LAMBDA_DEFAULT for every pair", "every j != i with d2(i, j) <= tau_i is in; c is their number",
                   "h = dot(e, n); u_a = e_a - h*n_a; g = I_j - I_i", "A_ab += u_a*u_b for the six a <= b; r_a += u_a*g",
                   "w = (double)c * (double)c; A_ab += w*(n_a*n_b)", "det = (A00*c00 + A01*c01) + A02*c02; M_ab = c_ab / det",
                   "d_a = (M_a0*r_0 + M_a1*r_1) + M_a2*r_2", "the gradient is exactly (0, 0, 0) where det is not finite or not > 0",
                   "s = dot(d, n), m_a = d_a - s*n_a", "rI = (Iq_j + dot(d, u)) - Ip_i", "G_a = dot(j_a, n), K_a = dot(j_a, m)",
                   "lg = lambda[pair], lp = 1.0 - lg", "Slot C(a, c) += lg*(G_a*G_c) + lp*(K_a*K_c) for a <= c",
                   "slot B(a) -= lg*(G_a*h) + lp*(K_a*rI)", "With lg == 1 these are the plane pass's statements",
                   "batch_color_moments, the reduction up to ICP_MOM_B + 5"):
        assert clause in text, clause


def test_color_null_batch_is_invalid(pkg):
    lib = pkg.load()
    v = np.full(12, -7.0)
    k = np.array([5, 5], dtype=np.intc)
    calls = (lambda: lib.icp_batch_set_intensities(None, v.ctypes.data_as(_pd), v.ctypes.data_as(_pd)),
             lambda: lib.icp_batch_estimate_intensity_gradients(None, k.ctypes.data_as(_pi), v.ctypes.data_as(_pd)),
             lambda: lib.icp_batch_set_intensity_gradients(None, v.ctypes.data_as(_pd)),
             lambda: lib.icp_batch_get_intensity_gradients(None, v.ctypes.data_as(_pd)),
             lambda: lib.icp_batch_set_color_weight(None, v.ctypes.data_as(_pd)),
             lambda: lib.icp_batch_set_color_weight(None, None))
    for call in calls:
        assert call() == pkg.capi.ICP_ERR_INVALID
        assert "null batch" in lib.icp_last_error().decode()
    assert (v == -7.0).all() and (k == 5).all()


def test_color_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.set_intensities).parameters
    assert list(prm) == ["self", "moving", "model"] and prm["moving"].default is None and prm["model"].default is None
    prm = inspect.signature(B.estimate_intensity_gradients).parameters
    assert list(prm) == ["self", "k", "want"] and prm["want"].default is False
    assert list(inspect.signature(B.set_intensity_gradients).parameters) == ["self", "grads"]
    assert list(inspect.signature(B.get_intensity_gradients).parameters) == ["self"]
    assert list(inspect.signature(B.set_color_weight).parameters) == ["self", "lam"]
    prm = inspect.signature(Ctx.register_batch_colored).parameters
    assert list(prm) == ["self", "pairs", "intensities", "k", "lam", "normals", "options"]
    assert prm["lam"].default == 0.968 and prm["normals"].default is None and prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    # what existed keeps its parameter list
    assert list(inspect.signature(B.begin).parameters) == ["self", "max_iter", "tol", "fixed_iterations", "metric"]
    assert list(inspect.signature(B.set_covariances).parameters) == ["self", "moving", "model"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_generalized).parameters) == ["self", "pairs", "k", "regularisation", "lam", "covariances", "options"]


def test_intensity_from_rgb(pkg):
    rgb = np.random.default_rng(2).uniform(0, 1, (50, 3)).astype(np.float32)
    I = pkg.intensity_from_rgb(rgb)
    c = rgb.astype(np.float64)
    assert I.dtype == np.float64 and I.shape == (50,) and I.flags.c_contiguous
    assert I.tobytes() == (((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0).tobytes()
    assert np.abs(I - rgb.mean(axis=1)).max() < 1e-6
    try:
        pkg.intensity_from_rgb(np.zeros((4, 2)))
    except ValueError:
        pass
    else:
        raise AssertionError("a (4, 2) array is not a colour array")


def test_host_loop_still_refuses_the_value(pkg):
    lib = pkg.load()
    prm = pkg.capi.icp_params(5, 1e-9, 0, pkg.capi.ICP_F64, pkg.capi.ICP_COLORED)
    h = C.c_void_p()
    assert lib.icp_host_loop_create(C.byref(prm), C.byref(h)) == pkg.capi.ICP_ERR_INVALID
