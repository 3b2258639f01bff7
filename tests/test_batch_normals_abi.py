"""CPU: the C ABI of the point normals (icp_batch_estimate_point_normals, icp_batch_set_point_normals, icp_batch_get_point_normals,
icp_batch_compute_features_stored, icp_diag_batch_centroids) is declared, exported and bound with the exact ctypes signatures, the
ICP_ORIENT_* constants match the header, the ABI version stays 2, the header states the rule's clauses, a NULL batch is refused
without a device with every output untouched, and the Python mirror carries the additions while what existed keeps its parameter
lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
_vp, _i, _pd, _pi = C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
ENTRIES = {
    "icp_batch_estimate_point_normals": (HEADER, [_vp, _i, _pd, _pd, _pd, _pd]),
    "icp_batch_set_point_normals": (HEADER, [_vp, _pd, _pd]),
    "icp_batch_get_point_normals": (HEADER, [_vp, _pd, _pd]),
    "icp_batch_compute_features_stored": (HEADER, [_vp, _pi, _pi, _pd, _pd]),
    "icp_diag_batch_centroids": (DIAG, [_vp, _pd]),
}


def test_normals_symbols_declared_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    for name, (header, args) in ENTRIES.items():
        src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in exported and hasattr(lib, name), name
        res, bound = pkg.capi.SIGNATURES[name]
        assert res is C.c_int and bound == args, name
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int icp_batch_estimate_point_normals\(icp_batch\* b, int orient, const double\* moving_viewpoints, "
                     r"const double\* model_viewpoints,\s*double\* moving_normals_out, double\* model_normals_out\);", src)
    for macro, value in (("ICP_ORIENT_NONE", 0), ("ICP_ORIENT_VIEWPOINT", 1), ("ICP_ORIENT_CENTROID", 2)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src) and getattr(pkg.capi, macro) == value, macro
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("computes both sides, always", "It needs covariances on both sides", "the message names the side",
                   "an unknown value is ICP_ERR_INVALID", "3 doubles per pair, each in that cloud's own frame",
                   "In the other modes the arrays are not read", "a host wait only when one is given",
                   "A refused call leaves the previous normals and everything else as they were", "neither discards nor advances it",
                   "The normals are a snapshot", "bit for bit in numpy", "+ - * / sqrt fabs copysign",
                   "cyclic Jacobi over (0,1), (0,2), (1,2) from v = I", "at most 64 sweeps", "off <= 1e-34 * dia || off == 0.0",
                   "icp_eigh3's range rule comes first", "largest magnitude lies beyond 2^+-400 is solved times 2^-+600",
                   "n does not depend on a power of two in C", "amax > 2^400 multiplies them by 2^-600", "0 < amax < 2^-400 by 2^+600",
                   "after the ascending order is fixed", "go through as they are, bit for bit",
                   "the same three compare-and-swaps of the order with the strict <", "n is column ord[0] of v, not renormalised",
                   "A zero matrix gives (1, 0, 0)", "n is exactly (0.0, 0.0, 0.0)", "to_a = v_a - (double)x_a",
                   "dt = (n_x*to_x + n_y*to_y) + n_z*to_z", "negated iff dt < 0", "With ICP_ORIENT_NONE nothing is negated",
                   "s_t += (double)x_j for j = t, t + 256", "total += s_t for t ascending", "v = total / (double)n",
                   "depend on that cloud, its covariances and its viewpoint alone", "the setter checks finiteness only",
                   "get on a side without normals is ICP_ERR_STATE", "no upload of normals", "a side without normals is ICP_ERR_STATE",
                   "two with ICP_ORIENT_CENTROID"):
        assert clause in text, clause


def test_normals_null_batch_is_invalid(pkg):
    lib = pkg.load()
    INVALID = pkg.capi.ICP_ERR_INVALID
    view, out = np.full(6, 2.5), np.full(12, -7.0)
    k = np.full(2, 5, dtype=np.intc)
    v, o = view.ctypes.data_as(_pd), out.ctypes.data_as(_pd)
    for mode in (0, 1, 2, 9):
        assert lib.icp_batch_estimate_point_normals(None, mode, v, v, o, o) == INVALID and "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_estimate_point_normals(None, 2, None, None, None, None) == INVALID
    assert lib.icp_batch_set_point_normals(None, v, v) == INVALID and "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_get_point_normals(None, o, o) == INVALID and "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_compute_features_stored(None, k.ctypes.data_as(_pi), k.ctypes.data_as(_pi), o, o) == INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_diag_batch_centroids(None, o) == INVALID and "null batch" in lib.icp_last_error().decode()
    assert (out == -7.0).all() and (view == 2.5).all() and (k == 5).all()


def test_normals_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.estimate_point_normals).parameters
    assert list(prm) == ["self", "orient", "viewpoints", "want"]
    assert prm["orient"].default == "centroid" and prm["viewpoints"].default is None and prm["want"].default is False
    assert list(inspect.signature(B.set_point_normals).parameters) == ["self", "moving", "model"]
    assert list(inspect.signature(B.get_point_normals).parameters) == ["self"]
    prm = inspect.signature(B.compute_features_stored).parameters
    assert list(prm) == ["self", "k", "k_model", "want"] and prm["k_model"].default is None and prm["want"].default is False
    assert list(inspect.signature(B.diag_centroids).parameters) == ["self"]
    assert "device_normals" in inspect.getsource(Ctx.register_batch_global)
    # what existed keeps its parameter list
    assert list(inspect.signature(B.compute_features).parameters) == ["self", "k", "normals", "k_model", "want"]
    assert list(inspect.signature(B.estimate_covariances).parameters) == ["self", "k", "k_model", "regularisation", "lam", "want"]
    assert list(inspect.signature(pkg.oriented_normals).parameters) == ["points", "covariances", "viewpoint"]
    assert list(inspect.signature(Ctx.register_batch_global).parameters) == ["self", "pairs", "voxel", "k", "hypotheses", "max_distance", "options"]
