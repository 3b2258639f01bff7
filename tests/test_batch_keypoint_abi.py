"""CPU: the C ABI of keypoint selection (icp_batch_select_keypoints, icp_keypoint_rule) is declared, exported and bound with the exact
ctypes signature, the ABI version stays 2, the header states the rule's clauses, a NULL batch is refused without a device with
every output untouched, and the Python mirror carries the addition while what existed keeps its parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
_pd, _p32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def test_keypoint_symbol_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    name = "icp_batch_select_keypoints"
    assert name in declared and name in exported
    assert name in pkg.capi.SIGNATURES and hasattr(lib, name)
    rule = pkg.capi.icp_keypoint_rule
    res, args = pkg.capi.SIGNATURES[name]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(rule), C.POINTER(rule), _p32, _p32, _pd, _pd, _p32, C.POINTER(C.c_void_p)]
    assert [(n, t) for n, t in rule._fields_] == [("kind", C.c_int), ("min_neighbours", C.c_int), ("salient_radius", C.c_double),
                                                  ("non_max_radius", C.c_double), ("gamma_21", C.c_double), ("gamma_32", C.c_double)]
    assert C.sizeof(rule) == 40
    assert re.search(r"typedef struct icp_keypoint_rule \{ int kind; int min_neighbours; double salient_radius; double non_max_radius; "
                     r"double gamma_21; double gamma_32; \} icp_keypoint_rule;", src)
    for macro, value in (("ICP_KEYPOINT_NONE", 0), ("ICP_KEYPOINT_ISS", 1)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src) and getattr(pkg.capi, macro) == value, macro
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("ts = (F)(salient_radius * salient_radius)", "tn = (F)(non_max_radius * non_max_radius)", "the gate's rule",
                   "every j of the cloud with d2(i, j) <= ts, i itself included at distance 0", "A point exactly on the radius is in",
                   "over the neighbourhood in ascending j", "e = (double)x_j - (double)x_i, s_a += e_a, S_ab += e_a * e_b",
                   "C_ab = (S_ab - (s_a * s_b) / (double)c) / (double)c", "cyclic Jacobi over (0,1), (0,2), (1,2)", "at most 64 sweeps",
                   "off <= 1e-34 * dia || off == 0.0", "the same ascending order w0 <= w1 <= w2",
                   "w0, w1, w2 are the scaled-back eigenvalues", "multiplied by 2^+-600 once the order is fixed",
                   "the saliency of a cloud times 2^e is 2^(2e) times the cloud's own",
                   "sal_i = w0 iff c >= min_neighbours && (w1 / w2) < gamma_21 && (w0 / w1) < gamma_32 && w0 > 0",
                   "sal_i is exactly 0.0", "A NaN fails every comparison", "M_i is every j with d2(i, j) <= tn, i included",
                   "|M_i| >= min_neighbours && sal_j <= sal_i for every j in M_i", "Equal saliencies keep each other",
                   "nothing is multiplied by a reciprocal", "+ - * / sqrt fabs copysign", "copied, not computed", "a -0.0 survives",
                   "-1 for a dropped point", "0.0 for a copied cloud", "never the moved cloud", "The loop does not notice",
                   "no output array is written", "names the first offending pair and the side", "min_neighbours outside [1, 65535]",
                   "a gamma that is not finite or not > 0", "ICP_ERR_EMPTY: a cloud would keep no point", "byte for byte, in the kept order",
                   "A side of src without descriptors gives a side without", "bit for bit in numpy", "four launches", "two host waits",
                   "LDS per block", "a cloud's outputs depend on that cloud and its rule alone"):
        assert clause in text, clause


def test_keypoint_null_batch_is_invalid(pkg):
    lib = pkg.load()
    rule = pkg.capi.icp_keypoint_rule
    rules = (rule * 2)(rule(1, 5, 0.1, 0.08, 0.975, 0.975), rule(0, 0, 0.0, 0.0, 0.0, 0.0))
    maps = np.full(8, -7, dtype=np.int32)
    sal = np.full(8, -7.0)
    counts = np.full(4, -7, dtype=np.int32)
    out = C.c_void_p(0x1234)
    rc = lib.icp_batch_select_keypoints(None, rules, rules, maps.ctypes.data_as(_p32), maps.ctypes.data_as(_p32), sal.ctypes.data_as(_pd),
                                        sal.ctypes.data_as(_pd), counts.ctypes.data_as(_p32), C.byref(out))
    assert rc == pkg.capi.ICP_ERR_INVALID and "null batch" in lib.icp_last_error().decode()
    assert out.value is None and (maps == -7).all() and (sal == -7.0).all() and (counts == -7).all()   # *out is NULL on any refusal
    assert (rules[0].kind, rules[0].min_neighbours, rules[0].salient_radius, rules[0].gamma_32, rules[1].kind) == (1, 5, 0.1, 0.975, 0)
    assert lib.icp_batch_select_keypoints(None, None, None, None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID


def test_keypoint_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.keypoints).parameters
    assert list(prm) == ["self", "moving", "model", "want_maps", "want_saliency"]
    assert prm["moving"].default is None and prm["model"].default is None
    assert prm["want_maps"].default is False and prm["want_saliency"].default is False
    # what existed keeps its parameter list
    assert list(inspect.signature(B.__init__).parameters) == ["self", "ctx", "pairs"]
    assert list(inspect.signature(B.downsample).parameters) == ["self", "voxel", "voxel_model", "want_maps"]
    assert list(inspect.signature(B.remove_outliers).parameters) == ["self", "moving", "model", "want_maps", "want_scores"]
    assert list(inspect.signature(B.compute_features).parameters) == ["self", "k", "normals", "k_model", "want"]
    assert list(inspect.signature(B.match_features).parameters) == ["self", "mutual"]
    assert list(inspect.signature(B.ransac).parameters) == ["self", "hypotheses", "max_distance", "edge_similarity", "seed"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_global).parameters) == ["self", "pairs", "voxel", "k", "hypotheses", "max_distance", "options"]
