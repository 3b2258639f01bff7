"""CPU: the C ABI of outlier removal (icp_batch_remove_outliers, icp_outlier_rule) is declared, exported and bound with the exact
ctypes signature, the ABI version stays 2, the header states the rules, a NULL batch is refused without a device with every
output untouched, and the Python mirror carries the addition while what existed keeps its parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
_pd, _p32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def test_outlier_symbol_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    name = "icp_batch_remove_outliers"
    assert name in declared and name in exported
    assert name in pkg.capi.SIGNATURES and hasattr(lib, name)
    rule = pkg.capi.icp_outlier_rule
    res, args = pkg.capi.SIGNATURES[name]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(rule), C.POINTER(rule), _p32, _p32, _pd, _pd, _pd, C.POINTER(C.c_void_p)]
    assert [(n, t) for n, t in rule._fields_] == [("kind", C.c_int), ("neighbours", C.c_int), ("value", C.c_double)] and C.sizeof(rule) == 16
    assert re.search(r"typedef struct icp_outlier_rule \{ int kind; int neighbours; double value; \} icp_outlier_rule;", src)
    for macro, value in (("ICP_OUTLIER_NONE", 0), ("ICP_OUTLIER_STATISTICAL", 1), ("ICP_OUTLIER_RADIUS", 2), ("ICP_OUTLIER_MAX_NEIGHBOURS", 32)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src) and getattr(pkg.capi, macro) == value, macro
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rules():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("(dx*dx + dy*dy) + dz*dz", "j != i by index", "a coincident point counts, at distance 0", "the k smallest d2(i, .) as a multiset",
                   "a correctly rounded double sqrt", "from the smallest to the largest, starting at 0.0", "divide once by (double)k",
                   "a granule is 64 consecutive points", "each granule is added from 0.0 in ascending index",
                   "the granule sums are added from 0.0 in ascending granule order", "mean = S / (double)n", "dev_i = dbar_i - mean, q_i = dev_i * dev_i",
                   "std = sqrt(Qsum / (double)(n - 1))", "thr = mean + a * std, one multiplication then one addition", "Keep iff dbar_i <= thr",
                   "a point on the threshold is kept", "Nothing is fused, nothing is multiplied by a reciprocal", "no floating-point atomics",
                   "thr2 = (F)(r * r)", "c_i = #{ j != i : d2(i, j) <= thr2 }", "keep iff c_i >= min", "copied, not computed", "a -0.0 survives",
                   "-1 for a removed point", "[mean, std, thr, kept]", "[0, 0, (double)thr2, kept]", "[0, 0, 0, n]", "The loop does not notice",
                   "no output array is written", "names the first offending pair and the side", "ICP_ERR_EMPTY: a cloud would keep no point",
                   "bit for bit in numpy", "three launches", "two host waits"):
        assert clause in text, clause


def test_outlier_null_batch_is_invalid(pkg):
    lib = pkg.load()
    rule = pkg.capi.icp_outlier_rule
    rules = (rule * 2)(rule(1, 8, 1.0), rule(2, 3, 0.5))
    maps = np.full(8, -7, dtype=np.int32)
    score = np.full(8, -7.0)
    stats = np.full(16, -7.0)
    out = C.c_void_p(0x1234)
    rc = lib.icp_batch_remove_outliers(None, rules, rules, maps.ctypes.data_as(_p32), maps.ctypes.data_as(_p32), score.ctypes.data_as(_pd),
                                       score.ctypes.data_as(_pd), stats.ctypes.data_as(_pd), C.byref(out))
    assert rc == pkg.capi.ICP_ERR_INVALID and "null batch" in lib.icp_last_error().decode()
    assert out.value is None and (maps == -7).all() and (score == -7.0).all() and (stats == -7.0).all()   # *out is NULL on any refusal
    assert (rules[0].kind, rules[0].neighbours, rules[0].value, rules[1].kind) == (1, 8, 1.0, 2)
    assert lib.icp_batch_remove_outliers(None, None, None, None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID


def test_outlier_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.remove_outliers).parameters
    assert list(prm) == ["self", "moving", "model", "want_maps", "want_scores"]
    assert prm["moving"].default is None and prm["model"].default is None
    assert prm["want_maps"].default is False and prm["want_scores"].default is False
    # what existed keeps its parameter list
    assert list(inspect.signature(B.__init__).parameters) == ["self", "ctx", "pairs"]
    assert list(inspect.signature(B.downsample).parameters) == ["self", "voxel", "voxel_model", "want_maps"]
    assert list(inspect.signature(B.get_clouds).parameters) == ["self"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_robust).parameters) == ["self", "pairs", "kernel", "scale", "options"]
    assert list(inspect.signature(Ctx.register_batch_multiscale).parameters) == ["self", "pairs", "voxels", "options"]
