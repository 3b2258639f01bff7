"""CPU: the surface of icp_batch_evaluate -- declared, exported, bound with the right ctypes signature, refused without a device
for a null batch -- and of its Python mirror."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("icp_batch_evaluate", "icp_diag_batch_eval_moments")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_declared_exported_and_bound(pkg):
    lib = pkg.load()
    main, diag = _header("icp_mi355x.h"), _header("icp_mi355x_diag.h")
    assert re.search(r"\bint\s+icp_batch_evaluate\s*\(\s*icp_batch\*\s*b,\s*int\s+metric,\s*const\s+double\*\s*max_dist", main)
    assert re.search(r"\bint\s+icp_diag_batch_eval_moments\s*\(\s*icp_batch\*\s*b,\s*int\s+pair,\s*double\*\s*out32\s*\)", diag)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert s in exported and s in pkg.capi.SIGNATURES and hasattr(lib, s), s
    vp, i, pd, pi32 = C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert pkg.capi.SIGNATURES["icp_batch_evaluate"] == (i, [vp, i, pd, C.POINTER(C.c_int), pi32, pd, pd, pd, pi32, C.POINTER(C.c_uint8)])
    assert pkg.capi.SIGNATURES["icp_diag_batch_eval_moments"] == (i, [vp, i, pd])
    assert lib.icp_batch_evaluate.restype is i and list(lib.icp_batch_evaluate.argtypes) == pkg.capi.SIGNATURES["icp_batch_evaluate"][1]


def test_abi_version_stays_2(pkg):
    assert pkg.load().icp_abi_version() == 2
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", _header("icp_mi355x.h"))


def test_null_batch_is_refused_without_a_device(pkg):
    lib = pkg.load()
    assert lib.icp_batch_evaluate(None, pkg.ICP_POINT_TO_POINT, None, None, None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    out = (C.c_double * 32)()
    assert lib.icp_diag_batch_eval_moments(None, 0, out) == pkg.capi.ICP_ERR_INVALID


def test_header_names_the_slots(pkg):
    diag = _header("icp_mi355x_diag.h")
    for name, value in (("ICP_EVAL_SD", 0), ("ICP_EVAL_CNT", 1), ("ICP_EVAL_SQ", 2), ("ICP_EVAL_SQQ", 5)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", diag), name
    assert (pkg.capi.EVAL_SD, pkg.capi.EVAL_CNT, pkg.capi.EVAL_SQ, pkg.capi.EVAL_SQQ) == (0, 1, 2, 5)
    assert pkg.capi.MOM_C + 20 < pkg.capi.ICP_NMOM


def test_python_mirror_signature(pkg):
    sig = inspect.signature(pkg.engine.Batch.evaluate)
    assert list(sig.parameters) == ["self", "max_distance", "metric", "want_matches"]
    assert sig.parameters["max_distance"].default is None
    assert sig.parameters["metric"].default == pkg.ICP_POINT_TO_POINT
    assert sig.parameters["want_matches"].default is False
    assert list(inspect.signature(pkg.engine.Batch.diag_eval_moments).parameters) == ["self", "b"]
