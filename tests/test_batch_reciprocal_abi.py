"""CPU: the C ABI of a batch's reciprocal matches (icp_batch_set_reciprocal, icp_diag_batch_reverse) is declared, exported and
bound with the exact ctypes signatures, the ABI version stays 2, a NULL batch is refused without a device, and the Python mirror
carries the two methods and the one-call entry that takes every option (Context.register_batch) -- while the earlier one-call
functions keep their parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
SYMBOL = "icp_batch_set_reciprocal"
DIAG_SYMBOL = "icp_diag_batch_reverse"


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))


def test_reciprocal_symbols_declared_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    assert SYMBOL in _declared(HEADER)
    assert DIAG_SYMBOL in _declared(DIAG)
    for s in (SYMBOL, DIAG_SYMBOL):
        assert s in exported
        assert s in pkg.capi.SIGNATURES and hasattr(lib, s)
    res, args = pkg.capi.SIGNATURES[SYMBOL]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_uint8)]
    res, args = pkg.capi.SIGNATURES[DIAG_SYMBOL]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_int32)]
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_reciprocal_header_states_the_rule():
    text = open(HEADER).read()
    assert "rev[idx[i]] == i" in text and "bit for bit" in text
    assert re.search(r"int\s+icp_batch_set_reciprocal\(icp_batch\*\s*b,\s*const uint8_t\*\s*on\);", text)
    assert re.search(r"int\s+icp_diag_batch_reverse\(icp_batch\*\s*b,\s*int32_t\*\s*rev_out\);", open(DIAG).read())


def test_reciprocal_null_batch_is_invalid(pkg):
    lib = pkg.load()
    v = np.array([1, 0], dtype=np.uint8)
    before = v.copy()
    assert lib.icp_batch_set_reciprocal(None, v.ctypes.data_as(C.POINTER(C.c_uint8))) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_set_reciprocal(None, None) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    rev = np.full(4, 7, dtype=np.int32)
    assert lib.icp_diag_batch_reverse(None, rev.ctypes.data_as(C.POINTER(C.c_int32))) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert np.array_equal(v, before) and (rev == 7).all()


def test_reciprocal_python_mirror(pkg):
    assert list(inspect.signature(pkg.engine.Batch.set_reciprocal).parameters) == ["self", "v"]
    assert list(inspect.signature(pkg.engine.Batch.diag_reverse).parameters) == ["self"]
    prm = inspect.signature(pkg.Context.register_batch).parameters
    assert list(prm) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations", "max_distance", "init", "trim",
                         "reciprocal"]
    want = dict(metric=pkg.ICP_POINT_TO_POINT, normals=None, max_iter=None, tol=1e-6, fixed_iterations=False, max_distance=None,
                init=None, trim=None, reciprocal=None)
    for name, default in want.items():
        assert prm[name].default == default and type(prm[name].default) is type(default), name
        assert prm[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    assert prm["pairs"].default is inspect.Parameter.empty
    gated = inspect.signature(pkg.Context._run_batch_gated).parameters
    assert list(gated)[-1] == "reciprocal" and gated["reciprocal"].default is None
    # the earlier one-call functions keep their lists: trim stays their last parameter, keyword-only ones included
    for fn in (pkg.Context.point_to_point_batch, pkg.Context.point_to_plane_batch_gated):
        assert list(inspect.signature(fn).parameters)[-1] == "trim", fn.__name__
        assert "reciprocal" not in inspect.signature(fn).parameters, fn.__name__
