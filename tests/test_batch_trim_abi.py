"""CPU: the C ABI of a batch's trimmed rejection (icp_batch_set_trim, icp_diag_batch_trim) is declared, exported and bound, the
ABI version stays 2, a NULL batch is refused without a device, the Python mirror carries the new method and parameter, and the
rank rule of the header -- K = ceil(rho * (double)n), clamped to [1, n] -- gives the figures the GPU tests build on."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
SYMBOL = "icp_batch_set_trim"
DIAG_SYMBOL = "icp_diag_batch_trim"


def rank(rho, n):
    """the header's rule: the product in double, rounded up, clamped to [1, n]"""
    return min(max(int(math.ceil(float(rho) * float(n))), 1), n)


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))


def test_trim_symbols_declared_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    assert SYMBOL in _declared(HEADER)
    assert DIAG_SYMBOL in _declared(DIAG)
    for s in (SYMBOL, DIAG_SYMBOL):
        assert s in exported
        assert s in pkg.capi.SIGNATURES and hasattr(lib, s)
    res, args = pkg.capi.SIGNATURES[SYMBOL]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_double)]
    res, args = pkg.capi.SIGNATURES[DIAG_SYMBOL]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_trim_header_no_longer_says_a_batch_cannot_trim():
    text = open(HEADER).read()
    assert "There is no trimmed" not in text
    assert SYMBOL in text


def test_trim_null_batch_is_invalid(pkg):
    lib = pkg.load()
    v = np.array([0.5, 1.0])
    before = v.copy()
    assert lib.icp_batch_set_trim(None, v.ctypes.data_as(C.POINTER(C.c_double))) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_set_trim(None, None) == pkg.capi.ICP_ERR_INVALID
    tau, k = C.c_double(0.0), C.c_int(0)
    assert lib.icp_diag_batch_trim(None, 0, C.byref(tau), C.byref(k)) == pkg.capi.ICP_ERR_INVALID
    assert np.array_equal(v, before)


def test_trim_python_mirror(pkg):
    assert callable(getattr(pkg.engine.Batch, "set_trim"))
    assert list(inspect.signature(pkg.engine.Batch.set_trim).parameters) == ["self", "v"]
    assert list(inspect.signature(pkg.engine.Batch.diag_trim).parameters) == ["self", "b"]
    for fn in (pkg.Context.point_to_point_batch, pkg.Context.point_to_plane_batch_gated):
        prm = inspect.signature(fn).parameters
        assert "trim" in prm and prm["trim"].default is None, fn.__name__
        assert list(prm)[-1] == "trim", fn.__name__   # trailing: the earlier positions stay where they were
    # the gate's and the initial transforms' parameters stay where they were
    assert inspect.signature(pkg.Context.point_to_point_batch).parameters["max_distance"].default is None
    assert inspect.signature(pkg.Context.point_to_point_batch).parameters["init"].default is None
    assert list(inspect.signature(pkg.Context.point_to_plane_batch_gated).parameters)[:3] == ["self", "pairs", "max_distance"]


def test_trim_rank_rule():
    assert rank(0.5, 270) == 135
    for n in (1, 2, 63, 270, 4097, 65536):
        for K in sorted({1, min(2, n), max(1, n // 2), max(1, n - 1), n}):
            assert rank((K - 0.5) / n, n) == K, (n, K)   # rho * n lies strictly between K - 1 and K
        assert rank(1.0 - 1e-9, n) == n
        assert rank(1.0, n) == n
        assert rank(1e-300, n) == 1 and rank(5e-324, n) == 1   # a tiny share still keeps one point
    assert rank(0.3, 200) == 60
