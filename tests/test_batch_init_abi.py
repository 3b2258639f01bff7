"""CPU: the C ABI of a batch's initial transforms (icp_batch_set_initial_transforms) is declared, exported and bound, the ABI
version stays 2, a NULL batch is refused without a device, and the Python mirror carries the new method and parameters."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
SYMBOL = "icp_batch_set_initial_transforms"


def test_init_symbol_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    assert SYMBOL in declared
    assert SYMBOL in exported
    assert SYMBOL in pkg.capi.SIGNATURES and hasattr(lib, SYMBOL)
    res, args = pkg.capi.SIGNATURES[SYMBOL]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_double)]
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_init_null_batch_is_invalid(pkg):
    lib = pkg.load()
    T = np.ascontiguousarray(np.broadcast_to(np.eye(4), (2, 4, 4)))
    before = T.copy()
    assert lib.icp_batch_set_initial_transforms(None, T.ctypes.data_as(C.POINTER(C.c_double))) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_set_initial_transforms(None, None) == pkg.capi.ICP_ERR_INVALID
    assert np.array_equal(T, before)


def test_init_python_mirror(pkg):
    assert callable(getattr(pkg.engine.Batch, "set_initial_transforms"))
    assert list(inspect.signature(pkg.engine.Batch.set_initial_transforms).parameters) == ["self", "T"]
    for fn in (pkg.Context.point_to_point_batch, pkg.Context.point_to_plane_batch_gated):
        prm = inspect.signature(fn).parameters
        assert "init" in prm and prm["init"].default is None, fn.__name__
    # the gate's own parameters stay where they were
    assert inspect.signature(pkg.Context.point_to_point_batch).parameters["max_distance"].default is None
    assert list(inspect.signature(pkg.Context.point_to_plane_batch_gated).parameters)[:3] == ["self", "pairs", "max_distance"]
