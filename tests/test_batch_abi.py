"""CPU: the batched point-to-point entry points (icp_batch_*, icp_point_to_point_batch) are declared, exported and bound, refuse
NULL handles without touching a device, and cannot be reached without a gfx950 device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
BATCH_SYMBOLS = ["icp_batch_begin", "icp_batch_create", "icp_batch_destroy", "icp_batch_done", "icp_batch_get_indices",
                 "icp_batch_get_moving", "icp_batch_loop_indices", "icp_batch_run", "icp_batch_state", "icp_point_to_point_batch"]


def test_batch_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    for name in BATCH_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
    assert lib.icp_abi_version() == 2   # additions only


def test_batch_max_points_constant(pkg):
    m = re.search(r"#define\s+ICP_BATCH_MAX_POINTS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 65536 == pkg.capi.ICP_BATCH_MAX_POINTS


def test_batch_null_handles_are_invalid(pkg):
    lib = pkg.load()
    bad = pkg.capi.ICP_ERR_INVALID
    prm = pkg.capi.icp_params(10, 1e-6, 0, pkg.ICP_F64, pkg.ICP_POINT_TO_POINT)
    k, a, st = C.c_int(0), C.c_int(0), C.c_int(0)
    buf = np.zeros(64)
    idx = np.zeros(8, dtype=np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert lib.icp_batch_begin(None, C.byref(prm)) == bad
    assert lib.icp_batch_run(None, 1, C.byref(k), C.byref(a)) == bad
    assert lib.icp_batch_state(None, 0, C.byref(st), None, None, None, 0, None) == bad
    assert lib.icp_batch_done(None, idx.ctypes.data_as(pi32)) == bad
    assert lib.icp_batch_get_moving(None, buf.ctypes.data) == bad
    assert lib.icp_batch_get_indices(None, idx.ctypes.data_as(pi32)) == bad
    assert lib.icp_batch_loop_indices(None, idx.ctypes.data_as(pi32)) == bad
    lib.icp_batch_destroy(None)   # a no-op
    # a NULL context: refused before anything is looked at, and no batch is handed out
    off = np.array([0, 4], dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    out = C.c_void_p(1234)
    assert lib.icp_batch_create(None, 1, buf.ctypes.data, off.ctypes.data_as(p64), buf.ctypes.data, off.ctypes.data_as(p64),
                                pkg.ICP_F64, C.byref(out)) == bad
    assert not out.value
    assert lib.icp_point_to_point_batch(None, 1, buf.ctypes.data, off.ctypes.data_as(p64), buf.ctypes.data, off.ctypes.data_as(p64),
                                        C.byref(prm), None, None, None, None, None, None, None) == bad


def test_batch_needs_a_device(pkg):
    """the batch entry points hang off a context, and a context without a gfx950 device fails loudly"""
    if pkg.load().icp_device_count() > 0:
        with pkg.Context(0) as ctx:   # a device: the batch is reachable, through a context
            assert ctx.batch([(np.zeros((3, 3)), np.ones((2, 3)))]).count == 1
        return
    with pytest.raises(pkg.IcpError) as e:
        pkg.Context(0)
    assert e.value.code == pkg.capi.ICP_ERR_NO_DEVICE
