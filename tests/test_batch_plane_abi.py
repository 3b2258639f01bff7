"""CPU: the batched point-to-plane entry points (icp_batch_set_model_normals, icp_batch_estimate_normals,
icp_point_to_plane_batch) are declared, exported and bound, the ABI version is unchanged (additions only), NULL handles are
refused without touching a device, and the Python mirror offers them."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
PLANE_SYMBOLS = ["icp_batch_set_model_normals", "icp_batch_estimate_normals", "icp_point_to_plane_batch"]


def test_plane_batch_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    for name in PLANE_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
    assert lib.icp_abi_version() == 2   # additions only
    m = re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 2


def test_plane_batch_null_handles_are_invalid(pkg):
    lib = pkg.load()
    bad = pkg.capi.ICP_ERR_INVALID
    buf = np.zeros(64)
    nbr = np.zeros(16, dtype=np.int32)
    assert lib.icp_batch_set_model_normals(None, buf.ctypes.data) == bad
    assert lib.icp_batch_set_model_normals(None, None) == bad
    assert lib.icp_batch_estimate_normals(None, buf.ctypes.data, nbr.ctypes.data_as(C.POINTER(C.c_int32))) == bad
    assert lib.icp_batch_estimate_normals(None, None, None) == bad
    # a NULL context: refused before anything is looked at, whatever the metric says
    off = np.array([0, 4], dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    for metric in (pkg.ICP_POINT_TO_PLANE, pkg.ICP_POINT_TO_POINT):
        prm = pkg.capi.icp_params(10, 1e-6, 0, pkg.ICP_F64, metric)
        for normals in (buf.ctypes.data, None):
            assert lib.icp_point_to_plane_batch(None, 1, buf.ctypes.data, off.ctypes.data_as(p64), buf.ctypes.data, off.ctypes.data_as(p64), normals,
                                                C.byref(prm), None, None, None, None, None, None, None) == bad
    assert b"null context" in lib.icp_last_error()


def test_plane_batch_python_mirror(pkg):
    from_ctx = inspect.signature(pkg.Context.point_to_plane_batch).parameters
    assert list(from_ctx)[1:] == ["pairs", "normals", "max_iter", "tol", "fixed_iterations"]
    assert from_ctx["normals"].default is None and from_ctx["max_iter"].default == 50
    Batch = sys.modules[pkg.Context.__module__].Batch
    assert inspect.signature(Batch.begin).parameters["metric"].default == pkg.capi.ICP_POINT_TO_POINT   # the default is unchanged
    assert "want_neighbours" in inspect.signature(Batch.estimate_normals).parameters
    assert callable(Batch.set_model_normals)
