"""CPU: the C ABI of voxel-grid downsampling (icp_batch_downsample, icp_batch_get_offsets, icp_batch_get_clouds) is declared,
exported and bound with exact ctypes signatures, the ABI version stays 2, the header states the rule, a NULL batch is refused
without a device with the outputs untouched, and the Python mirror carries the three additions while Batch.__init__ and
register_batch keep their parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
_pd, _p32, _p64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
SYMBOLS = {
    "icp_batch_downsample": [C.c_void_p, _pd, _pd, _p32, _p32, C.POINTER(C.c_void_p)],
    "icp_batch_get_offsets": [C.c_void_p, _p64, _p64],
    "icp_batch_get_clouds": [C.c_void_p, C.c_void_p, C.c_void_p],
}


def test_voxel_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    for name, want in SYMBOLS.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        res, args = pkg.capi.SIGNATURES[name]
        assert res is C.c_int and args == want, name
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("c = floor(((double)x - (double)lo) / v)", "floor(((double)hi - (double)lo) / v)", "<= 2097151", "first occurrence",
                   "bit for bit in numpy", "byte for byte", "a -0.0 survives", "s += (double)x_i over the members in ascending source index",
                   "(F)(s / (double)c)", "nothing is multiplied by a reciprocal", "no floating-point atomics", "exactly 0.0 copies",
                   "The loop does not notice", "four launches", "two host waits"):
        assert clause in text, clause


def test_voxel_null_batch_is_invalid(pkg):
    lib = pkg.load()
    v = np.full(2, 0.5)
    maps = np.full(8, -7, dtype=np.int32)
    out = C.c_void_p(0x1234)
    rc = lib.icp_batch_downsample(None, v.ctypes.data_as(_pd), v.ctypes.data_as(_pd), maps.ctypes.data_as(_p32), None, C.byref(out))
    assert rc == pkg.capi.ICP_ERR_INVALID and "null batch" in lib.icp_last_error().decode()
    assert out.value is None and (maps == -7).all() and (v == 0.5).all()   # *out is NULL on any refusal
    assert lib.icp_batch_downsample(None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID
    off = np.full(3, -7, dtype=np.int64)
    assert lib.icp_batch_get_offsets(None, off.ctypes.data_as(_p64), None) == pkg.capi.ICP_ERR_INVALID and (off == -7).all()
    buf = np.full((4, 3), -7.0, dtype=np.float32)
    assert lib.icp_batch_get_clouds(None, buf.ctypes.data, None) == pkg.capi.ICP_ERR_INVALID and (buf == -7.0).all()


def test_voxel_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.downsample).parameters
    assert list(prm) == ["self", "voxel", "voxel_model", "want_maps"]
    assert prm["voxel_model"].default is None and prm["want_maps"].default is False
    assert list(inspect.signature(B.get_clouds).parameters) == ["self"]
    prm = inspect.signature(Ctx.register_batch_multiscale).parameters
    assert list(prm) == ["self", "pairs", "voxels", "options"] and prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    # what existed keeps its parameter list
    assert list(inspect.signature(B.__init__).parameters) == ["self", "ctx", "pairs"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_robust).parameters) == ["self", "pairs", "kernel", "scale", "options"]
