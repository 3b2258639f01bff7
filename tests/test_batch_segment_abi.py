"""CPU: the C ABI of plane segmentation (icp_batch_segment_plane, icp_plane_rule, icp_plane_from_points, icp_plane_from_moments,
icp_diag_batch_segment) is declared, exported and bound with the exact ctypes signatures, the ABI version stays 2, the header states
the rule clause by clause, a NULL batch is refused without a device with every output untouched, and the Python mirror carries the
addition while what existed keeps its parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
_pd, _p32, _p8, _pi, _pu64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_uint64)


def test_segment_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(DIAG).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    rule = pkg.capi.icp_plane_rule
    want = {
        "icp_batch_segment_plane": [C.c_void_p, C.POINTER(rule), C.POINTER(rule), _pu64, _pd, _p32, _pi, _p8, _p8, _p32, _p32, C.POINTER(C.c_void_p)],
        "icp_plane_from_points": [_pd, _pd],
        "icp_plane_from_moments": [_pd, _pd, _pd],
        "icp_diag_batch_segment": [C.c_void_p, C.c_int, C.c_int, _p32, _p8, _pd, _p32],
    }
    for name, args in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name] == (C.c_int, args), name
    assert [(n, t) for n, t in rule._fields_] == [("kind", C.c_int), ("hypotheses", C.c_int), ("distance", C.c_double), ("axis", C.c_double * 3),
                                                  ("min_cos", C.c_double)]
    assert C.sizeof(rule) == 48
    assert re.search(r"typedef struct icp_plane_rule \{ int kind; int hypotheses; double distance; double axis\[3\]; double min_cos; \} icp_plane_rule;", src)
    for macro, value in (("ICP_PLANE_NONE", 0), ("ICP_PLANE_DETECT", 1), ("ICP_PLANE_REMOVE", 2), ("ICP_PLANE_KEEP", 3)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src) and getattr(pkg.capi, macro) == value, macro
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("draw(h, r) = mix(mix(mix(seed_p + side) + h) + r) % n", "side 0 for the moving cloud and 1 for the model", "sums modulo 2^64",
                   "a draw equal to an earlier slot is skipped", "at most 16 draws are used", "fewer than three distinct indices make the hypothesis invalid",
                   "u = b - a, v = c - a", "w = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx)", "l = sqrt((wx*wx + wy*wy) + wz*wz)",
                   "invalid unless l > 0 and l is finite", "a triple out of the heap at the origin is invalid",
                   "a plane through the origin still counts every point of the heap", "dropping zero returns is the caller's job",
                   "n = w / l, three divisions", "negated iff the component of largest magnitude is negative",
                   "the lowest index decides among equal magnitudes", "d = -((nx*ax + ny*ay) + nz*az)", "l leaves the double range",
                   "Such hypotheses are invalid, not wrong", "axis == (0, 0, 0) means none", "fabs((nx*ahx + ny*ahy) + nz*ahz) >= min_cos",
                   "s_i = ((nx*x + ny*y) + nz*z) + d", "fabs(s_i) <= distance", "A point on the threshold is in, a NaN is out",
                   "the largest count, the lowest h among equals", "With no valid hypothesis the cloud's status is ICP_ERR_EMPTY",
                   "such a cloud is copied", "granules of 64 consecutive points from the cloud's first point",
                   "each granule added from 0.0 in ascending index", "the granule sums added from 0.0 in ascending order", "c = S / (double)k",
                   "each divided once by (double)k", "icp_eigh3's eigenvector of the smallest eigenvalue", "a refit that fails it is dropped",
                   "returns the refit if its count is at least the winner's, else the winner", "The mask is the returned plane's",
                   "nothing is fused, nothing is multiplied by a reciprocal", "+ - * / sqrt fabs", "-1 for a removed point", "a -0.0 survives",
                   "copied, not computed", "The loop does not notice", "no output array is written", "names the first offending pair and the side",
                   "null seeds where any rule searches", "hypotheses outside [1, 65536]", "min_cos outside [0, 1]", "a searched cloud of n < 3",
                   "an ICP_PLANE_REMOVE cloud whose every point is an inlier", "an ICP_PLANE_KEEP cloud with no plane",
                   "its pair's seed and its side alone", "as if icp_batch_create had been called", "five for up to 4096 hypotheses",
                   "No floating-point atomics", "bit for bit (tests/batch_segment_ref.py)"):
        assert clause in text, clause


def test_segment_null_batch_is_invalid(pkg):
    lib = pkg.load()
    rule = pkg.capi.icp_plane_rule
    ax = (C.c_double * 3)(0.0, 0.0, 1.0)
    rules = (rule * 2)(rule(2, 100, 0.02, ax, 0.9), rule(3, 7, 0.5, ax, 0.0))
    seed = np.array([5, 6], dtype=np.uint64)
    planes, inl, st = np.full(16, -7.0), np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.intc)
    mask, maps = np.full(8, 9, dtype=np.uint8), np.full(8, -7, dtype=np.int32)
    out = C.c_void_p(0x1234)
    rc = lib.icp_batch_segment_plane(None, rules, rules, seed.ctypes.data_as(_pu64), planes.ctypes.data_as(_pd), inl.ctypes.data_as(_p32),
                                     st.ctypes.data_as(_pi), mask.ctypes.data_as(_p8), mask.ctypes.data_as(_p8), maps.ctypes.data_as(_p32),
                                     maps.ctypes.data_as(_p32), C.byref(out))
    assert rc == pkg.capi.ICP_ERR_INVALID and "null batch" in lib.icp_last_error().decode()
    assert out.value is None   # *out is NULL on any refusal
    assert (planes == -7.0).all() and (inl == -7).all() and (st == -7).all() and (mask == 9).all() and (maps == -7).all()
    assert (rules[0].kind, rules[0].hypotheses, rules[0].distance, rules[0].axis[2], rules[0].min_cos, rules[1].kind) == (2, 100, 0.02, 1.0, 0.9, 3)
    assert lib.icp_batch_segment_plane(None, None, None, None, None, None, None, None, None, None, None, None) == pkg.capi.ICP_ERR_INVALID
    assert lib.icp_diag_batch_segment(None, 0, 0, None, None, None, None) == pkg.capi.ICP_ERR_INVALID
    four = np.full(4, -7.0)
    assert lib.icp_plane_from_points(None, four.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID and (four == -7.0).all()
    assert lib.icp_plane_from_moments(None, None, four.ctypes.data_as(_pd)) == pkg.capi.ICP_ERR_INVALID and (four == -7.0).all()


def test_segment_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.segment_plane).parameters
    assert list(prm) == ["self", "moving", "model", "seed", "want_masks", "want_maps"]
    assert prm["moving"].default is None and prm["model"].default is None and prm["seed"].default == 0
    assert prm["want_masks"].default is False and prm["want_maps"].default is False
    assert list(inspect.signature(B.diag_segment).parameters) == ["self", "b", "side"]
    assert list(inspect.signature(pkg.plane_from_points).parameters) == ["abc"]
    assert list(inspect.signature(pkg.plane_from_moments).parameters) == ["centroid", "cov6"]
    assert "planes=rule" in Ctx.register_batch_global.__doc__
    # what existed keeps its parameter list
    assert list(inspect.signature(Ctx.register_batch_global).parameters) == ["self", "pairs", "voxel", "k", "hypotheses", "max_distance", "options"]
    assert list(inspect.signature(B.remove_outliers).parameters) == ["self", "moving", "model", "want_maps", "want_scores"]
    assert list(inspect.signature(B.keypoints).parameters) == ["self", "moving", "model", "want_maps", "want_saliency"]
    assert list(inspect.signature(B.downsample).parameters) == ["self", "voxel", "voxel_model", "want_maps"]
    assert list(inspect.signature(B.diag_ransac).parameters) == ["self", "b"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
