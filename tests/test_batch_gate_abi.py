"""CPU: the batch gate's C ABI (icp_batch_set_max_distance, icp_batch_get_inliers, icp_batch_loop_inliers) is declared, exported and
bound and refuses NULL handles without a device; and the host loop divides a pass's error by the count of the matches it measures
-- the PREVIOUS vector's ICP_MOM_CNT -- without moving a bit of any loop whose count never changes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ref_moments as rm
from clouds import ragged_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
GATE_SYMBOLS = ["icp_batch_set_max_distance", "icp_batch_get_inliers", "icp_batch_loop_inliers"]
GOLDEN_CASES = {   # tests/golden/make_host_loop_vectors.py: name -> (plane, fp64, max_iter, tol, fixed)
    "p2p_f32_fixed": (False, False, 5, 0.0, True),
    "p2p_f64_stop": (False, True, 12, 1e-4, False),
    "plane_f32_fixed": (True, False, 4, 0.0, True),
    "plane_f64_stop": (True, True, 12, 1e-4, False),
}


def test_gate_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    for name in GATE_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
    assert lib.icp_abi_version() == 2   # additions only
    assert lib.icp_strerror(pkg.capi.ICP_ERR_EMPTY).decode() == "no model point, or no correspondence within the maximum distance"


def test_gate_null_handles_are_invalid(pkg):
    lib = pkg.load()
    bad = pkg.capi.ICP_ERR_INVALID
    md = np.array([0.05, np.inf])
    mask = np.zeros(8, dtype=np.uint8)
    pu8 = C.POINTER(C.c_uint8)
    assert lib.icp_batch_set_max_distance(None, md.ctypes.data_as(C.POINTER(C.c_double))) == bad
    assert lib.icp_batch_set_max_distance(None, None) == bad
    assert lib.icp_batch_get_inliers(None, mask.ctypes.data_as(pu8)) == bad
    assert lib.icp_batch_loop_inliers(None, mask.ctypes.data_as(pu8)) == bad
    assert lib.icp_batch_get_inliers(None, None) == bad
    assert lib.icp_batch_loop_inliers(None, None) == bad
    assert not mask.any()


def test_host_loop_divides_the_error_by_the_previous_count(pkg):
    """vectors whose ICP_MOM_CNT differs from pass to pass, as a gated batch delivers them: err[k] = sqrt(ERR_k) / sqrt(CNT_{k-1}).
    (Before the gate the divisor was the current vector's count.)"""
    D, M = (a.astype(np.float64) for a in ragged_pair(200300, 200, 300))
    rng = np.random.default_rng(9)
    idx = rng.integers(0, M.shape[0], size=D.shape[0])
    terms = rm.p2p_point_terms(D, M, idx, idx)
    counts = [29, 200, 150, 64, 199]
    loop = pkg.distributed.HostLoop(max_iter=len(counts), tol=0.0, fixed_iterations=True, precision=pkg.ICP_F64)
    moms = []
    for k, c in enumerate(counts + [0]):
        mom = terms[rng.permutation(D.shape[0])[:max(c, 1)]].sum(axis=0)
        mom[rm.ERR] = 0.0 if k == 0 else 0.37 * (k + 1)
        if c == 0:   # the loop's last pass: the error alone
            mom[1:] = 0.0
        assert mom[rm.CNT] == float(c)
        moms.append(mom)
        done, _, _ = loop.advance(mom)
        assert done == (c == 0)
        if not done:
            loop.note_applied()
    err = loop.state()["err"]
    assert err.shape == (len(counts) + 1,) and err[0] == 0.0
    for k in range(1, len(counts) + 1):
        assert counts[k - 1] != (counts + [0])[k]
        assert err[k] == np.sqrt(moms[k][rm.ERR]) / np.sqrt(float(counts[k - 1])), k


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_host_loop_constant_count_bytes(pkg, golden, name):
    """fed vectors whose count is the same in every pass, every byte of done, R, t, err, T, iterations and passes is what the build
    before the gate returned (recorded by tests/golden/make_host_loop_vectors.py)"""
    plane, fp64, max_iter, tol, fixed = GOLDEN_CASES[name]
    z = np.load(os.path.join(golden, "host_loop_vectors.npz"))
    moms = z[f"{name}.mom"]
    counts = moms[:, rm.CNT]
    assert len(set(counts[counts > 0].tolist())) == 1 and moms.shape[0] >= 3
    loop = pkg.distributed.HostLoop(metric=pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT, max_iter=max_iter, tol=tol,
                                    fixed_iterations=fixed, precision=pkg.ICP_F64 if fp64 else pkg.ICP_F32)
    for k, mom in enumerate(moms):
        done, R, t = loop.advance(mom)
        assert done == bool(z[f"{name}.done"][k]), k
        assert R.reshape(9).tobytes() == z[f"{name}.R"][k].tobytes() and t.tobytes() == z[f"{name}.t"][k].tobytes(), k
        if not done:
            loop.note_applied()
    assert done
    st = loop.state()
    assert st["iterations"] == int(z[f"{name}.iterations"]) and st["passes"] == int(z[f"{name}.passes"])
    assert st["err"].tobytes() == z[f"{name}.err"].tobytes()
    assert np.ascontiguousarray(st["T"]).tobytes() == np.ascontiguousarray(z[f"{name}.T"]).tobytes()
