"""CPU: the C ABI of a batch's robust kernels (icp_batch_set_robust, icp_batch_get_weights, icp_host_loop_set_weighted, the
ICP_ROBUST_* constants and slot ICP_MOM_W) is declared, exported and bound with the exact ctypes signatures, the ABI version stays
2, a NULL batch is refused without a device, the Python mirror carries Batch.set_robust, Batch.get_weights and
Context.register_batch_robust while the earlier entries keep their parameter lists -- and the host loop, which needs no device,
solves a weighted vector with W in the place of CNT."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import batch_robust_ref as br
import ref_moments as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
SYMBOLS = {
    "icp_batch_set_robust": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)],
    "icp_batch_get_weights": [C.c_void_p, C.POINTER(C.c_double)],
    "icp_host_loop_set_weighted": [C.c_void_p, C.c_int],
}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))


def test_robust_symbols_declared_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    declared = _declared(HEADER)
    for s, want in SYMBOLS.items():
        assert s in declared and s in exported
        assert s in pkg.capi.SIGNATURES and hasattr(lib, s)
        res, args = pkg.capi.SIGNATURES[s]
        assert res is C.c_int and args == want, s
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_robust_header_states_the_contract(pkg):
    text = open(HEADER).read()
    for name, value in (("ICP_ROBUST_NONE", 0), ("ICP_ROBUST_HUBER", 1), ("ICP_ROBUST_CAUCHY", 2), ("ICP_ROBUST_TUKEY", 3), ("ICP_MOM_W", 29)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(pkg.capi, name) == value
    assert (br.NONE, br.HUBER, br.CAUCHY, br.TUKEY, br.MOM_W) == (0, 1, 2, 3, 29)
    assert re.search(r"int\s+icp_batch_set_robust\(icp_batch\*\s*b,\s*const int\*\s*kind,\s*const double\*\s*scale\);", text)
    assert re.search(r"int\s+icp_batch_get_weights\(icp_batch\*\s*b,\s*double\*\s*w_out\);", text)
    assert re.search(r"int\s+icp_host_loop_set_weighted\(icp_host_loop\*\s*h,\s*int\s+on\);", text)
    assert "k / sqrt(r2)" in text and "1 / (1 + r2 / k2)" in text and "(1 - r2/k2)^2" in text
    assert "ICP_MOM_W" in open(DIAG).read()


def test_robust_null_batch_is_invalid(pkg):
    lib = pkg.load()
    kind = np.array([1, 0], dtype=np.intc)
    scale = np.array([0.5, 0.5])
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    assert lib.icp_batch_set_robust(None, kind.ctypes.data_as(pi), scale.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_batch_set_robust(None, None, None) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    w = np.full(4, 7.0)
    assert lib.icp_batch_get_weights(None, w.ctypes.data_as(pd)) == pkg.capi.ICP_ERR_INVALID
    assert "null batch" in lib.icp_last_error().decode()
    assert (w == 7.0).all() and np.array_equal(kind, [1, 0])
    assert lib.icp_host_loop_set_weighted(None, 1) == pkg.capi.ICP_ERR_INVALID


def test_robust_python_mirror(pkg):
    assert list(inspect.signature(pkg.engine.Batch.set_robust).parameters) == ["self", "kind", "scale"]
    assert list(inspect.signature(pkg.engine.Batch.get_weights).parameters) == ["self"]
    prm = inspect.signature(pkg.Context.register_batch_robust).parameters
    assert list(prm) == ["self", "pairs", "kernel", "scale", "options"]
    assert prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(pkg.distributed.HostLoop.set_weighted).parameters) == ["self", "on"]
    # the earlier entries keep their lists (tests/test_batch_reciprocal_abi.py holds them; restated for the two this change is near)
    assert list(inspect.signature(pkg.Context.register_batch).parameters)[-1] == "reciprocal"
    assert list(inspect.signature(pkg.Context._run_batch_gated).parameters)[-1] == "reciprocal"


# ---- the host loop, device-free, on hand-made vectors -------------------------------------------------------------------------------
def _vector(seed, err, w_share):
    """a point-to-point vector of 50 kept points whose sums carry the weights w (W = sum w < CNT)"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((50, 3))
    a = 0.05
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Q = P @ R.T + np.array([0.02, -0.01, 0.03]) + 1e-3 * rng.standard_normal((50, 3))
    w = np.clip(rng.random(50) * w_share, 0.0, 1.0)
    mom, _ = br.weighted(False, P, Q, None, np.arange(50), w)
    mom[rm.ERR] = err
    return mom


def test_host_loop_weighted_solves_on_the_weight_sum(pkg):
    H = pkg.distributed.HostLoop
    moms = [_vector(1, 0.0, 1.0), _vector(2, 50 * 0.04, 0.7), _vector(3, 50 * 0.01, 0.9)]
    for m in moms:
        assert 0 < m[br.MOM_W] < m[rm.CNT] == 50.0
    told, plain, off = H(max_iter=10, tol=1e-9, precision=pkg.ICP_F64), H(max_iter=10, tol=1e-9, precision=pkg.ICP_F64), H(max_iter=10, tol=1e-9, precision=pkg.ICP_F64)
    told.set_weighted(1)
    off.set_weighted(1)
    off.set_weighted(0)
    for k, m in enumerate(moms):
        done, R, t = told.advance(m)
        assert not done
        Rw, tw = pkg.solve_point_to_point(br.with_cnt_from_w(m))
        assert R.tobytes() == np.asarray(Rw).reshape(3, 3).tobytes() and t.tobytes() == np.asarray(tw).tobytes(), k
        # the flag off: the answers of a loop never told, which solve on the vector as delivered
        (d0, R0, t0), (d1, R1, t1) = plain.advance(m), off.advance(m)
        R_plain, t_plain = pkg.solve_point_to_point(m)
        assert R0.tobytes() == R1.tobytes() == np.asarray(R_plain).reshape(3, 3).tobytes() and t0.tobytes() == t1.tobytes() == np.asarray(t_plain).tobytes()
        assert not d0 and not d1 and t0.tobytes() != t.tobytes()   # (dividing by W < CNT moves t)
        for h in (told, plain, off):
            h.note_applied()
    # err[k] = sqrt(ERR_k) / sqrt(CNT_{k-1}): the kept count, not the weight sum -- and the same in all three loops
    want = [0.0, np.sqrt(moms[1][rm.ERR]) / np.sqrt(50.0), np.sqrt(moms[2][rm.ERR]) / np.sqrt(50.0)]
    for h in (told, plain, off):
        st = h.state()
        assert st["passes"] == 3 and st["iterations"] == 2
        assert np.array_equal(st["err"][:3], want)
    assert told.state()["T"].tobytes() != plain.state()["T"].tobytes() and plain.state()["T"].tobytes() == off.state()["T"].tobytes()
    for h in (told, plain, off):
        h.close()


def test_host_loop_weight_sum_zero_is_empty(pkg):
    H = pkg.distributed.HostLoop
    m = _vector(4, 0.0, 1.0)
    dead = m.copy()
    dead[br.MOM_W] = 0.0
    for metric in (pkg.ICP_POINT_TO_POINT, pkg.ICP_POINT_TO_PLANE):
        h = H(metric=metric, max_iter=10, tol=1e-9, precision=pkg.ICP_F64)
        h.set_weighted(True)
        try:
            h.advance(dead)
            raise AssertionError("a matching pass whose weights add up to 0 must end the loop")
        except pkg.IcpError as e:
            assert e.code == pkg.capi.ICP_ERR_EMPTY
        h.close()
    # not told: W is not looked at
    h = H(max_iter=10, tol=1e-9, precision=pkg.ICP_F64)
    done, R, t = h.advance(dead)
    assert not done and np.isfinite(R).all()
    h.close()
    # the stop rule ended the loop on that very pass: ICP_OK, as for the count
    h = H(max_iter=10, tol=1e-3, precision=pkg.ICP_F64)
    h.set_weighted(True)
    h.advance(m)
    h.note_applied()
    dead[rm.ERR] = 50 * 1e-10
    done, _, _ = h.advance(dead)
    assert done and h.state()["iterations"] == 0
    h.close()
