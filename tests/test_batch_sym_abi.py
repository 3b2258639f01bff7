"""CPU: the C ABI of the symmetric metric (ICP_SYMMETRIC, icp_solve_symmetric, icp_host_loop_set_symmetric) is declared, exported and
bound with the exact ctypes signatures, the ABI version stays 2, the header states the rule, icp_solve_symmetric is the numpy
statements bit for bit, a host loop with the flag on registers the scene as the numpy loop does, the host loop still refuses the
values 3 and 4 as metrics, and the Python mirror carries the additions while what existed keeps its parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import batch_sym_ref as sr
import ref_moments as rm
from batch_ref import TOL_T, bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
_pd = C.POINTER(C.c_double)


def test_sym_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    want = {"icp_solve_symmetric": (C.c_int, [_pd, _pd, _pd, _pd]),
            "icp_host_loop_set_symmetric": (C.c_int, [C.c_void_p, C.c_int])}
    for name, (res, args) in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name][0] is res and pkg.capi.SIGNATURES[name][1] == args, name
    for decl in ("int icp_solve_symmetric(const double* mom , double* R9, double* t3, double* x6);",
                 "int icp_host_loop_set_symmetric(icp_host_loop* h, int on);"):
        assert decl in src, decl
    assert re.search(r"#define\s+ICP_SYMMETRIC\s+4\b", src) and pkg.capi.ICP_SYMMETRIC == 4 and pkg.ICP_SYMMETRIC == 4
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())
    assert re.search(r"typedef enum \{ ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1 \} icp_metric;", src)   # the enum is as it was


def test_header_states_the_rule():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("icp_batch_begin with ICP_SYMMETRIC needs point normals on both sides",
                   "the message names the side and the two calls that provide them",
                   "icp_batch_set_point_normals and icp_batch_estimate_point_normals discard it",
                   "batch_sym_moments, the reduction up to ICP_MOM_B + 5", "three launches, up to five, one download",
                   "Every operation is one IEEE double operation, nothing is fused, and the only functions used are + - *",
                   "dot(a, b) = (a0*b0 + a1*b1) + a2*b2", "np_a = dot(Rc[a], m0)", "np == m0 bit for bit",
                   "s = dot(np, nq); n_a = s < 0 ? nq_a - np_a : nq_a + np_a", "the sign rule is always on",
                   "e = p - q, g = p + q componentwise, h = dot(e, n)", "v0 = g1*n2 - g2*n1, v1 = g2*n0 - g0*n2, v2 = g0*n1 - g1*n0, v3..5 = n",
                   "Slot C(a, c) += v_a*v_c for a <= c; slot B(a) -= v_a*h; ICP_MOM_CNT = 1",
                   "A kept match whose n is exactly zero counts and adds zeros", "The points are not centred",
                   "a solution that is not finite, or whose l2 is not finite, is ICP_ERR_SINGULAR too",
                   "l2 = (a0*a0 + a1*a1) + a2*a2, c = 1.0 / sqrt(1.0 + l2), k = (c*c) / (1.0 + c)", "Ra_ab = c*E_ab + k*(a_a*a_b)",
                   "t'_a = c*tt_a; R = Ra Ra and t = Ra t', each entry a dot of a row with a column",
                   "the motion is p -> Ra (Ra p + t'), and a = 0 gives the identity"):
        assert clause in text, clause


def _call_solve(lib, mom, x6=True):
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    R, t, x = np.full(9, -7.0), np.full(3, -7.0), np.full(6, -7.0)
    rc = lib.icp_solve_symmetric(mom.ctypes.data_as(_pd), R.ctypes.data_as(_pd), t.ctypes.data_as(_pd), x.ctypes.data_as(_pd) if x6 else None)
    return rc, R.reshape(3, 3), t, x


def _system_vector(rng, n=40, scale=1.0):
    """the vector of n random symmetric matches: a well-posed 6 x 6 system"""
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    P, Q = rng.standard_normal((n, 3)) * scale, rng.standard_normal((n, 3)) * scale
    t = sr.terms(P, Q, unit(rng.standard_normal((n, 3))), unit(rng.standard_normal((n, 3))), np.arange(n), np.eye(3))
    return t.sum(axis=0)


def test_solve_symmetric_is_the_stated_statements_bit_for_bit(pkg):
    lib = pkg.load()
    rng = np.random.default_rng(5)
    largest = 0.0
    for k in range(40):
        mom = _system_vector(rng, 12 + k, scale=(0.01, 1.0, 30.0)[k % 3])
        rc, R, t, x = _call_solve(lib, mom)
        assert rc == pkg.capi.ICP_OK, k
        Cm, b = sr.system(mom)
        assert np.abs(Cm @ x - b).max() <= 1e-9 * np.abs(b).max(), k                 # x solves the slots' system
        wantR, wantt = sr.motion(x)
        assert bits_equal(R, wantR) and bits_equal(t, wantt), k                      # + - * / sqrt, contraction off
        largest = max(largest, float(np.linalg.norm(x[:3])))
        R2, t2, x2 = pkg.solve_symmetric(mom)
        assert bits_equal(R2, R) and bits_equal(t2, t) and bits_equal(x2, x)
        xp = pkg.solve_point_to_plane(mom)[2]
        assert bits_equal(xp, x), k                                                  # the plane solve's Cholesky
        rc, R3, t3, _ = _call_solve(lib, mom, x6=False)                              # x6 may be NULL
        assert rc == pkg.capi.ICP_OK and bits_equal(R3, R) and bits_equal(t3, t)
    assert largest > 0.5   # (rotations far from the small-angle range are among them)


def test_solve_symmetric_refusals(pkg):
    lib = pkg.load()
    INV, SING = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_SINGULAR
    mom = _system_vector(np.random.default_rng(6))
    v = np.zeros(9)
    p = v.ctypes.data_as(_pd)
    assert lib.icp_solve_symmetric(None, p, p, p) == INV
    assert lib.icp_solve_symmetric(mom.ctypes.data_as(_pd), None, p, p) == INV
    assert lib.icp_solve_symmetric(mom.ctypes.data_as(_pd), p, None, p) == INV
    assert _call_solve(lib, np.zeros(rm.NMOM))[0] == SING                            # no match at all
    flat = sr.terms(np.zeros((9, 3)) + np.arange(9)[:, None] * np.array([1.0, 0.5, 0.0]), np.zeros((9, 3)), np.tile([0.0, 0.0, 1.0], (9, 1)),
                    np.tile([0.0, 0.0, 1.0], (9, 1)), np.arange(9), np.eye(3)).sum(axis=0)
    assert _call_solve(lib, flat)[0] == SING                                         # parallel normals: a zero pivot
    big = mom.copy()
    big[rm.MB:rm.MB + 3] = 1e300                                                     # |a|^2 leaves the range
    rc, R, t, x = _call_solve(lib, big)
    assert rc == SING and (R == -7.0).all() and (t == -7.0).all()
    nan = mom.copy()
    nan[rm.MB + 4] = np.nan
    assert _call_solve(lib, nan)[0] == SING


def _host_loop_run(pkg, orc, sc, symmetric, passes):
    """the device-free loop driven by hand on the scene: orc.nn, the numpy terms, icp_host_loop_advance, the motion applied in
    double; the rotation error after every pass"""
    hl = pkg.distributed.HostLoop(metric=pkg.capi.ICP_POINT_TO_PLANE, max_iter=passes, tol=0.0, fixed_iterations=True, precision=pkg.capi.ICP_F64)
    if symmetric:
        hl.set_symmetric(True)
    P, T, ang, prev = sc["A"].copy(), np.eye(4), [], None
    try:
        for _ in range(passes):
            idx = orc.nn(P, sc["M"])
            t = sr.terms(P, sc["M"], sc["Np"], sc["Nq"], idx, T[:3, :3])
            mom = t.sum(axis=0)
            mom[rm.ERR] = 0.0 if prev is None else float(((sc["M"][prev] - P) ** 2).sum())
            done, R, tr = hl.advance(mom)
            if done:
                break
            P = P @ R.T + tr
            hl.note_applied()
            T = hl.state()["T"]
            ang.append(sr.angle_deg(T[:3, :3], sc["R"]))
            prev = idx
    finally:
        hl.close()
    return ang


def test_host_loop_with_the_flag_registers_the_scene(pkg, orc):
    sc = sr.scene(np.float64)
    passes = 6
    want = sr.reference_loop(orc, sc["A"], sc["M"], sc["Np"], sc["Nq"], passes, 0.0, truth=sc["R"])["ang"]
    got = _host_loop_run(pkg, orc, sc, True, passes)
    print(f"[sym host loop] rotation error per pass: {['%.4g' % a for a in got]} numpy {['%.4g' % a for a in want[:len(got)]]}")
    assert len(got) >= passes - 1
    for k, a in enumerate(got):
        assert abs(a - want[k]) < TOL_T, (k, a, want[k])
    assert got[1] < 0.1 and got[-1] < 1e-3
    # without the flag the same vectors go through the plane solve's Euler angles: another loop
    off = _host_loop_run(pkg, orc, sc, False, passes)
    assert abs(off[0] - want[0]) > 100 * TOL_T


def test_host_loop_still_refuses_the_values(pkg):
    lib = pkg.load()
    for metric in (3, 4):
        prm = pkg.capi.icp_params(5, 1e-9, 0, pkg.capi.ICP_F64, metric)
        h = C.c_void_p()
        assert lib.icp_host_loop_create(C.byref(prm), C.byref(h)) == pkg.capi.ICP_ERR_INVALID
    assert lib.icp_host_loop_set_symmetric(None, 1) == pkg.capi.ICP_ERR_INVALID


def test_sym_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(Ctx.register_batch_symmetric).parameters
    assert list(prm) == ["self", "pairs", "k", "orient", "normals", "options"]
    assert (prm["k"].default, prm["orient"].default, prm["normals"].default) == (20, "centroid", None)
    assert prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(pkg.solve_symmetric).parameters) == ["mom"]
    assert "ICP_SYMMETRIC" in B.begin.__doc__
    # what existed keeps its parameter list
    assert list(inspect.signature(pkg.solve_point_to_plane).parameters) == ["mom"]
    assert list(inspect.signature(B.begin).parameters) == ["self", "max_iter", "tol", "fixed_iterations", "metric"]
    assert list(inspect.signature(B.set_point_normals).parameters) == ["self", "moving", "model"]
    assert list(inspect.signature(B.estimate_point_normals).parameters) == ["self", "orient", "viewpoints", "want"]
    assert list(inspect.signature(B.diag_rotation).parameters) == ["self", "b"]
    assert list(inspect.signature(Ctx._run_batch_options).parameters) == ["self", "metric", "pairs", "normals", "max_iter", "tol", "fixed_iterations",
                                                                          "max_distance", "init", "trim", "reciprocal", "robust", "prepare"]
    assert list(inspect.signature(Ctx.register_batch).parameters) == ["self", "pairs", "metric", "normals", "max_iter", "tol", "fixed_iterations",
                                                                    "max_distance", "init", "trim", "reciprocal"]
    assert list(inspect.signature(Ctx.register_batch_colored).parameters) == ["self", "pairs", "intensities", "k", "lam", "normals", "options"]
    assert list(inspect.signature(Ctx.register_batch_generalized).parameters) == ["self", "pairs", "k", "regularisation", "lam", "covariances", "options"]
