"""CPU: the C ABI of batched Fast Global Registration (icp_batch_fgr, icp_fgr_params, icp_diag_batch_fgr, icp_diag_batch_fgr_times)
is declared, exported and bound with the exact ctypes signatures, the struct has the stated fields in the stated order and size,
the ABI version stays 2, a NULL batch is refused without a device, the header states the rules and the Python mirror carries the
additions."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "icp_mi355x_diag.h")
_pd, _pi, _p32 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int32)


def test_fgr_symbols_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(DIAG).read(), flags=re.S)
    declared = set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (icp_[a-z0-9_]+)", out))
    lib = pkg.load()
    prm = C.POINTER(pkg.capi.icp_fgr_params)
    want = {"icp_batch_fgr": (C.c_int, [C.c_void_p, prm, C.POINTER(C.c_uint64), _pd, _pd, _p32, _pd, _pi]),
            "icp_diag_batch_fgr": (C.c_int, [C.c_void_p, C.c_int, _p32, _pd, _pd, _pd]),
            "icp_diag_batch_fgr_times": (C.c_int, [C.c_void_p, _pd])}
    for name, (res, args) in want.items():
        assert name in declared and name in exported, name
        assert name in pkg.capi.SIGNATURES and hasattr(lib, name), name
        assert pkg.capi.SIGNATURES[name][0] is res and pkg.capi.SIGNATURES[name][1] == args, name
    assert lib.icp_abi_version() == 2   # additions only
    assert re.search(r"#define\s+ICP_ABI_VERSION\s+2\b", open(HEADER).read())


def test_fgr_params_layout(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct icp_fgr_params \{(.*?)\} icp_fgr_params;", src, flags=re.S)
    assert m
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("int", "iterations"), ("double", "max_distance"), ("double", "division_factor"), ("int", "decrease_every"),
                      ("int", "tuples"), ("double", "tuple_similarity")]
    S = pkg.capi.icp_fgr_params
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in S._fields_] == [(n, ctype[t]) for t, n in fields]
    assert C.sizeof(S) == 40 and [getattr(S, n).offset for _, n in fields] == [0, 8, 16, 24, 28, 32]
    p = S(64, 0.02, 1.4, 4, 0, 0.95)
    assert (p.iterations, p.max_distance, p.division_factor, p.decrease_every, p.tuples, p.tuple_similarity) == (64, 0.02, 1.4, 4, 0, 0.95)


def test_header_states_the_rules():
    text = re.sub(r"\s*\n\s*\*?\s*", " ", open(HEADER).read())
    for clause in ("Zhou, Park, Koltun, ECCV 2016", "registration_fgr_based_on_feature_matching", "seed may be NULL iff tuples == 0",
                   "deterministic without a seed", "every operation is one IEEE double operation, nothing is fused",
                   "RANSAC's own draw, triple and edge check with e = tuple_similarity",
                   "each position is used once, however often it occurs -- a deliberate deviation from Open3D, which repeats them",
                   "the order is ascending list position", "U_p < 3: status ICP_ERR_EMPTY, T the identity, every weight 0, objective 0",
                   "the sequential sums of the used moving and model points, in list order, divided by U_p",
                   "D2 == 0 or not finite: ICP_ERR_EMPTY", "mu = max(mu / division_factor, delta*delta)", "mu is never lowered below delta^2",
                   "p_a = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]", "r2 = (ex*ex + ey*ey) + ez*ez", "s = mu / (mu + r2); l = s*s",
                   "no sqrt is needed", "cn_x = (0, pz, -py, 1, 0, 0), cn_y = (-pz, 0, px, 0, 1, 0), cn_z = (py, -px, 0, 0, 0, 1)",
                   "C(r, c) += (w_x[r]*cn_x[c] + w_y[r]*cn_y[c]) + w_z[r]*cn_z[c] for r <= c",
                   "B(r) -= (w_x[r]*ex + w_y[r]*ey) + w_z[r]*ez", "ICP_MOM_ERR += l*r2 + mu*((1 - s)*(1 - s))",
                   "A correspondence whose p or r2 is not finite adds nothing and counts 0",
                   "goes through icp_solve_point_to_plane", "ends that pair with ICP_ERR_SINGULAR at the pose reached so far",
                   "objective_out is ICP_MOM_ERR of the pair's last iteration", "a used point gets its l, every other point 0.0",
                   "no floating-point atomics", "not on its neighbours or its position in the batch",
                   "a refused call leaves the batch as it was", "neither discards nor advances a registration under way"):
        assert clause in text, clause


def test_fgr_null_batch_is_invalid(pkg):
    lib = pkg.load()
    d = np.full(64, -7.0)
    i32 = np.full(4, -3, dtype=np.int32)
    st = np.array([5], dtype=np.intc)
    prm = pkg.capi.icp_fgr_params(64, 0.02, 1.4, 4, 0, 0.95)
    E = pkg.capi.ICP_ERR_INVALID
    pd = d.ctypes.data_as(_pd)
    assert lib.icp_batch_fgr(None, C.byref(prm), None, pd, pd, i32.ctypes.data_as(_p32), pd, st.ctypes.data_as(_pi)) == E
    assert "null batch" in lib.icp_last_error().decode()
    assert lib.icp_diag_batch_fgr(None, 0, i32.ctypes.data_as(_p32), pd, pd, pd) == E
    assert lib.icp_diag_batch_fgr_times(None, pd) == E
    assert (d == -7.0).all() and (i32 == -3).all() and st[0] == 5


def test_fgr_python_mirror(pkg):
    B, Ctx = pkg.engine.Batch, pkg.Context
    prm = inspect.signature(B.fgr).parameters
    assert list(prm) == ["self", "max_distance", "iterations", "division_factor", "decrease_every", "tuples", "tuple_similarity", "seed"]
    assert [prm[k].default for k in list(prm)[2:]] == [64, 1.4, 4, 0, 0.95, 0]
    assert list(inspect.signature(B.diag_fgr).parameters) == ["self", "b"]
    # what existed keeps its parameter list; method travels among the options
    assert list(inspect.signature(B.ransac).parameters) == ["self", "hypotheses", "max_distance", "edge_similarity", "seed"]
    prm = inspect.signature(Ctx.register_batch_global).parameters
    assert list(prm) == ["self", "pairs", "voxel", "k", "hypotheses", "max_distance", "options"] and prm["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert 'method="fgr"' in Ctx.register_batch_global.__doc__
