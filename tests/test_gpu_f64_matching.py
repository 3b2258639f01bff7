"""GPU: the fp64 matching path -- nn_match_row64_f64 (csrc/icp_k_f64.hip) and, under ICP_F64_SPARSE=0, nn_match_kernel<double> --
against the fp64 oracle on inputs chosen to be hard: randomised clouds of four kinds at three scales with full mantissas and signed
zeros, models of more than one round of 4096 chunks whose tied minima straddle the rounds, a far-apart pair that fills the hit list
in both rounds, clouds with more rows than the device has CUs (the 8-wave instantiation), exact twins on both sides of the point that
must win, seeded passes in the step-wise and the resident form, and scales at which every squared distance is 0 or +inf.

Every index comparison is bit-exact against orc.nn in float64 (first minimum of (dx*dx + dy*dy) + dz*dz): no tolerance.  Every test
asserts the form it claims to have run -- icp_nn_launch_info's threads (512: rows of 64 on the sparse structure; 256: the dense
kernel) and, for the 8-wave instantiation, more blocks than CUs (nn_launch_shape's rule).  The conditions that make the inputs what
they are said to be are shown on the CPU in tests/test_f64_clouds.py.
"""
import os

import numpy as np
import pytest

import clouds as cl
from switches import fresh_context

pytestmark = pytest.mark.gpu

FORMS = {"resident": {}, "resident_host_mailbox": {"ICP_MAILBOX": "host"}, "resident_plain_stores": {"ICP_MAILBOX": "plain"},
         "stepwise": {"ICP_RESIDENT": "0"}}
_REF = {}          # the oracle's answers for the fixed pairs, computed once


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def assert_form(c, sparse, waves=16):
    """the launch of the context's current clouds: sparse rows of 64 (8 waves where the rows outnumber the CUs, else 16) or dense"""
    info = c.nn_launch_info()
    assert info["threads"] == (512 if sparse else 256), info
    if sparse:
        assert info["splits"] == 1 and info["blocks"] == info["n_pad"] // 64, info
        assert (info["blocks"] > device_cus()) == (waves == 8), (info, device_cus())
    return info


def assert_same_indices(got, want, what):
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {len(want)} indices differ, first at point {i}: {int(got[i])} for {int(want[i])}")


def nn_threaded(orc, P, M):
    orc.set_threads(min(16, os.cpu_count() or 1))
    try:
        return orc.nn(P, M)
    finally:
        orc.set_threads(1)


def fixed_pair(orc, name):
    """(P, M, the oracle's indices) of a named pair of tests/clouds.py"""
    if name not in _REF:
        if name == "tie":
            P, M = cl.straddling_tie_pair()
        elif name == "far":
            P, M = cl.far_pair()
        elif name == "tie_8w":
            P, M = cl.straddling_tie_pair(n=cl.EIGHT_WAVE_N, replace=True)
        elif name == "underflow":
            P, M = cl.straddling_tie_pair(scale=cl.UNDERFLOW_SCALE)
        elif name == "overflow":
            P, M = cl.straddling_tie_pair(scale=cl.OVERFLOW_SCALE)
        else:
            raise KeyError(name)
        want = nn_threaded(orc, P, M)
        for a in (P, M, want):
            a.setflags(write=False)
        _REF[name] = (P, M, want)
    return _REF[name]


def checked_loop(c, pkg, orc, D, M, schedule, what):
    """a fixed-iterations loop of sum(schedule) - 1 matching passes driven by icp_loop_run in runs of `schedule` steps; after every
    run the correspondences must be the oracle's on the cloud as the device holds it -- whatever the trajectory has been"""
    passes = sum(schedule) - 1
    c.set_model(M)
    c.set_moving(D)
    c.loop_begin(pkg.ICP_POINT_TO_POINT, max_iter=passes, tol=0.0, fixed_iterations=True)
    k = -1
    for steps in schedule:
        took, done = c.loop_run(steps)
        assert took == steps
        k += steps
        assert done == (k == passes)
        if not done:
            assert_same_indices(c.get_indices(), orc.nn(c.get_moving(), M), f"{what}, pass {k} (runs of {schedule})")
    return c.loop_state()


# ---------------------------------------------------------------------------------------------------
# matching fuzz
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", ["1", "0"])
def test_f64_matching_fuzz_against_the_oracle(pkg, orc, monkeypatch, sparse):
    """randomised float64 clouds (uniform / clustered with duplicates / integer lattice / collinear, three scales, ragged sizes,
    signed zeros in every second case), the cloud's kind and the model's independent: indices bit-exact against the oracle"""
    cases = int(os.environ.get("ICP_FUZZ_CASES", "40"))                      # (a longer soak: ICP_FUZZ_CASES=1000)
    with fresh_context(pkg, monkeypatch, {"ICP_F64_SPARSE": sparse}) as c:
        for case, (n, m, kp, km, scale, P, Q) in enumerate(cl.f64_matching_cases(cl.F64_FUZZ_SEEDS[sparse], cases)):
            got, want = c.Matching(P, Q), orc.nn(P, Q)
            assert_form(c, sparse == "1")
            assert_same_indices(got, want, f"case {case}: n={n} m={m} cloud {kp} model {km} scale {scale:g}")


# ---------------------------------------------------------------------------------------------------
# the 8-wave instantiation: more rows than CUs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["clustered", "lattice"])
def test_eight_wave_blocks_small_models(pkg, orc, monkeypatch, kind):
    """16 448 points are 272 blocks: the 8-wave instantiation, on a clustered and on a lattice model of about 900 points (one find
    pass of two waves' worth of chunks, the other six idle), cold and -- two passes of a loop -- seeded"""
    rng = np.random.default_rng(1648 + len(kind))
    M = cl.fuzz_cloud(rng, 901, kind, 1.0, np.float64, signed_zeros=True)
    P = cl.fuzz_cloud(rng, cl.EIGHT_WAVE_N, "clustered" if kind == "lattice" else "uniform", 1.0, np.float64)
    if kind == "lattice":
        P = 3.0 * P                                       # (the lattice spans [-3, 3]: cover it)
        P[::7] = np.round(P[::7]) + 0.5                   # cell centres: 8-way ties
    with fresh_context(pkg, monkeypatch, {}) as c:
        got = c.Matching(P, M)
        assert_form(c, True, waves=8)
        assert_same_indices(got, nn_threaded(orc, P, M), f"{kind}, cold")
        checked_loop(c, pkg, orc, P, M, (1, 1, 1), f"{kind}, 8 waves")
        assert_form(c, True, waves=8)


def test_eight_wave_blocks_tied_minima_across_the_rounds(pkg, orc, monkeypatch):
    """the tie pair's model (two rounds) under 16 448 cell centres: the 8-wave blocks' round loop, exchange and tie rule"""
    P, M, want = fixed_pair(orc, "tie_8w")
    with fresh_context(pkg, monkeypatch, {}) as c:
        got = c.Matching(P, M)
        assert_form(c, True, waves=8)
        assert_same_indices(got, want, "tie pair, 16 448 centres, cold")


# ---------------------------------------------------------------------------------------------------
# rounds: models of 40 425 and 40 000 points
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["resident", "stepwise", "dense"])
@pytest.mark.parametrize("pair", ["tie", "far"])
def test_models_of_two_rounds(pkg, orc, monkeypatch, pair, form):
    """tied minima on both sides of the first round's end, and a pair so far apart that the hit list fills in both rounds: Matching
    (cold: the samples and the scan in one launch), then a fixed-iterations loop pass by pass.  dense: the model of a 700-point
    cloud is split over grid.y, and the ties lie across the segments as they lie across the rounds"""
    P, M, want = fixed_pair(orc, pair)
    env = {"ICP_F64_SPARSE": "0"} if form == "dense" else FORMS[form]
    with fresh_context(pkg, monkeypatch, env) as c:
        got = c.Matching(P, M)
        info = assert_form(c, form != "dense")
        if form == "dense":
            assert info["splits"] > 1, info
        assert M.shape[0] > cl.ROUND_POINTS and info["m_pad"] < cl.SPARSE_M_PAD_BELOW
        assert_same_indices(got, want, f"{pair} pair, {form}, Matching")
        checked_loop(c, pkg, orc, P, M, (1, 1, 1, 1), f"{pair} pair, {form}")
        checked_loop(c, pkg, orc, P, M, (2, 1, 1), f"{pair} pair, {form}")
        assert_form(c, form != "dense")


# ---------------------------------------------------------------------------------------------------
# seeded passes, and the resident form's seeds in LDS
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_f64_registration_fuzz_against_the_oracle(pkg, orc, monkeypatch, form):
    """randomised registrations on float64 models (uniform / clustered with duplicates / lattice; 300 to 2500 points): in runs of one
    step and in runs of two and three the indices after every run are the oracle's on the cloud the device holds, and the whole
    registration is the oracle's: iteration count, transform and error series (the bounds of test_fp64_forms_sparse_and_dense)"""
    rng = np.random.default_rng(6473)
    with fresh_context(pkg, monkeypatch, FORMS[form]) as c:
        for case in range(max(1, int(os.environ.get("ICP_FUZZ_CASES", "40")) // 5)):
            m = int(rng.integers(300, 2500))
            n = int(rng.integers(200, 2500))
            kind = str(rng.choice(["uniform", "clustered", "lattice"]))
            M = cl.fuzz_cloud(rng, m, kind, 1.0, np.float64, signed_zeros=True)
            a = rng.uniform(-0.05, 0.05, 3)
            Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
            Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
            Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
            D = (M[rng.integers(0, m, n)] + rng.uniform(-0.02, 0.02, 3)) @ (Rz @ Ry @ Rx) + 2e-3 * rng.standard_normal((n, 3))
            what = f"{form}, case {case}: n={n} m={m} model {kind}"
            checked_loop(c, pkg, orc, D, M, (1, 1, 1, 1, 1, 1), what)
            assert_form(c, True)
            checked_loop(c, pkg, orc, D, M, (2, 3, 2, 1), what)
            res = c.point_to_point(D, M, max_iter=15, tol=1e-7)
            want = orc.icp_p2p(D, M, 15, 1e-7)
            assert res.iterations == want["iterations"], (what, res.iterations, want["iterations"])
            assert rel(res.T, want["T"]) < 1e-9 and np.abs(res.err - want["err"]).max() < 1e-9, what
            assert_same_indices(res.idx, want["idx"], what + ", final correspondences")


# ---------------------------------------------------------------------------------------------------
# duplicates
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", ["1", "0"])
def test_exact_twins_resolve_to_the_lowest_index(pkg, orc, monkeypatch, sparse):
    """a model with exact twins (signed zeros mixed in) of a point at higher indices in its chunk, in other chunks and in the other
    round, hit exactly through the twins' own coordinates: the lowest index wins -- cold, among many other hits, and in the seeded
    passes of a loop (the twins stay tied bit for bit wherever the cloud goes)"""
    P, M, want = cl.twin_model()
    with fresh_context(pkg, monkeypatch, {"ICP_F64_SPARSE": sparse}) as c:
        got = c.Matching(P, M)
        assert_form(c, sparse == "1")
        assert_same_indices(got, want, "twins, cold")
        assert_same_indices(got, orc.nn(P, M), "twins, cold, the oracle")
        # among 40 000 other points as well: the twins' own chunks are then a few hits among many
        rng = np.random.default_rng(2223)
        P2 = np.concatenate([P, M[rng.integers(0, M.shape[0], 500)] + 1e-3 * rng.standard_normal((500, 3))])
        assert_same_indices(c.Matching(P2, M), orc.nn(P2, M), "twins among neighbours")
        checked_loop(c, pkg, orc, P2, M, (1, 1, 1), "twins among neighbours")


# ---------------------------------------------------------------------------------------------------
# extremes: every squared distance 0, every squared distance +inf
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", ["1", "0"])
@pytest.mark.parametrize("pair", ["underflow", "overflow"])
def test_extreme_scales_answer_point_zero(pkg, orc, monkeypatch, pair, sparse):
    """the tie pair times 1e-170 (every squared distance underflows to 0: 40 425 tied minima) and times 1e160 (every squared
    distance is +inf: nothing is ever below the bound): the first point of an ascending scan, index 0, as the oracle answers --
    from Matching, and from the passes of a two-pass loop (whose minimisation may refuse such sums: the correspondences are read
    either way)"""
    P, M, want = fixed_pair(orc, pair)
    assert not want.any()
    with fresh_context(pkg, monkeypatch, {"ICP_F64_SPARSE": sparse}) as c:
        got = c.Matching(P, M)
        assert_form(c, sparse == "1")
        assert got.min() >= 0 and got.max() < M.shape[0], (int(got.min()), int(got.max()))
        assert_same_indices(got, want, f"{pair}, Matching")
        c.set_model(M)
        c.set_moving(P)
        c.loop_begin(pkg.ICP_POINT_TO_POINT, max_iter=2, tol=0.0, fixed_iterations=True)
        for k in range(2):
            try:
                c.loop_enqueue()
                done = c.loop_complete()
            except pkg.IcpError as e:
                assert e.code in (pkg.capi.ICP_ERR_SINGULAR, pkg.capi.ICP_ERR_INVALID), e
                done = True
            got, Pk = c.get_indices(), c.get_moving()
            assert got.min() >= 0 and got.max() < M.shape[0], (k, int(got.min()), int(got.max()))
            if k == 0:
                assert np.array_equal(Pk, P)
            if np.isfinite(Pk).all():
                assert_same_indices(got, orc.nn(Pk, M), f"{pair}, pass {k}")
            if k == 0:
                assert_same_indices(got, want, f"{pair}, pass 0")
            if done:
                break
