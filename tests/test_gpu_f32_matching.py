"""GPU: the float32 matching kernels -- nn_match_row64, nn_match_sparse (rows of 128 at 16 / 8 / 4 waves, flat and through the box
hierarchy, own order and sorted views), the dense nn_match_f32_v2, nn_match_batch / nn_match_batch_rev -- against the oracle over
the whole float range: squared distances that are all 0, subnormal and not 0, partly +inf and all +inf, signed zeros, exact twins on
both sides of a chunk and of a 32 768-point super box, ties that straddle the super boxes, a cold bound wider than the model, and
rows in which points with a finite neighbour sit beside points with none.

Every index comparison is np.array_equal against orc.nn in the clouds' own precision: no tolerance.  A point whose every squared
distance overflowed matches point 0 (include/icp_mi355x.h).  Every test asserts the form it claims to have run: the threads, blocks
and splits of icp_nn_launch_info, the ICP_ROUTE_* bits of a loop's passes, and -- where pruning is the point -- the work counters.
What makes the inputs what they are said to be is shown on the CPU in tests/test_f32_clouds.py.
"""
import os

import numpy as np
import pytest

import clouds as cl
import ref_moments as rm
from switches import fresh_context
from test_gpu_parity import FUZZ_VARIANTS

pytestmark = pytest.mark.gpu


def _variant_env(sort, hier, row):
    env = {"ICP_SORT": sort, "ICP_NN_HIER": hier, "ICP_NN_ROW": row[:3] if row.startswith("128") else row}
    if row in ("128w8", "128w4"):
        env["ICP_NN_WAVES128"] = row[-1]
    return env


# the twelve variants of the fuzz of test_gpu_parity.py, the dense kernel, and both tails on the default plan
FORMS = {f"sort{s}-hier{h}-row{r}": _variant_env(s, h, r) for s, h, r in FUZZ_VARIANTS}
FORMS.update({"dense": {"ICP_NN_SPARSE": "0"}, "fused_tail": {"ICP_FUSED_TAIL": "1"}, "two_kernel": {"ICP_FUSED_TAIL": "0"}})
assert len(FORMS) == 15
_REF = {}          # the fixed pairs and the oracle's answers for them, computed once and left unchanged


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads(orc):
    orc.set_threads(min(16, os.cpu_count() or 1))
    yield
    orc.set_threads(1)


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def assert_form(c, form, m):
    """the launch of the context's current clouds is the form's: (info, moving points of one block's row).  nn_plan's rules: rows of
    64 are one segment of 8-wave blocks; rows of 128 are cut into segments while they are fewer than half the CUs and the model has
    1024 points for each, and run as 8- or 4-wave blocks only unsplit (the 4-wave form with the hierarchy); the dense kernel is 4
    waves over 128 points and every model point"""
    env, info, cus = FORMS[form], c.nn_launch_info(), device_cus()
    what = (form, info, cus)
    assert info["m_pad"] == -(-m // 16) * 16, what
    if env.get("ICP_NN_SPARSE") == "0":
        assert info["threads"] == 256 and info["blocks"] == info["n_pad"] // 128 * info["splits"], what
        return info, 128
    row = int(env.get("ICP_NN_ROW", "64"))
    if "ICP_NN_ROW" not in env:
        assert info["n_pad"] // 64 <= 2 * cus and info["m_pad"] < cl.SPARSE_M_PAD_BELOW, what     # the default plan's rows of 64
    assert info["blocks"] == info["n_pad"] // row * info["splits"], what
    if row == 64:
        assert info["threads"] == 512 and info["splits"] == 1, what
        return info, 64
    unsplit = info["n_pad"] // 128 >= cus // 2 or info["m_pad"] <= 1024
    assert (info["splits"] == 1) == unsplit, what
    waves = int(env.get("ICP_NN_WAVES128", "16")) if unsplit else 16
    assert info["threads"] == 64 * waves, what
    return info, 128


def assert_same_indices(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {len(want)} indices differ, first at point {i}: {int(got[i])} for {int(want[i])}"
                             f" (answers given: {np.unique(got[bad])[:6].tolist()}, wanted: {np.unique(want[bad])[:6].tolist()})")


PAIRS = [f"tie@{s:g}" for s in cl.F32_TIE_SCALES] + ["twins", "far", "mixed"]


def fixed_pair(orc, name):
    """(P, M, the oracle's indices) of a named float32 pair of tests/clouds.py"""
    if name not in _REF:
        if name.startswith("tie@"):
            P, M = cl.straddling_tie_pair(scale=float(name[4:]), dtype=np.float32)
        elif name == "tie_8w":
            P, M = cl.straddling_tie_pair(n=cl.EIGHT_WAVE_N, replace=True, dtype=np.float32)
        elif name == "twins":
            P, M, twin_want = cl.twin_model(dtype=np.float32)
        elif name == "far":
            P, M = cl.far_pair(dtype=np.float32)
        elif name == "mixed":
            P, M = cl.mixed_overflow_pair()
        else:
            raise KeyError(name)
        want = orc.nn(P, M)
        if name == "twins":
            assert np.array_equal(want, twin_want)
        for a in (P, M, want):
            a.setflags(write=False)
        _REF[name] = (P, M, want)
    return _REF[name]


def numeric_end(pkg, e):
    return e.code in (pkg.capi.ICP_ERR_SINGULAR, pkg.capi.ICP_ERR_INVALID)


# ---------------------------------------------------------------------------------------------------
# 1. the fuzz over the whole range
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_f32_matching_fuzz_over_the_range(pkg, orc, monkeypatch, form):
    """randomised float32 clouds (uniform / clustered with duplicates / integer lattice / collinear, ragged sizes, signed zeros in
    every second case) at nine scales from 1e-25 (every squared distance 0) through subnormal distances to 1e19 / 1e20 (some / all
    of them +inf), every scale at least twice: indices bit-exact against the oracle"""
    cases = int(os.environ.get("ICP_FUZZ_CASES", str(cl.F32_FUZZ_CASES)))          # (a longer soak: ICP_FUZZ_CASES=1000)
    seed = cl.F32_FUZZ_SEEDS[FORMS[form].get("ICP_SORT", "0")]
    with fresh_context(pkg, monkeypatch, FORMS[form]) as c:
        for case, (n, m, kp, km, scale, P, Q) in enumerate(cl.f32_matching_cases(seed, cases)):
            got, want = c.Matching(P, Q), orc.nn(P, Q)
            assert_form(c, form, m)
            assert_same_indices(got, want, f"{form}, case {case}: n={n} m={m} cloud {kp} model {km} scale {scale:g}")


# ---------------------------------------------------------------------------------------------------
# 2. the fixed pairs, cold, seeded and as the first pass of a loop, in every form
# ---------------------------------------------------------------------------------------------------
def first_loop_pass(c, pkg, P, M, want, form, what):
    """pass 0 of a loop on the resident clouds -- the fused tail of the form's kernel, or moments_kernel behind it -- : the route it
    took, its indices, and, where every answer is point 0, point 0's coordinates in the sums (sum q = n Q[0]: n equal floats add up
    exactly in double in any order; compact rows replace the low 16 mantissa bits of sum q.x alone by the pass's tag)"""
    B = pkg.capi
    c.loop_begin(pkg.ICP_POINT_TO_POINT, max_iter=1, tol=0.0, fixed_iterations=True)
    try:
        c.loop_enqueue()
        c.loop_complete()
    except pkg.IcpError as e:        # (a minimisation may refuse such sums: the pass's matches and vector are there either way)
        assert numeric_end(pkg, e), e
    mom, route = c.diag_loop_moments()
    tail = B.ROUTE_MOMENTS_KERNEL if form == "two_kernel" else B.ROUTE_FUSED_TAIL
    assert route & tail and not route & ((B.ROUTE_MOMENTS_KERNEL | B.ROUTE_FUSED_TAIL | B.ROUTE_ERROR_ONLY) & ~tail), (what, hex(route))
    assert np.array_equal(c.get_moving(), P), what
    assert_same_indices(c.get_indices(), want, f"{what}, first pass of a loop (route {route:#05x})")
    assert mom[rm.CNT] == float(P.shape[0]), (what, mom[rm.CNT])
    if not want.any():
        q0 = M[0].astype(np.float64) * P.shape[0]
        assert mom[rm.SQ + 1] == q0[1] and mom[rm.SQ + 2] == q0[2], f"{what}: sum q = {mom[rm.SQ:rm.SQ + 3]!r}, n Q[0] = {q0!r}"
        assert abs(mom[rm.SQ] - q0[0]) <= 2.0 ** -36 * abs(q0[0]), f"{what}: sum q.x = {mom[rm.SQ]!r}, n Q[0].x = {q0[0]!r}"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("pair", PAIRS)
def test_fixed_pairs_in_every_form(pkg, orc, monkeypatch, pair, form):
    """the tie pair at six scales (8 ties across the super boxes; subnormal distances; every distance 0; nearly every / every
    distance +inf), the twins, the far pair and the mixed cloud: a cold pass, a pass seeded with its matches, and the first pass of a
    loop (the row tails) -- all three equal to the oracle"""
    P, M, want = fixed_pair(orc, pair)
    with fresh_context(pkg, monkeypatch, FORMS[form]) as c:
        c.set_model(M)
        c.set_moving(P)
        c.nn_match_resident()
        info, _ = assert_form(c, form, M.shape[0])
        assert info["m_pad"] > cl.SUPER_BOX_POINTS or pair == "mixed"
        cold = c.get_indices()
        assert cold.min() >= 0 and cold.max() < M.shape[0], (pair, form, int(cold.min()), int(cold.max()))
        assert_same_indices(cold, want, f"{pair}, {form}, cold")
        c.nn_match_bench(1, seeded=True)
        assert_same_indices(c.get_indices(), want, f"{pair}, {form}, seeded")
        first_loop_pass(c, pkg, P, M, want, form, f"{pair}, {form}")
        assert_form(c, form, M.shape[0])


@pytest.mark.parametrize("form", list(FORMS))
def test_tie_pair_with_more_rows_than_cus(pkg, orc, monkeypatch, form):
    """the tie pair's model under 16 448 cell centres: 272 rows of 64 -- more than the device has CUs --, 136 rows of 128 -- enough
    for unsplit rows, so the 8- and 4-wave blocks of rows of 128 are reached"""
    P, M, want = fixed_pair(orc, "tie_8w")
    with fresh_context(pkg, monkeypatch, FORMS[form]) as c:
        c.set_model(M)
        c.set_moving(P)
        c.nn_match_resident()
        info, row = assert_form(c, form, M.shape[0])
        assert info["splits"] == 1 or form == "dense", (form, info)
        if row == 64:
            assert info["blocks"] == 272 > device_cus(), (form, info)
        assert_same_indices(c.get_indices(), want, f"16 448 centres, {form}, cold")
        c.nn_match_bench(1, seeded=True)
        assert_same_indices(c.get_indices(), want, f"16 448 centres, {form}, seeded")
        first_loop_pass(c, pkg, P, M, want, form, f"16 448 centres, {form}")


@pytest.mark.parametrize("form", list(FORMS))
def test_work_counters_show_the_pruning_and_the_lack_of_it(pkg, orc, monkeypatch, form):
    """the work-counting instantiation on the tie pair at scale 1 and on the far pair: the same answers, and the counters that show
    what the search left out.  Pairs evaluated in full = hits_full x a row's moving points x 8, pairs listed = hits_box x the same.
    The tie pair on a sorted view: fewer pairs in full than there are (in the lattice's own random order every chunk's box spans
    the model and nothing can be left out: measured 1.006 / 1.097 of n m_pad with rows of 64 / 128, the padding of the last row
    included; 0.086 on the sorted view with rows of 64).  The far pair in the clouds' own order (what tests/test_f32_clouds.py shows
    of the cold bound is shown for that order): the hit list of every row holds nearly every chunk.  It is the LIST that is
    nearly everything: once a point's bound has come down to its true minimum the per-point box test turns most listed chunks
    away, and hits_full was measured at 0.14 (rows of 64) to 0.29 (rows of 128) of n m_pad.  The dense kernel tests no box."""
    with fresh_context(pkg, monkeypatch, FORMS[form]) as c:
        for pair in ("tie@1", "far"):
            P, M, want = fixed_pair(orc, pair)
            c.set_model(M)
            c.set_moving(P)
            c.set_work_counting(True)
            try:
                c.nn_match_resident()
                w = c.get_work_counters()
            finally:
                c.set_work_counting(False)
            info, row = assert_form(c, form, M.shape[0])
            assert_same_indices(c.get_indices(), want, f"{pair}, {form}, counted")
            every_pair = P.shape[0] * info["m_pad"]
            full, listed = w["hits_full"] * row * 8, w["hits_box"] * row * 8
            print(f"[work] {form} {pair}: hits_full x {row} x 8 = {full / every_pair:.4f}, hits_box x {row} x 8 = {listed / every_pair:.4f} of n m_pad; find_boxes {w['find_boxes']} upper_boxes {w['upper_boxes']}")
            if form == "dense":
                assert w["find_boxes"] == 0 and w["upper_boxes"] == 0 and w["hits_box"] == 0 and w["hits_full"] == 0, (pair, w)
                continue
            assert w["block_passes"] == info["blocks"] and w["hits_box"] >= w["hits_full"] > 0, (pair, form, w)
            if pair == "tie@1" and FORMS[form].get("ICP_SORT") == "1":
                assert full < every_pair, (form, full / every_pair)
            if pair == "far" and FORMS[form].get("ICP_SORT") == "0":
                assert listed >= 0.95 * every_pair, (form, listed / every_pair)


# ---------------------------------------------------------------------------------------------------
# 3. seeded passes inside a loop
# ---------------------------------------------------------------------------------------------------
LOOPS = {"stepwise": {"ICP_RESIDENT": "0", "ICP_ARMED": "0"}, "armed": {"ICP_RESIDENT": "0"}, "resident": {},
         "stepwise_two_kernel": {"ICP_RESIDENT": "0", "ICP_ARMED": "0", "ICP_FUSED_TAIL": "0"}}
SCHEDULES = ((1, 1, 1, 1), (2, 2), (3, 1))     # every matching pass 0, 1, 2 ends a run once; passes 1 and 2 also as a later pass of a run
LOOP_PASSES = 3


@pytest.mark.parametrize("scale", [1e-20, 1.0])
@pytest.mark.parametrize("form", list(LOOPS))
def test_seeded_passes_inside_a_loop(pkg, orc, monkeypatch, form, scale):
    """three matching passes of a fixed-iterations loop on the tie pair, in runs of icp_loop_run: after every completed pass the
    correspondences are the oracle's on the cloud the device itself matched on -- no trajectory has to agree.  At 1e-20 every
    distance of every pass is subnormal, and the first pass's moment vector is held to ref_moments' exact sums at its derived bound
    (fused tail: compact rows; two-kernel tail: moments_kernel)."""
    B = pkg.capi
    P, M, want = fixed_pair(orc, f"tie@{scale:g}")
    two_kernel = form == "stepwise_two_kernel"
    tail = B.ROUTE_MOMENTS_KERNEL if two_kernel else B.ROUTE_FUSED_TAIL
    with fresh_context(pkg, monkeypatch, LOOPS[form]) as c:
        for schedule in SCHEDULES:
            c.set_model(M)
            c.set_moving(P)
            c.loop_begin(pkg.ICP_POINT_TO_POINT, max_iter=LOOP_PASSES, tol=0.0, fixed_iterations=True)
            k, checked = -1, []
            for steps in schedule:
                what = f"{form}, scale {scale:g}, runs of {schedule}, pass {k + steps}"
                refused = False
                try:
                    took, done = c.loop_run(steps)
                except pkg.IcpError as e:            # a host solve that refuses a pass's sums ends the case there ...
                    assert numeric_end(pkg, e), e
                    if steps > 1:
                        break
                    took, done, refused = 1, False, True   # ... behind the pass's own matches and vector, which are still read
                assert took == steps, what
                k += steps
                assert done == (k == LOOP_PASSES), what
                if done:
                    break
                mom, route = c.diag_loop_moments()
                form_bits = B.ROUTE_RESIDENT if form == "resident" else B.ROUTE_ARMED if (form == "armed" and steps >= 2) else 0
                assert route & tail and route & (B.ROUTE_RESIDENT | B.ROUTE_ARMED) == form_bits and not route & B.ROUTE_ERROR_ONLY, (what, hex(route))
                Pk, got = c.get_moving(), c.get_indices()
                if k == 0:
                    assert np.array_equal(Pk, P), what
                    assert_same_indices(got, want, what)
                else:
                    assert np.isfinite(Pk).all(), what
                    assert_same_indices(got, orc.nn(Pk, M), what)
                if k == 0 and scale < 1.0:
                    compact = not two_kernel
                    assert bool(route & B.ROUTE_COMPACT) == compact, (what, hex(route))
                    ref, maj = rm.p2p(P, M, want)
                    tol = rm.tolerance(maj, P.shape[0], compact)
                    assert mom[rm.CNT] == float(P.shape[0]) and mom[rm.ERR] == 0.0, what
                    for s in (rm.P2P_COMPACT_SLOTS if compact else rm.P2P_SLOTS):
                        assert abs(mom[s] - ref[s]) <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {ref[s]!r} tol {tol[s]:.3e}"
                checked.append(k)
                if refused:
                    break
            print(f"[loop] {form} scale {scale:g} runs of {schedule}: passes checked against the oracle {checked}")
            assert checked and checked[0] == schedule[0] - 1, (form, scale, schedule, checked)
            assert_form(c, "two_kernel" if two_kernel else "fused_tail", M.shape[0])


# ---------------------------------------------------------------------------------------------------
# 4. the batch kernels, float32 and float64
# ---------------------------------------------------------------------------------------------------
BATCH_N, BATCH_M = (1, 63, 65, 130), (1, 7, 513, 1030)       # across the quarter and sub-tile borders of BatchCfg
BATCH_SCALES = {np.float32: {"zero": cl.F32_ZERO_SCALE, "subnormal": cl.F32_SUBNORMAL_SCALES[1], "part_inf": cl.F32_PART_INF_SCALE, "inf": cl.F32_INF_SCALE},
                np.float64: {"zero": cl.UNDERFLOW_SCALE, "subnormal": 1e-157, "part_inf": 1e154, "inf": cl.OVERFLOW_SCALE}}


def batch_pairs(dtype, scale, apart):
    """the sixteen (n, m) pairs at one scale: uniform clouds on uniform, clustered (duplicates), lattice and collinear models in
    turn, signed zeros throughout; apart: the cloud shifted by 8 model widths before the scaling -- no two points of a pair are
    then nearer than 2 x scale in any coordinate"""
    rng = np.random.default_rng(1600)
    pairs = []
    for n in BATCH_N:
        for k, m in enumerate(BATCH_M):
            kind = cl.FUZZ_KINDS[(k + n) % 4]
            A = cl.fuzz_cloud(rng, n, "uniform" if kind != "lattice" else "lattice", scale, np.float64, True)
            pairs.append(((A + 8.0 * scale if apart else A).astype(dtype), cl.fuzz_cloud(rng, m, kind, scale, dtype, True)))
    return pairs


@pytest.mark.parametrize("what", ["zero", "subnormal", "part_inf", "inf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_kernels_at_the_ends_of_the_range(ctx, pkg, orc, dtype, what):
    """nn_match_batch and nn_match_batch_rev at the scale where every squared distance of the type is 0 / subnormal / partly +inf /
    +inf: after one pass of a fixed-iterations reciprocal batch the forward matches are the oracle's, and the reverse search's the
    oracle's with the clouds exchanged ("nothing found" is point 0 both ways)"""
    scale = BATCH_SCALES[dtype][what]
    pairs = batch_pairs(dtype, scale, apart=what == "inf")
    tiny = float(np.finfo(dtype).tiny)
    seen_inf = seen_fin = 0
    with np.errstate(over="ignore", under="ignore"):
        for A, M in pairs:                          # the scale does to these clouds what its name says
            assert A.dtype == M.dtype == dtype and np.isfinite(A).all() and np.isfinite(M).all()
            d = A[:, None, :] - M[None, :, :]
            d = d * d
            d = (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]
            assert d.dtype == dtype
            if what == "zero":
                assert (d == 0).all()
            elif what == "subnormal":
                assert (d < tiny).all() and (d > 0).any()
            elif what == "inf":
                assert np.isinf(d).all()
            else:
                seen_inf += int(np.isinf(d).sum())
                seen_fin += int(np.isfinite(d).sum())
    assert what != "part_inf" or (seen_inf > 1000 and seen_fin > 1000)
    want = [(orc.nn(A, M), orc.nn(M, A)) for A, M in pairs]
    if what in ("zero", "inf"):
        assert all(not f.any() and not r.any() for f, r in want)
    with ctx.batch(pairs) as bt:
        bt.set_reciprocal(True)
        bt.begin(max_iter=2, tol=0.0, fixed_iterations=True)
        bt.run(1)
        got_idx, got_rev = bt.get_indices(), bt.diag_reverse()
        for b, ((A, M), (fwd, rev)) in enumerate(zip(pairs, want)):
            tag = f"{what} ({scale:g}), pair {b}: n {A.shape[0]} m {M.shape[0]}"
            assert_same_indices(got_idx[b], fwd, tag + ", forward")
            assert_same_indices(got_rev[b], rev, tag + ", reverse")
