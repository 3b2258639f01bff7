"""GPU: statistical and radius outlier removal of a batch on the device (icp_batch_remove_outliers; Batch.remove_outliers).

The rules are stated in include/icp_mi355x.h and restated in numpy in tests/batch_outlier_ref.py; tests/test_batch_outlier_ref.py
pins that reference on hand cases.  This file compares the device with it for byte equality -- the new clouds, offsets, maps,
scores and stats -- in fp32 and fp64.  No tolerance is introduced: the score of a statistical point is a sum of correctly
rounded double square roots in a stated order, so the device's double sqrt is tested to the bit here."""
import ctypes as C

import numpy as np
import pytest

import batch_outlier_ref as ro
from batch_ref import CASES, bits_equal, final, gate_case, same_pair_bytes

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
STAT, RAD = "statistical", "radius"


def check_batch(ctx, pairs, moving, model, what):
    """the batch filtered on the device is the reference's, byte for byte: clouds, offsets, maps, scores, stats.  Returns the
    reference."""
    ref = ro.remove_pairs(pairs, moving, model)
    with ctx.batch(pairs) as src:
        nb, info = src.remove_outliers(moving, model, want_maps=True, want_scores=True)
        with nb:
            assert nb.count == len(pairs)
            assert np.array_equal(nb._moff, ro.vr.offsets([r[0] for r in ref["clouds"]])), (what, "moving offsets")
            assert np.array_equal(nb._qoff, ro.vr.offsets([r[1] for r in ref["clouds"]])), (what, "model offsets")
            got = nb.get_clouds()
            for b, ((YD, YM), (GD, GM)) in enumerate(zip(ref["clouds"], got)):
                assert bits_equal(GD, YD), (what, b, "moving cloud", GD.shape, YD.shape)
                assert bits_equal(GM, YM), (what, b, "model", GM.shape, YM.shape)
                for side in ("moving", "model"):
                    gm, gs = info[side + "_map"][b], info[side + "_score"][b]
                    wm, ws = ref[side + "_map"][b], ref[side + "_score"][b]
                    assert gs.dtype == np.float64 and bits_equal(gs, ws), (what, b, side, "score", int((gs != ws).sum()), float(np.abs(gs - ws).max()))
                    assert gm.dtype == np.int32 and np.array_equal(gm, wm), (what, b, side, "map")
            assert info["stats"].shape == (2 * len(pairs), 4) and bits_equal(info["stats"], ref["stats"]), (what, info["stats"], ref["stats"])
        back = src.get_clouds()   # the source holds what was uploaded
        for (D, M), (GD, GM) in zip(pairs, back):
            assert bits_equal(GD, D) and bits_equal(GM, M), (what, "source clouds")
    return ref


# 1 ------------------------------------------------------------------------------------------------------------------------
SIZES = (2, 63, 64, 65, 66, 257)
KS = {8: (1, 5, 8), 16: (9, 16), 32: (17, 32)}   # per register capacity of the scan's list


def size_pairs(dtype, cap):
    """one pair per size around a work item, plus one cloud of k + 1 points per k; statistical rules with the k of one capacity
    (a cloud too small for its k gets a radius rule), and radius, statistical and copied models of other sizes"""
    ks = KS[cap]
    sizes = SIZES + tuple(k + 1 for k in ks)
    pairs, moving, model = [], [], []
    for b, n in enumerate(sizes):
        m = sizes[(b + 3) % len(sizes)]
        pairs.append((ro.normal(n, 300 + b, dtype), ro.normal(m, 400 + b, dtype)))
        k = ks[b % len(ks)] if b < len(SIZES) else n - 1
        moving.append((STAT, k, (0.0, 0.5, 1.0, 2.0)[b % 4]) if n >= k + 1 else (RAD, 5.0, 1))
        kq = ks[(b + 1) % len(ks)]
        model.append([(RAD, 0.7, 2) if m >= 60 else (RAD, 5.0, 1), None, (STAT, kq, 1.0) if m >= kq + 1 else None][b % 3])
    return pairs, moving, model


@DTYPES
@pytest.mark.parametrize("cap", sorted(KS))
def test_outlier_sizes_and_k(ctx, dtype, cap):
    pairs, moving, model = size_pairs(dtype, cap)
    assert {r[1] for r in moving if r[0] == STAT} >= set(KS[cap])
    ref = check_batch(ctx, pairs, moving, model, f"sizes, capacity {cap}")
    assert any(0 < s[3] < p[0].shape[0] for s, p in zip(ref["stats"], pairs))   # something is removed, something kept


@DTYPES
def test_outlier_quarter_longer_than_a_sub_tile(ctx, dtype):
    """2 100 points: a wave's quarter (525) exceeds its LDS sub-tile of 512 (fp32) and 256 (fp64) points"""
    A, M = ro.normal(2100, 21, dtype), ro.normal(2100, 22, dtype)
    ref = check_batch(ctx, [(A, M)], (STAT, 16, 1.0), (RAD, 0.3, 5), "2100 points")
    assert 0 < ref["stats"][0][3] < 2100 and 0 < ref["stats"][1][3] < 2100


@DTYPES
def test_outlier_mixed_kinds_and_a_null_side(ctx, dtype):
    pairs = [(ro.normal(200 + 31 * b, 500 + b, dtype), ro.normal(150 + 17 * b, 600 + b, dtype)) for b in range(4)]
    moving = [(STAT, 8, 1.0), None, (RAD, 0.6, 3), (STAT, 20, 0.5)]
    ref = check_batch(ctx, pairs, moving, None, "model side NULL")
    assert all(bits_equal(r[1], p[1]) for r, p in zip(ref["clouds"], pairs)) and (ref["stats"][4:, 3] == [p[1].shape[0] for p in pairs]).all()
    check_batch(ctx, pairs, None, [(RAD, 0.6, 3), (STAT, 3, 2.0), None, (STAT, 12, 0.0)], "moving side NULL")
    check_batch(ctx, pairs, None, None, "both sides NULL")


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_outlier_lattice_coincident_far_and_threshold(ctx, dtype):
    """the lattice (equal distances across every quarter boundary, std == 0), coincident points, clouds far from the origin and
    radius counts decided exactly on the threshold"""
    L, Z, Fr, T = ro.lattice(dtype), ro.coincident(dtype), ro.far(dtype), ro.threshold_cloud(dtype)
    s2, s3 = float(np.sqrt(2.0)), float(np.sqrt(3.0))
    pairs =  [(L, L),         (Z, Z),          (Fr, Fr),        (T, T),        (T, T),          (L, T)]
    moving = [(STAT, 3, 0.0), (STAT, 8, 1.0),  (STAT, 8, 1.0),  (RAD, 1.0, 4), (RAD, s2, 10),   (STAT, 32, 0.0)]
    model =  [(STAT, 6, 0.0), (RAD, 1e-3, 39), (RAD, 0.5, 3),   (RAD, s3, 18), (RAD, float(np.float32(s2)), 6), (RAD, s3, 26)]
    if dtype == np.float64:
        model[5] = (RAD, s3, 18)   # (r * r stays below 3 in double: the space diagonals are out, and min = 26 would keep nothing)
    ref = check_batch(ctx, pairs, moving, model, "lattice, coincident, far, threshold")
    st = ref["stats"]
    assert st[0].tolist() == [0.5, 0.0, 0.5, 512.0] and st[6][3] == 216 and st[7][3] == 40
    assert st[3][3] == 125 - 8 and st[6 + 4][3] == 27


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_outlier_largest_cloud(ctx, dtype):
    """one cloud at ICP_BATCH_MAX_POINTS.  A full numpy reference would take minutes: the score bits of 256 sampled rows are the
    reference's, and the reference's statistic and decision on the device's own scores give the stats, the map and the cloud"""
    B, small = ro.normal(ro.MAX_POINTS, 12, dtype), ro.normal(65, 13, dtype)
    rule = (STAT, 8, 1.0)
    with ctx.batch([(B, small)]) as src:
        nb, info = src.remove_outliers(rule, None, want_maps=True, want_scores=True)
        with nb:
            got = nb.get_clouds()[0]
    score = info["moving_score"][0]
    rows = np.random.default_rng(14).choice(ro.MAX_POINTS, 256, replace=False)
    rows[:4] = (0, 63, 64, ro.MAX_POINTS - 1)
    assert bits_equal(score[rows], ro.dbar(B, rule[1], rows=rows))
    Y, m, _, st = ro.remove(B, rule, score=score)
    assert bits_equal(info["stats"][0], st) and 0 < st[3] < ro.MAX_POINTS and info["stats"][1].tolist() == [0, 0, 0, 65]
    assert np.array_equal(info["moving_map"][0], m) and bits_equal(got[0], Y) and bits_equal(got[1], small)


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_outlier_a_pairs_bits_are_its_own(ctx, dtype):
    """a pair's output is the same bytes alone, in a batch of 5 and with the pair order reversed.  Alone the scan runs with the
    register capacity of that pair's own k, in the batch with the capacity of the largest: the multiset does not depend on it"""
    pairs = [(ro.normal(n, 700 + b, dtype), ro.normal(m, 800 + b, dtype)) for b, (n, m) in enumerate([(63, 257), (64, 130), (65, 66), (257, 63), (130, 64)])]
    moving = [(STAT, 5, 1.0), (RAD, 0.8, 2), (STAT, 9, 0.5), None, (STAT, 32, 1.5)]
    model = [(RAD, 0.5, 2), (STAT, 17, 1.0), None, (STAT, 8, 0.0), (STAT, 16, 2.0)]

    def run(ps, a, b):
        with ctx.batch(ps) as src:
            nb, info = src.remove_outliers(a, b, want_maps=True, want_scores=True)
            with nb:
                return nb.get_clouds(), info

    ref = ro.remove_pairs(pairs, moving, model)
    five = run(pairs, moving, model)
    rev = run(pairs[::-1], moving[::-1], model[::-1])
    for b in range(5):
        one = run([pairs[b]], [moving[b]], [model[b]])
        for (clouds, info), k in ((five, b), (rev, 4 - b), (one, 0)):
            count = len(clouds)
            assert bits_equal(clouds[k][0], ref["clouds"][b][0]) and bits_equal(clouds[k][1], ref["clouds"][b][1]), b
            for side in ("moving", "model"):
                assert np.array_equal(info[side + "_map"][k], ref[side + "_map"][b]) and bits_equal(info[side + "_score"][k], ref[side + "_score"][b]), (b, side)
            assert bits_equal(info["stats"][k], ref["stats"][b]) and bits_equal(info["stats"][count + k], ref["stats"][5 + b]), b


# 5 ------------------------------------------------------------------------------------------------------------------------
def snapshot(pkg, bt):
    """everything a caller can read of a batch's loop, as bytes (or the error code that refuses it)"""
    out = []
    for name, fn in (("indices", bt.get_indices), ("loop_indices", bt.loop_indices), ("inliers", bt.get_inliers), ("moving", bt.get_moving),
                     ("done", bt.done), ("clouds", bt.get_clouds)):
        try:
            v = fn()
            out.append((name, [np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else tuple(x.tobytes() for x in a) for a in v]
                        if isinstance(v, list) else v.tobytes()))
        except pkg.IcpError as e:
            out.append((name, e.code))
    for b in range(bt.count):
        for name, fn in (("moments", bt.diag_moments), ("trim", bt.diag_trim)):
            try:
                v = fn(b)
                out.append((name, b, v.tobytes() if isinstance(v, np.ndarray) else (np.float64(v[0]).tobytes(), v[1])))
            except pkg.IcpError as e:
                out.append((name, b, e.code))
        try:
            st = bt.state(b)
            out.append(("state", b, st["status"], st["iterations"], st["passes"], st["err"].tobytes(), st["T"].tobytes()))
        except pkg.IcpError as e:
            out.append(("state", b, e.code))
    return out


@DTYPES
def test_outlier_refusals_leave_the_source_and_the_outputs_alone(ctx, pkg, dtype):
    INVALID, STATE, EMPTY = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE, pkg.capi.ICP_ERR_EMPTY
    Rule = pkg.capi.icp_outlier_rule
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES[:3]]
    lib = pkg.load()
    pd, p32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    good = (STAT, 8, 1.0)

    def raw(bt, moving, model):
        """the C call with every output given: (rc, message); *out must come back NULL and no output element may be written"""
        arr = lambda rules: None if rules is None else (Rule * bt.count)(*[Rule(*r) for r in rules])
        n, m = int(bt._moff[-1]), int(bt._qoff[-1])
        mm, qm = np.full(n, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32)
        ms, qs, st = np.full(n, -7.0), np.full(m, -7.0), np.full(8 * bt.count, -7.0)
        out = C.c_void_p(0x1234)
        rc = lib.icp_batch_remove_outliers(bt._h, arr(moving), arr(model), mm.ctypes.data_as(p32), qm.ctypes.data_as(p32), ms.ctypes.data_as(pd),
                                           qs.ctypes.data_as(pd), st.ctypes.data_as(pd), C.byref(out))
        msg = lib.icp_last_error().decode()
        assert out.value is None, msg
        assert (mm == -7).all() and (qm == -7).all() and (ms == -7.0).all() and (qs == -7.0).all() and (st == -7.0).all(), msg
        return rc, msg

    ok = [(1, 8, 1.0)] * 3
    with ctx.batch(pairs) as bt:
        bt.set_max_distance(0.3)
        bt.begin(max_iter=6, tol=1e-9)
        assert bt.run(2)[0] == 2
        before = snapshot(pkg, bt)
        bad_rules = [(7, 8, 1.0), (-1, 8, 1.0), (1, 0, 1.0), (1, 33, 1.0), (1, 8, -0.5), (1, 8, np.nan), (1, 8, np.inf), (2, 3, 0.0), (2, 3, -1.0),
                     (2, 3, np.nan), (2, 3, np.inf), (2, 0, 0.5), (2, 65536, 0.5)]
        for bad in bad_rules:
            for side in (0, 1):
                rules = list(ok)
                rules[1] = bad
                rc, msg = raw(bt, rules if side == 0 else ok, rules if side == 1 else ok)
                assert rc == INVALID and "pair 1" in msg and ("model" if side else "moving") in msg, (bad, side, msg)
                assert snapshot(pkg, bt) == before
        # a cloud that would keep no point (known after the first wait)
        rc, msg = raw(bt, ok, [(0, 0, 0.0), (0, 0, 0.0), (2, 1, 1e-9)])
        assert rc == EMPTY and "pair 2" in msg and "model" in msg, msg
        assert snapshot(pkg, bt) == before
        assert lib.icp_batch_remove_outliers(bt._h, None, None, None, None, None, None, None, None) == INVALID   # out == NULL
        with pytest.raises(pkg.IcpError) as e:   # ... and through Python
            bt.remove_outliers([good, (STAT, 40, 1.0), good])
        assert e.value.code == INVALID and "pair 1" in str(e.value)
        with pytest.raises(ValueError):
            bt.remove_outliers([good, good])
        with pytest.raises(ValueError):
            bt.remove_outliers(("median", 3, 1.0))
        # accepted: the source answers as before
        with bt.remove_outliers([good, good, None], (RAD, 0.5, 1))[0] as nb:
            assert nb.count == 3
        assert snapshot(pkg, bt) == before
    # n < k + 1, and a mean that is not finite (a squared distance overflows; known after the first wait): a batch without a loop
    huge = 1e30 if dtype == np.float32 else 1e200
    H = np.array([[huge, 0, 0], [-huge, 0, 0], [0, huge, 0]], dtype=dtype)
    with ctx.batch([pairs[0], (pairs[0][0], H)]) as bt:
        before = snapshot(pkg, bt)
        rc, msg = raw(bt, None, [(1, 8, 1.0), (1, 3, 1.0)])
        assert rc == INVALID and "pair 1" in msg and "model" in msg and "k + 1" in msg, msg
        rc, msg = raw(bt, None, [(1, 8, 1.0), (1, 2, 1.0)])
        assert rc == INVALID and "pair 1" in msg and "model" in msg and "not finite" in msg, msg
        assert snapshot(pkg, bt) == before
    # a context with a pending pass
    A, M = pairs[0]
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with c.batch(pairs[:2]) as bt:
            bt.begin(max_iter=6, tol=1e-9)
            assert bt.run(2)[0] == 2
            before = snapshot(pkg, bt)
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            with pytest.raises(pkg.IcpError) as e:
                bt.remove_outliers(good)
            assert e.value.code == STATE
            c.loop_complete()
            assert snapshot(pkg, bt) == before   # after the refusal the source answers as before
            with bt.remove_outliers(good)[0] as nb:
                assert nb.count == 2


@DTYPES
def test_outlier_the_loop_does_not_notice(ctx, pkg, dtype):
    """run src two steps, remove outliers between every two further steps: every export is that of a twin batch that never did"""
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            bt.set_max_distance(0.3)
            bt.set_trim(0.8)
            bt.begin(max_iter=12, tol=1e-6)
            assert bt.run(2)[0] == 2
        made = []
        steps = 2
        while True:
            if steps & 1:
                made.append(X.remove_outliers(None, [(RAD, 0.5, 2)] * 3 + [None])[0])
            else:
                made.append(X.remove_outliers((STAT, 8, 1.0), [(STAT, 16, 1.0)] * 3 + [None], want_maps=True, want_scores=True)[0])
            assert snapshot(pkg, X) == snapshot(pkg, Y), steps
            kx, ky = X.run(1), Y.run(1)
            assert kx == ky, (steps, kx, ky)
            if not ky[0]:
                break
            steps += 1
        assert steps >= 4 and X.done().all()
        fx, fy = final(X), final(Y)
        for b in range(len(pairs)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}")
        assert snapshot(pkg, X) == snapshot(pkg, Y)
    for nb in made:   # the source went first: the new batches are destroyed on their own
        assert nb.get_clouds()[0][0].dtype == dtype
        nb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@DTYPES
def test_outlier_the_new_batch_is_a_batch(ctx, pkg, dtype, plane):
    """remove outliers, downsample, estimate normals, register: the filtered batch runs as a batch created from the reference's
    clouds -- the thinned clouds, the normals, status, iterations, err series, idx, masks and the final cloud, bit for bit"""
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    moving = [(STAT, 8, 1.0), (STAT, 16, 1.0), (RAD, 0.3, 3), (STAT, 5, 2.0)]
    model = [(STAT, 8, 2.0), (RAD, 0.3, 2), (STAT, 12, 1.5), None]
    ref = ro.remove_pairs(pairs, moving, model)
    assert all(YM.shape[0] >= 5 for _, YM in ref["clouds"]) and any(s[3] < p[0].shape[0] for s, p in zip(ref["stats"], pairs))
    vm, vq = [0.5, 0.0, 0.5, 0.0], [0.0, 0.5, 0.5, 0.0]
    with ctx.batch(pairs) as src, src.remove_outliers(moving, model)[0] as X0, ctx.batch(ref["clouds"]) as Y0:
        with X0.downsample(vm, vq) as X, Y0.downsample(vm, vq) as Y:
            for (a, b), (c, d) in zip(X.get_clouds(), Y.get_clouds()):
                assert bits_equal(a, c) and bits_equal(b, d)
            nrm = []
            for bt in (X, Y):
                if plane:
                    nrm.append(bt.estimate_normals())
                bt.set_max_distance(0.5)
                bt.begin(max_iter=15, tol=1e-6, metric=metric)
            if plane:
                for a, b in zip(*nrm):
                    assert bits_equal(a, b)
            steps = 0
            while True:
                kx, ky = X.run(1), Y.run(1)
                assert kx == ky
                if not ky[0]:
                    break
                steps += 1
                assert snapshot(pkg, X) == snapshot(pkg, Y), steps
            fx, fy = final(X), final(Y)
            for b in range(len(pairs)):
                same_pair_bytes(fx[b], fy[b], f"pair {b}")
            assert steps >= 3
