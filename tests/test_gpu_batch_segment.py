"""GPU: the dominant plane of every cloud of a batch on the device (icp_batch_segment_plane; Batch.segment_plane).

The rule is stated in include/icp_mi355x.h and restated in numpy in tests/batch_segment_ref.py; tests/test_batch_segment_ref.py pins
that reference on hand cases.  This file compares the device with it for byte equality -- triples, validity, per-hypothesis counts,
winner, the four plane doubles, inlier counts, status, masks, maps and the new clouds -- in fp32 and fp64.  No tolerance is
introduced: the counts are integers, and every double is one stated operation."""
import ctypes as C

import numpy as np
import pytest

import batch_segment_ref as sr
from batch_ref import CASES, bits_equal, final, gate_case, same_pair_bytes

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
DET, REM, KEEP = sr.DETECT, sr.REMOVE, sr.KEEP


def device(src, moving, model, seeds):
    return src.segment_plane([sr.as_tuple(r) for r in moving], [sr.as_tuple(r) for r in model], seed=np.asarray(seeds, dtype=np.uint64),
                             want_masks=True, want_maps=True)


def same_as_reference(src, nb, info, ref, what):
    """everything the call and the diagnostic export report equals the reference's, byte for byte"""
    count = src.count
    got = nb.get_clouds()
    for b in range(count):
        for side, name in enumerate(("moving", "model")):
            r, k = ref[side][b], side * count + b
            at = (what, b, name)
            assert bits_equal(got[b][side], r["cloud"]), (at, "cloud", got[b][side].shape, r["cloud"].shape)
            assert np.array_equal(info[name + "_map"][b], r["map"]) and info[name + "_map"][b].dtype == np.int32, (at, "map")
            assert np.array_equal(info[name + "_mask"][b], r["mask"]) and info[name + "_mask"][b].dtype == np.uint8, (at, "mask")
            assert bits_equal(info["planes"][k], r["plane"]), (at, "plane", info["planes"][k], r["plane"])
            assert int(info["inliers"][k]) == r["inliers"] and int(info["status"][k]) == r["status"], (at, info["inliers"][k], r["inliers"], info["status"][k])
            if r["triples"] is None:
                continue
            d = src.diag_segment(b, side)
            assert np.array_equal(d["triples"], r["triples"]), (at, "triples")
            assert np.array_equal(d["valid"], r["valid"]), (at, "valid")
            assert bits_equal(d["planes"], r["planes"]), (at, "hypotheses")
            assert np.array_equal(d["counts"], r["counts"]), (at, "counts", int((d["counts"] != r["counts"]).sum()))
            if r["winner"] >= 0:
                assert r["winner"] == int(np.argmax(d["counts"]))


def check_batch(ctx, pairs, moving, model, seeds, what):
    ref = sr.segment_pairs(pairs, moving, model, seeds)
    with ctx.batch(pairs) as src:
        nb, info = device(src, moving, model, seeds)
        with nb:
            assert nb.count == len(pairs)
            same_as_reference(src, nb, info, ref, what)
        for (D, M), (GD, GM) in zip(pairs, src.get_clouds()):   # the source holds what was uploaded
            assert bits_equal(GD, D) and bits_equal(GM, M), (what, "source clouds")
    return ref


# 1 ------------------------------------------------------------------------------------------------------------------------
SIZES = (3, 4, 63, 64, 65, 130, 1000)
HYPS = (1, sr.GROUP - 1, sr.GROUP, sr.GROUP + 1)   # one, and one below, at and above the score kernel's group


def size_pairs(dtype):
    """one pair per size; half of every cloud lies on a plane of its own; the hypothesis counts cycle through HYPS, the kinds through
    DETECT, REMOVE and KEEP, and the 130-point cloud takes one hypothesis more than a scoring launch holds"""
    pairs, moving, model = [], [], []
    for b, n in enumerate(SIZES):
        m = SIZES[(b + 3) % len(SIZES)]
        pairs.append((sr.planted(n, 0.5, dtype, seed=100 + b, normal=(0.2, 0.1 * b, 1.0), offset=0.1),
                      sr.planted(m, 0.5, dtype, seed=200 + b, normal=(1.0, -0.3, 0.05 * b), offset=-0.2)))
        H = sr.CHUNK + 1 if n == 130 else HYPS[b % 4]
        moving.append(sr.rule((DET, REM, KEEP)[b % 3], 0.01, H))
        model.append(sr.rule((REM, KEEP, DET)[b % 3], 0.02, HYPS[(b + 1) % 4] if m > 4 else 40))
    return pairs, moving, model


@DTYPES
def test_segment_sizes_and_hypothesis_counts(ctx, dtype):
    pairs, moving, model = size_pairs(dtype)
    assert {r["hypotheses"] for r in moving} >= set(HYPS) | {sr.CHUNK + 1}
    seeds = [7 + b for b in range(len(pairs))]
    # (a KEEP cloud needs a plane and a REMOVE cloud a point off it: the reference says which rules the call accepts)
    ref = sr.segment_pairs(pairs, moving, model, seeds)
    for side, rules in enumerate((moving, model)):
        for b, r in enumerate(ref[side]):
            if r["cloud"].shape[0] == 0:
                rules[b] = sr.rule(DET, rules[b]["distance"], rules[b]["hypotheses"])
    ref = check_batch(ctx, pairs, moving, model, seeds, "sizes")
    assert any(r["refit"] for r in ref[0] + ref[1]) and any(0 < r["cloud"].shape[0] < p[0].shape[0] for r, p in zip(ref[0], pairs))


# 2 ------------------------------------------------------------------------------------------------------------------------
def threshold_cloud(dtype, distance):
    """an 8 x 8 lattice on z = 0, ten pairs of points at exactly z = +-distance (each pair above the same lattice point, next to
    each other in the cloud), four pairs at the next value of dtype above (fewer, so that no plane near z = distance / 2 gathers as
    many as z = 0)"""
    out = np.nextafter(dtype(distance), dtype(1.0))
    L = [[x, y, 0.0] for x in range(8) for y in range(8)]
    on = [[k % 8, k // 2, s * distance] for k in range(10) for s in (1.0, -1.0)]
    off = [[k % 8, 7 - k // 2, s * float(out)] for k in range(4) for s in (1.0, -1.0)]
    return np.ascontiguousarray(np.array(L[:32] + on + L[32:] + off, dtype=dtype))


@DTYPES
def test_segment_threshold(ctx, dtype):
    dist = 0.015625   # 2^-6: exactly representable, and small against the lattice's spacing -- no tilted plane gathers as many
    X = threshold_cloud(dtype, dist)
    ref = check_batch(ctx, [(X, X)], [sr.rule(DET, dist, 64)], [sr.rule(KEEP, dist, 64)], [3], "threshold")
    for r in (ref[0][0], ref[1][0]):
        assert r["plane"].tolist() == [0.0, 0.0, 1.0, 0.0] and np.signbit(r["plane"][3]) and r["inliers"] == 84
        z = X[:, 2].astype(np.float64)
        assert r["mask"][np.abs(z) == dist].all() and r["mask"][z == 0].all() and not r["mask"][np.abs(z) > dist].any()
        assert int((np.abs(z) == dist).sum()) == 20 and int((np.abs(z) > dist).sum()) == 8


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_segment_axis(ctx, dtype):
    """a large vertical patch and a smaller horizontal one: free, the vertical one wins; with axis = z and min_cos = 0.9, the
    horizontal one"""
    rng = np.random.default_rng(2)
    wall = np.column_stack([np.zeros(300), rng.uniform(0, 2, 300), rng.uniform(0, 2, 300)])
    floor = np.column_stack([rng.uniform(0, 2, 120), rng.uniform(0, 2, 120), np.zeros(120)])
    X = np.ascontiguousarray(np.vstack([wall, floor, rng.uniform(0, 2, (60, 3))])[rng.permutation(480)].astype(dtype))
    ref = check_batch(ctx, [(X, X)], [sr.rule(REM, 0.01, 300)], [sr.rule(KEEP, 0.01, 300, axis=(0, 0, 2.0), min_cos=0.9)], [9], "axis")
    free, held = ref[0][0], ref[1][0]
    assert abs(free["plane"][0]) > 0.999 and free["inliers"] >= 300 and free["cloud"].shape[0] == 480 - free["inliers"]
    assert abs(held["plane"][2]) > 0.999 and 120 <= held["inliers"] < 300 and held["cloud"].shape[0] == held["inliers"]


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_segment_kinds(ctx, dtype):
    A = sr.planted(257, 0.4, dtype, seed=31)
    A[5] = [-0.0, 0.5, -0.0]
    A[200, 1] = -0.0
    line = np.ascontiguousarray(np.outer(np.arange(70), [1.0, 2.0, -0.5]).astype(dtype))
    rl = lambda kind: sr.rule(kind, 0.004, 100)
    pairs = [(A, A), (A, A), (line, line), (A, line)]
    moving = [None, rl(REM), rl(DET), rl(DET)]
    model = [rl(DET), rl(KEEP), rl(REM), None]
    ref = check_batch(ctx, pairs, moving, model, [5, 5, 6, 7], "kinds")
    assert bits_equal(ref[0][0]["cloud"], A) and bits_equal(ref[1][0]["cloud"], A) and np.signbit(ref[1][0]["cloud"][5, 0])   # NONE and DETECT copy
    rem, keep = ref[0][1], ref[1][1]                                 # (the same cloud and seed, but the other side: another plane search)
    for r in (rem, keep):
        inl = r["mask"].astype(bool)
        want = A[~inl] if r is rem else A[inl]
        assert bits_equal(r["cloud"], want) and 0 < want.shape[0] < 257
    for r in (ref[0][2], ref[1][2]):                                 # collinear: no valid hypothesis -> ICP_ERR_EMPTY, copied
        assert r["status"] == sr.ERR_EMPTY and bits_equal(r["cloud"], line) and not r["plane"].any() and not r["mask"].any()
    # REMOVE and KEEP of one cloud under one seed and side are complementary and keep the order
    with ctx.batch([(A, A)]) as src:
        (r, ri), (k, ki) = device(src, [rl(REM)], [None], [5]), device(src, [rl(KEEP)], [None], [5])
        with r, k:
            R, K = r.get_clouds()[0][0], k.get_clouds()[0][0]
            inl = ri["moving_mask"][0].astype(bool)
            assert np.array_equal(ri["moving_mask"][0], ki["moving_mask"][0]) and bits_equal(ri["planes"], ki["planes"])
            assert bits_equal(R, A[~inl]) and bits_equal(K, A[inl]) and R.shape[0] + K.shape[0] == 257
            assert np.array_equal((ri["moving_map"][0] >= 0), ~(ki["moving_map"][0] >= 0))


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_segment_independence(ctx, dtype):
    """a pair alone, the same pair among pairs of other sizes, and in another position: the same bytes"""
    P = (sr.planted(300, 0.5, dtype, seed=41), sr.planted(130, 0.4, dtype, seed=42, normal=(1, 1, 0)))
    others = [(sr.planted(n, 0.5, dtype, seed=50 + n), sr.planted(m, 0.5, dtype, seed=60 + m)) for n, m in ((65, 1000), (1000, 3), (64, 64))]
    rm, rq = sr.rule(REM, 0.01, 70), sr.rule(KEEP, 0.01, 33)
    ro = sr.rule(DET, 0.02, 40)

    def outputs(pairs, at):
        k = len(pairs)
        with ctx.batch(pairs) as src:
            nb, info = device(src, [rm if b == at else ro for b in range(k)], [rq if b == at else None for b in range(k)],
                              [99 if b == at else b for b in range(k)])
            with nb:
                cl = nb.get_clouds()[at]
                dg = [src.diag_segment(at, s) for s in (0, 1)]
                return [cl[0].tobytes(), cl[1].tobytes()] + [info[n][at].tobytes() for n in ("moving_mask", "model_mask", "moving_map", "model_map")] + \
                       [info[n][[at, k + at]].tobytes() for n in ("planes", "inliers", "status")] + [d[n].tobytes() for d in dg for n in ("triples", "valid", "planes", "counts")]

    alone = outputs([P], 0)
    assert outputs([others[0], P, others[1], others[2]], 1) == alone
    assert outputs([others[2], others[1], others[0], P], 3) == alone


# 6 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
def test_segment_range(ctx, dtype, sign):
    """a cloud and its distance times 2^e, e = +-30 in fp32 and +-200 in fp64: the same triples, counts, masks and n, d scaled
    exactly -- and the reference's bits"""
    e = sign * (30 if dtype == np.float32 else 200)
    s = 2.0 ** e
    A, M = sr.planted(400, 0.5, dtype, seed=71, normal=(0.3, 0.4, 1.0)), sr.planted(130, 0.6, dtype, seed=72, normal=(1.0, 0.2, 0.1))
    As, Ms = (A.astype(np.float64) * s).astype(dtype), (M.astype(np.float64) * s).astype(dtype)
    assert np.array_equal(As.astype(np.float64), A.astype(np.float64) * s)   # (exact)
    base = check_batch(ctx, [(A, M)], [sr.rule(REM, 0.01, 100)], [sr.rule(KEEP, 0.01, 100)], [13], "range, base")
    big = check_batch(ctx, [(As, Ms)], [sr.rule(REM, 0.01 * s, 100)], [sr.rule(KEEP, 0.01 * s, 100)], [13], f"range, 2^{e}")
    for side in (0, 1):
        a, b = base[side][0], big[side][0]
        assert np.array_equal(a["triples"], b["triples"]) and np.array_equal(a["valid"], b["valid"]) and np.array_equal(a["counts"], b["counts"])
        assert np.array_equal(a["mask"], b["mask"]) and a["inliers"] == b["inliers"] and a["refit"] == b["refit"]
        assert bits_equal(a["plane"][:3], b["plane"][:3]) and bits_equal(np.float64(a["plane"][3] * s), b["plane"][3])
        assert a["inliers"] >= 0.4 * a["mask"].shape[0]


# 7 ------------------------------------------------------------------------------------------------------------------------
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
        try:
            out.append(("moments", b, bt.diag_moments(b).tobytes()))
        except pkg.IcpError as e:
            out.append(("moments", b, e.code))
        try:
            st = bt.state(b)
            out.append(("state", b, st["status"], st["iterations"], st["passes"], st["err"].tobytes(), st["T"].tobytes()))
        except pkg.IcpError as e:
            out.append(("state", b, e.code))
    return out


@DTYPES
def test_segment_refusals_leave_the_source_and_the_outputs_alone(ctx, pkg, dtype):
    INVALID, STATE, EMPTY = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE, pkg.capi.ICP_ERR_EMPTY
    Rule = pkg.capi.icp_plane_rule
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES[:3]]
    lib = pkg.load()
    pd, p32, p8, pu64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    mk = lambda kind, hyp, dist, axis=(0.0, 0.0, 0.0), mc=0.0: Rule(kind, hyp, dist, (C.c_double * 3)(*axis), mc)

    def raw(bt, moving, model, seeded=True):
        """the C call with every output given: (rc, message); *out must come back NULL and no output element may be written"""
        arr = lambda rules: None if rules is None else (Rule * bt.count)(*[mk(*r) for r in rules])
        n, m = int(bt._moff[-1]), int(bt._qoff[-1])
        mm, qm = np.full(n, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32)
        mk8, qk8 = np.full(n, 9, dtype=np.uint8), np.full(m, 9, dtype=np.uint8)
        pl, inl, st = np.full(8 * bt.count, -7.0), np.full(2 * bt.count, -7, dtype=np.int32), np.full(2 * bt.count, -7, dtype=np.intc)
        seed = np.arange(bt.count, dtype=np.uint64)
        out = C.c_void_p(0x1234)
        rc = lib.icp_batch_segment_plane(bt._h, arr(moving), arr(model), seed.ctypes.data_as(pu64) if seeded else None, pl.ctypes.data_as(pd),
                                         inl.ctypes.data_as(p32), st.ctypes.data_as(C.POINTER(C.c_int)), mk8.ctypes.data_as(p8), qk8.ctypes.data_as(p8),
                                         mm.ctypes.data_as(p32), qm.ctypes.data_as(p32), C.byref(out))
        msg = lib.icp_last_error().decode()
        assert out.value is None, msg
        assert (mm == -7).all() and (qm == -7).all() and (mk8 == 9).all() and (qk8 == 9).all() and (pl == -7.0).all() and (inl == -7).all() and (st == -7).all(), msg
        return rc, msg

    ok = [(2, 50, 0.01)] * 3
    with ctx.batch(pairs) as bt:
        bt.set_max_distance(0.3)
        bt.begin(max_iter=6, tol=1e-9)
        assert bt.run(2)[0] == 2
        with bt.segment_plane(("remove", 0.01, 20), ("detect", 0.01, 20), seed=1)[0]:   # (an accepted call first: the diagnostic export holds its hypotheses)
            pass
        before = snapshot(pkg, bt), [bt.diag_segment(1, s)["counts"].tobytes() for s in (0, 1)]
        now = lambda: (snapshot(pkg, bt), [bt.diag_segment(1, s)["counts"].tobytes() for s in (0, 1)])
        bad_rules = [(4, 50, 0.01), (-1, 50, 0.01), (2, 0, 0.01), (2, 65537, 0.01), (2, 50, -0.5), (2, 50, np.nan), (2, 50, np.inf),
                     (2, 50, 0.01, (np.nan, 0, 0), 0.5), (2, 50, 0.01, (0, np.inf, 0), 0.5), (2, 50, 0.01, (0, 0, 1), -0.1),
                     (2, 50, 0.01, (0, 0, 1), 1.5), (2, 50, 0.01, (0, 0, 1), np.nan)]
        for bad in bad_rules:
            for side in (0, 1):
                rules = list(ok)
                rules[1] = bad
                rc, msg = raw(bt, rules if side == 0 else ok, rules if side == 1 else ok)
                assert rc == INVALID and "pair 1" in msg and ("model" if side else "moving") in msg, (bad, side, msg)
        assert now() == before
        rc, msg = raw(bt, [(0, 0, 0.0), (1, 10, 0.01), (0, 0, 0.0)], None, seeded=False)   # null seeds where a rule searches
        assert rc == INVALID and "seed" in msg and "pair 1" in msg, msg
        # ICP_ERR_EMPTY for the whole call, both cases: a REMOVE cloud whose every point is an inlier, a KEEP cloud with no plane
        rc, msg = raw(bt, ok, [(0, 0, 0.0), (0, 0, 0.0), (2, 50, 1e6)])
        assert rc == EMPTY and "pair 2" in msg and "model" in msg, msg
        assert now() == before
        assert lib.icp_batch_segment_plane(bt._h, None, None, None, None, None, None, None, None, None, None, None) == INVALID   # out == NULL
        with pytest.raises(pkg.IcpError) as e:   # ... and through Python
            bt.segment_plane([("remove", 0.01), ("remove", 0.01, 0), ("remove", 0.01)])
        assert e.value.code == INVALID and "pair 1" in str(e.value)
        with pytest.raises(ValueError):
            bt.segment_plane([("remove", 0.01)] * 2)
        with pytest.raises(ValueError):
            bt.segment_plane(("peel", 0.01))
        assert now() == before
    line = np.ascontiguousarray(np.outer(np.arange(40), [1.0, -1.0, 0.25]).astype(dtype))
    two = np.ascontiguousarray(pairs[0][0][:2])
    with ctx.batch([pairs[0], (line, two)]) as bt:
        before = snapshot(pkg, bt)
        rc, msg = raw(bt, [(1, 10, 0.01), (3, 10, 0.01)], None)                        # KEEP with no plane
        assert rc == EMPTY and "pair 1" in msg and "moving" in msg and "no plane" in msg, msg
        rc, msg = raw(bt, None, [(0, 0, 0.0), (1, 10, 0.01)])                          # a searched cloud of n < 3
        assert rc == INVALID and "pair 1" in msg and "model" in msg and "3 points" in msg, msg
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_segment(0, 0)                                                      # no accepted call so far
        assert e.value.code == STATE and snapshot(pkg, bt) == before
        with bt.segment_plane([("detect", 0.01, 10), ("detect", 0.01, 10)], None, seed=3)[0] as nb:   # no plane under DETECT: copied
            assert bits_equal(nb.get_clouds()[1][0], line)
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_segment(0, 1)                                                      # that call did not search the models
        assert e.value.code == STATE
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
                bt.segment_plane(("remove", 0.01, 20))
            assert e.value.code == STATE
            c.loop_complete()
            assert snapshot(pkg, bt) == before   # after the refusal the source answers as before
            with bt.segment_plane(("remove", 0.01, 20))[0] as nb:
                assert nb.count == 2


@DTYPES
def test_segment_the_loop_does_not_notice(ctx, pkg, dtype):
    """run src two steps, segment between every two further steps: every export is that of a twin batch that never did"""
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
                made.append(X.segment_plane(None, [("keep", 0.05, 40)] * 3 + [None], seed=steps)[0])
            else:
                made.append(X.segment_plane(("remove", 0.02, 33), ("detect", 0.02, 64, (0, 0, 1), 0.5), seed=steps, want_masks=True, want_maps=True)[0])
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


# 8 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_segment_the_new_batch_is_a_batch(ctx, pkg, dtype):
    """segment, then register: the new batch runs as a batch created from the reference's clouds -- status, iterations, err series,
    idx, masks and the final cloud, bit for bit"""
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    moving = [sr.rule(REM, 0.05, 40), sr.rule(KEEP, 0.2, 33), None, sr.rule(DET, 0.05, 10)]
    model = [sr.rule(REM, 0.05, 64), None, sr.rule(REM, 0.1, 31), sr.rule(DET, 0.05, 10)]
    seeds = [1, 2, 3, 4]
    ref = sr.segment_pairs(pairs, moving, model, seeds)
    clouds = [(a["cloud"], b["cloud"]) for a, b in zip(*ref)]
    assert all(c[0].shape[0] >= 3 and c[1].shape[0] >= 3 for c in clouds) and any(c[0].shape[0] < p[0].shape[0] for c, p in zip(clouds, pairs))
    with ctx.batch(pairs) as src, device(src, moving, model, seeds)[0] as X, ctx.batch(clouds) as Y:
        assert np.array_equal(X._moff, Y._moff) and np.array_equal(X._qoff, Y._qoff)
        for bt in (X, Y):
            bt.set_max_distance(0.5)
            bt.begin(max_iter=15, tol=1e-6)
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


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_segment_hall(ctx):
    """the hall pair with the CPU test's rule (tests/test_batch_segment_ref.py::test_hall_wall): the device equals numpy bit for bit
    and meets the same share, >= 15 % (the reference measures 22.2 % on both clouds)"""
    P, Q = sr.hall()
    ref = sr.hall_reference()
    with ctx.batch([(P, Q)]) as src:
        nb, info = device(src, [sr.HALL_RULE], [sr.HALL_RULE], [sr.HALL_SEED])
        with nb:
            same_as_reference(src, nb, info, ([ref[0]], [ref[1]]), "hall")
            for k, X in enumerate((P, Q)):
                share = int(info["inliers"][k]) / X.shape[0]
                print(f"hall, device: {int(info['inliers'][k])} of {X.shape[0]} = {share:.4f}")
                assert share >= 0.15
                assert nb.get_clouds()[0][k].shape[0] == X.shape[0] - int(info["inliers"][k])


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_register_batch_global_planes_option(ctx, pkg):
    """register_batch_global(..., planes=rule) applies the rule before everything else: with a DETECT rule the clouds are copied, so
    the poses are the bytes of a run without the option, and extra["global"] carries the planes Batch.segment_plane reports"""
    pairs = [gate_case(*c, dtype=np.float32)[:2] for c in CASES[:2]]
    rl = ("detect", 0.05, 33)
    plain = ctx.register_batch_global(pairs, 0.0, 8, 64, 0.3, seed=5, max_iter=5)
    with_planes = ctx.register_batch_global(pairs, 0.0, 8, 64, 0.3, seed=5, max_iter=5, planes=rl)
    with ctx.batch(pairs) as src:
        nb, info = src.segment_plane(rl, rl, seed=5)
        nb.close()
    for b, (x, y) in enumerate(zip(plain, with_planes)):
        assert x.T.tobytes() == y.T.tobytes() and x.extra["global"]["T"].tobytes() == y.extra["global"]["T"].tobytes()
        assert "planes" not in x.extra["global"]
        assert bits_equal(y.extra["global"]["planes"], info["planes"][[b, 2 + b]])
        assert y.extra["global"]["plane_inliers"] == (int(info["inliers"][b]), int(info["inliers"][2 + b]))
    with pytest.raises(TypeError):
        ctx.register_batch_global(pairs, 0.0, 8, 64, 0.3, plains=rl)
