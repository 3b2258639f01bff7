"""GPU: ISS keypoints selected on the device (icp_batch_select_keypoints; Batch.keypoints, Context.register_batch_global(...,
keypoints=rule)) against the numpy restatement tests/batch_keypoint_ref.py.

    1  bit for bit -- saliency, maps, counts, output clouds, carried descriptors: clouds of 5, 63, 64, 65, 130, 257 and 520 points (a
       single ragged item, full items, ragged last items, up to nine items per cloud) on batch_feature_ref.blob, both dtypes, fp64 clouds with mantissas fp32 cannot hold, a rule of its own per cloud -- found by
       pick(), in the restatement alone, so that 20 to 60 % of the points are candidates (sal > 0) and a keypoint exists --
       ICP_KEYPOINT_NONE among them and a NULL side; a pair alone and at either end of a batch; clouds of one tile and just past it
    2  special clouds: a lattice with ties on both radii, coincident points (bit-equal saliency: kept or dropped together), a line
       (w0 == 0: ICP_ERR_EMPTY, the pair named), a cloud 1e4 from the origin
    3  carried descriptors: compute_features on the source, then keypoints: get_features of the new batch are the gathered rows,
       match_features on it is batch_feature_ref.match on those rows; a source without descriptors gives a batch without, on
       either side and on both (a source with descriptors on one side only cannot be made: icp_batch_compute_features and
       icp_diag_batch_set_features both set both sides)
    4  a loop under way on the source does not notice; every refusal, with the outputs untouched
    5  end to end on the dense bunny pair, see test_dense_bunny_end_to_end"""
import ctypes as C
import itertools

import numpy as np
import pytest

import batch_feature_ref as fr
import batch_keypoint_ref as kr
import batch_outlier_ref as orf
from batch_ref import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = (5, 63, 64, 65, 130, 257, 520)
_PICK = {}


def fine(X, seed):
    """fp64 clouds get mantissas fp32 cannot hold"""
    if X.dtype == np.float64:
        X = X + 1e-9 * np.random.default_rng(seed).standard_normal(X.shape)
    return np.ascontiguousarray(X)


def cloud(seed, n, dtype):
    X, N = fr.blob(seed, n, dtype)
    return fine(X, seed + 1), N


def pick(X):
    """(rule, keep, sal): the first rule of a fixed list under which, by the restatement, 20 to 60 % of the cloud's points are
    candidates and at least one is a keypoint.  Computed once per cloud and left unchanged"""
    key = (X.dtype.str, X.tobytes())
    if key not in _PICK:
        spacing = float(np.sqrt(orf.d2_rows(X, 0, X.shape[0]).astype(np.float64) + np.eye(X.shape[0]) * 1e300).min(axis=1).mean())
        found = None
        for a, b, g21, least in itertools.product((3.0, 2.2, 4.0, 1.6, 5.5, 1.2, 2.0, 1.8, 2.5, 1.4), (0.6, 0.9, 0.4, 0.2), (0.45, 0.975, 0.7, 0.3, 0.2, 0.1, 0.6, 0.85, 0.05), (3, 1, 2, 5)):
            r = kr.rule(round(a * spacing, 5), round(a * b * spacing, 5), g21, 0.975, least)
            keep, sal = kr.select(X, r)
            if 0.2 <= (sal > 0).mean() <= 0.6 and keep.any():
                found = (r, keep, sal)
                break
        assert found is not None, "no rule of the list makes 20 to 60 % of this cloud candidates"
        _PICK[key] = found
    return _PICK[key]


def reference(X, r):
    """(Y, map, sal) of one cloud by the restatement, through pick()'s cache where the rule is the picked one"""
    if r is not None:
        key = (X.dtype.str, X.tobytes())
        if key in _PICK and _PICK[key][0] == r:
            _, keep, sal = _PICK[key]
            return X[keep].copy(), np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32), sal
    return kr.keypoints(X, r)


def descriptors(seed, n):
    """(n, 33) float64 of arbitrary bytes: random values, a -0.0, an infinity and a NaN with a payload"""
    F = np.random.default_rng(seed).uniform(-100.0, 100.0, (n, fr.BINS))
    F[0, 0], F[n - 1, 32], F[n // 2, 7] = -0.0, np.inf, np.nan
    F.view(np.uint64)[n // 2, 8] = 0x7FF8_0000_DEAD_BEEF
    return np.ascontiguousarray(F)


def check(pairs, rules_m, rules_q, kb, info, feats=None, what=""):
    """everything a call returned against the restatement, bit for bit"""
    count = len(pairs)
    clouds = kb.get_clouds()
    got_f = kb.get_features() if feats is not None else None
    for b, (A, M) in enumerate(pairs):
        for side, X, r in ((0, A, None if rules_m is None else rules_m[b]), (1, M, None if rules_q is None else rules_q[b])):
            Y, m, sal = reference(X, r)
            tag = f"{what} pair {b} {'model' if side else 'moving'} n {X.shape[0]} rule {r}"
            gs = info["model_saliency" if side else "moving_saliency"][b]
            bad = np.flatnonzero(gs.view(np.uint64) != sal.view(np.uint64))
            assert bad.size == 0, f"{tag}: {bad.size} saliencies differ, first {bad[0]}: {gs[bad[0]]!r} / {sal[bad[0]]!r}"
            assert bits_equal(info["model_map" if side else "moving_map"][b], m), tag
            assert info["counts"][side * count + b] == Y.shape[0], tag
            assert clouds[b][side].dtype == X.dtype and bits_equal(clouds[b][side], Y), tag
            if feats is not None:
                assert bits_equal(got_f[side][b], feats[side][b][m >= 0]), tag


# 1 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_keypoints_bit_for_bit(ctx, pkg, dtype):
    movers = [cloud(200 + n, n, dtype)[0] for n in SIZES]
    models = [cloud(300 + n, n, dtype)[0] for n in reversed(SIZES)]
    movers[1][0, 0] = -0.0                                       # a copied cloud: the -0.0 survives
    rules_m = [None if b == 1 else pick(X)[0] for b, X in enumerate(movers)]
    rules_q = [None if b == 4 else pick(X)[0] for b, X in enumerate(models)]
    assert len({r for r in rules_m + rules_q if r is not None}) >= 4   # the rules differ within the batch
    pairs = list(zip(movers, models))
    feats = ([descriptors(10 + b, X.shape[0]) for b, X in enumerate(movers)], [descriptors(30 + b, X.shape[0]) for b, X in enumerate(models)])
    with ctx.batch(pairs) as bt:
        bt.diag_set_features(*feats)
        kb, info = bt.keypoints(moving=rules_m, model=rules_q, want_maps=True, want_saliency=True)
        with kb:
            check(pairs, rules_m, rules_q, kb, info, feats)
            assert np.signbit(kb.get_clouds()[1][0][0, 0])
            for b, X in enumerate(movers):
                if rules_m[b] is not None:
                    share = float((info["moving_saliency"][b] > 0).mean())
                    assert 0.2 <= share <= 0.6, (b, share)
        # a NULL side copies it; no outputs asked for
        kb, info = bt.keypoints(model=rules_q)
        with kb:
            assert set(info) == {"counts"} and (info["counts"][:len(pairs)] == [X.shape[0] for X in movers]).all()
            for b, (A, M) in enumerate(pairs):
                got = kb.get_clouds()[b]
                assert bits_equal(got[0], A) and bits_equal(got[1], reference(M, rules_q[b])[0])
            assert bits_equal(np.concatenate(kb.get_features()[0]), np.concatenate(feats[0]))
        assert all(bits_equal(a, b) for a, b in zip(bt.get_features()[0], feats[0]))   # the source keeps its own


@DTYPES
def test_a_pairs_keypoints_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X = (cloud(207, 300, dtype)[0], cloud(208, 130, dtype)[0])
    Y = (cloud(209, 130, dtype)[0], cloud(210, 65, dtype)[0])
    Z = (cloud(211, 70, dtype)[0], cloud(212, 520, dtype)[0])
    rule = lambda pr: (pick(pr[0])[0], pick(pr[1])[0])
    rx, ry, rz = rule(X), rule(Y), rule(Z)

    def run(pairs, rules):
        with ctx.batch(pairs) as bt:
            kb, info = bt.keypoints(moving=[r[0] for r in rules], model=[r[1] for r in rules], want_maps=True, want_saliency=True)
            with kb:
                check(pairs, [r[0] for r in rules], [r[1] for r in rules], kb, info)
                return info, kb.get_clouds()

    alone, ca = run([X], [rx])
    first, cf = run([X, Y, Z], [rx, ry, rz])
    last, cl = run([Z, Y, X], [rz, ry, rx])
    for f in ("moving_saliency", "model_saliency", "moving_map", "model_map"):
        assert bits_equal(alone[f][0], first[f][0]) and bits_equal(alone[f][0], last[f][2]), f
    for side in range(2):
        assert bits_equal(ca[0][side], cf[0][side]) and bits_equal(ca[0][side], cl[2][side])


@DTYPES
def test_clouds_longer_than_a_tile(ctx, pkg, dtype):
    """the saliency pass loads 2 048 (fp32) / 1 024 (fp64) points per tile and a wave of the selection 512 / 256 per sub-tile: a cloud
    just past one tile, whose quarters are just past one sub-tile, beside a cloud of exactly one tile"""
    tile = 2048 if dtype == np.float32 else 1024
    A, M = cloud(261, tile + 70, dtype)[0], cloud(262, tile, dtype)[0]
    rules_m, rules_q = [pick(A)[0]], [pick(M)[0]]
    with ctx.batch([(A, M)]) as bt:
        kb, info = bt.keypoints(moving=rules_m, model=rules_q, want_maps=True, want_saliency=True)
        with kb:
            check([(A, M)], rules_m, rules_q, kb, info)


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_special_clouds(ctx, pkg, dtype):
    lat = orf.lattice(dtype, side=6, step=0.5)                   # d2 of 1.0 and 0.25 are lattice distances: ties on both radii
    lat_rule = kr.rule(1.0, 0.5, 1.5, 1.5, 5)                    # (gammas above 1: the symmetric interior passes the ratio tests)
    co = orf.coincident(dtype)
    far = orf.far(dtype)[:200].copy()
    blob = cloud(221, 130, dtype)[0]
    rb, kb_, sb = pick(blob)
    best = np.flatnonzero(kb_)
    best = best[np.argsort(-sb[best])][:2]                       # the blob's two most salient keypoints, each planted a second time
    twin = np.ascontiguousarray(np.concatenate([blob[:40], blob[best], blob[40:]]))
    pairs = [(lat, co), (far, blob), (twin, blob)]
    rules_m, rules_q = [lat_rule, pick(far)[0], rb], [pick(co)[0], rb, None]
    with ctx.batch(pairs) as bt:
        kb, info = bt.keypoints(moving=rules_m, model=rules_q, want_maps=True, want_saliency=True)
        with kb:
            check(pairs, rules_m, rules_q, kb, info)
    sal, m = info["moving_saliency"][0], info["moving_map"][0]
    top = sal == sal.max()
    assert top.sum() >= 8 and (m[top] >= 0).all()                # the interior: bit-equal saliencies within tn of each other keep each other
    on = kr.within(lat, 1.0).sum(axis=1)
    assert on.max() == 33 and (on[top] == 33).all()              # ... and their neighbourhoods hold the six points exactly on the radius
    d = orf.d2_rows(co, 0, co.shape[0])
    twins = np.flatnonzero((d == 0).sum(axis=1) > 1)
    assert twins.size >= 40
    sq, mq = info["model_saliency"][0], info["model_map"][0]
    for i in twins:
        same = np.flatnonzero(d[i] == 0)
        assert (sq[same].view(np.uint64) == sq[i].view(np.uint64)).all() and ((mq[same] >= 0) == (mq[i] >= 0)).all(), i
    st, mt = info["moving_saliency"][2], info["moving_map"][2]
    for i in best:                                               # coincident keypoints: bit-equal saliency, both kept
        same = np.flatnonzero((twin == blob[i]).all(axis=1))
        assert same.size == 2 and st[same[0]].view(np.uint64) == st[same[1]].view(np.uint64) and (mt[same] >= 0).all(), i
    # a line: w0 == 0 for every point, no keypoint
    line = np.zeros((40, 3), dtype=dtype)
    line[:, 0] = np.arange(40) * 0.25
    assert (kr.saliency(line, kr.rule(0.8, 0.5, 0.975, 0.975, 3)) == 0.0).all()
    with ctx.batch([(blob, blob), (blob, line)]) as bt:
        with pytest.raises(pkg.IcpError) as e:
            bt.keypoints(moving=pick(blob)[0], model=[pick(blob)[0], kr.rule(0.8, 0.5, 0.975, 0.975, 3)])
        assert e.value.code == pkg.capi.ICP_ERR_EMPTY and "pair 1" in str(e.value) and "model" in str(e.value)


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_carried_descriptors(ctx, pkg, dtype):
    (A, NA), (M, NM) = cloud(231, 257, dtype), cloud(232, 130, dtype)
    (B, NB), (Q, NQ) = cloud(233, 65, dtype), cloud(234, 300, dtype)
    pairs = [(A, M), (B, Q)]
    rules_m, rules_q = [pick(A)[0], None], [pick(M)[0], pick(Q)[0]]
    with ctx.batch(pairs) as bt:
        with bt.keypoints(moving=rules_m, model=rules_q)[0] as kb:   # a source without descriptors gives a batch without
            for ask in ((True, True), (True, False), (False, True)):
                om = np.empty((int(kb._moff[-1]), 33)) if ask[0] else None
                oq = np.empty((int(kb._qoff[-1]), 33)) if ask[1] else None
                pd = C.POINTER(C.c_double)
                rc = kb._lib.icp_batch_get_features(kb._h, om.ctypes.data_as(pd) if ask[0] else None, oq.ctypes.data_as(pd) if ask[1] else None)
                assert rc == pkg.capi.ICP_ERR_STATE, ask
            with pytest.raises(pkg.IcpError) as e:
                kb.match_features()
            assert e.value.code == pkg.capi.ICP_ERR_STATE
        fm, fq = bt.compute_features(8, ([NA, NB], [NM, NQ]), want=True)
        bt.match_features()                                      # the source's own matches are not carried over
        kb, info = bt.keypoints(moving=rules_m, model=rules_q, want_maps=True, want_saliency=True)
        with kb:
            check(pairs, rules_m, rules_q, kb, info, (fm, fq))
            with pytest.raises(pkg.IcpError) as e:
                kb.ransac(10, 0.1)
            assert e.value.code == pkg.capi.ICP_ERR_STATE        # the new batch holds no matches
            fwd, rev, kept = kb.match_features(mutual=True)
            for b in range(2):
                rows_m, rows_q = fm[b][info["moving_map"][b] >= 0], fq[b][info["model_map"][b] >= 0]
                wf, wr, wk = fr.match(rows_m, rows_q, True)
                assert bits_equal(fwd[b], wf) and bits_equal(rev[b], wr) and bits_equal(kept[b], wk), b
            assert kb.ransac(50, 0.2, seed=3)[0]["status"] in (0, pkg.capi.ICP_ERR_EMPTY)
            assert kb.fgr(0.2, iterations=4)[0]["status"] in (0, pkg.capi.ICP_ERR_EMPTY, pkg.capi.ICP_ERR_SINGULAR)


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_loop_under_way_does_not_notice(ctx, pkg, dtype):
    (A, NA), (M, NM) = cloud(51, 200, dtype), cloud(52, 150, dtype)
    A = np.ascontiguousarray((A.astype(np.float64) @ fr.rodrigues((0, 0, 1), 4.0).T + 0.02).astype(dtype))
    ra, rm = pick(A)[0], pick(M)[0]

    def run(disturb):
        with ctx.batch([(A, M)]) as bt:
            bt.begin(max_iter=12, tol=1e-9)
            bt.run(3)
            if disturb:
                bt.keypoints(moving=ra, model=rm)[0].close()
                bt.compute_features(9, ([NA], [NM]))
                bt.keypoints(moving=ra, model=rm, want_maps=True, want_saliency=True)[0].close()
            while bt.run(1 << 20)[1] > 0:
                pass
            return bt.state(0), bt.get_moving()[0], bt.loop_indices()[0], bt.diag_moments(0)

    a, b = run(False), run(True)
    assert a[0]["iterations"] == b[0]["iterations"] and a[0]["status"] == b[0]["status"]
    assert bits_equal(a[0]["T"], b[0]["T"]) and bits_equal(np.asarray(a[0]["err"]), np.asarray(b[0]["err"]))
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and bits_equal(np.asarray(a[3]), np.asarray(b[3]))


def test_refusals_leave_the_outputs_alone(ctx, pkg):
    INVALID, STATE, EMPTY = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE, pkg.capi.ICP_ERR_EMPTY
    Rule = pkg.capi.icp_keypoint_rule
    lib = pkg.load()
    pd, p32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    clouds = [cloud(241 + b, n, np.float32)[0] for b, n in enumerate((130, 65, 70, 130, 65, 70))]
    pairs = [(clouds[b], clouds[3 + b]) for b in range(3)]
    good = (1, 3, 0.6, 0.4, 0.975, 0.975)                        # kind, min_neighbours, salient_radius, non_max_radius, gamma_21, gamma_32

    def raw(bt, moving, model):
        """the C call with every output given: (rc, message); *out must come back NULL and no output element may be written"""
        arr = lambda rules: None if rules is None else (Rule * bt.count)(*[Rule(*r) for r in rules])
        n, m = int(bt._moff[-1]), int(bt._qoff[-1])
        mm, qm, cn = np.full(n, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32), np.full(2 * bt.count, -7, dtype=np.int32)
        ms, qs = np.full(n, -7.0), np.full(m, -7.0)
        out = C.c_void_p(0x1234)
        rc = lib.icp_batch_select_keypoints(bt._h, arr(moving), arr(model), mm.ctypes.data_as(p32), qm.ctypes.data_as(p32), ms.ctypes.data_as(pd),
                                            qs.ctypes.data_as(pd), cn.ctypes.data_as(p32), C.byref(out))
        msg = lib.icp_last_error().decode()
        assert out.value is None, msg
        assert (mm == -7).all() and (qm == -7).all() and (ms == -7.0).all() and (qs == -7.0).all() and (cn == -7).all(), msg
        return rc, msg

    ok = [good] * 3
    with ctx.batch(pairs) as bt:
        src = [np.concatenate(x) for x in zip(*bt.get_clouds())]
        bad_rules = [(7,) + good[1:], (-1,) + good[1:], (1, 0) + good[2:], (1, 65536) + good[2:]]
        for at in (2, 3, 4, 5):                                  # either radius, either gamma: 0, negative, NaN, infinite
            for v in (0.0, -1.0, np.nan, np.inf):
                bad_rules.append(good[:at] + (v,) + good[at + 1:])
        for bad in bad_rules:
            for side in (0, 1):
                rules = list(ok)
                rules[1] = bad
                rc, msg = raw(bt, rules if side == 0 else ok, rules if side == 1 else ok)
                assert rc == INVALID and "pair 1" in msg and ("model" if side else "moving") in msg, (bad, side, msg)
        # a cloud that would keep no point (known after the first wait): nobody has 60 neighbours within 1e-6
        rc, msg = raw(bt, ok, [(0, 0, 0.0, 0.0, 0.0, 0.0)] * 2 + [(1, 60, 1e-6, 1e-6, 0.975, 0.975)])
        assert rc == EMPTY and "pair 2" in msg and "model" in msg, msg
        assert lib.icp_batch_select_keypoints(bt._h, None, None, None, None, None, None, None, None) == INVALID   # out == NULL
        with pytest.raises(ValueError):
            bt.keypoints(moving=[good[2:4], good[2:4]])          # one rule per pair
        with pytest.raises(ValueError):
            bt.keypoints(moving={"salient_radius": 0.5})
        with pytest.raises(ValueError):
            bt.keypoints(moving=(0.5,))
        # accepted: tuples of two to five values, dicts, None; the source holds what it held
        with bt.keypoints(moving=[(0.6, 0.4), {"salient_radius": 0.6, "non_max_radius": 0.4, "min_neighbours": 3}, None], model=(0.6, 0.4, 0.975, 0.975, 3))[0] as nb:
            assert nb.count == 3
        assert all(bits_equal(np.concatenate(x), s) for x, s in zip(zip(*bt.get_clouds()), src))
    # a context with a pending pass
    A, M = pairs[0]
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with c.batch(pairs[:2]) as bt:
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            with pytest.raises(pkg.IcpError) as e:
                bt.keypoints(moving=good[2:] + (3,))
            assert e.value.code == STATE
            rc, msg = raw(bt, ok[:2], ok[:2])
            assert rc == STATE
            c.loop_complete()
            with bt.keypoints(moving=(0.6, 0.4, 0.975, 0.975, 3))[0] as nb:
                assert nb.count == 2


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_dense_bunny_end_to_end(ctx, pkg, golden):
    """The dense bunny pair of batch_keypoint_ref.dense_bunny_pair: every 6th point, 5 992 and 5 991 points, disjoint samples, the
    moving cloud turned 149 degrees.  K = 24, rule (0.007, 0.00525, 0.975, 0.975, 5), mutual matches among the keypoints, 2 000
    hypotheses, 7.5 mm, edge check 0.9, seed 1, gate 1 cm.
    Conditions: the keypoint counts and the mutual-match count are the restatement's, exactly; the pose ransac returns is within 5
    degrees and 1.5 cm of the truth; a point-to-point batch on the full pair gated at 1 cm and started from it ends within 2 degrees;
    register_batch_global(..., keypoints=rule) returns the same bytes as the step-by-step sequence.
    The numpy restatement alone (tests/test_batch_keypoint_ref.py prints it): 427 and 422 keypoints, 179 mutual matches, 70 of them
    within 1 cm of the truth; seed 1: 65 inliers, 0.898 degrees and 2.68 mm -- more than a factor of two inside both bounds, so
    seed 1 stays."""
    A, M, Tt = kr.dense_bunny_pair(golden)
    K, H, MD, GATE, SEED, RULE = 24, 2000, 0.0075, 0.01, 1, kr.DENSE_RULE
    (YA, mapA, salA), (YM, mapM, salM) = kr.dense_bunny_keypoints(golden)
    with ctx.batch([(A, M)]) as bt:
        cm, cq = bt.estimate_covariances(K, None, regularisation="none", want=True)
        NA = pkg.oriented_normals(A, cm[0], A.astype(np.float64).mean(0))
        NM = pkg.oriented_normals(M, cq[0], M.astype(np.float64).mean(0))
        fm, fq = bt.compute_features(K, ([NA], [NM]), want=True)
        kb, info = bt.keypoints(moving=RULE, model=RULE, want_maps=True, want_saliency=True)
        with kb:
            fwd, rev, kept = kb.match_features(mutual=True)
            start = kb.ransac(H, MD, edge_similarity=0.9, seed=SEED)[0]
    n_kept, m_kept = int(info["counts"][0]), int(info["counts"][1])
    wf, wr, wk = fr.match(fm[0][mapA >= 0], fq[0][mapM >= 0], True)
    rot, trans = fr.angle_deg(start["T"][:3, :3] @ Tt[:3, :3].T), float(np.linalg.norm(start["T"][:3, 3] - Tt[:3, 3]))
    print(f"keypoints {n_kept} / {m_kept} (restated {YA.shape[0]} / {YM.shape[0]}), mutual matches {int(kept[0].sum())} (restated {int(wk.sum())}), "
          f"inliers {start['inliers']}, rot {rot:.3f} deg, trans {trans * 1e3:.2f} mm")
    assert (n_kept, m_kept) == (YA.shape[0], YM.shape[0]) == (427, 422)
    assert bits_equal(info["moving_map"][0], mapA) and bits_equal(info["model_map"][0], mapM)
    assert bits_equal(info["moving_saliency"][0], salA) and bits_equal(info["model_saliency"][0], salM)
    assert int(kept[0].sum()) == int(wk.sum()) and bits_equal(fwd[0], wf) and bits_equal(kept[0], wk)
    assert start["status"] == 0 and start["correspondences"] == int(wk.sum())
    assert rot < 5.0 and trans < 0.015
    fine_ = ctx.register_batch([(A, M)], max_distance=GATE, init=start["T"][None])[0]
    end = fr.angle_deg(fine_.T[:3, :3] @ Tt[:3, :3].T)
    print(f"refined {end:.3f} deg, {np.linalg.norm(fine_.T[:3, 3] - Tt[:3, 3]) * 1e3:.2f} mm")
    assert end < 2.0
    # the one-call entry runs the same sequence
    res = ctx.register_batch_global([(A, M)], 0.0, K, H, MD, seed=SEED, gate=GATE, keypoints=RULE)[0]
    assert bits_equal(res.extra["global"]["T"], start["T"]) and bits_equal(res.T, fine_.T)
    assert res.extra["global"]["keypoints"] == (n_kept, m_kept) and res.extra["global"]["inliers"] == start["inliers"]
