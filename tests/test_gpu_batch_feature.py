"""GPU: batched global registration (icp_batch_compute_features, icp_batch_match_features, icp_batch_score_transforms,
icp_batch_ransac; Batch.*, Context.register_batch_global) against the numpy restatement tests/batch_feature_ref.py.

    1  descriptors bit for bit: clouds of k + 1, 5, 63, 64, 65, 130, 257 and 520 points (a single lane, ragged and full work
       items, the sub-tile borders of 256 and 512 points), k in {3, 8, 9, 32} (the three list capacities), a cloud with coincident
       points (r2 == 0 skips, d2 == 0 weights skipped), a collinear cloud whose normals lie along the line (vv == 0: all-zero
       descriptors), a lattice (ties on tau), a cloud far from the origin, both dtypes; a pair alone and at either end of a batch
    2  matching: fwd, rev and kept for n, m in {1, 63, 65, 130}, with identical descriptors on several points
    3  scoring: points exactly on the threshold, an overflowing candidate, per_pair in {1, 65}
    4  RANSAC through icp_diag_batch_ransac: triples, validity, T against numpy's determinant-fixed Kabsch (1e-9), counts against
       numpy's scoring of the library's own matrices, the winner's order, the same seed the same bytes, neighbours, C_p < 3
    5  end to end on the bunny pair, see test_bunny_end_to_end
    6  refusals; a loop under way does not notice any of the calls"""
import numpy as np
import pytest

import batch_feature_ref as fr
import batch_outlier_ref as orf
from batch_ref import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = (5, 63, 64, 65, 130, 257, 520)
K_MODEL = {3: 8, 8: 3, 9: 32, 32: 9}   # the models' k: another list capacity in the same launch
_REF = {}


def ref_fpfh(X, N, k):
    """batch_feature_ref.fpfh, computed once per (cloud, normals, k)"""
    key = (X.dtype.str, X.tobytes(), N.tobytes(), k)
    if key not in _REF:
        _REF[key] = fr.fpfh(X, N, k)
    return _REF[key]


def fine(X, seed):
    """fp64 clouds get mantissas fp32 cannot hold"""
    if X.dtype == np.float64:
        X = X + 1e-9 * np.random.default_rng(seed).standard_normal(X.shape)
    return np.ascontiguousarray(X)


def unit(seed, n):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True))


def cloud(seed, n, dtype):
    X, N = fr.blob(seed, n, dtype)
    return fine(X, seed + 1), N


def special_models(dtype):
    """(cloud, normals): a lattice (ties at every rank), 300 points of which 40 coincide, a line of 40 points with its normals
    along it, a cloud 1e4 from the origin"""
    line = np.zeros((40, 3), dtype=dtype)
    line[:, 0] = np.arange(40) * 0.25
    far = orf.far(dtype)[:200].copy()
    return [(orf.lattice(dtype, side=6, step=0.5), unit(1, 216)), (orf.coincident(dtype), unit(2, 300)),
            (line, np.tile(np.array([1.0, 0.0, 0.0]), (40, 1))), (far, unit(3, 200))]


def differing(got, want):
    return np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(K_MODEL))
@DTYPES
def test_descriptors_bit_for_bit(ctx, pkg, dtype, k):
    kq = K_MODEL[k]
    movers = [cloud(100 + n, max(n, k + 1), dtype) for n in (k + 1,) + SIZES]
    models = special_models(dtype)
    models = [models[i % len(models)] for i in range(len(movers))]
    with ctx.batch([(A, M) for (A, _), (M, _) in zip(movers, models)]) as bt:
        fm, fq = bt.compute_features(k, ([N for _, N in movers], [N for _, N in models]), k_model=kq, want=True)
        gm, gq = bt.get_features()
        for b, ((A, NA), (M, NM)) in enumerate(zip(movers, models)):
            for got, want, what in ((fm[b], ref_fpfh(A, NA, k), "moving"), (fq[b], ref_fpfh(M, NM, kq), "model")):
                assert got.dtype == np.float64 and got.shape == want.shape
                bad = differing(got, want)
                assert bad.size == 0, f"pair {b} {what} k {k}/{kq}: {bad.size} points differ, first {bad[0]}: {got[bad[0]]!r} / {want[bad[0]]!r}"
            assert bits_equal(gm[b], fm[b]) and bits_equal(gq[b], fq[b])
        assert (fq[2] == 0.0).all()                              # the line: every pair term is skipped
        assert (fq[1][100:140] == 0.0).all() and np.abs(fq[1][:100]).max() > 0   # 40 coincident points: their k nearest are each other, every term skipped
        assert np.abs(fm[3].reshape(-1, 3, 11).sum(axis=2) - 100.0).max() < 1e-9


@DTYPES
def test_descriptors_capacity_16_over_sub_tiles(ctx, pkg, dtype):
    """the list capacity the cases above leave out, at both of its edges (k = 16 and k = 9), on the shapes at which the scan takes
    another path: 2100 points -- more than one LDS sub-tile per wave in either precision, a last chunk that is padded, work items
    that straddle the quarters -- and k + 1 points, three quarters nearly or wholly empty"""
    movers = [cloud(41, 2100, dtype), cloud(43, 10, dtype)]
    models = [cloud(45, 17, dtype), cloud(47, 2100, dtype)]
    ks, kq = [16, 9], [16, 9]
    with ctx.batch([(A, M) for (A, _), (M, _) in zip(movers, models)]) as bt:
        fm, fq = bt.compute_features(ks, ([N for _, N in movers], [N for _, N in models]), k_model=kq, want=True)
        for b, ((A, NA), (M, NM)) in enumerate(zip(movers, models)):
            for got, want, what in ((fm[b], ref_fpfh(A, NA, ks[b]), "moving"), (fq[b], ref_fpfh(M, NM, kq[b]), "model")):
                assert got.dtype == np.float64 and got.shape == want.shape
                bad = differing(got, want)
                assert bad.size == 0, f"pair {b} {what} k {ks[b]}/{kq[b]}: {bad.size} points differ, first {bad[0]}: {got[bad[0]]!r} / {want[bad[0]]!r}"


@DTYPES
def test_a_pairs_descriptors_do_not_depend_on_the_batch(ctx, pkg, dtype):
    (XA, XN), (XM, XMN) = cloud(7, 300, dtype), (orf.lattice(dtype, side=5, step=0.25), unit(5, 125))
    (YA, YN), (YM, YMN) = cloud(9, 130, dtype), cloud(11, 65, dtype)
    (ZA, ZN), (ZM, ZMN) = cloud(13, 70, dtype), cloud(15, 520, dtype)
    with ctx.batch([(XA, XM)]) as bt:
        alone = bt.compute_features(5, ([XN], [XMN]), k_model=7, want=True)   # a launch of capacity 8
    with ctx.batch([(XA, XM), (YA, YM), (ZA, ZM)]) as bt:
        first = bt.compute_features([5, 20, 32], ([XN, YN, ZN], [XMN, YMN, ZMN]), k_model=[7, 12, 9], want=True)   # capacity 32
    with ctx.batch([(ZA, ZM), (YA, YM), (XA, XM)]) as bt:
        last = bt.compute_features([32, 20, 5], ([ZN, YN, XN], [ZMN, YMN, XMN]), k_model=[9, 12, 7], want=True)
    for side in range(2):
        assert bits_equal(alone[side][0], first[side][0]) and bits_equal(alone[side][0], last[side][2])
        assert bits_equal(first[side][2], last[side][0]) and bits_equal(first[side][1], last[side][1])


# 2 ------------------------------------------------------------------------------------------------------------------------
def planted_descriptors(seed, n, m):
    """(n, 33) and (m, 33) with identical descriptors on several points of either side and exact ties between the sides"""
    rng = np.random.default_rng(seed)
    G = np.round(rng.uniform(0.0, 100.0, (m, 33)), 1)
    F = G[rng.integers(0, m, n)] + np.where(rng.random((n, 1)) < 0.5, 0.0, np.round(rng.uniform(-1, 1, (n, 33)), 1))
    if m >= 8:
        G[5] = G[2]
        G[m - 1] = G[2]
    if n >= 8:
        F[6] = F[1]
        F[n - 2] = F[1]
    return np.ascontiguousarray(F), np.ascontiguousarray(G)


@pytest.mark.parametrize("mutual", [True, False])
@DTYPES
def test_matching_equals_numpy(ctx, pkg, dtype, mutual):
    sizes = [(n, m) for n in (1, 63, 65, 130) for m in (1, 63, 65, 130)]
    rng = np.random.default_rng(3)
    pairs = [(rng.standard_normal((n, 3)).astype(dtype), rng.standard_normal((m, 3)).astype(dtype)) for n, m in sizes]
    desc = [planted_descriptors(10 + b, n, m) for b, (n, m) in enumerate(sizes)]
    with ctx.batch(pairs) as bt:
        bt.diag_set_features([F for F, _ in desc], [G for _, G in desc])
        fwd, rev, kept = bt.match_features(mutual=mutual)
        ties = 0
        for b, (F, G) in enumerate(desc):
            wf, wr, wk = fr.match(F, G, mutual)
            assert bits_equal(fwd[b], wf) and bits_equal(rev[b], wr) and bits_equal(kept[b], wk), (b, sizes[b])
            ties += int((wf == 2).sum()) if G.shape[0] >= 8 else 0
        assert ties > 0   # a query whose nearest descriptor sits on points 2, 5 and m - 1 answered 2


# 3 ------------------------------------------------------------------------------------------------------------------------
def listed_pair(seed, n, dtype):
    """(P, Q, F, G, ci, cj): a lattice cloud, its copy with every point pushed 0, 0.25, 0.5 or 0.75 along x, in another order, and
    descriptors that match point i to its copy"""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(rng.integers(-8, 9, (n, 3)).astype(dtype))
    perm = rng.permutation(n)
    Q = np.empty_like(P)
    push = np.zeros((n, 3), dtype=dtype)
    push[:, 0] = (np.arange(n) % 4) * 0.25
    Q[perm] = P + push
    G = np.round(rng.uniform(0, 100, (n, 33)), 2)
    F = np.empty_like(G)
    F[:] = G[perm]
    return P, Q, F, G, np.arange(n, dtype=np.int32), perm.astype(np.int32)


@DTYPES
def test_scoring_equals_numpy(ctx, pkg, dtype):
    n = 130
    P, Q, F, G, ci, cj = listed_pair(4, n, dtype)
    P2, Q2, F2, G2, ci2, cj2 = listed_pair(5, 65, dtype)
    huge = np.eye(4)
    huge[0, 0] = 3e38 if dtype == np.float32 else 1.5e308        # finite in the batch's precision; times a coordinate it is not
    rng = np.random.default_rng(6)
    many = np.tile(np.eye(4), (65, 1, 1))
    for c in range(1, 65):
        many[c, :3, :3] = fr.rodrigues(rng.standard_normal(3), rng.uniform(0, 3))
        many[c, :3, 3] = np.round(rng.uniform(-0.5, 0.5, 3), 2)
    many[64] = huge
    with ctx.batch([(P, Q), (P2, Q2)]) as bt:
        bt.diag_set_features([F, F2], [G, G2])
        fwd, _, kept = bt.match_features(mutual=True)
        assert np.array_equal(fwd[0], cj) and kept[0].all() and np.array_equal(fwd[1], cj2) and kept[1].all()
        # per_pair = 1, the identity: a push of exactly 0.5 lies on the threshold and counts
        got = bt.score_transforms(np.stack([np.eye(4), np.eye(4)]), 0.5)
        assert got.shape == (2, 1) and got[0, 0] == int((np.arange(n) % 4 <= 2).sum()) and got[1, 0] == int((np.arange(65) % 4 <= 2).sum())
        assert got[0, 0] == fr.score(P, Q, ci, cj, np.eye(4), 0.5)
        got = bt.score_transforms(np.stack([np.eye(4), np.eye(4)]), [0.25, np.inf])
        assert got[0, 0] == int((np.arange(n) % 4 <= 1).sum()) and got[1, 0] == 65
        # per_pair = 65, the overflowing candidate last
        got = bt.score_transforms(np.stack([many, many[::-1]]), [0.6, 0.3])
        for c in range(65):
            assert got[0, c] == fr.score(P, Q, ci, cj, many[c], 0.6), c
            assert got[1, c] == fr.score(P2, Q2, ci2, cj2, many[64 - c], 0.3), c
        assert got[0, 64] == fr.score(P, Q, ci, cj, huge, 0.6) and got[0, 0] > 0
        inf_counts = bt.score_transforms(np.stack([huge, huge]), None)
        assert inf_counts[0, 0] == fr.score(P, Q, ci, cj, huge, np.inf) and inf_counts[0, 0] < n   # a moved point that is not finite is a miss


# 4 ------------------------------------------------------------------------------------------------------------------------
def ransac_pair(seed, n, dtype, wrong=3):
    """a cloud, its rigidly moved copy, and descriptors whose forward matches are right except for every `wrong`-th point"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, 3)).astype(dtype)
    R, t = fr.rodrigues(rng.standard_normal(3), 140.0), rng.uniform(-1, 1, 3)
    Q = (P.astype(np.float64) @ R.T + t).astype(dtype)
    target = np.arange(n)
    target[::wrong] = rng.integers(0, n, target[::wrong].size)
    G = np.round(rng.uniform(0, 100, (n, 33)), 2)
    F = np.ascontiguousarray(G[target])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return P, Q, F, G, T


def check_ransac(bt, b, P, Q, F, G, seed, H, md, e, res):
    fwd, _, kept = fr.match(F, G, False)
    ci, cj = fr.correspondences(fwd, kept)
    dg = bt.diag_ransac(b)
    tr, valid = fr.hypotheses(P, Q, ci, cj, seed, H, e)
    assert np.array_equal(dg["triples"], tr)
    assert np.array_equal(dg["valid"], valid), np.flatnonzero(dg["valid"] != valid)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    for h in np.flatnonzero(valid):
        assert np.abs(dg["T"][h] - fr.kabsch(P64[ci[tr[h]]], Q64[cj[tr[h]]])).max() < 1e-9, h
        assert dg["counts"][h] == fr.score(P, Q, ci, cj, dg["T"][h], md), h
    assert (dg["counts"][valid == 0] == -1).all()
    assert res["correspondences"] == len(ci) and res["status"] == 0
    best = int(np.argmax(np.where(valid > 0, dg["counts"], -1)))   # the largest count, the lowest h among equals
    assert res["inliers"] >= dg["counts"][best]
    assert res["inliers"] == fr.score(P, Q, ci, cj, res["T"], md)
    if res["inliers"] == dg["counts"][best] and bits_equal(res["T"], dg["T"][best]):
        return "winner"
    hit = fr.hits(P, Q, ci, cj, dg["T"][best], md)
    assert np.abs(res["T"] - fr.kabsch(P64[ci[hit]], Q64[cj[hit]])).max() < 1e-9   # the refit over the winner's inliers
    return "refit"


@DTYPES
def test_ransac_equals_numpy(ctx, pkg, dtype):
    H, md, e = 96, 0.02, 0.9
    X = ransac_pair(31, 130, dtype)
    Y = ransac_pair(32, 65, dtype, wrong=2)
    tiny = (X[0][:2].copy(), X[1][:2].copy(), X[2][:2].copy(), X[3][:2].copy())
    with ctx.batch([(X[0], X[1]), (Y[0], Y[1]), (tiny[0], tiny[1])]) as bt:
        bt.diag_set_features([X[2], Y[2], tiny[2]], [X[3], Y[3], tiny[3]])
        bt.match_features(mutual=False)
        res = bt.ransac(H, md, edge_similarity=e, seed=[5, 6, 7])
        kinds = {check_ransac(bt, 0, *X[:4], 5, H, md, e, res[0]), check_ransac(bt, 1, *Y[:4], 6, H, md, e, res[1])}
        assert fr.angle_deg(res[0]["T"][:3, :3] @ X[4][:3, :3].T) < 0.1 and np.abs(res[0]["T"][:3, 3] - X[4][:3, 3]).max() < 1e-3
        assert abs(np.linalg.det(res[0]["T"][:3, :3]) - 1.0) < 1e-12
        # C_p < 3: empty, the identity
        assert res[2]["status"] == pkg.capi.ICP_ERR_EMPTY and res[2]["inliers"] == 0 and res[2]["correspondences"] == 2
        assert bits_equal(res[2]["T"], np.eye(4)) and not bt.diag_ransac(2)["valid"].any()
        # the same seed, the same bytes; the edge check off admits more hypotheses
        dg = bt.diag_ransac(0)
        again = bt.ransac(H, md, edge_similarity=e, seed=[5, 6, 7])
        dg2 = bt.diag_ransac(0)
        assert all(bits_equal(again[b]["T"], res[b]["T"]) and again[b]["inliers"] == res[b]["inliers"] for b in range(3))
        assert all(bits_equal(dg[f], dg2[f]) for f in dg)
        bt.ransac(H, md, edge_similarity=0.0, seed=[5, 6, 7])
        assert bt.diag_ransac(0)["valid"].sum() > dg["valid"].sum() and bt.diag_ransac(0)["valid"].all()
    # a pair's result is unchanged by its neighbours and by its position
    with ctx.batch([(Y[0], Y[1]), (X[0], X[1])]) as bt:
        bt.diag_set_features([Y[2], X[2]], [Y[3], X[3]])
        bt.match_features(mutual=False)
        swapped = bt.ransac(H, md, edge_similarity=e, seed=[6, 5])
        assert bits_equal(swapped[1]["T"], res[0]["T"]) and bits_equal(swapped[0]["T"], res[1]["T"])
        assert swapped[1]["inliers"] == res[0]["inliers"] and all(bits_equal(bt.diag_ransac(1)[f], dg[f]) for f in dg)
    assert kinds <= {"winner", "refit"}


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_bunny_end_to_end(ctx, pkg, golden, dtype):
    """The bunny pair of batch_feature_ref.bunny_pair: 1 498 points each, disjoint samples, the moving cloud turned 149 degrees.
    Conditions: the pose ransac returns is within 10 degrees and 1 cm of the truth; a point-to-point batch gated at 1 cm and
    started from it ends within 2 degrees; the same batch started from the identity ends more than 30 degrees away.
    The numpy restatement alone (k = 24, normals facing each cloud's centroid, mutual matches, 2 000 hypotheses of the stated
    generator, 7.5 mm, edge check 0.9; batch_ref.reference_loop gated at 1 cm, 40 iterations, tol 1e-6), both dtypes alike:
    391 mutual correspondences, 117 of them within 1 cm of the truth; seed 1: 136 valid hypotheses, 94 inliers, 2.25 degrees and
    3.9 mm, refined to 1.20 degrees and 2.2 mm; seeds 2, 3, 4: 1.00, 1.21, 1.87 degrees and 2.5, 3.0, 4.0 mm; from the identity
    the loop ends 150.8 degrees away."""
    A, M, Tt = fr.bunny_pair(golden)
    A, M = A.astype(dtype), M.astype(dtype)
    K, H, MD, GATE, SEED = 24, 2000, 0.0075, 0.01, 1
    with ctx.batch([(A, M)]) as bt:
        cm, cq = bt.estimate_covariances(K, None, regularisation="none", want=True)
        NA = pkg.oriented_normals(A, cm[0], A.astype(np.float64).mean(0))
        NM = pkg.oriented_normals(M, cq[0], M.astype(np.float64).mean(0))
        bt.compute_features(K, ([NA], [NM]))
        fwd, rev, kept = bt.match_features(mutual=True)
        start = bt.ransac(H, MD, edge_similarity=0.9, seed=SEED)[0]
    assert start["status"] == 0 and start["correspondences"] == int(kept[0].sum())
    print(f"correspondences {start['correspondences']} inliers {start['inliers']} "
          f"rot {fr.angle_deg(start['T'][:3, :3] @ Tt[:3, :3].T):.3f} deg trans {np.linalg.norm(start['T'][:3, 3] - Tt[:3, 3]) * 1e3:.2f} mm")
    assert fr.angle_deg(start["T"][:3, :3] @ Tt[:3, :3].T) < 10.0
    assert np.linalg.norm(start["T"][:3, 3] - Tt[:3, 3]) < 0.01
    fine_ = ctx.register_batch([(A, M)], max_distance=GATE, init=start["T"][None])[0]
    cold = ctx.register_batch([(A, M)], max_distance=GATE)[0]
    print(f"refined {fr.angle_deg(fine_.T[:3, :3] @ Tt[:3, :3].T):.3f} deg, from the identity {fr.angle_deg(cold.T[:3, :3] @ Tt[:3, :3].T):.3f} deg")
    assert fr.angle_deg(fine_.T[:3, :3] @ Tt[:3, :3].T) < 2.0
    assert fr.angle_deg(cold.T[:3, :3] @ Tt[:3, :3].T) > 30.0
    # the one-call entry runs the same sequence
    res = ctx.register_batch_global([(A, M)], 0.0, K, H, MD, seed=SEED, gate=GATE)[0]
    assert bits_equal(res.extra["global"]["T"], start["T"]) and bits_equal(res.T, fine_.T)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, pkg):
    E, S = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    (A, NA), (M, NM) = cloud(41, 70, np.float32), cloud(42, 20, np.float32)

    def code(fn):
        with pytest.raises(pkg.IcpError) as err:
            fn()
        return err.value.code, str(err.value)

    with ctx.batch([(A, M)]) as bt:
        assert code(bt.get_features)[0] == S
        assert code(lambda: bt.match_features())[0] == S
        assert code(lambda: bt.score_transforms(np.eye(4)[None], 0.1))[0] == S
        assert code(lambda: bt.ransac(10, 0.1))[0] == S
        for k, kq in ((2, 5), (33, 5), (5, 2), (5, 33)):
            assert code(lambda: bt.compute_features(k, ([NA], [NM]), k_model=kq))[0] == E
        c, msg = code(lambda: bt.compute_features(8, ([NA], [NM]), k_model=20))
        assert c == E and "pair 0" in msg and "model" in msg          # 20 points: fewer than k + 1
        bad = NM.copy()
        bad[3, 1] = np.nan
        c, msg = code(lambda: bt.compute_features(8, ([NA], [bad]), k_model=8))
        assert c == E and "pair 0" in msg and "model" in msg
        bad = NA.copy()
        bad[0, 0] = np.inf
        assert code(lambda: bt.compute_features(8, ([bad], [NM]), k_model=8))[0] == E
        assert code(bt.get_features)[0] == S                          # a refused call leaves the batch as it was
        bt.compute_features(8, ([NA], [NM]), k_model=8)
        assert code(lambda: bt.score_transforms(np.eye(4)[None], 0.1))[0] == S
        bt.match_features()
        T = np.eye(4)[None].copy()
        for at, v in (((0, 3, 3), 2.0), ((0, 3, 0), 1e-3), ((0, 0, 0), np.nan), ((0, 1, 3), 1e39)):
            Tb = T.copy()
            Tb[at] = v
            assert code(lambda: bt.score_transforms(Tb, 0.1))[0] == E, at
        for md in (0.0, -1.0, np.nan):
            assert code(lambda: bt.score_transforms(T, md))[0] == E
        for args in ((0, 0.1, 0.9), (65537, 0.1, 0.9), (10, 0.0, 0.9), (10, np.inf, 0.9), (10, np.nan, 0.9), (10, 0.1, 1.0), (10, 0.1, -0.1), (10, 0.1, np.nan)):
            assert code(lambda: bt.ransac(*args))[0] == E, args
        assert bt.ransac(10, 0.1)[0]["status"] in (0, pkg.capi.ICP_ERR_EMPTY)
        bt.compute_features(8, ([NA], [NM]), k_model=8)               # new descriptors discard the matches
        assert code(lambda: bt.ransac(10, 0.1))[0] == S


@DTYPES
def test_a_loop_under_way_does_not_notice(ctx, pkg, dtype):
    (A, NA), (M, NM) = cloud(51, 200, dtype), cloud(52, 150, dtype)
    A = np.ascontiguousarray((A.astype(np.float64) @ fr.rodrigues((0, 0, 1), 4.0).T + 0.02).astype(dtype))

    def run(disturb):
        with ctx.batch([(A, M)]) as bt:
            bt.begin(max_iter=12, tol=1e-9)
            bt.run(3)
            if disturb:
                bt.compute_features(9, ([NA], [NM]))
                bt.get_features()
                bt.match_features()
                bt.score_transforms(np.eye(4)[None], 0.1)
                bt.ransac(40, 0.1, seed=3)
            while bt.run(1 << 20)[1] > 0:
                pass
            return bt.state(0), bt.get_moving()[0], bt.loop_indices()[0], bt.diag_moments(0)

    a, b = run(False), run(True)
    assert a[0]["iterations"] == b[0]["iterations"] and a[0]["status"] == b[0]["status"]
    assert bits_equal(a[0]["T"], b[0]["T"]) and bits_equal(np.asarray(a[0]["err"]), np.asarray(b[0]["err"]))
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and bits_equal(np.asarray(a[3]), np.asarray(b[3]))
