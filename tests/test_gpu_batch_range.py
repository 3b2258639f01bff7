"""GPU: the batched neighbourhood calls across the floating-point range (icp_batch_estimate_covariances,
icp_batch_estimate_point_normals, icp_batch_select_keypoints, icp_batch_remove_outliers, icp_batch_downsample,
icp_batch_compute_features_stored) against two references that know nothing of their rules: a cloud times 2^e must give the scale-1
answer exactly scaled, and a normal must be LAPACK's (tests/batch_range_ref.py).  The numpy restatements, which
tests/test_batch_range_ref.py holds to the same two references on the CPU, are compared byte for byte as everywhere else.

One batch holds every exponent of the dtype (batch_range_ref.E64, E32) as pairs of their own behind a scale-1 witness, two pairs per
exponent -- blobs of 200 and 65 points, and of 130 and 65 -- so every call is one launch sequence.

    1  covariances, k = 8 (the list's capacity 8) and k = 9 (16): raw and Frobenius bytes are the numpy rule's; raw is the witness's
       times 2^(2e) exactly, Frobenius the witness's bytes
    2  point normals in the three modes are the numpy rule's bytes; unoriented, every scaled pair's are the witness's bytes, and they
       lie within 1e-9 rad of LAPACK's under the gap mask
    3  given covariances times 2^m for every m of MAGS: the m = 0 normals' bytes, within 1e-9 rad of LAPACK's; rank-1, rank-2 and zero
       matrices at 2^+-1000
    4  keypoints under the radii times 2^e: saliency the witness's times 2^(2e) exactly; maps, counts and clouds the numpy rule's and
       the witness's
    5  outliers (statistical 8 : 1.0, radius 0.3 * 2^e : 3) and voxels (0.25 * 2^e): the numpy rule's bytes; maps the witness's,
       points and statistical scores exactly scaled (a radius score is a count: the witness's)
    6  FPFH from the stored normals: the numpy rule's and the witness's bytes
    7  a scaled pair alone and beside the others in reversed order: the same bytes"""
import numpy as np
import pytest

import batch_feature_ref as fr
import batch_gicp_ref as gr
import batch_normals_ref as nr
import batch_range_ref as rr
from batch_ref import bits_equal
from test_gpu_batch_keypoint import check as check_keypoints
from test_gpu_batch_normals import MODES, check as check_normals
from test_gpu_batch_outlier import check_batch as check_outliers
from test_gpu_batch_voxel import check_batch as check_voxels

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
BLOBS = (((311, 200), (312, 65)), ((313, 130), (314, 65)))   # per exponent two pairs of (seed, points): moving, model
PER = len(BLOBS)
_BATCH = {}


def batch_of(dtype):
    """(exps, pairs): exps[b] the exponent of pair b -- the witness's 0 first --, pairs[b] = (moving, model) times 2^exps[b].
    Made once per dtype and left unchanged"""
    key = np.dtype(dtype).str
    if key not in _BATCH:
        exps, pairs = [], []
        for e in (0,) + rr.exponents(dtype):
            for (sa, na), (sm, nm) in BLOBS:
                exps.append(e)
                pairs.append((rr.scaled(rr.blob(sa, na, dtype), e), rr.scaled(rr.blob(sm, nm, dtype), e)))
        _BATCH[key] = (exps, pairs)
    return _BATCH[key]


def up(a, p):
    """a times 2^p in a's dtype"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(a, p).astype(a.dtype)


def each(exps, sides):
    """(b, side, e, array of pair b, array of its witness) over a call's per-side, per-pair lists"""
    for side in range(2):
        for b, e in enumerate(exps):
            yield b, side, e, sides[side][b], sides[side][b % PER]


# 1 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("k", [8, 9])
def test_covariances(ctx, dtype, k):
    exps, pairs = batch_of(dtype)
    with ctx.batch(pairs) as bt:
        raw = bt.estimate_covariances(k, None, regularisation="none", want=True)
        fro = bt.estimate_covariances(k, None, regularisation="frobenius", lam=rr.LAM, want=True)
    for b, side, e, C, W in each(exps, raw):
        want, _ = gr.covariances(pairs[b][side], k, gr.COV_NONE)
        assert bits_equal(C, want), f"raw: pair {b} side {side} e {e}: {int((C != want).any(axis=1).sum())} points differ from the numpy rule"
        assert np.isfinite(C).all() and bits_equal(C, up(W, 2 * e)), f"raw: pair {b} side {side} e {e}: not the witness's times 2^{2 * e}"
    for b, side, e, C, W in each(exps, fro):
        want, _ = gr.covariances(pairs[b][side], k, gr.COV_FROBENIUS, rr.LAM)
        assert bits_equal(C, want), f"frobenius: pair {b} side {side} e {e}: {int((C != want).any(axis=1).sum())} points differ from the numpy rule"
        assert bits_equal(C, W), f"frobenius: pair {b} side {side} e {e}: {int((C != W).any(axis=1).sum())} points differ from the witness"


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_point_normals(ctx, dtype):
    exps, pairs = batch_of(dtype)
    vw = (np.stack([rr.viewpoint(e) for e in exps]), np.stack([-rr.viewpoint(e) for e in exps]))
    with ctx.batch(pairs) as bt:
        covs = bt.estimate_covariances(rr.K, None, regularisation="none", want=True)
        for name, mode in MODES:
            got = bt.estimate_point_normals(name, viewpoints=vw if mode == nr.VIEWPOINT else None, want=True)
            check_normals(pairs, covs, got, mode, vw, name)
            for b, side, e, N, W in each(exps, got):
                assert bits_equal(N, W), f"{name}: pair {b} side {side} e {e}: {int((N != W).any(axis=1).sum())} normals differ from the witness"
            if mode == nr.NONE:
                for b, side, e, N, _ in each(exps, got):
                    rr.check_lapack(N, covs[side][b], f"pair {b} side {side} e {e}")


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_given_covariances(ctx, dtype):
    (sa, na), (sm, nm) = BLOBS[0]
    A, M = rr.blob(sa, na, dtype), rr.blob(sm, nm, dtype)
    small = rr.blob(315, 12, dtype)
    r1, _, r2 = rr.deficient()
    low, high = (np.concatenate([np.ldexp(r1, m), np.ldexp(r2, m), np.zeros((4, 6))]) for m in (-1000, 1000))
    pairs = [(A, M)] * len(rr.MAGS) + [(small, small)]
    with ctx.batch(pairs) as bt:
        own = bt.estimate_covariances(rr.K, None, regularisation="none", want=True)
        CA, CM = rr.exact6(own[0][0]), rr.exact6(own[1][0])       # the witness's covariances, exact at every power of two
        given = ([np.ldexp(CA, m) for m in rr.MAGS] + [low], [np.ldexp(CM, m) for m in rr.MAGS] + [high])
        for side in range(2):
            for m, S in zip(rr.MAGS, given[side]):
                assert np.ldexp(S, -m).tobytes() == (CA, CM)[side].tobytes(), m
        bt.set_covariances(*given)
        got = bt.estimate_point_normals("none", want=True)
    check_normals(pairs, given, got, nr.NONE, None, "given")
    mid = rr.MAGS.index(0)
    for side in range(2):
        for b, m in enumerate(rr.MAGS):
            N = got[side][b]
            assert bits_equal(N, got[side][mid]), f"side {side} 2^{m}: {int((N != got[side][mid]).any(axis=1).sum())} normals differ from those at 2^0"
            rr.check_lapack(N, given[side][b], f"side {side} 2^{m}")
        D = got[side][len(rr.MAGS)]
        rr.check_deficient(D[:4], D[4:8], D[8:], f"side {side}")


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_keypoints(ctx, dtype):
    exps, pairs = batch_of(dtype)
    rules = [[rr.keypoint_rule(e, p[side].shape[0]) for e, p in zip(exps, pairs)] for side in range(2)]
    with ctx.batch(pairs) as bt:
        kb, info = bt.keypoints(moving=rules[0], model=rules[1], want_maps=True, want_saliency=True)
        with kb:
            check_keypoints(pairs, rules[0], rules[1], kb, info)
            clouds = kb.get_clouds()
    count = len(pairs)
    for b, side, e, sal, W in each(exps, (info["moving_saliency"], info["model_saliency"])):
        assert 0 < (W > 0).sum() < W.size                         # the rule decides something
        assert bits_equal(sal, up(W, 2 * e)), f"pair {b} side {side} e {e}: {int((sal != up(W, 2 * e)).sum())} saliencies are not the witness's times 2^{2 * e}"
    for b, side, e, m, W in each(exps, (info["moving_map"], info["model_map"])):
        assert (W >= 0).any() and bits_equal(m, W), f"pair {b} side {side} e {e}: the map is not the witness's"
        assert info["counts"][side * count + b] == info["counts"][side * count + b % PER]
        assert bits_equal(clouds[b][side], up(clouds[b % PER][side], e)), f"pair {b} side {side} e {e}: the keypoints are not the witness's times 2^{e}"


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_outliers(ctx, dtype):
    exps, pairs = batch_of(dtype)
    radius = [rr.radius_rule(e) for e in exps]
    moving = [rr.STAT if b % PER == 0 else radius[b] for b in range(len(pairs))]   # either rule on either side, on every size
    model = [radius[b] if b % PER == 0 else rr.STAT for b in range(len(pairs))]
    ref = check_outliers(ctx, pairs, moving, model, "range")     # the device's bytes are these
    for side, name in enumerate(("moving", "model")):
        for b, e in enumerate(exps):
            w = b % PER
            stat = (moving, model)[side][b] is rr.STAT
            m, W = ref[name + "_map"][b], ref[name + "_map"][w]
            assert 0 < (W >= 0).sum() < W.size and bits_equal(m, W), f"pair {b} {name} e {e}: the map is not the witness's"
            s, S = ref[name + "_score"][b], ref[name + "_score"][w]
            assert bits_equal(s, up(S, e) if stat else S), f"pair {b} {name} e {e}: {int((s != (up(S, e) if stat else S)).sum())} scores are not the witness's, scaled"
            assert bits_equal(ref["clouds"][b][side], up(ref["clouds"][w][side], e)), f"pair {b} {name} e {e}: the kept points"


@DTYPES
def test_voxels(ctx, dtype):
    exps, pairs = batch_of(dtype)
    v = np.array([rr.voxel_edge(e) for e in exps])
    ref = check_voxels(ctx, pairs, v, v, "range")                # the device's bytes are these, maps included
    _, mm, qm = rr.vr.downsample_pairs(pairs, v, v)
    for b, side, e, m, W in each(exps, (mm, qm)):
        assert 1 < W.max() + 1 < W.size and bits_equal(m, W), f"pair {b} side {side} e {e}: the map is not the witness's"
        assert bits_equal(ref[b][side], up(ref[b % PER][side], e)), f"pair {b} side {side} e {e}: the points are not the witness's times 2^{e}"


# 6 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_descriptors_from_stored_normals(ctx, dtype):
    exps, pairs = batch_of(dtype)
    with ctx.batch(pairs) as bt:
        bt.estimate_covariances(rr.K, None, regularisation="none")
        bt.estimate_point_normals("centroid")
        feats = bt.compute_features_stored(rr.K, want=True)
        normals = bt.get_point_normals()
    for b, side, e, F, W in each(exps, feats):
        assert bits_equal(normals[side][b], normals[side][b % PER]), f"pair {b} side {side} e {e}: the stored normals"
        want = fr.fpfh(pairs[b][side], normals[side][b], rr.K)
        assert np.abs(W).max() > 0 and bits_equal(F, want), f"pair {b} side {side} e {e}: {int((F != want).any(axis=1).sum())} descriptors differ from the numpy rule"
        assert bits_equal(F, W), f"pair {b} side {side} e {e}: {int((F != W).any(axis=1).sum())} descriptors differ from the witness"


# 7 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_scaled_pairs_bytes_do_not_depend_on_the_batch(ctx, dtype):
    exps, pairs = batch_of(dtype)

    def run(ps, es, at):
        """everything the calls above return for pair `at` of the batch ps"""
        out = []
        with ctx.batch(ps) as bt:
            for reg in ("frobenius", "none"):
                c = bt.estimate_covariances(rr.K, None, regularisation=reg, lam=rr.LAM, want=True)
                out += [c[0][at], c[1][at]]
            n = bt.estimate_point_normals("centroid", want=True)
            f = bt.compute_features_stored(rr.K, want=True)
            out += [n[0][at], n[1][at], f[0][at], f[1][at]]
            rules = [[rr.keypoint_rule(e, p[side].shape[0]) for e, p in zip(es, ps)] for side in range(2)]
            kb, info = bt.keypoints(moving=rules[0], model=rules[1], want_maps=True, want_saliency=True)
            with kb:
                out += [info["moving_saliency"][at], info["model_saliency"][at], info["moving_map"][at], info["model_map"][at], *kb.get_clouds()[at]]
            ob, info = bt.remove_outliers([rr.STAT] * len(ps), [rr.radius_rule(e) for e in es], want_maps=True, want_scores=True)
            with ob:
                out += [info["moving_score"][at], info["model_score"][at], info["moving_map"][at], info["model_map"][at], *ob.get_clouds()[at]]
            v = np.array([rr.voxel_edge(e) for e in es])
            vb, mm, qm = bt.downsample(v, v, want_maps=True)
            with vb:
                out += [mm[at], qm[at], *vb.get_clouds()[at]]
        return out

    for b in (PER, len(pairs) - 1):                               # the lowest exponent's first pair, the highest's last
        alone = run([pairs[b]], [exps[b]], 0)
        beside = run(pairs[::-1], exps[::-1], len(pairs) - 1 - b)
        assert len(alone) == len(beside) and all(bits_equal(x, y) for x, y in zip(alone, beside)), (b, exps[b])
