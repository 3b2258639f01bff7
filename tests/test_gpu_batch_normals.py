"""GPU: point normals made and kept on the device (icp_batch_estimate_point_normals, icp_batch_set_point_normals,
icp_batch_get_point_normals, icp_batch_compute_features_stored, icp_diag_batch_centroids; Batch.estimate_point_normals and
Context.register_batch_global(..., device_normals=True)) against the numpy restatement tests/batch_normals_ref.py.

    1  bit for bit in all three modes -- clouds of 4 (k = 3), 63, 64, 65 and 130 points (a single ragged item, a full item, ragged
       last items, three items), pairs of different sizes in one batch, both dtypes, fp64 clouds with mantissas fp32 cannot hold; the
       covariances are the device's own estimate, read back, so the comparison is of the normals alone
    2  special clouds: 1e6 from the origin, exactly planar, collinear, coincident ((1, 0, 0)), a viewpoint that makes one point's dt
       exactly 0, given covariances with the zero matrix and two equal eigenvalues; an fp64 cloud of extent 1e200 whose estimated
       covariances overflow (normals exactly zero) beside a healthy pair
    3  centroids bit for bit for clouds of 1, 255, 256, 257 and 513 points with given covariances
    4  a pair alone, with the pairs swapped and inside a batch of another size: the same bytes
    5  the stored route: compute_features_stored == compute_features(get_point_normals()); set -> get round-trips; new descriptors
       discard the matches
    6  a loop under way does not notice
    7  every refusal, with the kept normals untouched; batches made from a batch hold none
    8  end to end on the bunny pair, see test_bunny_end_to_end_with_device_normals"""
import ctypes as C

import numpy as np
import pytest

import batch_feature_ref as fr
import batch_normals_ref as nr
from batch_ref import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
MODES = (("none", nr.NONE), ("centroid", nr.CENTROID), ("viewpoint", nr.VIEWPOINT))
_pd = C.POINTER(C.c_double)


def cloud(seed, n, dtype):
    """a bumpy sphere; fp64 clouds get mantissas fp32 cannot hold"""
    X = fr.blob(seed, n, dtype)[0]
    if X.dtype == np.float64:
        X = X + 1e-9 * np.random.default_rng(seed + 1).standard_normal(X.shape)
    return np.ascontiguousarray(X)


def views(pairs, seed):
    """(moving, model), each (count, 3): a viewpoint of its own per cloud, outside it"""
    rng = np.random.default_rng(seed)
    return rng.uniform(2.0, 4.0, (len(pairs), 3)) * rng.choice([-1.0, 1.0], (len(pairs), 3)), rng.uniform(-4.0, 4.0, (len(pairs), 3))


def check(pairs, covs, got, mode, vw, what=""):
    """a call's normals of every cloud against the restatement, bit for bit"""
    want = nr.normals_pairs(pairs, covs[0], covs[1], mode, vw)
    for side in range(2):
        for b in range(len(pairs)):
            g, w = got[side][b], want[side][b]
            bad = np.flatnonzero((g.view(np.uint64) != w.view(np.uint64)).any(axis=1))
            assert bad.size == 0, f"{what} pair {b} {'model' if side else 'moving'} n {w.shape[0]}: {bad.size} normals differ, first {bad[0]}: {g[bad[0]]!r} / {w[bad[0]]!r}"
    return want


def psd(seed, n):
    """(n, 6) random symmetric positive semi-definite matrices"""
    R = np.random.default_rng(seed).standard_normal((n, 3, 3))
    S = R @ R.transpose(0, 2, 1)
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))


# 1 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_normals_bit_for_bit(ctx, pkg, dtype):
    pairs = [(cloud(301, 4, dtype), cloud(302, 63, dtype)), (cloud(303, 64, dtype), cloud(304, 65, dtype)), (cloud(305, 130, dtype), cloud(306, 4, dtype))]
    vw = views(pairs, 7)
    with ctx.batch(pairs) as bt:
        covs = bt.estimate_covariances([3, 8, 9], [8, 7, 3], regularisation="none", want=True)
        for name, mode in MODES:
            got = bt.estimate_point_normals(name, viewpoints=vw if mode == nr.VIEWPOINT else None, want=True)
            want = check(pairs, covs, got, mode, vw, name)
            kept = bt.get_point_normals()
            assert all(bits_equal(kept[s][b], want[s][b]) for s in range(2) for b in range(3)), name
            if mode == nr.CENTROID:
                cm, cq = bt.diag_centroids()
                for b, (A, M) in enumerate(pairs):
                    assert bits_equal(cm[b], nr.centroid(A)) and bits_equal(cq[b], nr.centroid(M)), b
        flipped = [np.abs(a - b).max() > 0 for a, b in zip(nr.normals_pairs(pairs, *covs, nr.NONE)[0], want[0])]
        assert any(flipped)                                       # the orientation does something
        # one (3,) viewpoint serves every cloud; a Frobenius-regularised covariance is as good as a raw one
        covs = bt.estimate_covariances([3, 8, 9], [8, 7, 3], regularisation="frobenius", lam=1e-3, want=True)
        one = np.array([0.3, -2.0, 5.0])
        got = bt.estimate_point_normals("viewpoint", viewpoints=one, want=True)
        check(pairs, covs, got, nr.VIEWPOINT, (np.tile(one, (3, 1)), np.tile(one, (3, 1))), "one viewpoint")
        for N in got[0] + got[1]:
            assert np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-12


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_special_clouds(ctx, pkg, dtype):
    rng = np.random.default_rng(17)
    far = np.ascontiguousarray((cloud(311, 130, dtype).astype(np.float64) + 1e6).astype(dtype))
    plane = np.zeros((70, 3), dtype=dtype)
    plane[:, :2] = rng.uniform(-1.0, 1.0, (70, 2))
    line = np.zeros((65, 3), dtype=dtype)
    line[:, 0] = np.arange(65) * 0.25 + rng.uniform(0.0, 0.1, 65)
    same = np.ascontiguousarray(np.tile(np.array([[0.125, -0.75, 2.5]], dtype=dtype), (40, 1)))   # (40 of these add up exactly: the centroid is the point)
    flat, given = cloud(312, 66, dtype), cloud(313, 64, dtype)
    pairs = [(far, plane), (line, same), (flat, given)]
    with ctx.batch(pairs) as bt:
        cm, cq = bt.estimate_covariances(8, None, regularisation="none", want=True)
        assert (cq[0][:, [2, 4, 5]] == 0).all()                   # exactly planar: nothing along z
        assert (cm[1][:, 1:] == 0).all() and (cq[1] == 0).all()   # collinear: xx alone; coincident: the zero matrix
        cm[2] = np.tile(np.array([3.0, 0.0, 0.0, 2.0, 0.0, 1.0]), (66, 1))   # diag(3, 2, 1): the normal is (0, 0, 1)
        cq[2] = psd(5, 64)
        cq[2][:4] = 0.0                                           # the zero matrix
        Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        for r, lam in enumerate(((1.0, 1.0, 2.0), (1.0, 2.0, 2.0), (0.5, 0.5, 0.5))):   # two (three) equal eigenvalues, turned and not
            S = Q @ np.diag(lam) @ Q.T
            S = (S + S.T) / 2.0
            cq[2][4 + r] = (S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2])
            cq[2][8 + r] = (lam[0], 0.0, 0.0, lam[1], 0.0, lam[2])
        bt.set_covariances(cm, cq)
        vm, vq = views(pairs, 9)
        vm[2] = (5.0, 5.0, float(flat[0, 2]))                     # point 0 of `flat`: to_z == 0 and n == (0, 0, 1): dt is exactly 0
        for name, mode in MODES:
            got = bt.estimate_point_normals(name, viewpoints=(vm, vq) if mode == nr.VIEWPOINT else None, want=True)
            check(pairs, (cm, cq), got, mode, (vm, vq), name)
            if mode != nr.VIEWPOINT:
                assert bits_equal(got[1][1], np.tile(np.array([1.0, 0.0, 0.0]), (40, 1))), name   # coincident points: exactly (1, 0, 0)
            if mode == nr.NONE:
                assert bits_equal(got[1][2][:4], np.tile(np.array([1.0, 0.0, 0.0]), (4, 1)))      # the zero matrix
        z = got[0][2]                                             # (the viewpoint mode's)
        assert bits_equal(z[0], np.array([0.0, 0.0, 1.0]))        # dt == 0 does not flip
        above = flat[:, 2].astype(np.float64) > vm[2][2]
        assert above.any() and (~above).any() and (z[above, 2] == -1.0).all() and (z[~above, 2] == 1.0).all()
        assert (np.abs(got[1][0][:, 2]) == 1.0).all()             # the plane's normals are +-z exactly


def test_overflowing_covariances_give_zero_normals(ctx, pkg):
    """fp64, extent 1e200: d2, the squares and the sums of the covariance rule overflow; what the Jacobi makes of it is not finite,
    so the normals are exactly zero on both sides, in every mode; the healthy pair beside it is what it is alone"""
    big = (cloud(321, 70, np.float64) * 1e200, cloud(322, 66, np.float64) * 1e200)
    well = (cloud(323, 65, np.float64), cloud(324, 130, np.float64))
    with ctx.batch([well]) as bt:
        bt.estimate_covariances(8, None, regularisation="none")
        alone = bt.estimate_point_normals("centroid", want=True)
    with ctx.batch([big, well]) as bt:
        covs = bt.estimate_covariances(8, None, regularisation="none", want=True)
        assert not np.isfinite(covs[0][0]).all(axis=1).any() and not np.isfinite(covs[1][0]).all(axis=1).any()
        for name, mode in MODES:
            got = bt.estimate_point_normals(name, viewpoints=np.zeros(3) if mode == nr.VIEWPOINT else None, want=True)
            check([big, well], covs, got, mode, (np.zeros((2, 3)), np.zeros((2, 3))), name)
            assert bits_equal(got[0][0], np.zeros((70, 3))) and bits_equal(got[1][0], np.zeros((66, 3))), name
        got = bt.estimate_point_normals("centroid", want=True)
        assert bits_equal(got[0][1], alone[0][0]) and bits_equal(got[1][1], alone[1][0])


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_centroids_bit_for_bit(ctx, pkg, dtype):
    sizes = ((1, 255), (256, 257), (513, 1))
    pairs = [(np.ascontiguousarray(cloud(330 + b, max(n, 2), dtype)[:n] * 3.0 + 0.7), np.ascontiguousarray(cloud(340 + b, max(m, 2), dtype)[:m] - 2.0))
             for b, (n, m) in enumerate(sizes)]
    covs = ([psd(50 + b, n) for b, (n, _) in enumerate(sizes)], [psd(60 + b, m) for b, (_, m) in enumerate(sizes)])
    with ctx.batch(pairs) as bt:
        bt.set_covariances(*covs)
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_centroids()
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        bt.estimate_point_normals("viewpoint", viewpoints=np.ones(3))
        with pytest.raises(pkg.IcpError) as e:                   # still none: the centroid kernel runs for "centroid" alone
            bt.diag_centroids()
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        got = bt.estimate_point_normals("centroid", want=True)
        cm, cq = bt.diag_centroids()
        for b, (A, M) in enumerate(pairs):
            assert bits_equal(cm[b], nr.centroid(A)) and bits_equal(cq[b], nr.centroid(M)), (b, cm[b], nr.centroid(A), cq[b], nr.centroid(M))
        check(pairs, covs, got, nr.CENTROID, None)
        bt.estimate_point_normals("none")                         # a later call in another mode leaves the centroids
        assert bits_equal(bt.diag_centroids()[0], cm)


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_pairs_normals_do_not_depend_on_the_batch(ctx, pkg, dtype):
    X = (cloud(351, 300, dtype), cloud(352, 130, dtype))
    Y = (cloud(353, 65, dtype), cloud(354, 257, dtype))
    Z = (cloud(355, 70, dtype), cloud(356, 64, dtype))
    vx = (np.array([3.0, -2.0, 0.5]), np.array([0.1, 4.0, -3.0]))

    def run(pairs, at, name):
        vm, vq = np.ones((len(pairs), 3)), -np.ones((len(pairs), 3))
        vm[at], vq[at] = vx
        with ctx.batch(pairs) as bt:
            bt.estimate_covariances(8, None, regularisation="none")
            N = bt.estimate_point_normals(name, viewpoints=(vm, vq), want=True)
            cent = bt.diag_centroids() if name == "centroid" else (np.zeros((len(pairs), 3)),) * 2
            return N[0][at], N[1][at], cent[0][at], cent[1][at]

    for name, _ in MODES:
        alone = run([X], 0, name)
        for other in (run([X, Y], 0, name), run([Y, X], 1, name), run([Z, Y, X], 2, name), run([X, Z, Y], 0, name)):
            assert all(bits_equal(a, b) for a, b in zip(alone, other)), name


# 5 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_stored_route(ctx, pkg, dtype):
    pairs = [(cloud(361, 130, dtype), cloud(362, 65, dtype)), (cloud(363, 64, dtype), cloud(364, 200, dtype))]
    with ctx.batch(pairs) as bt:
        bt.estimate_covariances(9, None, regularisation="none")
        bt.estimate_point_normals("centroid")
        sm, sq = bt.compute_features_stored(9, k_model=8, want=True)
        nm, nq = bt.get_point_normals()
        hm, hq = bt.compute_features(9, (nm, nq), k_model=8, want=True)
        assert all(bits_equal(a, b) for a, b in zip(sm + sq, hm + hq))
        assert any(np.abs(f).max() > 0 for f in sm)
        assert all(bits_equal(a, b) for a, b in zip(bt.get_features()[0], sm))
        # new descriptors discard the matches
        bt.match_features()
        bt.ransac(20, 0.2)
        bt.compute_features_stored(9)
        with pytest.raises(pkg.IcpError) as e:
            bt.ransac(20, 0.2)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        # set -> get round-trips exactly, whatever finite values: nothing is normalised
        rng = np.random.default_rng(3)
        gm = [rng.uniform(-1e3, 1e3, A.shape) for A, _ in pairs]
        gq = [rng.uniform(-1e-3, 1e-3, M.shape) for _, M in pairs]
        gm[0][0], gq[1][-1] = (-0.0, 0.0, 5e-324), (1.7e308, -1.7e308, -0.0)
        bt.set_point_normals(moving=gm)
        got = bt.get_point_normals()
        assert all(bits_equal(a, b) for a, b in zip(got[0], gm)) and all(bits_equal(a, b) for a, b in zip(got[1], nq))   # a None side stays
        bt.set_point_normals(model=gq)
        got = bt.get_point_normals()
        assert all(bits_equal(a, b) for a, b in zip(got[0] + got[1], gm + gq))
        # the stored route on given normals is the host route on the same
        bt.set_point_normals([fr.blob(70 + b, A.shape[0], dtype)[1] for b, (A, _) in enumerate(pairs)],
                             [fr.blob(80 + b, M.shape[0], dtype)[1] for b, (_, M) in enumerate(pairs)])
        um, uq = bt.get_point_normals()
        a = bt.compute_features_stored(7, want=True)
        b_ = bt.compute_features(7, (um, uq), want=True)
        assert all(bits_equal(x, y) for x, y in zip(a[0] + a[1], b_[0] + b_[1]))
        want = fr.fpfh(pairs[1][0], um[1], 7)
        assert bits_equal(a[0][1], want)                          # ... and the restated descriptors


# 6 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_loop_under_way_does_not_notice(ctx, pkg, dtype):
    A, M = cloud(371, 200, dtype), cloud(372, 150, dtype)
    A = np.ascontiguousarray((A.astype(np.float64) @ fr.rodrigues((0, 0, 1), 4.0).T + 0.02).astype(dtype))

    def run(disturb):
        with ctx.batch([(A, M)]) as bt:
            bt.estimate_covariances(8, None, regularisation="none")   # (before the loop: new covariances would discard it)
            bt.begin(max_iter=12, tol=1e-9)
            bt.run(2)
            if disturb:
                bt.estimate_point_normals("centroid")
                bt.compute_features_stored(8)
                bt.estimate_point_normals("viewpoint", viewpoints=np.array([1.0, 2.0, 3.0]), want=True)
                bt.set_point_normals(model=[np.ones((150, 3))])
                bt.get_point_normals()
                bt.diag_centroids()
            while bt.run(1 << 20)[1] > 0:
                pass
            return bt.state(0), bt.get_moving()[0], bt.loop_indices()[0], bt.diag_moments(0)

    a, b = run(False), run(True)
    assert a[0]["iterations"] == b[0]["iterations"] and a[0]["status"] == b[0]["status"] and a[0]["iterations"] > 2
    assert bits_equal(a[0]["T"], b[0]["T"]) and bits_equal(np.asarray(a[0]["err"]), np.asarray(b[0]["err"]))
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and bits_equal(np.asarray(a[3]), np.asarray(b[3]))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_normals_alone(ctx, pkg):
    INVALID, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    lib = pkg.load()
    dtype = np.float32
    pairs = [(cloud(381, 70, dtype), cloud(382, 65, dtype)), (cloud(383, 64, dtype), cloud(384, 130, dtype))]
    n, m = 134, 195

    def est(bt, mode, vm, vq, want=True):
        """the C call; (rc, message); with want, both outputs are given and no element of them may be written on a refusal"""
        om, oq = np.full((n, 3), -7.0), np.full((m, 3), -7.0)
        rc = lib.icp_batch_estimate_point_normals(bt._h, mode, None if vm is None else vm.ctypes.data_as(_pd), None if vq is None else vq.ctypes.data_as(_pd),
                                                  om.ctypes.data_as(_pd) if want else None, oq.ctypes.data_as(_pd) if want else None)
        msg = lib.icp_last_error().decode()
        assert rc != 0 and (om == -7.0).all() and (oq == -7.0).all(), msg
        return rc, msg

    def unchanged(bt, before):
        now = bt.get_point_normals()
        return all(bits_equal(a, b) for a, b in zip(now[0] + now[1], before[0] + before[1]))

    ok = np.ones((2, 3))
    with ctx.batch(pairs) as bt:
        # nothing yet: no covariances, no normals
        for side, name in ((0, "moving clouds"), (1, "models")):
            out = np.empty((m if side else n, 3))
            rc = lib.icp_batch_get_point_normals(bt._h, None if side else out.ctypes.data_as(_pd), out.ctypes.data_as(_pd) if side else None)
            assert rc == STATE and name in lib.icp_last_error().decode()
        rc, msg = est(bt, 2, None, None)
        assert rc == STATE and "moving clouds" in msg, msg
        with pytest.raises(pkg.IcpError) as e:
            bt.compute_features_stored(8)
        assert e.value.code == STATE and "moving clouds" in str(e.value)
        bt.estimate_covariances(None, 8, regularisation="none")   # the models alone
        rc, msg = est(bt, 0, None, None)
        assert rc == STATE and "moving clouds" in msg, msg
        # normals on one side only
        bt.set_point_normals(moving=[np.ones((70, 3)), np.ones((64, 3))])
        with pytest.raises(pkg.IcpError) as e:
            bt.compute_features_stored(8)
        assert e.value.code == STATE and "models" in str(e.value)
        with pytest.raises(pkg.IcpError) as e:
            bt.get_point_normals()
        assert e.value.code == STATE
        bt.set_point_normals(model=[np.full((65, 3), 0.5), np.full((130, 3), -0.5)])
        before = bt.get_point_normals()
        rc, msg = est(bt, 1, ok, ok)                              # given normals, and still no covariances of the moving clouds
        assert rc == STATE and "moving clouds" in msg and unchanged(bt, before), msg
    with ctx.batch(pairs) as bt:
        bt.estimate_covariances(8, None, regularisation="none")
        before = bt.estimate_point_normals("centroid", want=True)
        feats = bt.compute_features_stored(8, want=True)
        cent = bt.diag_centroids()
        for mode in (3, -1, 7):
            rc, msg = est(bt, mode, ok, ok)
            assert rc == INVALID and "orientation" in msg and unchanged(bt, before), (mode, msg)
        rc, msg = est(bt, 1, None, ok)
        assert rc == INVALID and "moving_viewpoints" in msg and unchanged(bt, before), msg
        rc, msg = est(bt, 1, ok, None)
        assert rc == INVALID and "model_viewpoints" in msg and unchanged(bt, before), msg
        for bad in (np.nan, np.inf, -np.inf):
            for side in (0, 1):
                v = ok.copy()
                v[1, 2] = bad
                rc, msg = est(bt, 1, v if side == 0 else ok, v if side == 1 else ok, want=bool(side))
                assert rc == INVALID and "pair 1" in msg and ("model" if side else "moving") in msg and unchanged(bt, before), (bad, side, msg)
        # in the other modes the arrays are not read: a NaN there is nobody's business
        bad = np.full((2, 3), np.nan)
        assert lib.icp_batch_estimate_point_normals(bt._h, 2, bad.ctypes.data_as(_pd), None, None, None) == 0 and unchanged(bt, before)
        # the setter and the getter
        assert lib.icp_batch_set_point_normals(bt._h, None, None) == INVALID and unchanged(bt, before)
        assert lib.icp_batch_get_point_normals(bt._h, None, None) == INVALID
        for side in (0, 1):
            for v in (np.nan, np.inf):
                g = [np.ones((65, 3)), np.ones((130, 3))] if side else [np.ones((70, 3)), np.ones((64, 3))]
                g[1][5, 1] = v
                with pytest.raises(pkg.IcpError) as e:
                    bt.set_point_normals(**{"model" if side else "moving": g})
                assert e.value.code == INVALID and "pair 1" in str(e.value) and ("model" if side else "moving") in str(e.value) and unchanged(bt, before)
        with pytest.raises(ValueError):
            bt.set_point_normals(moving=[np.ones((70, 3))])
        with pytest.raises(ValueError):
            bt.estimate_point_normals("viewpoint", viewpoints=np.ones(2))
        # the stored descriptors keep compute_features' refusals
        k = np.full(2, 8, dtype=np.intc)
        pi = C.POINTER(C.c_int)
        assert lib.icp_batch_compute_features_stored(bt._h, None, k.ctypes.data_as(pi), None, None) == INVALID and "k_moving" in lib.icp_last_error().decode()
        assert lib.icp_batch_compute_features_stored(bt._h, k.ctypes.data_as(pi), None, None, None) == INVALID and "k_model" in lib.icp_last_error().decode()
        for kk in (2, 33):                                        # out of range
            with pytest.raises(pkg.IcpError) as e:
                bt.compute_features_stored([8, kk])
            assert e.value.code == INVALID and "pair 1" in str(e.value) and "moving" in str(e.value)
        assert lib.icp_diag_batch_centroids(bt._h, None) == INVALID
        now = bt.get_features()
        assert all(bits_equal(a, b) for a, b in zip(now[0] + now[1], feats[0] + feats[1])) and unchanged(bt, before)
        assert bits_equal(bt.diag_centroids()[0], cent[0]) and bits_equal(bt.diag_centroids()[1], cent[1])
        # the normals are a snapshot: later covariances leave them in place
        bt.estimate_covariances(5, None, regularisation="frobenius")
        bt.set_covariances(model=[psd(1, 65), psd(2, 130)])
        assert unchanged(bt, before)
        # batches made from this one hold none
        made = [bt.downsample(0.3), bt.remove_outliers()[0], bt.keypoints()[0]]
        for nb in made:
            with nb:
                with pytest.raises(pkg.IcpError) as e:
                    nb.get_point_normals()
                assert e.value.code == STATE
                with pytest.raises(pkg.IcpError) as e:
                    nb.compute_features_stored(3)
                assert e.value.code == STATE
        assert unchanged(bt, before)
    # a context with a pending pass
    A, M = pairs[0]
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with c.batch(pairs) as bt:
            bt.estimate_covariances(8, None, regularisation="none")
            before = bt.estimate_point_normals("none", want=True)
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            assert est(bt, 2, None, None)[0] == STATE
            for call in (lambda: bt.set_point_normals(moving=before[0]), bt.get_point_normals, lambda: bt.compute_features_stored(8), bt.diag_centroids):
                with pytest.raises(pkg.IcpError) as e:
                    call()
                assert e.value.code == STATE
            c.loop_complete()
            assert unchanged(bt, before)
            bt.estimate_point_normals("centroid")


# 8 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_bunny_end_to_end_with_device_normals(ctx, pkg, golden, dtype):
    """The bunny pair of batch_feature_ref.bunny_pair, set up as test_gpu_batch_feature.test_bunny_end_to_end sets it up (k = 24,
    mutual matches, 2 000 hypotheses, 7.5 mm, edge check 0.9, seed 1) with the normals made on the device, facing the centroids.
    Conditions, those of that test: the pose ransac returns is within 10 degrees and 1 cm of the truth; a point-to-point batch gated
    at 1 cm and started from it ends within 2 degrees; the same batch started from the identity ends more than 30 degrees away.
    The numpy restatement alone with the rule's normals (tests/test_batch_normals_ref.py prints it): 391 mutual correspondences, 115
    of them within 1 cm of the truth; seed 1: 87 inliers, 1.718 degrees and 2.59 mm, refined to 0.701 degrees -- inside half of
    every bound, so seed 1 stays; from the identity the loop ends 150.750 degrees away."""
    A, M, Tt = fr.bunny_pair(golden)
    A, M = A.astype(dtype), M.astype(dtype)
    K, H, MD, GATE, SEED = 24, 2000, 0.0075, 0.01, 1
    err = lambda T: (fr.angle_deg(T[:3, :3] @ Tt[:3, :3].T), float(np.linalg.norm(T[:3, 3] - Tt[:3, 3])))
    with ctx.batch([(A, M)]) as bt:
        covs = bt.estimate_covariances(K, None, regularisation="none", want=True)
        got = bt.estimate_point_normals("centroid", want=True)
        check([(A, M)], covs, got, nr.CENTROID, None, "bunny")
        bt.compute_features_stored(K)
        fwd, rev, kept = bt.match_features(mutual=True)
        start = bt.ransac(H, MD, edge_similarity=0.9, seed=SEED)[0]
    assert start["status"] == 0 and start["correspondences"] == int(kept[0].sum())
    res = ctx.register_batch_global([(A, M)], 0.0, K, H, MD, seed=SEED, gate=GATE, device_normals=True)[0]
    host = ctx.register_batch_global([(A, M)], 0.0, K, H, MD, seed=SEED, gate=GATE)[0]
    cold = ctx.register_batch([(A, M)], max_distance=GATE)[0]
    hs = host.extra["global"]
    print(f"device normals: correspondences {start['correspondences']} inliers {start['inliers']} rot {err(start['T'])[0]:.3f} deg "
          f"trans {err(start['T'])[1] * 1e3:.2f} mm, refined {err(res.T)[0]:.3f} deg {err(res.T)[1] * 1e3:.2f} mm; "
          f"host normals: correspondences {hs['correspondences']} inliers {hs['inliers']} rot {err(hs['T'])[0]:.3f} deg "
          f"trans {err(hs['T'])[1] * 1e3:.2f} mm, refined {err(host.T)[0]:.3f} deg {err(host.T)[1] * 1e3:.2f} mm; "
          f"from the identity {err(cold.T)[0]:.3f} deg")
    assert err(start["T"])[0] < 10.0 and err(start["T"])[1] < 0.01
    assert err(res.T)[0] < 2.0
    assert err(cold.T)[0] > 30.0
    # the one-call entry runs the same sequence; a given viewpoint serves both sides, as on the host route
    assert bits_equal(res.extra["global"]["T"], start["T"]) and res.extra["global"]["inliers"] == start["inliers"]
    fine_ = ctx.register_batch([(A, M)], max_distance=GATE, init=start["T"][None])[0]
    assert bits_equal(res.T, fine_.T)
    seen = ctx.register_batch_global([(A, M)], 0.0, K, H, MD, seed=SEED, gate=GATE, device_normals=True, viewpoint=np.array([0.0, 0.1, 0.5]))[0]
    assert seen.extra["global"]["status"] == 0
