"""What the range tests of the batched neighbourhood calls share (tests/test_batch_range_ref.py, test_gpu_batch_range.py): clouds and
covariances times exact powers of two, and two references that know nothing of the rules under test.  Nothing here touches a device.

    equivariance  every operation of the rules -- + - * / sqrt, comparisons, floor of a quotient -- commutes with a multiplication
                  by 2^e as long as no intermediate leaves the normal range: a cloud times 2^e must give the scale-1 answer, exactly
                  scaled.  Squared distances and covariances scale by 2^(2e), outlier scores and voxel points by 2^e; normals,
                  Frobenius-regularised covariances, maps, counts and FPFH descriptors do not change at all.  scaled() makes the
                  clouds and refuses an exponent that would cost a bit; E64 and E32 are the exponents per dtype -- E64 passes
                  2^+-200 in the coordinates, where a covariance passes 2^+-400 and its squares leave the double range, which
                  the range rule of icp_eigh3 (batch_keypoint_ref.range_scale) exists for.  An fp32 cloud's covariances are formed
                  in double and stay far inside.
    LAPACK        lapack_normals(): np.linalg.eigh on every matrix divided by the power of two at or above its largest magnitude
                  (np.frexp: exact), the eigenvector of the smallest eigenvalue, and the mask w1 - w0 >= 1e-3 * w2 under which that
                  eigenvector is determined to about 10 eps norm / gap (tests/test_batch_normals_ref.py, where TOL comes from).
    MAGS          the powers of two for given covariances: both sides of the rule's 2^+-400, the middle, and 2^+-1000 where an
                  eigenvalue scaled back may leave the range.

Intensity gradients (icp_batch_estimate_gradients) are left out: the tangent constraint adds cnt^2 n n^T, which is scale-free, to
terms that scale with the cloud, so that rule is not equivariant and has no exact scaled answer.
"""
import numpy as np

import batch_feature_ref as fr
import batch_gicp_ref as gr
import batch_keypoint_ref as kr
import batch_normals_ref as nr
import batch_outlier_ref as orf
import batch_voxel_ref as vr

E64 = (-450, -300, -258, -100, 100, 258, 300, 450)
E32 = (-52, -40, 40, 56)
MAGS = (-1000, -600, -401, -399, 0, 399, 401, 600, 1000)
TOL = 1e-9              # rad, under the gap mask: test_normals_agree_with_lapack_on_the_bunny's
MASKED = 0.10           # the share of points the gap mask may leave out: that test's

K = 8                   # neighbours of the covariance, outlier and FPFH rules
LAM = 1e-3
RS, RN = 0.35, 0.2      # ISS radii at scale 1, of a blob of 200 points
STAT = ("statistical", 8, 1.0)
RADIUS, RADIUS_MIN = 0.3, 3
VOXEL = 0.25
VIEW = np.array([0.3, -2.0, 5.0])   # a viewpoint at scale 1, outside the blobs


def exponents(dtype):
    return E64 if np.dtype(dtype) == np.float64 else E32


def scaled(X, e):
    """X times 2^e in X's own dtype, exactly: every non-zero coordinate stays normal and finite, and scaling back gives the bytes"""
    X = np.ascontiguousarray(X)
    Y = np.ldexp(X, e).astype(X.dtype)
    nz = X != 0
    assert np.isfinite(Y).all() and (np.abs(Y[nz]) >= np.finfo(X.dtype).tiny).all(), (X.dtype, e)
    assert np.ldexp(Y, -e).astype(X.dtype).tobytes() == X.tobytes(), (X.dtype, e)
    return Y


def blob(seed, n, dtype):
    """batch_feature_ref.blob, the points alone"""
    return fr.blob(seed, n, dtype)[0]


def angle(a, b):
    """(n,) rad between the directions a and b (n, 3), up to sign: arctan2 of the cross and dot products"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def lapack_normals(C6):
    """(N (n, 3), gap (n,) bool): LAPACK's eigenvector of the smallest eigenvalue of every matrix of C6 (n, 6), each divided by the
    power of two at or above its largest magnitude first, and the mask w1 - w0 >= 1e-3 * w2 of LAPACK's own eigenvalues"""
    C6 = np.asarray(C6, dtype=np.float64)
    _, ex = np.frexp(np.abs(C6).max(axis=1))                     # amax = m * 2^ex, m in [0.5, 1)
    w, Z = np.linalg.eigh(gr.full(np.ldexp(C6, -ex[:, None])))
    return np.ascontiguousarray(Z[:, :, 0]), (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]


def check_lapack(N, C6, what=""):
    """the normals N (n, 3) of the covariances C6 against LAPACK's: within TOL under the gap mask, which leaves out at most MASKED
    of the points.  Returns the largest angle"""
    want, gap = lapack_normals(C6)
    assert (~gap).mean() <= MASKED, f"{what}: the gap mask leaves out {100.0 * (~gap).mean():.1f} %"
    ang = angle(np.asarray(N, dtype=np.float64), want)
    worst = float(ang[gap].max())
    assert worst <= TOL, f"{what}: {int((ang[gap] > TOL).sum())} of {int(gap.sum())} normals beyond {TOL} rad of LAPACK's, the largest angle {worst:.3e}"
    return worst


def gapped(seed, n):
    """(n, 6): symmetric positive definite matrices Q diag(l) Q^T with l0 in [0.05, 0.5], l1 in [1, 2], l2 in [3, 6], divided by the
    power of two at or above the largest magnitude: 2^m times such a matrix is exact for every m of MAGS"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    lam = np.stack([rng.uniform(0.05, 0.5, n), rng.uniform(1.0, 2.0, n), rng.uniform(3.0, 6.0, n)], axis=1)
    A = (Q * lam[:, None, :]) @ Q.transpose(0, 2, 1)
    A = (A + A.transpose(0, 2, 1)) / 2.0
    return unit6(np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], axis=1))


def unit6(C6):
    """C6 (n, 6) with every matrix divided by the power of two at or above its largest magnitude (a zero matrix stays)"""
    C6 = np.asarray(C6, dtype=np.float64)
    _, ex = np.frexp(np.abs(C6).max(axis=1))
    return np.ascontiguousarray(np.ldexp(C6, -ex[:, None]))


def exact6(C6, bits=20):
    """unit6(C6) with every entry rounded to a multiple of 2^-bits: no entry lies more than `bits` binary places below the largest
    magnitude (in [0.5, 1)), so 2^m times the matrix is exact down to m = -1000, where an entry that small would be subnormal.  The
    matrices move by 1e-6 of their norm: covariances still, and LAPACK is given the same"""
    return np.ascontiguousarray(np.ldexp(np.rint(np.ldexp(unit6(C6), bits)), -bits))


def deficient():
    """(rank1 (4, 6), v (4, 3), rank2 (4, 6)): v v^T and v v^T + u u^T from integer vectors -- every entry a small integer, exact at
    any power of two.  A rank-1 matrix has no gap: its normal is any unit vector orthogonal to v.  A rank-2 matrix has w0 == 0
    and a gap: its normal is v x u."""
    v = np.array([[1.0, 2.0, 3.0], [2.0, -1.0, 0.0], [0.0, 0.0, 5.0], [3.0, 1.0, -2.0]])
    u = np.array([[2.0, 0.0, -1.0], [1.0, 1.0, 4.0], [1.0, -3.0, 0.0], [-1.0, 2.0, 2.0]])
    six = lambda a: np.stack([a[:, 0] * a[:, 0], a[:, 0] * a[:, 1], a[:, 0] * a[:, 2], a[:, 1] * a[:, 1], a[:, 1] * a[:, 2], a[:, 2] * a[:, 2]], axis=1)
    return six(v), v, six(v) + six(u)


def check_deficient(N1, N2, Nzero, what=""):
    """the normals of deficient()'s matrices at any power of two, and of zero matrices: a rank-1 normal is a unit vector orthogonal to
    v within TOL, a rank-2 normal is LAPACK's within TOL, a zero matrix gives exactly (1, 0, 0)"""
    r1, v, r2 = deficient()
    N1, N2, Nzero = (np.asarray(a, dtype=np.float64) for a in (N1, N2, Nzero))
    assert np.abs(np.linalg.norm(N1, axis=1) - 1.0).max() < 1e-14, what
    off = np.abs(np.pi / 2.0 - angle(N1, v / np.linalg.norm(v, axis=1, keepdims=True)))
    assert off.max() <= TOL, f"{what}: a rank-1 normal {off.max():.3e} rad from the plane orthogonal to v"
    want, gap = lapack_normals(r2)
    assert gap.all()
    assert angle(N2, want).max() <= TOL, f"{what}: a rank-2 normal {angle(N2, want).max():.3e} rad from LAPACK's"
    assert Nzero.tobytes() == np.tile(np.array([1.0, 0.0, 0.0]), (Nzero.shape[0], 1)).tobytes(), what


# ---- the rules at scale 2^e --------------------------------------------------------------------------------------------------------
def keypoint_rule(e, n=200):
    """the ISS rule of a blob of n points times 2^e: the radii RS and RN of the 200-point blob, times sqrt(200 / n) -- the spacing of n
    points on the same surface -- so that a smaller blob still has salient points and keypoints"""
    s = np.sqrt(200.0 / n)
    return kr.rule(float(np.ldexp(RS * s, e)), float(np.ldexp(RN * s, e)))


def radius_rule(e):
    return ("radius", float(np.ldexp(RADIUS, e)), RADIUS_MIN)


def voxel_edge(e):
    return float(np.ldexp(VOXEL, e))


def viewpoint(e):
    return np.ldexp(VIEW, e)


def rules_at(X, N, e):
    """everything the numpy rules make of the cloud X times 2^e (N: unit normals for the descriptors), as a dict"""
    Y = scaled(X, e)
    raw, _ = gr.covariances(Y, K, gr.COV_NONE)
    fro, _ = gr.covariances(Y, K, gr.COV_FROBENIUS, LAM)
    kp = kr.keypoints(Y, keypoint_rule(e, Y.shape[0]))
    st, ra = orf.remove(Y, STAT), orf.remove(Y, radius_rule(e))
    vx = vr.downsample(Y, voxel_edge(e))
    return dict(cloud=Y, raw=raw, frobenius=fro,
                normals={mode: nr.normals(Y, raw, mode, viewpoint(e)) for mode in (nr.NONE, nr.CENTROID, nr.VIEWPOINT)},
                saliency=kp[2], keypoint_map=kp[1], stat_score=st[2], stat_map=st[1], radius_score=ra[2], radius_map=ra[1],
                voxel_points=vx[0], voxel_map=vx[1], fpfh=fr.fpfh(Y, N, K))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_equivariant(got, one, e, what=""):
    """`got`, the results at scale 2^e (a dict as rules_at makes it, or any part of it), against `one`, the scale-1 results"""
    up = lambda a, p: np.ldexp(a, p).astype(a.dtype)
    expect = dict(raw=lambda: up(one["raw"], 2 * e), frobenius=lambda: one["frobenius"], saliency=lambda: up(one["saliency"], 2 * e),
                  keypoint_map=lambda: one["keypoint_map"], stat_score=lambda: up(one["stat_score"], e), stat_map=lambda: one["stat_map"],
                  radius_score=lambda: one["radius_score"], radius_map=lambda: one["radius_map"],
                  voxel_points=lambda: up(one["voxel_points"], e), voxel_map=lambda: one["voxel_map"], fpfh=lambda: one["fpfh"])
    for name, g in got.items():
        if name == "cloud":
            continue
        if name == "normals":
            for mode, N in g.items():
                assert same(N, one["normals"][mode]), f"{what} e {e}: normals, orientation {mode}: {int((N != one['normals'][mode]).any(axis=1).sum())} differ"
            continue
        want = expect[name]()
        assert same(g, want), f"{what} e {e}: {name}: {int((g != want).sum())} of {want.size} values differ"


_ONE = {}


def witness(seed, n, dtype):
    """(X, N, rules_at(X, N, 0)) of the blob, computed once per session and left unchanged"""
    key = (seed, n, np.dtype(dtype).str)
    if key not in _ONE:
        X, N = fr.blob(seed, n, dtype)
        _ONE[key] = (X, N, rules_at(X, N, 0))
    return _ONE[key]
