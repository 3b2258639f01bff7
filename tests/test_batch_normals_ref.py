"""CPU: the numpy restatement of the point-normal rule (tests/batch_normals_ref.py) -- its Jacobi with eigenvectors against icp_eigh3
bit for bit, its normals against LAPACK's (engine.oriented_normals) on the bunny's covariances, the special matrices, the centroid,
and the bunny pair end to end with the restated normals, whose printed numbers are what the conditions of the GPU end-to-end test
(tests/test_gpu_batch_normals.py) rest on."""
import numpy as np
import pytest

import batch_feature_ref as fr
import batch_gicp_ref as gr
import batch_normals_ref as nr
from batch_ref import keep_within, reference_loop

K, H, MD, GATE, SEED = 24, 2000, 0.0075, 0.01, 1   # the end-to-end test's settings


def sym6(A):
    """(k, 3, 3) symmetric -> (6, k): xx, xy, xz, yy, yz, zz"""
    return np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]])


def rot(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q


def matrices():
    rng = np.random.default_rng(23)
    R = rng.standard_normal((40, 3, 3))
    psd = R @ R.transpose(0, 2, 1)                               # random symmetric positive semi-definite
    diagonal = np.stack([np.diag(np.abs(rng.standard_normal(3))) for _ in range(8)] + [np.diag([3.0, 2.0, 1.0]), np.diag([1.0, 1.0, 1.0])])
    v, u = rng.standard_normal((8, 3)), rng.standard_normal((8, 3))
    rank1 = v[:, :, None] * v[:, None, :]
    rank2 = rank1 + u[:, :, None] * u[:, None, :]
    equal = []                                                   # two equal eigenvalues: the smallest pair, the largest pair, all three
    for lam in ((1.0, 1.0, 2.0), (1.0, 2.0, 2.0), (0.0, 0.0, 5.0), (0.5, 0.5, 0.5), (0.25, 0.25, 4.0)):
        equal.append(np.diag(lam))
        for _ in range(3):
            Q = rot(rng)
            A = Q @ np.diag(lam) @ Q.T
            equal.append((A + A.T) / 2.0)
    sets = dict(psd=psd, diagonal=diagonal, rank1=rank1, rank2=rank2, zero=np.zeros((2, 3, 3)), equal=np.stack(equal))
    for name in list(sets):
        sets[name + "_tiny"] = sets[name] * 1e-300
        sets[name + "_huge"] = sets[name] * 1e150
    return sets


def test_jacobi_with_vectors_equals_icp_eigh3_bit_for_bit(pkg):
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    for name, A in matrices().items():
        w, n, Z = nr.jacobi(sym6(A))
        for k in range(A.shape[0]):
            want_w, want_Z = pkg.eigh3(A[k])
            want_Z = np.asarray(want_Z, dtype=np.float64).reshape(3, 3)
            assert np.array_equal(u64(w[:, k]), u64(want_w)), (name, k, w[:, k], want_w)
            assert np.array_equal(u64(n[:, k]), u64(want_Z[:, 0])), (name, k, n[:, k], want_Z[:, 0])   # the chosen column
            assert np.array_equal(u64(Z[:, :, k]), u64(want_Z)), (name, k)
    _, n, _ = nr.jacobi(sym6(np.zeros((1, 3, 3))))
    assert n[:, 0].tobytes() == np.array([1.0, 0.0, 0.0]).tobytes()   # a zero matrix gives (1, 0, 0)


def test_special_covariances():
    X = np.zeros((4, 3))
    cov = np.zeros((4, 6))
    cov[1] = (np.inf, 0, 0, 1, 0, 1)                             # an infinite entry on the diagonal: the stop test holds at once
    cov[2] = (np.nan, 0, 0, 1, 0, 1)
    cov[3] = (1, np.inf, 0, 1, 0, 1)                             # an infinite entry off the diagonal
    N = nr.normals(X, cov, nr.NONE)
    assert np.isfinite(N).all()                                   # the non-finite rule: what is kept is always finite
    assert N[0].tobytes() == np.array([1.0, 0.0, 0.0]).tobytes()
    # exactly zero normals stay +0.0 whatever the viewpoint: dt is 0 or NaN, never < 0
    Z = nr.normals(X + 1.0, np.full((4, 6), np.nan), nr.VIEWPOINT, (-5.0, -5.0, -5.0))
    assert Z.tobytes() == np.zeros((4, 3)).tobytes()


def test_overflowing_covariances_give_zero_normals():
    """an fp64 cloud of extent 1e200: the squares of the covariance rule overflow, the sums are inf - inf"""
    X = fr.blob(71, 40, np.float64)[0] * 1e200
    with np.errstate(over="ignore", invalid="ignore"):
        C, _ = gr.covariances(X, 8, gr.COV_NONE)
    assert not np.isfinite(C).all(axis=1).any()
    for mode, view in ((nr.NONE, None), (nr.CENTROID, None), (nr.VIEWPOINT, (0.0, 0.0, 0.0))):
        assert nr.normals(X, C, mode, view).tobytes() == np.zeros((40, 3)).tobytes(), mode


@pytest.mark.parametrize("n", [1, 4, 255, 256, 257, 513])
def test_centroid_is_the_strided_sum(n):
    X = np.random.default_rng(n).uniform(-3.0, 5.0, (n, 3)).astype(np.float32)
    got = nr.centroid(X)
    want = np.empty(3)
    for a in range(3):                                           # the header's statements, as plain loops
        total = 0.0
        for t in range(256):
            s = 0.0
            for j in range(t, n, 256):
                s += float(X[j, a])
            total += s
        want[a] = total / float(n)
    assert got.tobytes() == want.tobytes()
    assert np.abs(got - X.astype(np.float64).mean(0)).max() <= 1e-12 * 5.0 * max(1, n)


def bunny_covariances(golden):
    if "cov" not in _BUNNY:
        A, M, Tt = fr.bunny_pair(golden)
        _BUNNY["cov"] = (A, M, Tt, gr.covariances(A, K, gr.COV_NONE)[0], gr.covariances(M, K, gr.COV_NONE)[0])
    return _BUNNY["cov"]


_BUNNY = {}


def test_normals_agree_with_lapack_on_the_bunny(pkg, golden):
    """engine.oriented_normals (np.linalg.eigh) against the restated rule on the covariances of the thinned bunny sample.  Both
    solvers are accurate to about 10 eps norm(C) / gap: 2e-12 rad where w1 - w0 >= 1e-3 w2."""
    A, M, _, CA, CM = bunny_covariances(golden)
    for X, C6 in ((A, CA), (M, CM)):
        view = nr.centroid(X)
        mine = nr.normals(X, C6, nr.VIEWPOINT, view)
        theirs = pkg.oriented_normals(X, C6, view)
        w = np.linalg.eigvalsh(gr.full(C6))
        gap = (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]
        dot = (mine * theirs).sum(1)
        ang = np.arctan2(np.linalg.norm(np.cross(mine, theirs), axis=1), np.abs(dot))   # up to sign
        to = view[None, :] - X.astype(np.float64)
        dt = (theirs * to).sum(1)
        clear = gap & (np.abs(dt) > 1e-9 * np.linalg.norm(to, axis=1))
        print(f"{X.shape[0]} points: gap condition fails for {100.0 * (~gap).mean():.2f} %, gap or sign condition for {100.0 * (~clear).mean():.2f} %; "
              f"largest angle under the gap condition {ang[gap].max():.3e} rad")
        assert gap.mean() > 0.9
        assert (ang[gap] <= 1e-9).all()
        assert (dot[clear] > 0).all()
        assert np.abs(np.linalg.norm(mine, axis=1) - 1.0).max() < 1e-14   # not renormalised, and unit all the same


def test_a_clouds_normals_do_not_depend_on_the_other_pairs(golden):
    A, M, _, CA, CM = bunny_covariances(golden)
    B, CB = A[:130], CA[:130]
    alone = nr.normals_pairs([(B, M)], [CB], [CM])
    swapped = nr.normals_pairs([(A, A), (B, M)], [CA, CB], [CA, CM])
    assert alone[0][0].tobytes() == swapped[0][1].tobytes() and alone[1][0].tobytes() == swapped[1][1].tobytes()
    other = nr.normals_pairs([(B, M), (A, B)], [CB, CA], [CM, CB])
    assert alone[0][0].tobytes() == other[0][0].tobytes() and alone[1][0].tobytes() == other[1][0].tobytes()


def bunny_restated(golden, seeds=(SEED,)):
    """the whole restated path with the rule's normals: correspondences and, per seed, RANSAC's result and its pose errors"""
    A, M, Tt, CA, CM = bunny_covariances(golden)
    FA = fr.fpfh(A, nr.normals(A, CA, nr.CENTROID), K)
    FM = fr.fpfh(M, nr.normals(M, CM, nr.CENTROID), K)
    fwd, _, kept = fr.match(FA, FM, True)
    ci, cj = fr.correspondences(fwd, kept)
    moved = A[ci].astype(np.float64) @ Tt[:3, :3].T + Tt[:3, 3]
    good = int((np.linalg.norm(moved - M[cj].astype(np.float64), axis=1) < 0.01).sum())
    out = dict(corr=int(ci.size), good=good, seeds={})
    for s in seeds:
        r = fr.ransac(A, M, ci, cj, s, H, MD, 0.9)
        out["seeds"][s] = (r, fr.angle_deg(r["T"][:3, :3] @ Tt[:3, :3].T), float(np.linalg.norm(r["T"][:3, 3] - Tt[:3, 3])))
    return out


def test_bunny_pair_restated_with_the_rules_normals(orc, golden):
    """The numbers the GPU end-to-end test's conditions rest on (tests/test_gpu_batch_normals.py quotes what this prints): the start
    pose at the test's seed inside half of 10 degrees and 1 cm, the gated loop from it inside half of 2 degrees.
    Printed: 391 correspondences, 115 of them within 1 cm of the truth; seed 1: 87 inliers, 1.718 degrees and 2.59 mm, refined to
    0.701 degrees; from the identity the loop ends 150.750 degrees away."""
    A, M, Tt, _, _ = bunny_covariances(golden)
    ref = bunny_restated(golden)
    r, rot_, trans = ref["seeds"][SEED]
    print(f"correspondences {ref['corr']}, within 1 cm of the truth {ref['good']}; seed {SEED}: inliers {r['inliers']}, rot {rot_:.3f} deg, trans {trans * 1e3:.2f} mm")
    assert r["status"] == 0
    assert rot_ < 5.0 and trans < 0.005
    start = (A.astype(np.float64) @ r["T"][:3, :3].T + r["T"][:3, 3]).astype(A.dtype)
    w = reference_loop(orc, start, M, keep_within(GATE), 40, 1e-6)
    end = fr.angle_deg((w["T"] @ r["T"])[:3, :3] @ Tt[:3, :3].T)
    cold = reference_loop(orc, A, M, keep_within(GATE), 40, 1e-6)
    away = fr.angle_deg(cold["T"][:3, :3] @ Tt[:3, :3].T) if cold["kept"][-1] else 180.0
    print(f"refined {end:.3f} deg; from the identity {away:.3f} deg")
    assert end < 1.0 and away > 30.0
