"""CPU: the numpy restatement of the ISS keypoint rule (tests/batch_keypoint_ref.py) -- its Jacobi against icp_eigh3 bit for bit and
against LAPACK, the properties of the selection, ties on both radii, and the dense bunny pair end to end, whose printed counts and
errors are what the conditions of the GPU end-to-end test rest on."""
import numpy as np
import pytest

import batch_feature_ref as fr
import batch_keypoint_ref as kr
import batch_outlier_ref as orf

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def sym6(A):
    """(k, 3, 3) symmetric -> (6, k): xx, xy, xz, yy, yz, zz"""
    return np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]])


def matrices():
    rng = np.random.default_rng(11)
    R = rng.standard_normal((40, 3, 3))
    random = R + R.transpose(0, 2, 1)
    diagonal = np.stack([np.diag(rng.standard_normal(3)) for _ in range(8)])
    v = rng.standard_normal((8, 3))
    rank1 = v[:, :, None] * v[:, None, :]
    psd = R @ R.transpose(0, 2, 1)                                # what a covariance looks like
    near = psd + 1e-9 * random                                    # many sweeps' worth of off-diagonal mass
    return dict(random=random, diagonal=diagonal, rank1=rank1, zero=np.zeros((2, 3, 3)), psd=psd, near=near,
                tiny=random * 1e-300, huge=random * 1e150, tiny_psd=psd * 1e-300, huge_psd=psd * 1e150)


def test_jacobi_equals_icp_eigh3_bit_for_bit(pkg):
    for name, A in matrices().items():
        w = kr.jacobi_eigenvalues(sym6(A))
        for k in range(A.shape[0]):
            want, _ = pkg.eigh3(A[k])
            got = np.ascontiguousarray(w[:, k])
            assert np.array_equal(got.view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64)), (name, k, got, want)


def test_jacobi_agrees_with_lapack():
    M = matrices()
    for name in ("random", "diagonal", "rank1", "zero", "psd", "near"):
        A = M[name]
        w = kr.jacobi_eigenvalues(sym6(A)).T
        ref = np.linalg.eigvalsh(A)
        # 1e-12 of the trace; an indefinite matrix, whose trace may be near 0, is measured against the trace of |A|, sum |lambda|
        scale = np.trace(A, axis1=1, axis2=2) if name in ("rank1", "zero", "psd", "near") else np.abs(ref).sum(axis=1)
        assert (np.abs(w - ref).max(axis=1) <= 1e-12 * scale).all(), name
        assert (np.diff(w, axis=1) >= 0).all(), name


def bumpy(n, dtype, seed=5):
    return fr.blob(seed, n, dtype)[0]


def test_no_two_keypoints_within_the_non_max_radius_unless_equal():
    X = bumpy(700, np.float32)
    r = kr.rule(0.35, 0.3, 0.975, 0.975, 5)
    keep, sal = kr.select(X, r)
    assert 3 <= keep.sum() < (sal > 0).sum()                      # the suppression removed candidates and left keypoints
    near = kr.within(X, r[1])
    k = np.flatnonzero(keep)
    for i in k:
        for j in k[near[i, k]]:
            assert sal[i] == sal[j], (i, j)
    # coincident points have bit-equal saliency and keep each other
    Y = np.concatenate([X, X[k[:2]]])
    keep2, sal2 = kr.select(Y, r)
    for a, i in enumerate(k[:2]):
        assert sal2[700 + a] == sal2[i] and keep2[700 + a] == keep2[i]


@DTYPES
def test_a_planar_lattice_has_no_keypoint(dtype):
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.5
    X = np.ascontiguousarray(np.concatenate([g, np.zeros((g.shape[0], 1))], axis=1).astype(dtype))
    keep, sal = kr.select(X, kr.rule(1.1, 0.8, 0.975, 0.975, 3))
    assert (sal == 0.0).all() and not keep.any()                  # w0 == 0 everywhere: exactly 0.0, never a keypoint


def test_min_neighbours_above_the_densest_neighbourhood_empties_the_set():
    X = bumpy(300, np.float32)
    r = kr.rule(0.4, 0.3, 0.975, 0.975, 5)
    assert kr.select(X, r)[0].any()
    densest = int(kr.within(X, r[0]).sum(axis=1).max())
    keep, sal = kr.select(X, r[:4] + (densest + 1,))
    assert (sal == 0.0).all() and not keep.any()
    keep, sal = kr.select(X, r[:4] + (densest,))
    assert (sal > 0).sum() <= int((kr.within(X, r[0]).sum(axis=1) == densest).sum())


@DTYPES
def test_a_point_exactly_on_either_radius_counts(dtype):
    """the integer lattice 5 x 5 x 5: every d2 is exact, and 4 and 1 are lattice distances -- six points lie exactly on a radius of
    2 about the centre and six on a radius of 1.  Gammas of 2 let the symmetric lattice (eigenvalue ratios of 1) pass the ratio tests."""
    X = orf.lattice(dtype, side=5, step=1.0)
    centre = int(np.flatnonzero((X == 2).all(axis=1))[0])
    below = lambda r: float(np.nextafter(np.float64(r), 0.0)) if dtype == np.float64 else float(np.nextafter(np.float32(r), np.float32(0.0))) * (1 - 1e-9)
    d = orf.d2_rows(X, centre, centre + 1)[0]
    # the salient radius: 33 lattice points within 2 of the centre, 6 of them at exactly 2
    assert (d == 4).sum() == 6 and kr.within(X, 2.0)[centre].sum() == 33 and kr.within(X, 2.0)[centre][d == 4].all()
    assert kr.within(X, below(2.0))[centre].sum() == 27
    assert kr.saliency(X, kr.rule(2.0, 1.0, 2.0, 2.0, 33))[centre] > 0
    assert kr.saliency(X, kr.rule(2.0, 1.0, 2.0, 2.0, 34))[centre] == 0.0
    assert kr.saliency(X, kr.rule(below(2.0), 1.0, 2.0, 2.0, 27))[centre] > 0
    assert kr.saliency(X, kr.rule(below(2.0), 1.0, 2.0, 2.0, 28))[centre] == 0.0
    # the non-max radius: |M_centre| = 7 at 1, six of them exactly on it
    sal = np.random.default_rng(3).uniform(1.0, 2.0, 125)
    sal[centre] = 3.0
    assert kr.select(X, kr.rule(2.0, 1.0, 2.0, 2.0, 7), sal=sal)[0][centre]
    assert not kr.select(X, kr.rule(2.0, 1.0, 2.0, 2.0, 8), sal=sal)[0][centre]
    # a higher saliency exactly on the radius suppresses; a hair inside the radius it does not; an equal one never does
    on = int(np.flatnonzero((X == (3, 2, 2)).all(axis=1))[0])
    sal[on] = 4.0
    assert not kr.select(X, kr.rule(2.0, 1.0, 2.0, 2.0, 1), sal=sal)[0][centre]
    assert kr.select(X, kr.rule(2.0, below(1.0), 2.0, 2.0, 1), sal=sal)[0][centre]
    sal[on] = 3.0
    keep = kr.select(X, kr.rule(2.0, 1.0, 2.0, 2.0, 1), sal=sal)[0]
    assert keep[centre] and keep[on]


def dense_bunny_reference(golden):
    """the whole restatement on the dense bunny pair: dict of the keypoint maps, their counts, the descriptors of the kept points,
    the mutual matches among them and the RANSAC result at seed 1.  Computed once per session."""
    if "ref" in _DENSE:
        return _DENSE["ref"]
    A, M, Tt = kr.dense_bunny_pair(golden)
    K, H, MD, SEED = 24, 2000, 0.0075, 1
    out = dict(A=A, M=M, Tt=Tt)
    feats, kept = [], kr.dense_bunny_keypoints(golden)
    for X in (A, M):
        d, tau, _ = fr.neighbourhood(X, K)
        _, C = kr.covariances(X, d <= tau[:, None])              # the covariance rule's neighbourhood and sums, ICP_COV_NONE
        N = fr.oriented_normals(X, np.ascontiguousarray(C.T), X.astype(np.float64).mean(0))
        feats.append(fr.fpfh(X, N, K))
    (YA, mapA, salA), (YM, mapM, salM) = kept
    FA, FM = feats[0][mapA >= 0], feats[1][mapM >= 0]
    fwd, rev, keep = fr.match(FA, FM, True)
    ci, cj = fr.correspondences(fwd, keep)
    res = fr.ransac(YA, YM, ci, cj, SEED, H, MD, 0.9)
    moved = YA[ci].astype(np.float64) @ Tt[:3, :3].T + Tt[:3, 3]
    good = int((np.linalg.norm(moved - YM[cj].astype(np.float64), axis=1) < 0.01).sum())
    out.update(YA=YA, YM=YM, mapA=mapA, mapM=mapM, salA=salA, salM=salM, FA=FA, FM=FM, fwd=fwd, rev=rev, keep=keep, ransac=res, good=good,
               rot=fr.angle_deg(res["T"][:3, :3] @ Tt[:3, :3].T), trans=float(np.linalg.norm(res["T"][:3, 3] - Tt[:3, 3])))
    _DENSE["ref"] = out
    return out


_DENSE = {}


def test_dense_bunny_pair_restated(golden):
    """The numbers the GPU end-to-end test's conditions rest on (tests/test_gpu_batch_keypoint.py quotes what this prints)."""
    ref = dense_bunny_reference(golden)
    print(f"points {ref['A'].shape[0]} / {ref['M'].shape[0]}, keypoints {ref['YA'].shape[0]} / {ref['YM'].shape[0]}, "
          f"mutual matches {int(ref['keep'].sum())}, within 1 cm of the truth {ref['good']}, seed 1: inliers {ref['ransac']['inliers']}, "
          f"rot {ref['rot']:.3f} deg, trans {ref['trans'] * 1e3:.2f} mm")
    assert ref["A"].shape[0] == 5992 and ref["M"].shape[0] == 5991
    assert 300 <= ref["YA"].shape[0] <= 600 and 300 <= ref["YM"].shape[0] <= 600   # "a few hundred salient points"
    assert ref["ransac"]["status"] == 0
    assert ref["rot"] < 2.5 and ref["trans"] < 0.0075              # a factor of two inside the GPU test's 5 degrees and 1.5 cm
