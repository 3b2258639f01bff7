"""CPU: the numpy restatement of the generalized metric (tests/batch_gicp_ref.py) on its own -- the covariance rule by hand, its
edge cases, the terms against the plane pass's, and the reference loop on a known motion."""
import numpy as np

import batch_gicp_ref as gr
import batch_outlier_ref as orf
import batch_ref
import ref_moments as rm


def test_lattice_point_by_hand():
    """the centre of a 3 x 3 x 3 lattice of step 0.5 with k = 6: the 6th nearest other point is a face neighbour at d2 = 0.25, so
    the neighbourhood is the centre and its 6 face neighbours, c = 7; s = 0, S_aa = 2 * 0.25 = 0.5, S_ab = 0: C = (0.5 / 7) I
    exactly; frobenius: f = sqrt(3) * 0.5 / 7.  k = 7 reaches into the 12 edge neighbours at d2 = 0.5, all tied: c = 19, S_aa =
    0.5 + 8 * 0.25 = 2.5"""
    for dtype in (np.float32, np.float64):
        X = orf.lattice(dtype, side=3, step=0.5)
        C, cnt = gr.covariances(X, 6, gr.COV_NONE, rows=[13])
        assert cnt[0] == 7 and C[0].tolist() == [0.5 / 7, 0.0, 0.0, 0.5 / 7, 0.0, 0.5 / 7]
        C, cnt = gr.covariances(X, 7, gr.COV_NONE, rows=[13])
        assert cnt[0] == 19 and C[0].tolist() == [2.5 / 19, 0.0, 0.0, 2.5 / 19, 0.0, 2.5 / 19]
        Cf, _ = gr.covariances(X, 6, gr.COV_FROBENIUS, 1e-3, rows=[13])
        v = np.float64(0.5) / 7
        f = np.sqrt(((v * v + v * v) + v * v) + 2.0 * 0.0)
        assert Cf[0].tolist() == [v / f + 1e-3, 0.0, 0.0, v / f + 1e-3, 0.0, v / f + 1e-3]
        # a corner: its 3 edge neighbours, then 3 face diagonals -- k = 3 keeps 4 points, one-sided: s != 0
        C, cnt = gr.covariances(X, 3, gr.COV_NONE, rows=[0])
        assert cnt[0] == 4 and C[0].tolist() == [(0.25 - 0.25 / 4) / 4, (0.0 - 0.25 / 4) / 4, (0.0 - 0.25 / 4) / 4,
                                                 (0.25 - 0.25 / 4) / 4, (0.0 - 0.25 / 4) / 4, (0.25 - 0.25 / 4) / 4]


def test_coincident_points_give_lambda_identity():
    X = orf.coincident(np.float32)   # points 100 .. 139 coincide: tau = 0 for k <= 39, every difference is 0
    C, cnt = gr.covariances(X, 8, gr.COV_FROBENIUS, 0.25, rows=[100, 139])
    assert (cnt == 40).all() and (C == np.array([0.25, 0, 0, 0.25, 0, 0.25])).all()
    assert not np.signbit(C).any()
    C, _ = gr.covariances(X, 8, gr.COV_NONE, rows=[100])
    assert (C == 0.0).all() and not np.signbit(C).any()


def test_far_cloud_loses_nothing():
    """a cloud carried 1e4 from the origin in fp32: the rule takes differences against the query, so the covariance is the one of
    the SAME stored points moved back exactly -- a power-of-two shift would be exact; here the test states it directly: the
    result equals the covariance formed from e = x_j - x_i in double, and is far from what a mean-of-products formula gives"""
    X = orf.far(np.float32)
    k = 10
    C, cnt = gr.covariances(X, k, gr.COV_NONE)
    X64 = X.astype(np.float64)
    for i in (0, 17, X.shape[0] - 1):
        d = orf.d2_rows(X, i, i + 1)[0]
        o = d.copy()
        o[i] = np.inf
        tau = np.sort(o)[k - 1]
        nb = np.flatnonzero(d <= tau)
        assert nb.size == cnt[i] and i in nb
        e = X64[nb] - X64[i]
        want = np.cov(e.T, bias=True)
        got = gr.full(C[i:i + 1])[0]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.linalg.eigvalsh(got).min() >= -1e-18
    # k + 1 points: one neighbourhood, the whole cloud, for every point
    Y = X[:k + 1]
    C, cnt = gr.covariances(Y, k, gr.COV_NONE)
    assert (cnt == k + 1).all()
    want = np.cov(Y.astype(np.float64).T, bias=True)
    assert np.abs(gr.full(C) - want[None]).max() <= 1e-9 * np.abs(want).max()


def test_rank_one_information_gives_the_plane_terms():
    """with M = n n^T in place of adj(S) / det the statements are a plane pass's: the terms from a covariance pair whose S^-1 is
    nearly n n^T / eps agree with ref_moments' plane terms times 1 / eps to the order of eps; and directly, the algebra on M"""
    rng = np.random.default_rng(5)
    n = 200
    P = rng.standard_normal((n, 3))
    M = P + 0.01 * rng.standard_normal((n, 3))
    N = rng.standard_normal((n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    idx = rng.permutation(n)
    want = rm.plane_point_terms(P, M, N, idx)
    # S = Cq + R Cp R^T with Cp = 0 and Cq = I - (1 - eps) n n^T: S^-1 = I + (1 / eps - 1) n n^T
    eps = 1e-9
    t, valid, Minv = gr.terms(P, M, idx, np.zeros((n, 6)), gr.from_normals(N, eps), np.eye(3))
    assert valid.all()
    Ni = N[idx]
    assert np.abs(Minv * eps - np.einsum("na,nb->nab", Ni, Ni)).max() < 1e-6
    for s in rm.PLANE_SLOTS:
        scale = np.abs(want[:, s]).max()
        assert np.abs(t[:, s] * eps - want[:, s]).max() < 1e-5 * max(scale, 1.0), s
    # signs and slots, independently of any inverse: J^T M J and -J^T M e by matrices
    t, valid, Minv = gr.terms(P, M, idx, gr.from_normals(N, 0.1), gr.from_normals(N, 0.3), batch_ref.rot("z", 0.3))
    for i in (0, 57, 199):
        p, e = P[i], P[i] - M[idx[i]]
        J = np.concatenate([np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]).T, np.eye(3)], axis=1)   # 3 x 6: columns j_a
        R = batch_ref.rot("z", 0.3)
        S = gr.full(gr.from_normals(N, 0.3))[idx[i]] + R @ gr.full(gr.from_normals(N, 0.1))[i] @ R.T
        Mi = np.linalg.inv(S)
        assert np.abs(Minv[i] - Mi).max() < 1e-9
        H, g = J.T @ Mi @ J, -J.T @ Mi @ e
        o = rm.MC
        for a in range(6):
            for c in range(a, 6):
                assert abs(t[i, o] - H[a, c]) < 1e-9 * max(1.0, abs(H[a, c]))
                o += 1
        assert np.abs(t[i, rm.MB:rm.MB + 6] - g).max() < 1e-9


def test_singular_sum_is_not_valid():
    """raw covariances of a planar cloud on both sides, unrotated: S has an exact zero row and column, det == 0"""
    P = np.zeros((10, 3))
    P[:, :2] = np.random.default_rng(2).standard_normal((10, 2))
    Cz = np.zeros((10, 6))
    Cz[:, 0] = Cz[:, 3] = 1.0
    t, valid, _ = gr.terms(P, P, np.arange(10), Cz, Cz, np.eye(3))
    assert not valid.any()


def test_reference_loop_recovers_a_known_motion(orc):
    """a non-planar sheet moved by a small rigid motion, the model the moved copy of the same points: the loop's T is that motion
    to batch_ref.TOL_T, from estimated covariances (k = 12) and from covariances made of normals"""
    A = gr.surface(9, 400, np.float64)
    T = batch_ref.hom(batch_ref.rot("z", 0.04) @ batch_ref.rot("x", -0.03), np.array([0.03, -0.02, 0.025]))
    M = np.ascontiguousarray(A @ T[:3, :3].T + T[:3, 3])
    Cp, _ = gr.covariances(A, 12)
    Cq, _ = gr.covariances(M, 12)
    res = gr.gicp_loop(orc, A, M, Cp, Cq, 50, 1e-12)
    assert not res["empty"] and batch_ref.rel(res["T"], T) < batch_ref.TOL_T, batch_ref.rel(res["T"], T)
    assert res["err"][-1] < 1e-6 and (res["idx"] == np.arange(400)).all()
    nrm = np.stack([-0.6 * np.cos(2 * A[:, 0]) - 0.1 * A[:, 1], 0.6 * np.sin(3 * A[:, 1]) - 0.1 * A[:, 0], np.ones(400)], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    res = gr.gicp_loop(orc, A, M, gr.from_normals(nrm), gr.from_normals(nrm @ T[:3, :3].T), 50, 1e-12)
    assert batch_ref.rel(res["T"], T) < batch_ref.TOL_T
