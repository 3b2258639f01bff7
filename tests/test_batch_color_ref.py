"""CPU: the numpy restatement of the colored metric (tests/batch_color_ref.py) on its own -- the gradient rule on a field whose
gradient is known, its fallback, the terms against the plane pass's, and the reference loop on the textured surfaces geometry
alone cannot register."""
import numpy as np

import batch_color_ref as cr
import batch_outlier_ref as orf
import batch_ref
import ref_moments as rm


def test_linear_field_on_a_plane_gives_its_tangential_gradient():
    """points of a tilted plane, I = I0 + a . x: every difference g = a . e = a_t . u in real arithmetic (e lies in the plane), so
    the least-squares fit returns a_t = a - (a . n) n, the part of a across the normal, whatever the neighbourhood.  The fit's
    rounding error is about cond(A) u |a|; on a lattice of step 0.5 the tangential part of A is at least 2 * 0.25 per direction
    (a corner's two edge neighbours) against c^2 <= 24^2 along the normal, cond(A) < 2e3, so 1e-12 leaves a factor of ten"""
    nrm = np.array([0.3, -0.2, 0.9])
    nrm /= np.linalg.norm(nrm)
    b1 = np.cross(nrm, [1.0, 0.0, 0.0])
    b1 /= np.linalg.norm(b1)
    b2 = np.cross(nrm, b1)
    uv = np.stack(np.meshgrid(np.arange(15), np.arange(15), indexing="ij"), -1).reshape(-1, 2) * 0.5
    X = np.ascontiguousarray(uv[:, :1] * b1 + uv[:, 1:] * b2 + np.array([0.5, -0.25, 2.0]))
    a = np.array([0.7, -1.1, 0.4])
    I = 0.3 + X @ a
    N = np.tile(nrm, (X.shape[0], 1))
    want = a - (a @ nrm) * nrm
    for k in (3, 8, 20):
        D, cnt = cr.gradients(X, N, I, k)
        assert (cnt >= k).all() and cnt.max() <= 24
        print(f"[color ref] linear field, k {k}: max |d - a_t| = {np.abs(D - want).max():.3e}")
        assert np.abs(D - want).max() < 1e-12, (k, np.abs(D - want).max())
        assert np.abs(D @ nrm).max() < 1e-12   # no part along the normal


def test_duplicates_give_exact_zeros():
    """40 coincident points: tau = 0, every e is 0, A = c^2 n n^T has rank one, det is not > 0 -- (0, 0, 0) exactly; and a cloud
    that is one point throughout"""
    X = orf.coincident(np.float32)
    rng = np.random.default_rng(8)
    N = rng.standard_normal(X.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    I = rng.uniform(0, 1, X.shape[0])
    D, cnt = cr.gradients(X, N, I, 8, rows=np.arange(100, 140))
    assert (cnt == 39).all() and (D == 0.0).all()
    Y = np.tile(np.array([[1.5, -2.0, 0.25]]), (12, 1))
    D, cnt = cr.gradients(Y, N[:12].astype(np.float64), I[:12], 5)
    assert (cnt == 11).all() and (D == 0.0).all() and D.shape == (12, 3)


def test_lambda_one_gives_the_plane_terms_byte_for_byte():
    rng = np.random.default_rng(5)
    n = 200
    P = rng.standard_normal((n, 3))
    M = P + 0.01 * rng.standard_normal((n, 3))
    N = rng.standard_normal((n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    idx = rng.permutation(n)
    want = rm.plane_point_terms(P, M, N, idx)
    got = cr.terms(P, M, N, idx, rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.standard_normal((n, 3)), 1.0)
    for s in (rm.CNT,) + rm.PLANE_SLOTS:
        assert got[:, s].tobytes() == want[:, s].tobytes(), s
    # and with another lambda: J^T (lg n n^T + lp m m^T) J and -J^T (lg n h + lp m rI), by matrices
    Ip, Iq, D, lam = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.standard_normal((n, 3)), 0.75
    got = cr.terms(P, M, N, idx, Ip, Iq, D, lam)
    for i in (0, 57, 199):
        p, q, nn, d = P[i], M[idx[i]], N[idx[i]], D[idx[i]]
        J = np.concatenate([np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]).T, np.eye(3)], axis=1)   # 3 x 6: columns j_a
        e = p - q
        h = e @ nn
        m = d - (d @ nn) * nn
        rI = Iq[idx[i]] + d @ (e - h * nn) - Ip[i]
        H = J.T @ (lam * np.outer(nn, nn) + (1 - lam) * np.outer(m, m)) @ J
        g = -J.T @ (lam * nn * h + (1 - lam) * m * rI)
        o = rm.MC
        for a in range(6):
            for c in range(a, 6):
                assert abs(got[i, o] - H[a, c]) < 1e-12 * max(1.0, abs(H[a, c]))
                o += 1
        assert np.abs(got[i, rm.MB:rm.MB + 6] - g).max() < 1e-12


def run_textured(orc, c, lam):
    pair = cr.textured(c)
    D, _ = cr.gradients(pair["M"], pair["N"], pair["Iq"], cr.K_TEX)
    res = cr.color_loop(orc, pair["A"], pair["M"], pair["N"], pair["Ip"], pair["Iq"], D, lam, cr.ITER_TEX, 0.0,
                        keep=batch_ref.keep_within(cr.GATE_TEX))
    return pair, res


def test_recovery_on_a_flat_and_on_a_curved_textured_surface(orc):
    """the flat plane z = 0 with exact normals: point-to-plane's system has three exact zero columns (it cannot start); the colored
    loop ends with a pose error below one tenth of its start.  The gently curved z = 0.05 (x^2 - y^2): point-to-plane slides
    along the surface, the colored loop ends below one fifth of its end error"""
    flat, res = run_textured(orc, 0.0, cr.LAMBDA_DEFAULT)
    start, end = cr.pose_error(np.eye(4), flat), cr.pose_error(res["T"], flat)
    print(f"[color ref] flat: start {start:.3e} end {end:.3e} ratio {end / start:.4f} (bound 0.1)")
    assert not res["empty"] and not res["singular"] and 0.02 < start < 0.05
    assert end < 0.1 * start
    _, plane = run_textured(orc, 0.0, 1.0)
    assert plane["singular"] or not np.isfinite(plane["T"]).all() or cr.pose_error(plane["T"], flat) > 0.5 * start

    curved, res = run_textured(orc, 0.05, cr.LAMBDA_DEFAULT)
    _, plane = run_textured(orc, 0.05, 1.0)
    e_col, e_pl = cr.pose_error(res["T"], curved), cr.pose_error(plane["T"], curved)
    print(f"[color ref] curved: start {cr.pose_error(np.eye(4), curved):.3e} colored {e_col:.3e} plane {e_pl:.3e} ratio {e_col / e_pl:.4f} (bound 0.2)")
    assert not res["empty"] and not res["singular"] and not plane["singular"]
    assert e_col < 0.2 * e_pl
    _, half = run_textured(orc, 0.05, 0.5)
    print(f"[color ref] curved, lambda 0.5: {cr.pose_error(half['T'], curved):.3e}")
    assert cr.pose_error(half["T"], curved) < 0.2 * e_pl
