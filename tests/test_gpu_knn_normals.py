"""GPU: the point-to-plane front end -- the 4-neighbour search and the PCA normals, single pair and batched, both precisions -- held
to the rule of include/icp_mi355x.h (icp_estimate_normals) as tests/knn_ref.py states it in numpy, across the float range: squared
distances that are all zero, subnormal, past the fp32 oracle's sentinel of 10000, near the top of the range, partly +inf and all
+inf; model sizes at every launch shape of knn4_f32_v2 (one and two query blocks; one, two, three, nine and eleven model segments;
a second LDS tile per wave); exact ties across every border at which two of its lists are merged.  What the clouds are is shown on
the CPU in tests/test_knn_ref.py.

A rank that does not exist holds index 0 (knn4_merge_kernel used to pass knn4_f32_v2's 0x7fffffff on, and normals_kernel read the
model at that index), and a covariance that is not finite gives the normal (+0, +0, +0) (pca_normal used to store NaNs)."""
import numpy as np
import pytest

import knn_ref as kr
from test_gpu_plane_and_programs import _clouds, assert_same_plane_run, rel

pytestmark = pytest.mark.gpu


def front_end(ctx, Q):
    ctx.set_model(Q)
    nrm, nbr = ctx.estimate_normals(want_neighbours=True)
    assert nbr.shape == (Q.shape[0], 4) and nbr.dtype == np.int32 and nrm.shape == Q.shape and nrm.dtype == Q.dtype
    return nrm, nbr


def assert_rule(nbr, Q, name):
    assert nbr.min() >= 0 and nbr.max() < Q.shape[0], (name, int(nbr.min()), int(nbr.max()))
    want = kr.rule(Q)[0]
    assert nbr.tobytes() == want.tobytes(), (name, "rows that differ:", np.flatnonzero((nbr != want).any(axis=1))[:8].tolist())


# 1 ----------------------------------------------------------------------------------------------------------------------------
def test_fp32_neighbours_sizes_and_borders(ctx):
    geom = {m: tuple(ctx.diag_knn4_geometry(m)[k] for k in ("n_pad", "blocks_x", "splits", "seg_len", "tiles")) for m in kr.SIZED_M}
    assert geom == kr.GEOMETRY_256, geom                       # (an MI355X has 256 CUs)
    assert [geom[m][1] for m in kr.SIZED_M[:4]] == [1, 1, 1, 2] and {1, 2, 3, 9} <= {g[2] for g in geom.values()}
    assert geom[12001][4] == 2 and all(geom[m][4] == 1 for m in kr.SIZED_M[:-1])
    for m in kr.SIZED_M:
        Q = kr.sized(m)
        assert_rule(front_end(ctx, Q)[1], Q, f"sized({m})")
    for m in kr.TWIN_M:
        Q, triples = kr.border_twins(m, geom[m])
        nbr = front_end(ctx, Q)[1]
        assert_rule(nbr, Q, f"border_twins({m})")
        for third, lo, hi in triples:                          # (what the equality says at the borders, spelled out)
            assert tuple(nbr[third, :2]) == tuple(nbr[lo, :2]) == tuple(nbr[hi, :2]) == (lo, hi)   # (rank 0, dropped: the third copy)
    Q = kr.coincident(300)
    nbr = front_end(ctx, Q)[1]
    assert_rule(nbr, Q, "coincident(300)")
    assert (nbr[5:] == np.array([1, 2, 3, 4])).all()


# 2, 3 -------------------------------------------------------------------------------------------------------------------------
def test_fp32_neighbours_over_the_range(ctx):
    for name, Q in kr.scale_clouds(np.float32):
        nbr = front_end(ctx, Q)[1]
        assert_rule(nbr, Q, name)
        if name.startswith("apart"):
            assert (nbr == 0).all()


def test_fp64_neighbours_over_the_range(ctx, orc):
    for name, Q in kr.scale_clouds(np.float64):
        nbr = front_end(ctx, Q)[1]
        assert_rule(nbr, Q, name)
        assert np.array_equal(nbr, orc.knn4(Q)), name
        if name.startswith("apart"):
            assert (nbr == 0).all()


# 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_neighbours_and_normals_over_the_range(ctx, dtype):
    """one batch holds every scale cloud of the dtype, and brink(), as a model: the neighbours are the rule's, and neighbours and
    normals are icp_estimate_normals' on each model alone, bit for bit (the contract of test_gpu_batch_plane.py, at the ends of the
    range)"""
    clouds = kr.scale_clouds(dtype) + [("brink-5", kr.brink(dtype))]
    D = np.zeros((1, 3), dtype=dtype)
    with ctx.batch([(D, Q) for _, Q in clouds]) as bt:
        nrm, nbr = bt.estimate_normals(want_neighbours=True)
    for k, (name, Q) in enumerate(clouds):
        assert nbr[k].shape == (Q.shape[0], 4) and nbr[k].dtype == np.int32
        assert_rule(nbr[k], Q, name)
        one_nrm, one_nbr = front_end(ctx, Q)
        assert nbr[k].tobytes() == one_nbr.tobytes(), name
        assert nrm[k].dtype == one_nrm.dtype and nrm[k].shape == one_nrm.shape and nrm[k].tobytes() == one_nrm.tobytes(), name


# 5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_normals_over_the_range(ctx, orc, dtype):
    """knn_ref.check_normals on every cloud: exact zeros where the covariance is not finite, no NaN anywhere, and everywhere else the
    gates of test_normals_match_oracle_up_to_sign on the covariance divided by its largest entry"""
    seen_nonfinite = 0
    for name, Q in kr.normals_clouds(dtype):
        nrm, nbr = front_end(ctx, Q)
        assert_rule(nbr, Q, name)
        A, finite = kr.covariance_rule(Q, nbr)
        try:
            ok = kr.check_normals(nrm, A, finite, Q, nbr, orc)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
        seen_nonfinite += int((~finite).sum())
        if name in kr.NORMAL_DEFINED_MIN[dtype]:
            assert ok.mean() >= kr.NORMAL_DEFINED_MIN[dtype][name], (name, ok.mean())
    assert seen_nonfinite >= 10


# 6 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grid", "random"])
def test_point_to_plane_past_the_sentinel(ctx, pkg, orc, golden, which):
    """the 40 x 40 grid and the 1500 normal points, times 1000 in double and rounded once: every neighbourhood lies past the fp32
    oracle's sentinel, so the normals come from the oracle's eigen-solve on the rule's neighbours.  The error is a length: its gate
    and the stop threshold are the ones of test_point_to_plane_loop times 1000; the transform's relative gate is unchanged."""
    D, M = ((1000.0 * X.astype(np.float64)).astype(np.float32) for X in _clouds(pkg, golden, which))
    nbr, d5 = kr.rule(M)
    assert (d5[:, 4] >= kr.SENTINEL).mean() >= 0.5
    normals = orc.normals(M, nbr)[0]
    res = ctx.point_to_plane(D, M, normals=normals, max_iter=50, tol=1e-3)
    want = orc.icp_p2plane_f32x(D, M, normals, 50, 1e-3)
    assert_same_plane_run(res, want, 1e-3, length=1000.0)
    assert res.err[-1] < 0.5 * res.err[1]
    res2 = ctx.point_to_plane(D, M, normals=None, max_iter=50, tol=1e-3)
    assert rel(res2.T, res.T) < 5e-3


# 7 ----------------------------------------------------------------------------------------------------------------------------
def test_point_to_plane_with_unusable_normals_is_reported(ctx, pkg, orc):
    """a float32 model whose points are all +inf apart and normals=None: no rank exists, every neighbour is point 0, every
    covariance is exactly zero -- finite, so by the rule the normal is not (0, 0, 0) but the eigen-solve's answer to a zero matrix,
    the first axis -- and with all normals parallel the first pivot of the 6 x 6 system is zero -> ICP_ERR_SINGULAR, as
    test_point_to_plane_degenerate_is_reported expects for its case; and the context goes on working"""
    M = kr.apart(300, np.float32)
    nrm, nbr = front_end(ctx, M)
    assert (nbr == 0).all() and nrm.tobytes() == np.tile(np.array([[1, 0, 0]], dtype=np.float32), (300, 1)).tobytes()
    with pytest.raises(pkg.IcpError) as e:
        ctx.point_to_plane(M[::3].copy(), M, normals=None, max_iter=3)
    assert e.value.code == pkg.capi.ICP_ERR_SINGULAR
    D = pkg.datasets.synthetic_grid(16, np.float32)
    Q = pkg.datasets.make_model_gpu(D, *pkg.datasets.P2P_GPU)
    res = ctx.point_to_plane(D, Q, normals=None, max_iter=50, tol=1e-6)
    want = orc.icp_p2plane_f32x(D, Q, orc.normals(Q, orc.knn4(Q))[0], 50, 1e-6)
    assert rel(res.T, want["T"]) < 5e-3 and res.err[-1] < 0.5 * res.err[1]
