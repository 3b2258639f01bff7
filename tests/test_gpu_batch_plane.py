"""GPU: batched point-to-plane ICP (icp_batch_set_model_normals, icp_batch_estimate_normals, icp_point_to_plane_batch;
Batch.set_model_normals / estimate_normals / begin(metric=...), Context.point_to_plane_batch).

The neighbours and normals of every pair's model must be those of icp_estimate_normals on that model alone (and the oracle's
neighbours), bit for bit; every pair's loop must be the loop icp_point_to_plane runs for it alone: held to the CPU oracle with
the gates of test_gpu_plane_and_programs.py (err 1e-5 absolute, T and the moved cloud 1e-5 relative, idx equal, equal iteration
counts where the oracle's own stop decisions sit far from the threshold), every pass's moment vector to the exact plane sums
(ref_moments.py) at the derived bound, and with bits that do not depend on the other pairs of the batch.
"""
import ctypes as C

import numpy as np
import pytest

import clouds as cl
import ref_moments as rm
from batch_ref import TOL_E, TOL_T, degenerate_pair, five_pairs, fp32_pairs, knn_models, oracle_normals, rel, same_result_bits

pytestmark = pytest.mark.gpu


def handle_results(bt, pkg, **begin):
    """a whole registration on a Batch handle, per pair as Context.point_to_plane_batch reports it"""
    bt.begin(**begin)
    while bt.run(1000)[1]:
        pass
    idx, moved = bt.loop_indices(), bt.get_moving()
    out = []
    for b in range(bt.count):
        st = bt.state(b)
        out.append(pkg.Result(T=st["T"].copy(), iterations=st["iterations"], passes=st["passes"], err=st["err"], idx=idx[b], moved=moved[b],
                              extra={"status": st["status"]}))
    return out


# 1 (model sizes around the kernels' granules: batch_ref.KNN_M) -------------------------------------------------------------
def check_normals_against_single(ctx, models, got_nrm, got_nbr, orc=None):
    for k, M in enumerate(models):
        ctx.set_model(M)
        nrm, nbr = ctx.estimate_normals(want_neighbours=True)
        assert got_nbr[k].shape == (M.shape[0], 4) and got_nbr[k].dtype == np.int32
        assert np.array_equal(got_nbr[k], nbr), f"model {k} (m={M.shape[0]}): neighbours differ from icp_estimate_normals"
        if orc is not None:
            assert np.array_equal(got_nbr[k], orc.knn4(M)), f"model {k} (m={M.shape[0]}): neighbours differ from the oracle"
        assert got_nrm[k].dtype == nrm.dtype and got_nrm[k].shape == nrm.shape
        assert got_nrm[k].tobytes() == nrm.tobytes(), f"model {k} (m={M.shape[0]}): normals differ in their bits from icp_estimate_normals"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_neighbours_and_normals_ragged(ctx, pkg, orc, dtype):
    models = knn_models(dtype)
    D = np.zeros((1, 3), dtype=dtype)
    with ctx.batch([(D, M) for M in models]) as bt:
        nrm, nbr = bt.estimate_normals(want_neighbours=True)
        only = bt.estimate_normals()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(nrm, only))
    check_normals_against_single(ctx, models, nrm, nbr, orc)   # (the oracle's kNN follows the dtype: orc_knn4_f32 / orc_knn4_f64)


def test_batch_neighbours_and_normals_largest_model(ctx, pkg):
    M = cl.ragged_pair(77, 1, pkg.capi.ICP_BATCH_MAX_POINTS)[1]
    with ctx.batch([(np.zeros((1, 3), dtype=np.float32), M)]) as bt:
        nrm, nbr = bt.estimate_normals(want_neighbours=True)
    check_normals_against_single(ctx, [M], nrm, nbr)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_batch_plane_refusals(ctx, pkg, orc):
    lib, B = pkg.load(), pkg.capi
    PLANE = B.ICP_POINT_TO_PLANE
    pairs = [cl.ragged_pair(1, 30, 40), cl.ragged_pair(2, 10, 4), cl.ragged_pair(3, 20, 17)]
    with ctx.batch(pairs) as bt:   # a model of 4 points among good ones
        with pytest.raises(pkg.IcpError) as e:
            bt.estimate_normals()
        assert e.value.code == B.ICP_ERR_INVALID and "pair 1" in str(e.value)
        with pytest.raises(pkg.IcpError) as e:
            bt.begin(max_iter=5, metric=PLANE)
        assert e.value.code == B.ICP_ERR_INVALID
    pairs = [cl.ragged_pair(1, 30, 40), cl.ragged_pair(3, 200, 170)]
    good = [oracle_normals(orc, M) for _, M in pairs]
    with ctx.batch(pairs) as bt:
        with pytest.raises(pkg.IcpError) as e:   # no normals yet
            bt.begin(max_iter=5, metric=PLANE)
        assert e.value.code == B.ICP_ERR_INVALID
        assert lib.icp_batch_set_model_normals(bt._h, None) == B.ICP_ERR_INVALID
        bt.set_model_normals(good)
        for poison in (np.nan, np.inf):
            bad = [good[0], good[1].copy()]
            bad[1][169, 2] = poison
            with pytest.raises(pkg.IcpError) as e:
                bt.set_model_normals(bad)
            assert e.value.code == B.ICP_ERR_INVALID
        want = ctx.point_to_plane_batch(pairs, normals=good, max_iter=6, tol=0.0, fixed_iterations=True)
        got = handle_results(bt, pkg, max_iter=6, tol=0.0, fixed_iterations=True, metric=PLANE)   # the earlier set is still in force
        for a, b in zip(got, want):
            same_result_bits(a, b)
        # new normals in the middle of a loop discard it
        bt.begin(max_iter=6, tol=0.0, fixed_iterations=True, metric=PLANE)
        assert bt.run(2) == (2, 2)
        bt.set_model_normals(good)
        with pytest.raises(pkg.IcpError) as e:
            bt.run(1)
        assert e.value.code == B.ICP_ERR_STATE
        bt.begin(max_iter=6, tol=0.0, fixed_iterations=True, metric=PLANE)
        assert bt.run(2) == (2, 2)
        bt.estimate_normals()
        with pytest.raises(pkg.IcpError) as e:
            bt.run(1)
        assert e.value.code == B.ICP_ERR_STATE
    # the one-call form refuses the other metric
    D, M = pairs[0]
    moff, qoff = np.array([0, D.shape[0]], dtype=np.int64), np.array([0, M.shape[0]], dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    prm = B.icp_params(10, 1e-6, 0, pkg.ICP_F32, B.ICP_POINT_TO_POINT)
    T = np.zeros(16)
    assert lib.icp_point_to_plane_batch(ctx._h, 1, D.ctypes.data, moff.ctypes.data_as(p64), M.ctypes.data, qoff.ctypes.data_as(p64),
                                        good[0].ctypes.data, C.byref(prm), T.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None,
                                        None) == B.ICP_ERR_INVALID


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(ctx, pkg, orc, golden):
    """test 3's batch, its oracle normals and runs, and the batched result -- shared by the tests below, never modified"""
    pairs = five_pairs(pkg, golden)
    normals = [oracle_normals(orc, M) for _, M in pairs]
    wants = [orc.icp_p2plane_f32x(D, M, N, 50, 1e-5) for (D, M), N in zip(pairs, normals)]
    res = ctx.point_to_plane_batch(pairs, normals=normals, max_iter=50, tol=1e-5)
    return pairs, normals, wants, res


def test_batch_plane_each_pair_against_oracle(pkg, five):
    pairs, normals, wants, res = five
    # the oracle's own stop decisions: no E or |dE| of these runs comes within 3.6e-6 of the tolerance (and its variants agree to
    # 4.2e-7 in E), so the iteration counts must be equal
    assert [w["iterations"] for w in wants] == [2, 3, 3, 1, 5]
    assert [w["passes"] for w in wants] == [3, 4, 4, 2, 6]
    for r, w in zip(res, wants):
        assert r.extra["status"] == pkg.capi.ICP_OK
        assert r.iterations == w["iterations"] and r.passes == w["passes"]
        assert np.abs(r.err - w["err"]).max() < TOL_E
        assert rel(r.T, w["T"]) < TOL_T
        assert rel(r.moved, w["moved"]) < TOL_T
        assert np.array_equal(r.idx, w["idx"])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_batch_plane_device_estimated_normals(ctx, pkg, five):
    pairs, _, _, res = five
    with ctx.batch(pairs) as bt:
        est = bt.estimate_normals()
    a = ctx.point_to_plane_batch(pairs, normals=None, max_iter=50, tol=1e-5)
    b = ctx.point_to_plane_batch(pairs, normals=est, max_iter=50, tol=1e-5)
    for x, y, r in zip(a, b, res):
        same_result_bits(x, y)
        assert x.extra["status"] == pkg.capi.ICP_OK
        assert rel(x.T, r.T) < 5e-3   # (test_point_to_plane_loop's gate: the sign of a normal does not matter)


# 5 ------------------------------------------------------------------------------------------------------------------------
# (pairs of fewer than 6 moving points are left out on purpose: their 6 x 6 system is rank-deficient and only rounding decides
# whether Cholesky passes)
RAGGED = [(63, 17), (64, 64), (65, 130), (130, 257), (200, 9), (1025, 17), (130, 4097), (777, 16), (1000, 2049), (5000, 3000), (130, 65536)]


def test_batch_plane_ragged_pairs(ctx, pkg, orc):
    assert RAGGED[-1][1] == pkg.capi.ICP_BATCH_MAX_POINTS
    pairs = [cl.ragged_pair(n * 1000 + m, n, m) for n, m in RAGGED]
    normals = [oracle_normals(orc, M) for _, M in pairs]
    res = ctx.point_to_plane_batch(pairs, normals=normals, max_iter=4, tol=0.0, fixed_iterations=True)
    with ctx.batch(pairs) as bt:
        bt.set_model_normals(normals)
        bt.begin(max_iter=4, tol=0.0, fixed_iterations=True, metric=pkg.capi.ICP_POINT_TO_PLANE)
        while bt.run(64)[1]:
            pass
        loop_idx = bt.loop_indices()
    for r, li, (D, M), N in zip(res, loop_idx, pairs, normals):
        want = orc.icp_p2plane_f32x(D, M, N, 4, 0.0, fixed=True)
        assert want["passes"] == 4
        assert r.extra["status"] == pkg.capi.ICP_OK and r.passes == 4
        assert np.abs(r.err - want["err"]).max() < TOL_E
        assert rel(r.T, want["T"]) < TOL_T
        assert np.array_equal(r.idx, want["idx"])
        assert np.array_equal(li, r.idx)


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_plane_moments(ctx, pkg, orc, dtype):
    """every pass's vector against the exact plane sums of (P_k, Q, normals, idx_k) and of (P_k, Q, idx_{k-1}), on slots ERR, CNT
    and the 27 plane slots, within ref_moments.tolerance (no tag term: the batch has no compact rows)"""
    STEPS = 3
    cases = [(n, m) for m in cl.MODEL_M for n in cl.BATCH_N]
    pairs = [cl.case_pair(n, m, dtype) for n, m in cases]
    normals = [oracle_normals(orc, cl.case_pair(n, m)[1]).astype(dtype) for n, m in cases]   # the fp32 model's, cast
    steps_done = [0] * len(pairs)
    worst = 0.0
    with ctx.batch(pairs) as bt:
        bt.set_model_normals(normals)
        bt.begin(max_iter=STEPS + 1, tol=0.0, fixed_iterations=True, metric=pkg.capi.ICP_POINT_TO_PLANE)
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_moments(0)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        prev = [None] * len(pairs)
        for k in range(STEPS):
            running = ~bt.done()
            took, _ = bt.run(1)
            assert took == (1 if running.any() else 0)
            moving, idx = bt.get_moving(), bt.get_indices()
            for b in np.flatnonzero(running):
                P, Q, N, mom = moving[b], pairs[b][1], normals[b], bt.diag_moments(b)
                n = P.shape[0]
                idx_prev = prev[b]["idx"] if prev[b] is not None else None
                want, maj = rm.plane(P, Q, N, idx[b], P if idx_prev is not None else None, idx_prev)
                tol = rm.tolerance(maj, n)
                what = f"{np.dtype(dtype).name} n={n} m={Q.shape[0]} pass {k}"
                assert mom[rm.CNT] == float(n), f"{what}: CNT {mom[rm.CNT]!r}"
                if idx_prev is None:
                    assert mom[rm.ERR] == 0.0, f"{what}: ERR {mom[rm.ERR]!r} without a transform"
                for s in (rm.ERR, rm.CNT) + rm.PLANE_SLOTS:
                    dev = abs(mom[s] - want[s])
                    assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
                    if tol[s] > 0:
                        worst = max(worst, dev / tol[s])
                if prev[b] is not None:   # the front end: P_k is apply_rt(P_{k-1}) with the host solve of pass k-1's vector, bit for bit
                    R, t, _ = pkg.solve_point_to_plane(prev[b]["mom"])
                    assert rm.apply_rt(prev[b]["P"], R, t).tobytes() == P.tobytes(), f"{what}: moved points differ in their bits"
                prev[b] = dict(P=P, idx=idx[b], mom=mom)
                steps_done[b] += 1
        for b, (n, m) in enumerate(cases):
            st = bt.state(b)
            if n >= 63:
                assert steps_done[b] == STEPS and st["status"] == pkg.capi.ICP_OK, (n, m, steps_done[b], st["status"])
            else:   # one point: six unknowns
                assert steps_done[b] >= 1
                assert steps_done[b] == STEPS or st["status"] == pkg.capi.ICP_ERR_SINGULAR, (n, m, steps_done[b], st["status"])
    print(f"[moments] batch/plane_{np.dtype(dtype).name}: largest |device - exact| / tol = {worst:.4f}")


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_batch_plane_pair_bits_do_not_depend_on_neighbours(ctx, pkg, orc):
    ds = pkg.datasets
    G = ds.synthetic_grid(24, np.float32)
    X = (G, ds.make_model_gpu(G, *ds.P2P_GPU))
    others = [cl.ragged_pair(s, n, m) for s, (n, m) in enumerate([(100, 300), (1025, 17), (64, 64), (5, 2000), (700, 900), (333, 1), (2048, 129)])]
    nX, nO = oracle_normals(orc, X[1]), [oracle_normals(orc, M) for _, M in others]
    kw = dict(max_iter=50, tol=1e-5)
    alone = ctx.point_to_plane_batch([X], normals=[nX], **kw)[0]
    first = ctx.point_to_plane_batch([X] + others, normals=[nX] + nO, **kw)[0]
    sixth = ctx.point_to_plane_batch(others[:5] + [X] + others[5:], normals=nO[:5] + [nX] + nO[5:], **kw)[5]
    assert alone.extra["status"] == pkg.capi.ICP_OK and alone.passes >= 3
    same_result_bits(alone, first)
    same_result_bits(alone, sixth)


def test_batch_plane_is_deterministic(ctx, pkg, five):
    pairs, normals, _, res = five
    again = ctx.point_to_plane_batch(pairs, normals=normals, max_iter=50, tol=1e-5)
    for x, y in zip(res, again):
        same_result_bits(x, y)
    with ctx.batch(pairs) as bt:   # begin starts again from the uploaded clouds
        bt.set_model_normals(normals)
        for _ in range(2):
            got = handle_results(bt, pkg, max_iter=50, tol=1e-5, metric=pkg.capi.ICP_POINT_TO_PLANE)
            for x, y in zip(res, got):
                same_result_bits(x, y)


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_batch_plane_degenerate_pair_ends_alone(ctx, pkg, five):
    pairs, normals, _, res = five
    bad, bad_n = degenerate_pair()
    got = ctx.point_to_plane_batch(pairs[:2] + [bad] + pairs[2:], normals=normals[:2] + [bad_n] + normals[2:], max_iter=50, tol=1e-5)
    assert got[2].extra["status"] == pkg.capi.ICP_ERR_SINGULAR and got[2].passes == 0
    for x, y in zip(res, got[:2] + got[3:]):
        same_result_bits(x, y)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_batch_plane_against_single_pair_path(ctx, pkg, five):
    pairs, normals, _, res = five
    for r, (D, M), N in zip(res, pairs, normals):
        one = ctx.point_to_plane(D, M, normals=N, max_iter=50, tol=1e-5)
        assert r.iterations == one.iterations
        assert rel(r.T, one.T) < TOL_T


def test_batch_plane_fp64_against_single_pair_path(ctx, pkg, five):
    """the float64 batch is held to Context.point_to_plane of each pair alone (both against the fp64 oracle: test_gpu_plane_f64.py)"""
    pairs, normals, _, _ = five
    pairs = [(D.astype(np.float64), M.astype(np.float64)) for D, M in pairs]
    normals = [N.astype(np.float64) for N in normals]
    res = ctx.point_to_plane_batch(pairs, normals=normals, max_iter=50, tol=1e-5)
    for r, (D, M), N in zip(res, pairs, normals):
        one = ctx.point_to_plane(D, M, normals=N, max_iter=50, tol=1e-5)
        assert r.extra["status"] == pkg.capi.ICP_OK and r.moved.dtype == np.float64
        assert r.iterations == one.iterations and r.passes == one.passes
        assert rel(r.T, one.T) < TOL_T
        assert np.abs(r.err - one.err).max() < TOL_E
        assert np.array_equal(r.idx, one.idx)


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_batch_point_to_point_is_untouched_by_normals(ctx, pkg, orc, golden):
    pairs = fp32_pairs(pkg, golden)
    with ctx.batch(pairs) as bt:
        plain = handle_results(bt, pkg, max_iter=40, tol=1e-6)
    with ctx.batch(pairs) as bt:
        bt.set_model_normals([oracle_normals(orc, M) for _, M in pairs])
        held = handle_results(bt, pkg, max_iter=40, tol=1e-6, metric=pkg.capi.ICP_POINT_TO_POINT)
        bt.estimate_normals()
        estimated = handle_results(bt, pkg, max_iter=40, tol=1e-6)
    for a, b, c in zip(plain, held, estimated):
        assert a.passes > 1
        same_result_bits(a, b)
        same_result_bits(a, c)
