"""GPU: batched point-to-point ICP (icp_batch_*, Context.point_to_point_batch / Context.batch).

Every pair of a batch must run the loop icp_point_to_point runs for it alone: against the CPU oracle with the bar of
test_gpu_parity.py (indices bit-exact per pass, T within 1e-5 relative, err within 1e-5), and with bits that do not depend on
the other pairs of the batch, their sizes or its order.
"""
import ctypes as C

import numpy as np
import pytest

from batch_ref import TOL_E, TOL_T, assert_same_run, fp32_pairs, fp64_pairs, rel, same_result_bits
from clouds import ragged_pair   # (one home for the construction: the moment tests use the same clouds)

pytestmark = pytest.mark.gpu


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_batch_fp64_each_pair_against_oracle(ctx, pkg, orc):
    pairs = fp64_pairs(pkg, orc)
    res = ctx.point_to_point_batch(pairs, max_iter=200, tol=1e-5)
    wants = [orc.icp_p2p(D, M, 200, 1e-5) for D, M in pairs]
    assert len({w["iterations"] for w in wants}) >= 4   # the pairs stop at different passes: the batch runs on without them
    assert wants[2]["iterations"] == 56
    for r, w in zip(res, wants):
        assert r.extra["status"] == pkg.capi.ICP_OK
        assert r.iterations == w["iterations"] and r.passes == w["passes"]
        assert rel(r.T, w["T"]) < TOL_T
        assert rel(r.moved, w["moved"]) < TOL_T
        assert np.abs(r.err - w["err"]).max() < TOL_E
        assert np.array_equal(r.idx, w["idx"])


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_batch_fp32_against_oracle(ctx, pkg, orc, golden, fixed):
    pairs = fp32_pairs(pkg, golden)
    res = ctx.point_to_point_batch(pairs, max_iter=40, tol=1e-6, fixed_iterations=fixed)
    for r, (D, M) in zip(res, pairs):
        want = orc.icp_p2p_f32x(D, M, 40, 1e-6, fixed=fixed)
        assert r.extra["status"] == pkg.capi.ICP_OK
        assert_same_run(r.iterations, r.err, r.T, want, 1e-6, fp32=True)
        if fixed:
            assert r.passes == want["passes"] == 40
        if r.iterations == want["iterations"]:
            assert np.array_equal(r.idx, want["idx"])


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_indices_bit_exact_every_pass(ctx, pkg, orc, golden, dtype):
    pairs = fp64_pairs(pkg, orc) if dtype == np.float64 else fp32_pairs(pkg, golden)
    max_iter, tol = (200, 1e-5) if dtype == np.float64 else (40, 1e-6)
    with ctx.batch(pairs) as bt:
        bt.begin(max_iter=max_iter, tol=tol)
        passes, compared = 0, 0
        while True:
            k, active = bt.run(1)
            assert k == 1
            done = bt.done()
            assert int((~done).sum()) == active
            moving, idx = bt.get_moving(), bt.get_indices()
            for b in np.flatnonzero(~done):   # the cloud pass k was matched on, as the device holds it
                assert np.array_equal(idx[b], orc.nn(moving[b], pairs[b][1])), f"pass {passes}, pair {b}"
                compared += 1
            passes += 1
            if active == 0:
                break
        assert bt.run(1) == (0, 0)
        for b, (D, M) in enumerate(pairs):
            st = bt.state(b)
            want = orc.icp_p2p(D, M, max_iter, tol) if dtype == np.float64 else orc.icp_p2p_f32x(D, M, max_iter, tol)
            assert_same_run(st["iterations"], st["err"], st["T"], want, tol, fp32=(dtype == np.float32))
    assert compared >= passes


# 4 ------------------------------------------------------------------------------------------------------------------------
RAGGED = [(1, 1), (1, 5), (3, 17), (16, 16), (9, 30), (200, 9), (1025, 17), (130, 4097), (777, 16), (5000, 3000), (130, 65536)]


def test_batch_ragged_pairs(ctx, pkg, orc):
    assert RAGGED[-1][1] == pkg.capi.ICP_BATCH_MAX_POINTS
    pairs = [ragged_pair(n * 1000 + m, n, m) for n, m in RAGGED]
    res = ctx.point_to_point_batch(pairs, max_iter=12, tol=1e-9)
    with ctx.batch(pairs) as bt:
        bt.begin(max_iter=12, tol=1e-9)
        while bt.run(64)[1]:
            pass
        loop_idx = bt.loop_indices()
    for r, li, (D, M) in zip(res, loop_idx, pairs):
        want = orc.icp_p2p_f32x(D, M, 12, 1e-9)
        assert_same_run(r.iterations, r.err, r.T, want, 1e-9, fp32=True)
        assert r.idx.min() >= 0 and r.idx.max() < M.shape[0]
        assert np.array_equal(li, r.idx)
        if r.iterations == want["iterations"]:
            assert np.array_equal(r.idx, want["idx"])


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_pair_bits_do_not_depend_on_neighbours(ctx, pkg, orc, dtype):
    D = orc.synth_icp_cpu(24)[0].astype(dtype)
    X = (D, pkg.datasets.make_model_cpu(D, (0.3, -0.2, 0.1), (0.2, 0.1, -0.1)).astype(dtype))
    others = [ragged_pair(s, n, m) for s, (n, m) in enumerate([(100, 300), (1025, 17), (64, 64), (5, 2000), (700, 900), (333, 1), (2048, 129)])]
    others = [(a.astype(dtype), b.astype(dtype)) for a, b in others]
    alone = ctx.point_to_point_batch([X], max_iter=60, tol=1e-7)[0]
    first = ctx.point_to_point_batch([X] + others, max_iter=60, tol=1e-7)[0]
    sixth = ctx.point_to_point_batch(others[:5] + [X] + others[5:], max_iter=60, tol=1e-7)[5]
    assert alone.passes > 3
    same_result_bits(alone, first)
    same_result_bits(alone, sixth)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_batch_is_deterministic(ctx, pkg, orc, golden):
    for pairs, it, tol in [(fp64_pairs(pkg, orc), 200, 1e-5), (fp32_pairs(pkg, golden), 40, 1e-6)]:
        a = ctx.point_to_point_batch(pairs, max_iter=it, tol=tol)
        b = ctx.point_to_point_batch(pairs, max_iter=it, tol=tol)
        for x, y in zip(a, b):
            same_result_bits(x, y)
        with ctx.batch(pairs) as bt:   # begin starts again from the uploaded clouds
            for _ in range(2):
                bt.begin(max_iter=it, tol=tol)
                while bt.run(1000)[1]:
                    pass
                for k, x in enumerate(a):
                    st = bt.state(k)
                    assert st["iterations"] == x.iterations and st["T"].tobytes() == x.T.tobytes()


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_against_single_pair_path(ctx, pkg, orc, golden, dtype):
    pairs = fp64_pairs(pkg, orc) if dtype == np.float64 else fp32_pairs(pkg, golden)
    it, tol = (200, 1e-5) if dtype == np.float64 else (40, 1e-6)
    res = ctx.point_to_point_batch(pairs, max_iter=it, tol=tol)
    for r, (D, M) in zip(res, pairs):
        one = ctx.point_to_point(D, M, max_iter=it, tol=tol)
        if dtype == np.float64:
            assert r.iterations == one.iterations
        else:
            assert abs(r.iterations - one.iterations) <= 1
        assert rel(r.T, one.T) < TOL_T


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_batch_leaves_the_context_alone(pkg, orc):
    D, M = orc.synth_icp_cpu(32)
    pairs = fp64_pairs(pkg, orc)
    with pkg.Context(0) as c:   # the registration alone
        c.set_model(M)
        c.set_moving(D)
        c.loop_begin(max_iter=200, tol=1e-5)
        assert c.loop_run(1000)[1]
        plain = c.loop_state()
        plain_idx, plain_moved = c.loop_indices(), c.get_moving()
    with pkg.Context(0) as c:   # the same, with a whole batch between the upload and the loop
        c.set_model(M)
        c.set_moving(D)
        rec = c.recoveries()
        c.point_to_point_batch(pairs, max_iter=200, tol=1e-5)
        c.loop_begin(max_iter=200, tol=1e-5)
        assert c.loop_run(1000)[1]
        st = c.loop_state()
        assert st["iterations"] == plain["iterations"] and st["T"].tobytes() == plain["T"].tobytes()
        assert st["err"].tobytes() == plain["err"].tobytes()
        assert c.loop_indices().tobytes() == plain_idx.tobytes() and c.get_moving().tobytes() == plain_moved.tobytes()
        assert c.recoveries() == rec
        # a batch call between an enqueue and its complete is refused
        with c.batch(pairs[:2]) as bt:
            c.loop_begin(max_iter=200, tol=1e-5)
            c.loop_enqueue()
            with pytest.raises(pkg.IcpError) as e:
                bt.begin(max_iter=10, tol=1e-5)
            assert e.value.code == pkg.capi.ICP_ERR_STATE
            with pytest.raises(pkg.IcpError) as e:
                c.point_to_point_batch(pairs[:2], max_iter=10, tol=1e-5)
            assert e.value.code == pkg.capi.ICP_ERR_STATE
            c.loop_complete()
            bt.begin(max_iter=10, tol=1e-5)
            assert bt.run(1)[0] == 1


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_batch_refusals(ctx, pkg):
    lib = pkg.load()
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 3))
    p64 = C.POINTER(C.c_int64)

    def create(count, moff, qoff, data=X, precision=pkg.ICP_F64):
        moff, qoff = np.asarray(moff, dtype=np.int64), np.asarray(qoff, dtype=np.int64)
        out = C.c_void_p(0)
        rc = lib.icp_batch_create(ctx._h, count, data.ctypes.data, moff.ctypes.data_as(p64), data.ctypes.data, qoff.ctypes.data_as(p64),
                                  precision, C.byref(out))
        return rc, out.value

    bad = pkg.capi.ICP_ERR_INVALID
    assert create(0, [0], [0]) == (bad, None)                          # count 0
    assert create(2, [0, 5, 5], [0, 5, 9]) == (bad, None)              # non-increasing (an empty cloud)
    assert create(2, [0, 5, 4], [0, 5, 9]) == (bad, None)              # decreasing
    assert create(1, [1, 5], [0, 5]) == (bad, None)                    # not zero-based
    assert create(1, [0, 5], [0, 0]) == (bad, None)                    # an empty model
    big = np.zeros((pkg.capi.ICP_BATCH_MAX_POINTS + 1, 3))
    assert create(1, [0, 5], [0, big.shape[0]], data=big) == (bad, None)   # a cloud over the limit
    Y = X.copy()
    Y[37, 1] = np.nan
    assert create(2, [0, 10, 20], [0, 10, 40], data=Y) == (bad, None)  # a NaN in one pair
    Y[37, 1] = np.inf
    assert create(2, [0, 10, 20], [0, 10, 40], data=Y) == (bad, None)
    rc, h = create(2, [0, 10, 20], [0, 10, 40])
    assert rc == 0 and h
    try:
        prm = pkg.capi.icp_params(10, 1e-6, 0, pkg.ICP_F64, pkg.ICP_POINT_TO_PLANE)
        assert lib.icp_batch_begin(C.c_void_p(h), C.byref(prm)) == bad    # point-to-plane
        prm = pkg.capi.icp_params(10, 1e-6, 0, pkg.ICP_F32, pkg.ICP_POINT_TO_POINT)
        assert lib.icp_batch_begin(C.c_void_p(h), C.byref(prm)) == bad    # another precision
        k, a = C.c_int(0), C.c_int(0)
        assert lib.icp_batch_run(C.c_void_p(h), 1, C.byref(k), C.byref(a)) == pkg.capi.ICP_ERR_STATE   # no begin
    finally:
        lib.icp_batch_destroy(C.c_void_p(h))
    moff, qoff = np.array([0, 10], dtype=np.int64), np.array([0, 10], dtype=np.int64)
    prm = pkg.capi.icp_params(10, 1e-6, 0, pkg.ICP_F64, pkg.ICP_POINT_TO_PLANE)
    T = np.zeros(16)
    assert lib.icp_point_to_point_batch(ctx._h, 1, X.ctypes.data, moff.ctypes.data_as(p64), X.ctypes.data, qoff.ctypes.data_as(p64),
                                        C.byref(prm), T.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None, None) == bad


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_batch_scale_256_pairs(ctx, pkg, orc):
    D = orc.synth_icp_cpu(32)[0]
    rng = np.random.default_rng(11)
    models = [pkg.datasets.make_model_cpu(D, tuple(rng.uniform(-0.3, 0.3, 3)), tuple(rng.uniform(-0.3, 0.3, 3))) for _ in range(256)]
    pairs = [(D, M) for M in models]
    res = ctx.point_to_point_batch(pairs, max_iter=200, tol=1e-5)
    assert all(r.extra["status"] == pkg.capi.ICP_OK for r in res)
    for b in range(0, 256, 16):
        w = orc.icp_p2p(D, models[b], 200, 1e-5)
        r = res[b]
        assert r.iterations == w["iterations"] and rel(r.T, w["T"]) < TOL_T and np.abs(r.err - w["err"]).max() < TOL_E
        assert np.array_equal(r.idx, w["idx"]) and rel(r.moved, w["moved"]) < TOL_T
    for b in (3, 100, 201, 255):
        same_result_bits(ctx.point_to_point_batch([pairs[b]], max_iter=200, tol=1e-5)[0], res[b])
