"""GPU: voxel-grid downsampling of a batch on the device (icp_batch_downsample, icp_batch_get_offsets, icp_batch_get_clouds;
Batch.downsample, Batch.get_clouds, Context.register_batch_multiscale).

The rule is stated in include/icp_mi355x.h and restated in numpy in tests/batch_voxel_ref.py; tests/test_batch_voxel_ref.py pins
that reference -- counts, populations, the identity and single-cell cases, the quotients that round below an integer -- on every
cloud used here.  This file compares the device with it for byte equality: clouds, maps, offsets and counts, in fp32 and fp64.
No tolerance is introduced; the only one used is the project's end-to-end 1e-5 (test_gpu_batch.py) where a numpy loop in
double is run beside the multiscale registration."""
import ctypes as C

import numpy as np
import pytest

import batch_voxel_ref as vr
from batch_ref import (CASES, TOL_E, TOL_T, apply, assert_same_run, bits_equal, compose, final, gate_case, reference_loop, rel, run_to_end,
                       same_pair_bytes, same_result_bits, t0f)

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def per_pair(v, count):
    return np.full(count, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)


def check_batch(ctx, pairs, vm, vq, what):
    """the batch downsampled on the device is the reference's, byte for byte: clouds, maps, offsets, counts.  Returns the
    reference clouds."""
    vm, vq = per_pair(vm, len(pairs)), per_pair(vq, len(pairs))
    ref, mm, qm = vr.downsample_pairs(pairs, vm, vq)
    with ctx.batch(pairs) as src:
        nb, gm, gq = src.downsample(vm, vq, want_maps=True)
        with nb:
            assert nb.count == len(pairs)
            assert np.array_equal(nb._moff, vr.offsets([r[0] for r in ref])), (what, "moving offsets")
            assert np.array_equal(nb._qoff, vr.offsets([r[1] for r in ref])), (what, "model offsets")
            got = nb.get_clouds()
            for b, ((YD, YM), (GD, GM)) in enumerate(zip(ref, got)):
                assert GD.shape == YD.shape and GM.shape == YM.shape, (what, b, GD.shape, YD.shape, GM.shape, YM.shape)
                assert bits_equal(GD, YD), (what, b, "moving cloud")
                assert bits_equal(GM, YM), (what, b, "model")
                assert gm[b].dtype == np.int32 and np.array_equal(gm[b], mm[b]), (what, b, "moving map")
                assert gq[b].dtype == np.int32 and np.array_equal(gq[b], qm[b]), (what, b, "model map")
        back = src.get_clouds()   # the source holds what was uploaded
        for (D, M), (GD, GM) in zip(pairs, back):
            assert bits_equal(GD, D) and bits_equal(GM, M), (what, "source clouds")
    return ref


# 1 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_voxel_granules(ctx, dtype):
    """one pair per size around a work item (64), the key tile and a chunk of the scan; cells of 1 to about 10 points"""
    ref = check_batch(ctx, vr.granule_pairs(dtype), vr.GRANULE_V, vr.GRANULE_V, "granules")
    assert [r[0].shape[0] for r in ref] == [1, 2, 57, 55, 59, 307, 318, 301, 449, 187, 192]


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_voxel_extremes(ctx, dtype):
    Z, X, S = vr.coincident(dtype), vr.normal(300, 11, dtype), vr.signed_zeros(dtype)
    vX, vS = vr.identity_voxel(X), vr.identity_voxel(S)
    #        coincident points     all alone      one cell      -0.0 coarse / alone     v = 0 on one side only
    pairs = [(Z, X),               (X, S),        (X, Z),       (S, S),                 (X, Z),          (Z, X)]
    vm =    [0.5,                  vX,            1e6,          vr.GRANULE_V,           0.0,             0.5]
    vq =    [0.5,                  vS,            1e6,          vS,                     0.5,             0.0]
    ref = check_batch(ctx, pairs, vm, vq, "extremes")
    assert ref[0][0].shape[0] == 199                                          # 40 coincident points in one cell
    assert bits_equal(ref[1][0], X) and bits_equal(ref[1][1], S)              # every point alone: the input
    assert ref[2][0].shape[0] == 1 and ref[2][1].shape[0] == 1                # every point in one cell
    assert np.signbit(ref[3][1][17]).all()                                    # a -0.0 survives
    assert bits_equal(ref[4][0], X) and ref[4][1].shape[0] == 199             # copied / thinned
    assert ref[5][0].shape[0] == 199 and bits_equal(ref[5][1], X)


@DTYPES
@pytest.mark.parametrize("alone", [True, False], ids=["alone", "one_cell"])
def test_voxel_largest_cloud(ctx, dtype, alone):
    """one pair at ICP_BATCH_MAX_POINTS: every point alone (the widest scan), every point in one cell (the longest sequential sum)"""
    B, small = vr.normal(vr.MAX_POINTS, 12, dtype), vr.normal(65, 13, dtype)
    v = vr.identity_voxel(B) if alone else 1e6
    ref = check_batch(ctx, [(B, small)], v, 0.0, "largest cloud")
    assert ref[0][0].shape[0] == (vr.MAX_POINTS if alone else 1)


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_voxel_boundaries(ctx, dtype):
    """exact quotients, quotients that round below the integer (a reciprocal in place of the division moves them), negative
    coordinates and clouds far from the origin"""
    H, (T, _), Fr, Ng = vr.half_lattice(dtype), vr.tenth_lattice(dtype), vr.far(dtype), vr.negative(dtype)
    ref = check_batch(ctx, [(H, T), (T, H), (Fr, Ng), (Ng, Fr)], [1.0, 0.1, 0.5, 0.5], [0.1, 1.0, 0.5, 0.5], "boundaries")
    assert ref[0][0].shape[0] == 75 and ref[1][0].shape[0] == (408 if dtype == np.float32 else 564)


# 4 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_voxel_a_pairs_bits_are_its_own(ctx, dtype):
    """a pair's output is the same bytes alone, in a batch of 5 and with the pair order reversed; a different v per pair"""
    pairs = vr.granule_pairs(dtype)[2:7]
    vm, vq = [0.3, 0.5, 0.0, 0.7, 0.4], [0.6, 0.0, 0.2, 0.5, 0.9]

    def run(ps, a, b):
        with ctx.batch(ps) as src:
            nb, gm, gq = src.downsample(a, b, want_maps=True)
            with nb:
                return nb.get_clouds(), gm, gq

    ref, mm, qm = vr.downsample_pairs(pairs, vm, vq)
    five = run(pairs, vm, vq)
    rev = run(pairs[::-1], vm[::-1], vq[::-1])
    for b in range(5):
        one = run([pairs[b]], [vm[b]], [vq[b]])
        for got, k in ((five, b), (rev, 4 - b), (one, 0)):
            assert bits_equal(got[0][k][0], ref[b][0]) and bits_equal(got[0][k][1], ref[b][1]), b
            assert np.array_equal(got[1][k], mm[b]) and np.array_equal(got[2][k], qm[b]), b


# 5 ------------------------------------------------------------------------------------------------------------------------
def snapshot(pkg, bt):
    """everything a caller can read of a batch's loop, as bytes (or the error code that refuses it)"""
    out = []
    for name, fn in (("indices", bt.get_indices), ("loop_indices", bt.loop_indices), ("inliers", bt.get_inliers), ("moving", bt.get_moving),
                     ("done", bt.done), ("clouds", bt.get_clouds)):
        try:
            v = fn()
            out.append((name, [np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else tuple(x.tobytes() for x in a) for a in v]
                        if isinstance(v, list) else v.tobytes()))
        except pkg.IcpError as e:
            out.append((name, e.code))
    for b in range(bt.count):
        for name, fn in (("moments", bt.diag_moments), ("trim", bt.diag_trim)):
            try:
                v = fn(b)
                out.append((name, b, v.tobytes() if isinstance(v, np.ndarray) else (np.float64(v[0]).tobytes(), v[1])))
            except pkg.IcpError as e:
                out.append((name, b, e.code))
        try:
            st = bt.state(b)
            out.append(("state", b, st["status"], st["iterations"], st["passes"], st["err"].tobytes(), st["T"].tobytes()))
        except pkg.IcpError as e:
            out.append(("state", b, e.code))
    return out


@DTYPES
def test_voxel_refusals_leave_the_source_alone(ctx, pkg, dtype):
    INVALID, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES[:3]]
    lib = pkg.load()
    pd = C.POINTER(C.c_double)
    with ctx.batch(pairs) as bt:
        bt.set_max_distance(0.3)
        bt.begin(max_iter=6, tol=1e-9)
        assert bt.run(2)[0] == 2
        before = snapshot(pkg, bt)
        for bad in (np.nan, -0.5, np.inf, -np.inf):
            for side in (0, 1):
                v = np.array([0.5, 0.5, 0.5])
                v[1] = bad
                args = (v, 0.5) if side == 0 else (0.5, v)
                with pytest.raises(pkg.IcpError) as e:
                    bt.downsample(*args)
                assert e.value.code == INVALID and "pair 1" in str(e.value), (bad, side, str(e.value))
                assert snapshot(pkg, bt) == before
        # *out is NULL on a refusal
        v = np.array([0.5, -1.0, 0.5])
        out = C.c_void_p(0x1234)
        assert lib.icp_batch_downsample(bt._h, v.ctypes.data_as(pd), None, None, None, C.byref(out)) == INVALID and out.value is None
        assert lib.icp_batch_downsample(bt._h, None, None, None, None, None) == INVALID
        # a grid too fine for the cloud's extent: extent / v >= 2^21, on the model of pair 2
        M = pairs[2][1]
        extent = float((M.max(axis=0).astype(np.float64) - M.min(axis=0).astype(np.float64)).max())
        fine = extent / 2.0 ** 21
        assert vr.top_cell(M, fine) > vr.MAX_CELL
        out = C.c_void_p(0x1234)
        vq = np.array([0.5, 0.5, fine])
        rc = lib.icp_batch_downsample(bt._h, None, vq.ctypes.data_as(pd), None, None, C.byref(out))
        msg = lib.icp_last_error().decode()
        assert rc == INVALID and out.value is None and "pair 2" in msg and "model" in msg and "too fine" in msg, msg
        assert snapshot(pkg, bt) == before
        with pytest.raises(pkg.IcpError) as e:   # ... and on a moving cloud
            bt.downsample([vr.identity_voxel(pairs[0][0]) / 3.0, 0.5, 0.5], 0.5)
        assert e.value.code == INVALID and "pair 0" in str(e.value) and "moving" in str(e.value)
        assert snapshot(pkg, bt) == before
        # just inside the range: accepted
        with bt.downsample(0.5, [0.5, 0.5, vr.identity_voxel(M)]) as nb:
            assert nb.get_clouds()[2][1].shape == M.shape
        assert snapshot(pkg, bt) == before
    # a context with a pending pass
    A, M = pairs[0]
    with pkg.Context(0) as c:
        c.set_model(M)
        c.set_moving(A)
        with c.batch(pairs[:2]) as bt:
            bt.begin(max_iter=6, tol=1e-9)
            assert bt.run(2)[0] == 2
            before = snapshot(pkg, bt)
            c.loop_begin(max_iter=10, tol=1e-5)
            c.loop_enqueue()
            with pytest.raises(pkg.IcpError) as e:
                bt.downsample(0.5)
            assert e.value.code == STATE
            with pytest.raises(pkg.IcpError) as e:
                bt.get_clouds()
            assert e.value.code == STATE
            c.loop_complete()
            assert snapshot(pkg, bt) == before   # after the refusal the source answers as before
            with bt.downsample(0.5) as nb:
                assert nb.count == 2


@DTYPES
def test_voxel_the_loop_does_not_notice(ctx, pkg, dtype):
    """run src two steps, downsample, run on: every export is that of a twin batch that was never downsampled"""
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    with ctx.batch(pairs) as X, ctx.batch(pairs) as Y:
        for bt in (X, Y):
            bt.set_max_distance(0.3)
            bt.set_trim(0.8)
            bt.begin(max_iter=12, tol=1e-6)
            assert bt.run(2)[0] == 2
        made = []
        steps = 2
        while True:
            if steps & 1:
                made.append(X.downsample(0.0, 0.6))
            else:
                made.append(X.downsample(0.4, want_maps=True)[0])
            assert snapshot(pkg, X) == snapshot(pkg, Y), steps
            kx, ky = X.run(1), Y.run(1)
            assert kx == ky, (steps, kx, ky)
            if not ky[0]:
                break
            steps += 1
        assert steps >= 4 and X.done().all()
        fx, fy = final(X), final(Y)
        for b in range(len(pairs)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}")
            assert_same_run(fx[b]["st"]["iterations"], fx[b]["st"]["err"], fx[b]["st"]["T"], fy[b]["st"], 1e-6, fp32=dtype == np.float32)
        assert snapshot(pkg, X) == snapshot(pkg, Y)
    for nb in made:   # the source went first: the new batches are destroyed on their own
        assert nb.get_clouds()[0][0].dtype == dtype
        nb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@DTYPES
def test_voxel_the_new_batch_is_a_batch(ctx, pkg, dtype, plane):
    """the downsampled batch runs as a batch created from the numpy-downsampled clouds: status, iterations, err series, idx, masks,
    moment vectors and the final cloud, bit for bit, with a gate and a trim (point-to-plane: normals estimated on the device)"""
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    vm, vq = [0.4, 0.25, 0.5, 0.4], [0.4, 0.5, 0.25, 0.0]
    ref, _, _ = vr.downsample_pairs(pairs, vm, vq)
    assert all(YM.shape[0] >= 5 for _, YM in ref)
    with ctx.batch(pairs) as src, src.downsample(vm, vq) as X, ctx.batch(ref) as Y:
        nrm = []
        for bt in (X, Y):
            if plane:
                nrm.append(bt.estimate_normals())
            bt.set_max_distance(0.5)
            bt.set_trim(0.85)
            bt.begin(max_iter=15, tol=1e-6, metric=metric)
        if plane:
            for a, b in zip(*nrm):
                assert bits_equal(a, b)
        steps = 0
        while True:
            kx, ky = X.run(1), Y.run(1)
            assert kx == ky
            if not ky[0]:
                break
            steps += 1
            assert snapshot(pkg, X) == snapshot(pkg, Y), steps
        fx, fy = final(X), final(Y)
        for b in range(len(pairs)):
            same_pair_bytes(fx[b], fy[b], f"pair {b}")
        assert steps >= 3 and any(f["st"]["passes"] >= 3 for f in fy)


# 7 ------------------------------------------------------------------------------------------------------------------------
VOXELS = [0.5, 0.25, 0]


@pytest.mark.parametrize("plane", [False, True], ids=["p2p", "plane"])
@DTYPES
def test_multiscale_is_the_hand_written_sequence(ctx, pkg, dtype, plane):
    pairs = [gate_case(*c, dtype=dtype)[:2] for c in CASES]
    metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    gates = [1.0, 0.5, np.array([0.2, 0.3, 0.2, np.inf])]
    res = ctx.register_batch_multiscale(pairs, VOXELS, metric=metric, max_iter=20, tol=1e-6, max_distance=gates, trim=0.9)
    # by hand: downsample / set_initial_transforms / register, level by level
    T, levels = None, []
    with ctx.batch(pairs) as full:
        for v, g in zip(VOXELS, gates):
            bt = full.downsample(v) if v else full
            if plane:
                bt.estimate_normals()
            bt.set_max_distance(g)
            bt.set_initial_transforms(T)
            bt.set_trim(0.9)
            fin = run_to_end(bt, metric, 20)
            T = np.stack([f["st"]["T"] for f in fin])
            levels.append([(v, c[0].shape[0], c[1].shape[0], f["st"]) for c, f in zip(bt.get_clouds(), fin)])
            if bt is not full:
                bt.close()
    for b, r in enumerate(res):
        assert len(r.extra["levels"]) == 3
        for lv, (v, n, m, st) in zip(r.extra["levels"], [lvl[b] for lvl in levels]):
            assert (lv["voxel"], lv["n"], lv["m"], lv["status"], lv["iterations"]) == (float(v), n, m, st["status"], st["iterations"]), b
            assert bits_equal(lv["T"], st["T"]), b
        f = fin[b]
        assert r.extra["status"] == f["st"]["status"] and r.iterations == f["st"]["iterations"] and r.passes == f["st"]["passes"]
        assert bits_equal(r.T, f["st"]["T"]) and bits_equal(r.err, f["st"]["err"]) and bits_equal(r.idx, f["idx"])
        assert bits_equal(r.moved, f["moved"]) and bits_equal(r.extra["inliers"], f["linl"])
        n = [lv["n"] for lv in r.extra["levels"]]
        assert n[0] <= n[1] < n[2] == pairs[b][0].shape[0] and (b == 3 or n[0] < n[1])   # (the 68 points of the last case: 22 cells at both edges)


@DTYPES
def test_multiscale_against_a_numpy_loop(ctx, pkg, orc, dtype):
    """level by level on the reference's clouds: orc.nn + ref_numpy.minimize from the previous level's T (batch_ref.reference_loop,
    every match kept); T and err within the project's end-to-end 1e-5, equal iteration counts"""
    pairs = [gate_case(c[0], c[1], 0, dtype=dtype)[:2] for c in CASES]
    res = ctx.register_batch_multiscale(pairs, VOXELS, max_iter=30, tol=1e-6)
    keep_all = lambda d: np.ones(d.shape, dtype=bool)
    for b, (r, (A, M)) in enumerate(zip(res, pairs)):
        T = None
        for lv, v in zip(r.extra["levels"], VOXELS):
            YA, YM = vr.downsample(A, v)[0], vr.downsample(M, v)[0]
            assert (lv["n"], lv["m"]) == (YA.shape[0], YM.shape[0])
            start = YA if T is None else apply(YA, T)
            want = reference_loop(orc, start, YM, keep_all, 30, 1e-6)
            want["T"] = want["T"] if T is None else compose(want["T"], t0f(T, dtype))
            print(f"[multiscale numpy] {np.dtype(dtype).name} pair {b} v {v}: iterations {lv['iterations']} / {want['iterations']}, "
                  f"T rel {rel(lv['T'], want['T']):.3e}")
            assert lv["status"] == pkg.capi.ICP_OK and lv["iterations"] == want["iterations"], (b, v, lv["iterations"], want["iterations"])
            assert rel(lv["T"], want["T"]) < TOL_T, (b, v)
            T = lv["T"]   # (the device's: the next level starts where the device stood)
        n = min(len(r.err), len(want["err"]))
        print(f"[multiscale numpy] pair {b}: final err {r.err[-1]!r} / {want['err'][-1]!r}")
        assert np.abs(r.err[:n] - want["err"][:n]).max() < TOL_E and rel(r.T, want["T"]) < TOL_T


def test_multiscale_argument_checks(ctx, pkg):
    pairs = [gate_case(*c)[:2] for c in CASES[:2]]
    nrm = [np.tile(np.array([[0, 0, 1]], dtype=np.float32), (M.shape[0], 1)) for _, M in pairs]
    with pytest.raises(TypeError):
        ctx.register_batch_multiscale(pairs, [0.5, 0], max_itr=3)
    with pytest.raises(ValueError):
        ctx.register_batch_multiscale(pairs, [0.5, 0], metric=pkg.ICP_POINT_TO_PLANE, normals=nrm)
    with pytest.raises(ValueError):
        ctx.register_batch_multiscale(pairs, [])
    with pytest.raises(pkg.IcpError) as e:
        ctx.register_batch_multiscale(pairs, [-0.5, 0])
    assert e.value.code == pkg.capi.ICP_ERR_INVALID
    # caller-given normals with full-resolution levels only; robust options by keyword; None = full resolution
    res = ctx.register_batch_multiscale(pairs, [None, 0], metric=pkg.ICP_POINT_TO_PLANE, normals=nrm, max_iter=3, kernel="huber", scale=0.1)
    assert len(res) == 2 and all("weights" in r.extra and len(r.extra["levels"]) == 2 for r in res)
    one = ctx.register_batch(pairs, max_iter=5)
    ms = ctx.register_batch_multiscale(pairs, [0], max_iter=5)
    for a, b in zip(one, ms):   # a single full-resolution level is register_batch
        same_result_bits(a, b)
