"""GPU: the values a batch holds per point -- covariances, intensities, intensity gradients, point normals, descriptors and the
model normals -- as their set and get calls behave, whichever attribute: a statement of behaviour that the library's shared
attribute path (csrc/icp_batch.cpp, PointAttr) has to keep, written against the build before it.

One batch of 3 pairs per dtype, the moving clouds of 1, 63 and 129 points, the models of 64, 65 and 129 (the models start at 64:
icp_batch_estimate_normals needs 5 model points), so that every cloud but the first starts behind padding and the sides' planes differ.

    1  per attribute: one side set alone comes back byte for byte; the side never set is refused with ICP_ERR_STATE; a NaN in
       pair 1's model is refused with ICP_ERR_INVALID and what the batch held comes back bit for bit; NULL for every array is
       ICP_ERR_INVALID.  (The descriptors' setter is a diagnostic that needs both sides and scans nothing: its NaN is kept.)
    2  the model normals, which have no getter: what icp_batch_estimate_normals returns, given back through
       icp_batch_set_model_normals, runs the point-to-plane loop of the estimated normals bit for bit; a refused call changes nothing
    3  what a set call discards and what it leaves: gradients after new model intensities or new model normals, a begun loop after
       new covariances but not after new point normals, the matches after new descriptors"""
import ctypes as C

import numpy as np
import pytest

import batch_gicp_ref as gr
from batch_ref import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
N_MOVING, N_MODEL = (1, 63, 129), (64, 65, 129)
PD = C.POINTER(C.c_double)


def make_pairs(dtype):
    return [(gr.blob(10 + b, n, dtype), gr.blob(20 + b, m, dtype)) for b, (n, m) in enumerate(zip(N_MOVING, N_MODEL))]


def values(seed, sizes, width):
    """one float64 array per cloud, (points, width) or (points,) for width None: no two values of a side alike"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n,) if width is None else (n, width)) for n in sizes]


def ptr(a):
    return None if a is None else a.ctypes.data_as(PD)


def flat(arrays):
    return None if arrays is None else np.ascontiguousarray(np.concatenate(arrays))


def code(call):
    try:
        call()
    except Exception as e:   # (IcpError: the package's, whichever alias it was imported under)
        return e.code
    return 0


def same(got, want):
    return len(got) == len(want) and all(bits_equal(g, w) for g, w in zip(got, want))


# 1 ------------------------------------------------------------------------------------------------------------------------
# (name, width, setter(bt, moving, model), the C setter and getter)
TWO_SIDED = [("covariances", 6, lambda bt, a, q: bt.set_covariances(a, q), "icp_batch_set_covariances", "icp_batch_get_covariances"),
             ("intensities", None, lambda bt, a, q: bt.set_intensities(a, q), "icp_batch_set_intensities", None),
             ("point normals", 3, lambda bt, a, q: bt.set_point_normals(a, q), "icp_batch_set_point_normals", "icp_batch_get_point_normals")]


@DTYPES
@pytest.mark.parametrize("attr", TWO_SIDED, ids=[a[0].replace(" ", "_") for a in TWO_SIDED])
def test_two_sided_attribute(ctx, pkg, dtype, attr):
    name, width, put, c_set, c_get = attr
    lib = pkg.load()
    INVALID, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    vm, vq = values(1, N_MOVING, width), values(2, N_MODEL, width)
    w = width or 1

    def get(bt, moving=True, model=True):
        """the C getter for the sides asked for: (rc, moving arrays or None, model arrays or None)"""
        om = np.full((sum(N_MOVING), w), -7.0) if moving else None
        oq = np.full((sum(N_MODEL), w), -7.0) if model else None
        rc = getattr(lib, c_get)(bt._h, ptr(om), ptr(oq))
        cut = lambda o, sizes: None if o is None else [c.reshape(c.shape[0] if width is None else (-1, w)) for c in np.split(o, np.cumsum(sizes)[:-1])]
        return rc, cut(om, N_MOVING), cut(oq, N_MODEL)

    with ctx.batch(make_pairs(dtype)) as bt:
        assert getattr(lib, c_set)(bt._h, None, None) == INVALID                      # NULL-NULL
        if c_get is None:
            # intensities have no getter: the colored begin names the side that is missing, and the gradient estimate reads the models'
            put(bt, vm, None)
            bt.estimate_normals()
            assert code(lambda: bt.estimate_intensity_gradients(5)) == STATE          # the side never set
            assert code(lambda: bt.begin(metric=pkg.ICP_COLORED)) == INVALID and "models" in lib.icp_last_error().decode()
            put(bt, None, vq)
            g = bt.estimate_intensity_gradients(5, want=True)
            bad = [v.copy() for v in vq]
            bad[1][7] = np.nan
            assert code(lambda: put(bt, None, bad)) == INVALID and "pair 1, model" in lib.icp_last_error().decode()
            assert same(bt.get_intensity_gradients(), g)                              # the refusal discarded nothing ...
            assert same(bt.estimate_intensity_gradients(5, want=True), g)             # ... and the intensities are the earlier ones
            return
        put(bt, vm, None)                                                             # the moving side alone
        rc, gm, _ = get(bt, model=False)
        assert rc == 0 and same(gm, vm)
        rc, _, gq = get(bt, moving=False)
        assert rc == STATE and "models" in lib.icp_last_error().decode() and (np.concatenate(gq) == -7.0).all()
        assert get(bt)[0] == STATE
        assert getattr(lib, c_get)(bt._h, None, None) == INVALID
        put(bt, None, vq)                                                             # the models alone: the moving side stays
        rc, gm, gq = get(bt)
        assert rc == 0 and same(gm, vm) and same(gq, vq)
        bad = [v.copy() for v in vq]
        bad[1][7] = np.nan
        assert code(lambda: put(bt, vm, bad)) == INVALID and "pair 1, model" in lib.icp_last_error().decode()
        rc, gm, gq = get(bt)
        assert rc == 0 and same(gm, vm) and same(gq, vq)
    with ctx.batch(make_pairs(dtype)) as bt:                                          # the models first: the moving side is the one never set
        put(bt, None, vq)
        rc, _, gq = get(bt, moving=False)
        assert rc == 0 and same(gq, vq)
        rc, _, _ = get(bt, model=False)
        assert rc == STATE and "moving clouds" in lib.icp_last_error().decode()


@DTYPES
def test_gradients_and_descriptors(ctx, pkg, dtype):
    lib = pkg.load()
    INVALID, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    grads = values(3, N_MODEL, 3)
    fm, fq = values(4, N_MOVING, pkg.capi.ICP_FEATURE_BINS), values(5, N_MODEL, pkg.capi.ICP_FEATURE_BINS)
    with ctx.batch(make_pairs(dtype)) as bt:
        # gradients: the models only
        assert code(bt.get_intensity_gradients) == STATE
        assert lib.icp_batch_set_intensity_gradients(bt._h, None) == INVALID
        assert lib.icp_batch_get_intensity_gradients(bt._h, None) == INVALID
        bt.set_intensity_gradients(grads)
        assert same(bt.get_intensity_gradients(), grads)
        bad = [g.copy() for g in grads]
        bad[1][7, 2] = np.nan
        assert code(lambda: bt.set_intensity_gradients(bad)) == INVALID and "pair 1" in lib.icp_last_error().decode()
        assert same(bt.get_intensity_gradients(), grads)
        # descriptors: rows, not planes; the diagnostic setter takes both sides or nothing and scans nothing
        om, oq = np.empty((sum(N_MOVING), 33)), np.empty((sum(N_MODEL), 33))
        assert lib.icp_batch_get_features(bt._h, ptr(om), None) == STATE and "moving clouds" in lib.icp_last_error().decode()
        assert lib.icp_batch_get_features(bt._h, None, ptr(oq)) == STATE and "models" in lib.icp_last_error().decode()
        assert lib.icp_batch_get_features(bt._h, None, None) == INVALID
        for a, q in ((None, None), (flat(fm), None), (None, flat(fq))):
            assert lib.icp_diag_batch_set_features(bt._h, ptr(a), ptr(q)) == INVALID
        assert code(bt.get_features) == STATE                                         # the refusals left nothing behind
        bt.diag_set_features(fm, fq)
        gm, gq = bt.get_features()
        assert same(gm, fm) and same(gq, fq)
        assert lib.icp_batch_get_features(bt._h, None, ptr(oq)) == 0 and bits_equal(oq, flat(fq))   # one side alone
        assert lib.icp_batch_get_features(bt._h, ptr(om), None) == 0 and bits_equal(om, flat(fm))
        nan = [f.copy() for f in fq]
        nan[1][7, 32] = np.nan
        bt.diag_set_features(fm, nan)                                                 # (not scanned: kept as given)
        assert same(bt.get_features()[1], nan)


# 2 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_model_normals_through_the_plane_loop(ctx, pkg, dtype):
    lib = pkg.load()
    INVALID, STATE = pkg.capi.ICP_ERR_INVALID, pkg.capi.ICP_ERR_STATE
    pairs = make_pairs(dtype)

    def run(bt):
        bt.begin(max_iter=4, metric=pkg.ICP_POINT_TO_PLANE)
        bt.run(8)
        out = [bt.state(b) for b in range(bt.count)]
        return [(s["status"], s["iterations"], s["passes"], s["T"].tobytes(), s["err"].tobytes()) for s in out], bt.get_moving()

    with ctx.batch(pairs) as bt:
        assert code(lambda: bt.begin(metric=pkg.ICP_POINT_TO_PLANE)) == INVALID      # no normals yet
        bt.set_intensities(None, values(6, N_MODEL, None))
        assert code(lambda: bt.estimate_intensity_gradients(5)) == STATE and "normals" in lib.icp_last_error().decode()
        normals = bt.estimate_normals()
        assert [n.shape for n in normals] == [(m, 3) for m in N_MODEL] and all(n.dtype == dtype for n in normals)
        want, moved = run(bt)
    with ctx.batch(pairs) as bt:
        assert lib.icp_batch_set_model_normals(bt._h, None) == INVALID
        bt.set_model_normals(normals)
        got, moved2 = run(bt)
        assert got == want and same(moved2, moved)
        bad = [n.copy() for n in normals]
        bad[1][7, 1] = np.nan
        assert code(lambda: bt.set_model_normals(bad)) == INVALID
        got, moved2 = run(bt)                                                         # the earlier normals, bit for bit
        assert got == want and same(moved2, moved)


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_invalidations(ctx, pkg, dtype):
    STATE = pkg.capi.ICP_ERR_STATE
    Iq, grads = values(7, N_MODEL, None), values(8, N_MODEL, 3)
    cm, nm = values(9, N_MOVING, 6), values(10, N_MOVING, 3)
    fm, fq = values(11, N_MOVING, 33), values(12, N_MODEL, 33)
    with ctx.batch(make_pairs(dtype)) as bt:
        normals = bt.estimate_normals()
        bt.set_intensity_gradients(grads)
        bt.set_intensities(values(13, N_MOVING, None), None)                          # the moving side: the gradients stay
        assert same(bt.get_intensity_gradients(), grads)
        bt.set_intensities(None, Iq)                                                  # new model intensities
        assert code(bt.get_intensity_gradients) == STATE
        bt.set_intensity_gradients(grads)
        bt.set_model_normals(normals)                                                 # new model normals
        assert code(bt.get_intensity_gradients) == STATE
        # a begun loop
        bt.begin(max_iter=5)
        bt.run(1)
        before = bt.state(1)
        bt.set_point_normals(nm, None)                                                # the loop does not read them
        after = bt.state(1)
        assert after["iterations"] == before["iterations"] and after["T"].tobytes() == before["T"].tobytes()
        assert bt.run(1)[0] == 1
        bt.set_covariances(cm, None)
        assert code(lambda: bt.state(1)) == STATE and code(lambda: bt.run(1)) == STATE
        # the matches
        bt.diag_set_features(fm, fq)
        bt.match_features(mutual=False)
        T = np.tile(np.eye(4), (bt.count, 1, 1))
        assert bt.score_transforms(T, None).shape == (bt.count, 1)
        bt.diag_set_features(fm, fq)
        assert code(lambda: bt.score_transforms(T, None)) == STATE
