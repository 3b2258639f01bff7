"""CPU, no library: what the Python batch layer (engine.Batch and the batch entry points of engine.Context) hands to the C ABI.
A stub stands where libicp_mi355x.so would: it records every call with its arguments -- scalars by value, pointers as NULL or
"ptr", and the arrays, rule structs and icp_params this layer builds by content -- and answers ICP_OK.  Every expectation is
written out here; nothing is loaded from a recording.  Three pairs, (n, m) = (5, 7), (6, 6), (9, 4).

The entry points are pinned as the ordered list of the calls that change state (create, set_*, estimate_*, compute_*, match_*,
the four thinning calls, begin, run, ransac / fgr, destroy) and as the multiset of the downloads between run and destroy, whose
order among themselves is free.  register_batch_global's default normals route puts numpy's eigenvectors between a download and
an upload: that upload (icp_batch_compute_features' normals) is pinned as non-NULL only."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

SHAPES = ((5, 7), (6, 6), (9, 4))
COUNT, N, M = 3, 20, 17
MOFF, QOFF = (0, 5, 11, 20), (0, 7, 13, 17)
F32, F64 = 0, 1                      # capi.ICP_F32, capi.ICP_F64
P2P, PLANE, GICP, COLORED, SYMMETRIC = 0, 1, 2, 3, 4
EYE = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)
READS = {"icp_batch_state", "icp_batch_loop_indices", "icp_batch_loop_inliers", "icp_batch_get_moving", "icp_batch_get_weights",
         "icp_batch_get_offsets", "icp_batch_get_clouds"}
THINNING = ("icp_batch_downsample", "icp_batch_remove_outliers", "icp_batch_select_keypoints", "icp_batch_segment_plane")
_D, _I, _U8, _U64, _I64 = C.c_double, C.c_int, C.c_uint8, C.c_uint64, C.c_int64
# the pointer arguments recorded by content: call -> {argument position: (element type, length from the batch's layout)}
CONTENT = {
    "icp_batch_create": {3: (_I64, "count+1"), 5: (_I64, "count+1")},
    "icp_batch_set_max_distance": {1: (_D, "count")},
    "icp_batch_set_trim": {1: (_D, "count")},
    "icp_batch_set_color_weight": {1: (_D, "count")},
    "icp_batch_downsample": {1: (_D, "count"), 2: (_D, "count")},
    "icp_batch_evaluate": {2: (_D, "count")},
    "icp_batch_score_transforms": {3: (_D, "count")},
    "icp_batch_set_reciprocal": {1: (_U8, "count")},
    "icp_batch_set_robust": {1: (_I, "count"), 2: (_D, "count")},
    "icp_batch_set_initial_transforms": {1: (_D, "count*16")},
    "icp_batch_estimate_covariances": {1: (_I, "count"), 2: (_I, "count")},
    "icp_batch_estimate_intensity_gradients": {1: (_I, "count")},
    "icp_batch_compute_features": {1: (_I, "count"), 2: (_I, "count")},
    "icp_batch_compute_features_stored": {1: (_I, "count"), 2: (_I, "count")},
    "icp_batch_segment_plane": {3: (_U64, "count")},
    "icp_batch_ransac": {2: (_U64, "count")},
    "icp_batch_fgr": {2: (_U64, "count")},
    "icp_batch_set_covariances": {1: (_D, "n*6"), 2: (_D, "m*6")},
    "icp_batch_set_intensities": {1: (_D, "n"), 2: (_D, "m")},
    "icp_batch_set_point_normals": {1: (_D, "n*3"), 2: (_D, "m*3")},
    "icp_batch_set_intensity_gradients": {1: (_D, "m*3")},
}
# arguments that are raw addresses (array.ctypes.data), not scalars
ADDRESSES = {"icp_batch_create": (2, 4), "icp_batch_set_model_normals": (1,), "icp_batch_get_clouds": (1, 2), "icp_batch_get_moving": (1,),
             "icp_batch_estimate_normals": (1,)}


class StubLib:
    """records (name, normalised arguments) of every call and returns ICP_OK, or the code `fail` holds for that name once
    `skip` earlier calls of it have passed"""

    def __init__(self):
        self.calls, self.layout, self.label = [], {}, {1: "ctx"}
        self.fail, self.skip = {}, {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _length(self, lay, key):
        return eval(key, {}, {"count": lay["count"], "n": lay["moff"][-1], "m": lay["qoff"][-1]})

    def _norm(self, name, i, a, lay):
        if a is None or isinstance(a, (bool, float, str)):
            return a
        if isinstance(a, int):
            if i not in ADDRESSES.get(name, ()):
                return a
            if name != "icp_batch_set_model_normals":
                return "ptr"
            ctype = C.c_double if lay["prec"] == F64 else C.c_float   # the upload is read in the batch's own precision
            return tuple((ctype * (3 * lay["qoff"][-1])).from_address(a))
        if isinstance(a, C.c_void_p):
            return self.label[a.value]
        if hasattr(a, "_obj"):   # ctypes.byref(x)
            x = a._obj
            return (type(x).__name__,) + tuple(getattr(x, f) for f, _ in x._fields_) if isinstance(x, C.Structure) else "out"
        if isinstance(a, C.Array):   # the rule structs, field by field
            return [tuple(tuple(v) if isinstance(v, C.Array) else v for v in (getattr(r, f) for f, _ in r._fields_)) for r in a]
        if isinstance(a, C._Pointer):
            if i not in CONTENT.get(name, {}):
                return "ptr"
            ctype, key = CONTENT[name][i]
            assert type(a) is C.POINTER(ctype), (name, i, type(a))
            return tuple(a[: self._length(lay, key)])
        raise TypeError(f"{name}: argument {i} is a {type(a).__name__}")

    def _call(self, name, args):
        if name in ("icp_strerror", "icp_last_error"):
            return b"stub"
        if name == "icp_destroy":   # the context's own handle: not this layer
            return None
        if name == "icp_batch_create":
            lay = {"count": args[1], "moff": [0] * (args[1] + 1), "qoff": [0] * (args[1] + 1), "prec": args[6]}
        else:
            lay = self.layout.get(args[0].value)   # (None for the one-call entries, which take the context)
        self.calls.append((name, tuple(self._norm(name, i, a, lay) for i, a in enumerate(args))))
        if name in self.fail:
            if self.skip.get(name, 0) == 0:
                return self.fail[name]
            self.skip[name] -= 1
        if name == "icp_batch_create" or name in THINNING:
            h = len(self.label) + 100
            self.label[h] = f"b{len(self.label)}"
            if name == "icp_batch_create":
                lay = {"count": args[1], "moff": list(args[3][: args[1] + 1]), "qoff": list(args[5][: args[1] + 1]), "prec": args[6]}
            self.layout[h] = lay   # a thinned batch keeps its source's layout
            args[-1]._obj.value = h
        elif name == "icp_batch_get_offsets":
            for p, off in ((args[1], lay["moff"]), (args[2], lay["qoff"])):
                for b, v in enumerate(off):
                    p[b] = v
        elif name == "icp_batch_get_clouds":
            ctype = C.c_double if lay["prec"] == F64 else C.c_float
            for addr, total in ((args[1], lay["moff"][-1]), (args[2], lay["qoff"][-1])):
                out = (ctype * (3 * total)).from_address(addr)
                out[:] = [0.5 * i + (i % 7) for i in range(3 * total)]
        elif name == "icp_batch_estimate_covariances":
            for p, total in ((args[5], lay["moff"][-1]), (args[6], lay["qoff"][-1])):
                for i in range(6 * total if p is not None else 0):   # diag(1, 2, 3): finite eigenvectors for oriented_normals
                    p[i] = (1.0, 0.0, 0.0, 2.0, 0.0, 3.0)[i % 6]
        elif name in ("icp_batch_ransac", "icp_batch_fgr"):
            for i in range(16 * lay["count"]):
                args[3][i] = EYE[i % 16]
        return 0


def c(name, *args):
    return ("icp_batch_" + name, args)


def params(max_iter, tol, fixed, prec, metric):
    return ("icp_params", max_iter, tol, fixed, prec, metric)


def writes(calls):
    return [x for x in calls if x[0] not in READS]


def reads(calls):
    """the downloads as {(name, batch): how often}"""
    return dict(Counter((x[0][len("icp_batch_"):], x[1][0]) for x in calls if x[0] in READS))


def destroyed(calls):
    return [x[1][0] for x in calls if x[0] == "icp_batch_destroy"]


def created(stub):
    return sorted(v for v in stub.label.values() if v != "ctx")


def clouds(dtype=np.float32):
    """three pairs whose coordinates are exact in float32"""
    return [((np.arange(3 * n).reshape(n, 3) * 0.25 + b).astype(dtype), (np.arange(3 * m).reshape(m, 3) * 0.5 - b).astype(dtype))
            for b, (n, m) in enumerate(SHAPES)]


def per_model(width=3, scale=0.125):
    return [np.arange(m * width, dtype=np.float64).reshape(m, width) * scale + b for b, (_, m) in enumerate(SHAPES)]


def per_moving(width=3, scale=0.125):
    return [np.arange(n * width, dtype=np.float64).reshape(n, width) * scale - b for b, (n, _) in enumerate(SHAPES)]


def flat(arrays, dtype=np.float64):
    return tuple(np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in arrays]).tolist())


@pytest.fixture
def stub(pkg, monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(pkg.capi, "load", lambda: lib)   # capi.check names a failure through the library
    return lib


@pytest.fixture
def sctx(pkg, stub):
    """a Context around the stub: no device, no library"""
    ctx = pkg.Context.__new__(pkg.Context)
    ctx._lib, ctx._h, ctx._dtype, ctx._n, ctx._m = stub, C.c_void_p(1), None, 0, 0
    return ctx


@pytest.fixture
def bt(pkg, sctx, stub):
    bt = pkg.engine.Batch(sctx, clouds())
    del stub.calls[:]
    return bt


def rec(stub, fn, *args, **kw):
    """the calls fn makes, and what it returned"""
    del stub.calls[:]
    out = fn(*args, **kw)
    return list(stub.calls), out


def refusal(exc, message, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and e.value.args[0] == message, e.value.args


# ---- Batch: construction, begin, close ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, prec", [(np.float32, F32), (np.float64, F64)])
def test_create_begin_close(pkg, sctx, stub, dtype, prec):
    calls, bt = rec(stub, pkg.engine.Batch, sctx, clouds(dtype))
    assert calls == [c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, prec, "out")]
    assert (bt.count, tuple(bt._moff), tuple(bt._qoff), bt._model_shapes, bt._max_iter) == (3, MOFF, QOFF, [(7, 3), (6, 3), (4, 3)], 0)
    assert rec(stub, bt.begin)[0] == [c("begin", "b1", params(40, 1e-6, 0, prec, P2P))]
    assert rec(stub, bt.begin, max_iter=7, tol=0.5, fixed_iterations=True, metric=SYMMETRIC)[0] == [c("begin", "b1", params(7, 0.5, 1, prec, SYMMETRIC))]
    assert bt._max_iter == 7
    assert rec(stub, bt.run, 5) == ([c("run", "b1", 5, "out", "out")], (0, 0))
    assert rec(stub, bt.close)[0] == [c("destroy", "b1")]
    assert rec(stub, bt.close)[0] == []
    refusal(ValueError, "a batch needs at least one pair", pkg.engine.Batch, sctx, [])


# ---- Batch: one value per pair --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, what", [("set_max_distance", "maximum distance"), ("set_trim", "share to keep"), ("set_color_weight", "lambda")])
def test_per_pair_double_setters(bt, stub, method, what):
    f, name = getattr(bt, method), method
    assert rec(stub, f, None)[0] == [c(name, "b1", None)]
    assert rec(stub, f, 0.5)[0] == [c(name, "b1", (0.5, 0.5, 0.5))]
    assert rec(stub, f, 2)[0] == [c(name, "b1", (2.0, 2.0, 2.0))]
    assert rec(stub, f, np.float32(0.25))[0] == [c(name, "b1", (0.25, 0.25, 0.25))]
    assert rec(stub, f, [0.5, 1, np.inf])[0] == [c(name, "b1", (0.5, 1.0, np.inf))]
    assert rec(stub, f, np.array([3, 2, 1], dtype=np.int32)[::1])[0] == [c(name, "b1", (3.0, 2.0, 1.0))]
    assert rec(stub, f, np.arange(6.0)[::2])[0] == [c(name, "b1", (0.0, 2.0, 4.0))]   # a strided view is made contiguous
    del stub.calls[:]
    for bad in ([1.0, 2.0], np.ones((3, 1)), np.ones(4)):
        refusal(ValueError, f"one {what} per pair (or a scalar)", f, bad)
    assert stub.calls == []   # a refusal reaches no C call


def test_set_color_weight_default_is_null(bt, stub):
    assert rec(stub, bt.set_color_weight)[0] == [c("set_color_weight", "b1", None)]


def test_set_reciprocal(bt, stub):
    f = bt.set_reciprocal
    assert rec(stub, f, None)[0] == [c("set_reciprocal", "b1", None)]
    assert rec(stub, f, True)[0] == [c("set_reciprocal", "b1", (1, 1, 1))]
    assert rec(stub, f, False)[0] == [c("set_reciprocal", "b1", (0, 0, 0))]
    assert rec(stub, f, np.True_)[0] == [c("set_reciprocal", "b1", (1, 1, 1))]
    assert rec(stub, f, [True, False, True])[0] == [c("set_reciprocal", "b1", (1, 0, 1))]
    assert rec(stub, f, np.array([0, 2, 0]))[0] == [c("set_reciprocal", "b1", (0, 1, 0))]
    for bad in ([True, False], 1, np.ones((3, 1))):
        refusal(ValueError, "one reciprocity flag per pair (or a bool, or None)", f, bad)


def test_set_robust(bt, stub):
    f = bt.set_robust
    assert rec(stub, f, None)[0] == [c("set_robust", "b1", None, None)]
    assert rec(stub, f, None, 3.0)[0] == [c("set_robust", "b1", None, None)]          # the scale of no kernel is not read
    assert rec(stub, f, None, [1.0, 2.0])[0] == [c("set_robust", "b1", None, None)]   # ... nor checked
    assert rec(stub, f, "huber", 2.0)[0] == [c("set_robust", "b1", (1, 1, 1), (2.0, 2.0, 2.0))]
    assert rec(stub, f, "cauchy")[0] == [c("set_robust", "b1", (2, 2, 2), None)]      # kinds without scales: a NULL scale
    assert rec(stub, f, "none", 1)[0] == [c("set_robust", "b1", (0, 0, 0), (1.0, 1.0, 1.0))]
    assert rec(stub, f, 3, [0.5, 1.5, 2.5])[0] == [c("set_robust", "b1", (3, 3, 3), (0.5, 1.5, 2.5))]
    assert rec(stub, f, np.int64(2), 4.0)[0] == [c("set_robust", "b1", (2, 2, 2), (4.0, 4.0, 4.0))]
    assert rec(stub, f, ["huber", None, 3], scale=None)[0] == [c("set_robust", "b1", (1, 0, 3), None)]
    assert rec(stub, f, ("tukey", "none", np.int32(1)), (1.0, 2.0, 3.0))[0] == [c("set_robust", "b1", (3, 0, 1), (1.0, 2.0, 3.0))]
    refusal(ValueError, "one robust kernel per pair (or one for every pair, or None)", f, ["huber", "huber"], 1.0)
    refusal(ValueError, "one scale per pair (or a scalar)", f, "huber", [1.0, 2.0])
    refusal(KeyError, "welsch", f, "welsch", 1.0)
    refusal(KeyError, "welsch", f, ["huber", "welsch", None], 1.0)


def test_set_initial_transforms(bt, stub):
    f = bt.set_initial_transforms
    T = np.arange(16.0).reshape(4, 4)
    one = tuple(float(i) for i in range(16))
    assert rec(stub, f, None)[0] == [c("set_initial_transforms", "b1", None)]
    assert rec(stub, f, T)[0] == [c("set_initial_transforms", "b1", one * 3)]
    assert rec(stub, f, T.astype(np.float32).tolist())[0] == [c("set_initial_transforms", "b1", one * 3)]
    per = np.stack([T, T + 100.0, -T])
    assert rec(stub, f, per)[0] == [c("set_initial_transforms", "b1", tuple(float(i) for i in range(16)) + tuple(float(i) + 100.0 for i in range(16))
                                      + tuple(-float(i) for i in range(16)))]
    for bad in (np.zeros((2, 4, 4)), np.zeros((3, 3)), np.zeros(16), 1.0):
        refusal(ValueError, "one (4, 4) initial transform for every pair, or (count, 4, 4)", f, bad)


def test_cov_k_callers(bt, stub):
    """the int k arrays: estimate_covariances, estimate_intensity_gradients, compute_features, compute_features_stored"""
    f = bt.estimate_covariances
    assert rec(stub, f) == ([c("estimate_covariances", "b1", (20, 20, 20), (20, 20, 20), 1, 1e-3, None, None)], None)
    assert rec(stub, f, 5, None, regularisation="none", lam=0.5)[0] == [c("estimate_covariances", "b1", (5, 5, 5), (5, 5, 5), 0, 0.5, None, None)]
    assert rec(stub, f, [3, 4, 5], 7, regularisation=None)[0] == [c("estimate_covariances", "b1", (3, 4, 5), (7, 7, 7), 0, 1e-3, None, None)]
    assert rec(stub, f, np.int64(6), np.array([8, 9, 10]), regularisation=1)[0] == [c("estimate_covariances", "b1", (6, 6, 6), (8, 9, 10), 1, 1e-3, None, None)]
    assert rec(stub, f, 4.0)[0] == [c("estimate_covariances", "b1", (4, 4, 4), (4, 4, 4), 1, 1e-3, None, None)]
    calls, (om, oq) = rec(stub, f, None, 9, want=True)   # k None: the moving side is left as it is
    assert calls == [c("estimate_covariances", "b1", None, (9, 9, 9), 1, 1e-3, None, "ptr")]
    assert om is None and [a.shape for a in oq] == [(7, 6), (6, 6), (4, 6)]
    calls, (om, oq) = rec(stub, f, 3, want=True)
    assert calls == [c("estimate_covariances", "b1", (3, 3, 3), (3, 3, 3), 1, 1e-3, "ptr", "ptr")]
    assert [a.shape for a in om] == [(5, 6), (6, 6), (9, 6)] and [a.shape for a in oq] == [(7, 6), (6, 6), (4, 6)]
    refusal(ValueError, "one k per pair (or a scalar)", f, [3, 4])
    refusal(ValueError, "one model k per pair (or a scalar)", f, 3, [3, 4])
    refusal(KeyError, "ridge", f, 3, regularisation="ridge")
    g = bt.estimate_intensity_gradients
    assert rec(stub, g) == ([c("estimate_intensity_gradients", "b1", (8, 8, 8), None)], None)
    calls, out = rec(stub, g, [3, 4, 5], want=True)
    assert calls == [c("estimate_intensity_gradients", "b1", (3, 4, 5), "ptr")] and [a.shape for a in out] == [(7, 3), (6, 3), (4, 3)]
    refusal(ValueError, "one k per pair (or a scalar)", g, [3, 4, 5, 6])
    nm, nq = per_moving(), per_model()
    assert rec(stub, bt.compute_features, 5, (nm, nq))[0] == [c("compute_features", "b1", (5, 5, 5), (5, 5, 5), "ptr", "ptr", None, None)]
    assert rec(stub, bt.compute_features, [5, 6, 7], (nm, nq), k_model=4, want=True)[0] == [
        c("compute_features", "b1", (5, 6, 7), (4, 4, 4), "ptr", "ptr", "ptr", "ptr")]
    refusal(ValueError, "one model k per pair (or a scalar)", bt.compute_features, 5, (nm, nq), k_model=[1])
    refusal(ValueError, "one array of moving normals per pair", bt.compute_features, 5, (nm[:2], nq))
    refusal(ValueError, "a pair's model normals must be (points, 3)", bt.compute_features, 5, (nm, nq[::-1]))
    assert rec(stub, bt.compute_features_stored, 5)[0] == [c("compute_features_stored", "b1", (5, 5, 5), (5, 5, 5), None, None)]
    assert rec(stub, bt.compute_features_stored, 5, [6, 7, 8], want=True)[0] == [c("compute_features_stored", "b1", (5, 5, 5), (6, 7, 8), "ptr", "ptr")]
    refusal(ValueError, "one k per pair (or a scalar)", bt.compute_features_stored, [5])


def test_evaluate_and_score_transforms(bt, stub):
    calls, out = rec(stub, bt.evaluate)
    assert calls == [c("evaluate", "b1", P2P, None, "ptr", "ptr", "ptr", "ptr", "ptr", None, None)]
    assert len(out) == 3 and all(sorted(d) == ["fitness", "information", "inliers", "rmse", "status"] for d in out)
    calls, out = rec(stub, bt.evaluate, 0.5, metric=PLANE, want_matches=True)
    assert calls == [c("evaluate", "b1", PLANE, (0.5, 0.5, 0.5), "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr")]
    assert all(sorted(d) == ["fitness", "idx", "information", "inliers", "inliers_mask", "rmse", "status"] for d in out)
    assert [d["idx"].shape for d in out] == [(5,), (6,), (9,)] and all(d["inliers_mask"].dtype == bool for d in out)
    assert rec(stub, bt.evaluate, [1, np.inf, 3])[0] == [c("evaluate", "b1", P2P, (1.0, np.inf, 3.0), "ptr", "ptr", "ptr", "ptr", "ptr", None, None)]
    refusal(ValueError, "one evaluation distance per pair (or a scalar)", bt.evaluate, [1.0, 2.0])
    T = np.zeros((3, 4, 4))
    assert rec(stub, bt.score_transforms, T, None)[0] == [c("score_transforms", "b1", 1, "ptr", None, "ptr")]
    calls, out = rec(stub, bt.score_transforms, np.zeros((3, 2, 4, 4)), [1.0, 2.0, 3.0])
    assert calls == [c("score_transforms", "b1", 2, "ptr", (1.0, 2.0, 3.0), "ptr")] and out.shape == (3, 2)
    refusal(ValueError, "one maximum distance per pair (or a scalar)", bt.score_transforms, T, [1.0])
    refusal(ValueError, "candidate transforms must be (count, per_pair, 4, 4)", bt.score_transforms, np.zeros((2, 4, 4)), None)


# ---- Batch: one array per pair against a side's layout ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_set_model_normals(pkg, sctx, stub, dtype):
    bt = pkg.engine.Batch(sctx, clouds(dtype))
    nq = per_model()
    assert rec(stub, bt.set_model_normals, nq)[0] == [c("set_model_normals", "b1", flat(nq))]   # (0.125 steps: exact in float32)
    assert rec(stub, bt.set_model_normals, (n.astype(np.float32).tolist() for n in nq))[0] == [c("set_model_normals", "b1", flat(nq))]
    refusal(ValueError, "one array of normals per pair", bt.set_model_normals, nq[:2])
    refusal(ValueError, "a pair's normals must have the shape of its model", bt.set_model_normals, nq[::-1])
    refusal(ValueError, "a cloud is an (N, 3) array", bt.set_model_normals, [n.ravel() for n in nq])
    refusal(ValueError, "a pair's normals must have the shape of its model", bt.set_model_normals, per_moving())


def test_side_uploads(bt, stub):
    """covariances, intensities, point normals and gradients: float64 whatever the batch's dtype, moving then model"""
    cm, cq = per_moving(6), per_model(6)
    assert rec(stub, bt.set_covariances, cm, cq)[0] == [c("set_covariances", "b1", flat(cm), flat(cq))]
    assert rec(stub, bt.set_covariances, None, [a.astype(np.float32) for a in cq])[0] == [c("set_covariances", "b1", None, flat(cq))]
    assert rec(stub, bt.set_covariances, cm)[0] == [c("set_covariances", "b1", flat(cm), None)]
    assert rec(stub, bt.set_covariances)[0] == [c("set_covariances", "b1", None, None)]
    refusal(ValueError, "one array of moving covariances per pair", bt.set_covariances, cm[:2], cq)
    refusal(ValueError, "a pair's model covariances must be (points, 6)", bt.set_covariances, cm, cm)
    refusal(ValueError, "a pair's moving covariances must be (points, 6)", bt.set_covariances, per_moving(3), cq)
    im, iq = [a[:, 0].copy() for a in per_moving()], [a[:, 1] for a in per_model()]   # (the model's: strided views)
    assert rec(stub, bt.set_intensities, im, iq)[0] == [c("set_intensities", "b1", flat(im), flat(iq))]
    assert rec(stub, bt.set_intensities, model=iq)[0] == [c("set_intensities", "b1", None, flat(iq))]
    refusal(ValueError, "one array of model intensities per pair", bt.set_intensities, im, iq + iq)
    refusal(ValueError, "a pair's moving intensities must be (points,)", bt.set_intensities, iq, iq)
    refusal(ValueError, "a pair's model intensities must be (points,)", bt.set_intensities, im, [a[:, None] for a in iq])
    nm, nq = per_moving(), per_model()
    assert rec(stub, bt.set_point_normals, nm, nq)[0] == [c("set_point_normals", "b1", flat(nm), flat(nq))]
    assert rec(stub, bt.set_point_normals, None, nq)[0] == [c("set_point_normals", "b1", None, flat(nq))]
    refusal(ValueError, "one array of model normals per pair", bt.set_point_normals, nm, nq[1:])
    refusal(ValueError, "a pair's moving normals must be (points, 3)", bt.set_point_normals, nq, nq)
    assert rec(stub, bt.set_intensity_gradients, iter(nq))[0] == [c("set_intensity_gradients", "b1", flat(nq))]
    refusal(ValueError, "a pair's model gradients must be (points, 3)", bt.set_intensity_gradients, nm)
    refusal(ValueError, "one array of model gradients per pair", bt.set_intensity_gradients, nq[:1])


# ---- Batch: the four thinning calls and their rules -------------------------------------------------------------------------------
def shapes(per_pair):
    return [a.shape for a in per_pair]


MOVING, MODEL = [(5,), (6,), (9,)], [(7,), (6,), (4,)]


def test_downsample(pkg, bt, stub):
    calls, out = rec(stub, bt.downsample, 0.5)
    assert calls == [c("downsample", "b1", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), None, None, "out"), c("get_offsets", "b2", "ptr", "ptr")]
    assert isinstance(out, pkg.engine.Batch) and out._ctx is bt._ctx
    assert (out.count, out._dtype, tuple(out._moff), tuple(out._qoff), out._model_shapes, out._max_iter) == (
        3, np.float32, MOFF, QOFF, [(7, 3), (6, 3), (4, 3)], 0)
    assert rec(stub, bt.downsample, [0.5, 0, 2], 0.25)[0][0] == c("downsample", "b1", (0.5, 0.0, 2.0), (0.25, 0.25, 0.25), None, None, "out")
    calls, (out, mm, qm) = rec(stub, bt.downsample, 1, [1, 2, 3], want_maps=True)
    assert calls == [c("downsample", "b1", (1.0, 1.0, 1.0), (1.0, 2.0, 3.0), "ptr", "ptr", "out"), c("get_offsets", "b4", "ptr", "ptr")]
    assert shapes(mm) == MOVING and shapes(qm) == MODEL and all(a.dtype == np.int32 for a in mm + qm)
    refusal(ValueError, "one voxel edge per pair (or a scalar)", bt.downsample, [0.5, 0.5])
    refusal(ValueError, "one model voxel edge per pair (or a scalar)", bt.downsample, 0.5, [0.5, 0.5])
    assert rec(stub, out.close)[0] == [c("destroy", "b4")]


def test_remove_outliers(pkg, bt, stub):
    calls, (out, info) = rec(stub, bt.remove_outliers)
    assert calls == [c("remove_outliers", "b1", None, None, None, None, None, None, "ptr", "out"), c("get_offsets", "b2", "ptr", "ptr")]
    assert isinstance(out, pkg.engine.Batch) and out.count == 3 and out._dtype == np.float32 and tuple(out._qoff) == QOFF
    assert sorted(info) == ["stats"] and info["stats"].shape == (6, 4)
    calls, (_, info) = rec(stub, bt.remove_outliers, ("statistical", 8, 1.5), ("radius", 0.3, 4), want_maps=True)
    assert calls[0] == c("remove_outliers", "b1", [(1, 8, 1.5)] * 3, [(2, 4, 0.3)] * 3, "ptr", "ptr", None, None, "ptr", "out")
    assert sorted(info) == ["model_map", "moving_map", "stats"] and shapes(info["moving_map"]) == MOVING and shapes(info["model_map"]) == MODEL
    calls, (_, info) = rec(stub, bt.remove_outliers, model=[("statistical", 4.0, 2), None, ("radius", 1, 2.0)], want_scores=True)
    assert calls[0] == c("remove_outliers", "b1", None, [(1, 4, 2.0), (0, 0, 0.0), (2, 2, 1.0)], None, None, "ptr", "ptr", "ptr", "out")
    assert sorted(info) == ["model_score", "moving_score", "stats"] and shapes(info["moving_score"]) == MOVING and shapes(info["model_score"]) == MODEL
    assert info["moving_score"][0].dtype == np.float64
    _, (_, info) = rec(stub, bt.remove_outliers, want_maps=True, want_scores=True)
    assert sorted(info) == ["model_map", "model_score", "moving_map", "moving_score", "stats"]
    refusal(ValueError, "one moving rule per pair (or a single rule)", bt.remove_outliers, [("radius", 1.0, 2)] * 2)
    refusal(ValueError, "one model rule per pair (or a single rule)", bt.remove_outliers, None, [None] * 4)
    refusal(ValueError, "unknown outlier rule 'median': 'statistical', 'radius' or None", bt.remove_outliers, ("median", 1, 2.0))
    # a single rule is a 3-tuple that starts with a str: a list reads as one rule per pair
    refusal(ValueError, "unknown outlier rule 's': 'statistical', 'radius' or None", bt.remove_outliers, ["statistical", 8, 1.5])
    refusal(ValueError, "one model rule per pair (or a single rule)", bt.remove_outliers, None, ("radius", 1.0))


def test_keypoints(pkg, bt, stub):
    calls, (out, info) = rec(stub, bt.keypoints)
    assert calls == [c("select_keypoints", "b1", None, None, None, None, None, None, "ptr", "out"), c("get_offsets", "b2", "ptr", "ptr")]
    assert isinstance(out, pkg.engine.Batch) and sorted(info) == ["counts"] and info["counts"].shape == (6,) and info["counts"].dtype == np.int32
    iss = [(1, 5, 0.5, 0.25, 0.975, 0.975)] * 3   # kind, min_neighbours, salient_radius, non_max_radius, gamma_21, gamma_32
    calls, (_, info) = rec(stub, bt.keypoints, (0.5, 0.25), {"salient_radius": 0.5, "non_max_radius": 0.25}, want_maps=True)
    assert calls[0] == c("select_keypoints", "b1", iss, iss, "ptr", "ptr", None, None, "ptr", "out")
    assert sorted(info) == ["counts", "model_map", "moving_map"] and shapes(info["moving_map"]) == MOVING and shapes(info["model_map"]) == MODEL
    per = [(1, 0.5, 0.75), None, {"non_max_radius": 2, "salient_radius": 3, "min_neighbours": 7.0, "gamma_32": 0.5}]
    calls, (_, info) = rec(stub, bt.keypoints, (1.0, 2.0, 0.9, 0.8, 3), per, want_saliency=True)
    assert calls[0] == c("select_keypoints", "b1", [(1, 3, 1.0, 2.0, 0.9, 0.8)] * 3,
                         [(1, 5, 1.0, 0.5, 0.75, 0.975), (0, 0, 0.0, 0.0, 0.0, 0.0), (1, 7, 3.0, 2.0, 0.975, 0.5)], None, None, "ptr", "ptr", "ptr", "out")
    assert sorted(info) == ["counts", "model_saliency", "moving_saliency"]
    assert shapes(info["moving_saliency"]) == MOVING and shapes(info["model_saliency"]) == MODEL and info["model_saliency"][2].dtype == np.float64
    assert rec(stub, bt.keypoints, (1.0, 2.0, 0.9, 0.8))[0][0][1][1] == [(1, 5, 1.0, 2.0, 0.9, 0.8)] * 3
    text = "a keypoint rule is (salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbours=5)"
    refusal(ValueError, text, bt.keypoints, (0.5,))
    refusal(ValueError, text, bt.keypoints, None, (0.5, 0.25, 0.9, 0.9, 5, 1))
    refusal(ValueError, text, bt.keypoints, [(0.5, 0.25), (0.5,), None])
    needs = "a keypoint rule needs salient_radius and non_max_radius, and may hold ('gamma_21', 'gamma_32', 'min_neighbours')"
    refusal(ValueError, needs, bt.keypoints, {"salient_radius": 0.5, "non_max_radius": 0.25, "gamma": 0.9})
    refusal(ValueError, needs, bt.keypoints, {"salient_radius": 0.5})
    refusal(ValueError, "one moving keypoint rule per pair (or a single rule)", bt.keypoints, [(0.5, 0.25)] * 2)
    # a single rule is a dict, or a tuple that starts with a scalar: a list reads as one rule per pair
    refusal(ValueError, "one model keypoint rule per pair (or a single rule)", bt.keypoints, None, [0.5, 0.25])
    refusal(ValueError, "one moving keypoint rule per pair (or a single rule)", bt.keypoints, ())


def test_segment_plane(pkg, bt, stub):
    calls, (out, info) = rec(stub, bt.segment_plane)
    assert calls == [c("segment_plane", "b1", None, None, (0, 0, 0), "ptr", "ptr", "ptr", None, None, None, None, "out"),
                     c("get_offsets", "b2", "ptr", "ptr")]
    assert isinstance(out, pkg.engine.Batch) and sorted(info) == ["inliers", "planes", "status"] and bt._segment_hyp == [0] * 6
    assert info["planes"].shape == (6, 4) and info["inliers"].shape == (6,) and info["status"].shape == (6,)
    zero = (0.0, 0.0, 0.0)   # kind, hypotheses, distance, axis, min_cos
    calls, (_, info) = rec(stub, bt.segment_plane, ("remove", 0.02), {"kind": "detect", "distance": 0.5, "axis": (1, 0, 0)}, seed=7, want_masks=True)
    assert calls[0] == c("segment_plane", "b1", [(2, 1000, 0.02, zero, 0.0)] * 3, [(1, 1000, 0.5, (1.0, 0.0, 0.0), 0.0)] * 3, (7, 7, 7),
                         "ptr", "ptr", "ptr", "ptr", "ptr", None, None, "out")
    assert sorted(info) == ["inliers", "model_mask", "moving_mask", "planes", "status"] and bt._segment_hyp == [1000] * 6
    assert shapes(info["moving_mask"]) == MOVING and shapes(info["model_mask"]) == MODEL and info["moving_mask"][0].dtype == np.uint8
    per = [("keep", 1, 50.0), None, {"distance": 0.25, "kind": "remove", "min_cos": 0.5, "hypotheses": 9}]
    calls, (_, info) = rec(stub, bt.segment_plane, ("keep", 0.1, 50, (0, 0, 2), 0.9), per, seed=[1, 2, 3], want_maps=True)
    assert calls[0] == c("segment_plane", "b1", [(3, 50, 0.1, (0.0, 0.0, 2.0), 0.9)] * 3,
                         [(3, 50, 1.0, zero, 0.0), (0, 0, 0.0, zero, 0.0), (2, 9, 0.25, zero, 0.5)], (1, 2, 3),
                         "ptr", "ptr", "ptr", None, None, "ptr", "ptr", "out")
    assert sorted(info) == ["inliers", "model_map", "moving_map", "planes", "status"] and bt._segment_hyp == [50, 50, 50, 50, 0, 9]
    assert shapes(info["moving_map"]) == MOVING and shapes(info["model_map"]) == MODEL and info["model_map"][0].dtype == np.int32
    assert rec(stub, bt.segment_plane, None, ("detect", 0.5, 20, [0, 1, 0]))[0][0][1][1:3] == (None, [(1, 20, 0.5, (0.0, 1.0, 0.0), 0.0)] * 3)
    assert bt._segment_hyp == [0, 0, 0, 20, 20, 20]
    text = "a plane rule is (kind, distance, hypotheses=1000, axis=(0, 0, 0), min_cos=0.0)"
    refusal(ValueError, text, bt.segment_plane, ("remove",))
    refusal(ValueError, text, bt.segment_plane, None, ("remove", 0.1, 10, (0, 0, 1), 0.5, 1))
    needs = "a plane rule needs kind and distance, and may hold ('hypotheses', 'axis', 'min_cos')"
    refusal(ValueError, needs, bt.segment_plane, {"kind": "remove", "distance": 0.1, "seed": 3})
    refusal(ValueError, needs, bt.segment_plane, {"kind": "remove"})
    refusal(ValueError, needs, bt.segment_plane, [None, None, {"distance": 0.1}])
    refusal(ValueError, "unknown plane rule kind 'fit': 'detect', 'remove', 'keep' or None", bt.segment_plane, ("fit", 0.1))
    refusal(ValueError, "a plane rule's axis has three components", bt.segment_plane, ("keep", 0.1, 10, (0, 1)))
    refusal(ValueError, "one moving plane rule per pair (or a single rule)", bt.segment_plane, [("keep", 0.1)] * 4)
    # a single rule is a dict, or a tuple that starts with a str: a list reads as one rule per pair
    refusal(ValueError, "one model plane rule per pair (or a single rule)", bt.segment_plane, None, ["keep", 0.1])
    refusal(ValueError, "one model plane rule per pair (or a single rule)", bt.segment_plane, None, ())


# ---- Context: the driving entry points ------------------------------------------------------------------------------------------
RUN = 1 << 20
CREATE = c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, F32, "out")
NO_GATE, NO_INIT = c("set_max_distance", "b1", None), c("set_initial_transforms", "b1", None)
KEYS = ["fitness", "inliers", "status"]
K20, K5 = (20, 20, 20), (5, 5, 5)


def loop(h, max_iter, metric, tol=1e-6, fixed=0, prec=F32):
    return [c("begin", h, params(max_iter, tol, fixed, prec, metric)), c("run", h, RUN, "out", "out")]


def downloads(h, weights=False, states=3):
    """what a finished loop's results are made of"""
    out = {("state", h): states, ("loop_indices", h): 1, ("loop_inliers", h): 1, ("get_moving", h): 1}
    if weights:
        out[("get_weights", h)] = 1
    return out


def drive(stub, fn, *args, **kw):
    """(the calls that change state, the downloads, fn's result); every batch made is destroyed exactly once, and a loop's
    downloads lie between its run and its destroy"""
    before = created(stub)
    calls, out = rec(stub, fn, *args, **kw)
    assert sorted(destroyed(calls)) == [h for h in created(stub) if h not in before]
    for i, (name, a) in enumerate(calls):
        if name in READS - {"icp_batch_get_offsets", "icp_batch_get_clouds"}:
            assert ("icp_batch_run", a[0]) in [(x[0], x[1][0]) for x in calls[:i]] and ("icp_batch_destroy", (a[0],)) in calls[i:]
    return writes(calls), reads(calls), out


def extras(results):
    assert len(results) == 3
    keys = {tuple(sorted(r.extra)) for r in results}
    assert len(keys) == 1
    return list(keys.pop())


def failing(pkg, stub, name, fn, *args, skip=0, **kw):
    """fn with the stub's `name` answering ICP_ERR_STATE (after `skip` good calls): the error surfaces, every batch goes once"""
    stub.fail, stub.skip = {name: -7}, {name: skip}
    del stub.calls[:]
    with pytest.raises(pkg.IcpError) as e:
        fn(*args, **kw)
    assert e.value.code == -7 and e.value.args[0].startswith(name + ": error -7")
    assert stub.calls[-1][0] == "icp_batch_destroy" and created(stub)
    assert sorted(destroyed(stub.calls)) == created(stub)
    return destroyed(stub.calls)


@pytest.mark.parametrize("dtype, prec", [(np.float32, F32), (np.float64, F64)])
def test_point_to_point_batch(pkg, sctx, stub, dtype, prec):
    create = c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, prec, "out")
    w, r, out = drive(stub, sctx.point_to_point_batch, clouds(dtype), max_distance=0.5)
    assert w == [create, c("set_max_distance", "b1", (0.5, 0.5, 0.5)), NO_INIT] + loop("b1", 40, P2P, prec=prec) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    assert [o.idx.shape for o in out] == MOVING and [o.moved.shape for o in out] == [(5, 3), (6, 3), (9, 3)] and out[0].moved.dtype == dtype
    T = np.arange(16.0).reshape(4, 4)
    w, r, out = drive(stub, sctx.point_to_point_batch, clouds(dtype), 7, 0.5, True, None, T, [1.0, 0.5, 0.25])
    assert w == [create, c("set_max_distance", "b2", None), c("set_initial_transforms", "b2", tuple(float(i) for i in range(16)) * 3),
                 c("set_trim", "b2", (1.0, 0.5, 0.25))] + loop("b2", 7, P2P, 0.5, 1, prec) + [c("destroy", "b2")]
    assert r == downloads("b2") and extras(out) == KEYS
    calls, out = rec(stub, sctx.point_to_point_batch, clouds(dtype))   # no option: the one-call C entry, no Batch
    assert [x[0] for x in calls] == ["icp_point_to_point_batch"] and extras(out) == ["status"]


def test_point_to_point_batch_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_begin", sctx.point_to_point_batch, clouds(), trim=0.5) == ["b1"]


@pytest.mark.parametrize("dtype, prec", [(np.float32, F32), (np.float64, F64)])
def test_point_to_plane_batch_gated(pkg, sctx, stub, dtype, prec):
    create = c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, prec, "out")
    w, r, out = drive(stub, sctx.point_to_plane_batch_gated, clouds(dtype), [0.5, 1.5, np.inf])
    assert w == [create, c("estimate_normals", "b1", "ptr", None), c("set_max_distance", "b1", (0.5, 1.5, np.inf)), NO_INIT] + loop(
        "b1", 50, PLANE, prec=prec) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    nq = per_model()
    w, r, out = drive(stub, sctx.point_to_plane_batch_gated, clouds(dtype), None, nq, max_iter=9, init=np.eye(4), trim=0.75)
    assert w == [create, c("set_model_normals", "b2", flat(nq)), c("set_max_distance", "b2", None), c("set_initial_transforms", "b2", EYE * 3),
                 c("set_trim", "b2", (0.75, 0.75, 0.75))] + loop("b2", 9, PLANE, prec=prec) + [c("destroy", "b2")]
    assert r == downloads("b2") and extras(out) == KEYS


def test_point_to_plane_batch_gated_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_estimate_normals", sctx.point_to_plane_batch_gated, clouds(), 0.5) == ["b1"]


def test_register_batch(pkg, sctx, stub):
    w, r, out = drive(stub, sctx.register_batch, clouds())
    assert w == [CREATE, NO_GATE, NO_INIT] + loop("b1", 40, P2P) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    w, r, out = drive(stub, sctx.register_batch, clouds(), PLANE, None, None, 0.25, True, 2.0, np.eye(4), 0.5, [True, False, True])
    assert w == [CREATE, c("estimate_normals", "b2", "ptr", None), c("set_max_distance", "b2", (2.0, 2.0, 2.0)),
                 c("set_initial_transforms", "b2", EYE * 3), c("set_trim", "b2", (0.5, 0.5, 0.5)), c("set_reciprocal", "b2", (1, 0, 1))] + loop(
        "b2", 50, PLANE, 0.25, 1) + [c("destroy", "b2")]
    assert r == downloads("b2") and extras(out) == KEYS
    w, r, out = drive(stub, sctx.register_batch, clouds(), reciprocal=False, max_iter=3)   # False is given: the call is made
    assert w == [CREATE, c("set_max_distance", "b3", None), c("set_initial_transforms", "b3", None), c("set_reciprocal", "b3", (0, 0, 0))] + loop(
        "b3", 3, P2P) + [c("destroy", "b3")]


def test_register_batch_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_run", sctx.register_batch, clouds()) == ["b1"]


def test_register_batch_robust(pkg, sctx, stub):
    w, r, out = drive(stub, sctx.register_batch_robust, clouds(), "huber", 2.0)
    assert w == [CREATE, NO_GATE, NO_INIT, c("set_robust", "b1", (1, 1, 1), (2.0, 2.0, 2.0))] + loop("b1", 40, P2P) + [c("destroy", "b1")]
    assert r == downloads("b1", weights=True) and extras(out) == KEYS + ["weights"] and [o.extra["weights"].shape for o in out] == MOVING
    nq = per_model()
    w, r, out = drive(stub, sctx.register_batch_robust, clouds(), ["tukey", None, 2], [1.0, 2.0, 3.0], metric=PLANE, normals=nq, tol=0.5,
                      fixed_iterations=True, max_distance=4.0, init=np.eye(4), trim=[1.0, 0.5, 0.5], reciprocal=True)
    assert w == [CREATE, c("set_model_normals", "b2", flat(nq)), c("set_max_distance", "b2", (4.0, 4.0, 4.0)), c("set_initial_transforms", "b2", EYE * 3),
                 c("set_trim", "b2", (1.0, 0.5, 0.5)), c("set_reciprocal", "b2", (1, 1, 1)), c("set_robust", "b2", (3, 0, 2), (1.0, 2.0, 3.0))] + loop(
        "b2", 50, PLANE, 0.5, 1) + [c("destroy", "b2")]
    assert r == downloads("b2", weights=True) and extras(out) == KEYS + ["weights"]
    w, r, out = drive(stub, sctx.register_batch_robust, clouds(), None, 1.0, max_iter=5)   # no kernel is still a robust run: the call, the weights
    assert w == [CREATE, c("set_max_distance", "b3", None), c("set_initial_transforms", "b3", None), c("set_robust", "b3", None, None)] + loop(
        "b3", 5, P2P) + [c("destroy", "b3")]
    assert r == downloads("b3", weights=True) and extras(out) == KEYS + ["weights"]
    refusal(TypeError, "register_batch_robust: unknown option(s) ['k', 'lam']", sctx.register_batch_robust, clouds(), "huber", 1.0, lam=1, k=3)


def test_register_batch_robust_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_set_robust", sctx.register_batch_robust, clouds(), "huber", 1.0) == ["b1"]


def test_register_batch_generalized(pkg, sctx, stub):
    w, r, out = drive(stub, sctx.register_batch_generalized, clouds())
    assert w == [CREATE, c("estimate_covariances", "b1", K20, K20, 1, 1e-3, None, None), NO_GATE, NO_INIT] + loop("b1", 50, GICP) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    w, r, out = drive(stub, sctx.register_batch_generalized, clouds(), (5, [6, 7, 8]), "none", 0.5, max_iter=4, tol=0.25, fixed_iterations=True,
                      max_distance=[1.0, 2.0, 3.0], init=np.eye(4), trim=0.5, reciprocal=[False, True, False])
    assert w == [CREATE, c("estimate_covariances", "b2", K5, (6, 7, 8), 0, 0.5, None, None), c("set_max_distance", "b2", (1.0, 2.0, 3.0)),
                 c("set_initial_transforms", "b2", EYE * 3), c("set_trim", "b2", (0.5, 0.5, 0.5)), c("set_reciprocal", "b2", (0, 1, 0))] + loop(
        "b2", 4, GICP, 0.25, 1) + [c("destroy", "b2")]
    assert r == downloads("b2") and extras(out) == KEYS
    cm, cq = per_moving(6), per_model(6)
    w, r, out = drive(stub, sctx.register_batch_generalized, clouds(), covariances=(cm, cq))   # the caller's covariances: nothing is estimated
    assert w == [CREATE, c("set_covariances", "b3", flat(cm), flat(cq)), c("set_max_distance", "b3", None), c("set_initial_transforms", "b3", None)] + loop(
        "b3", 50, GICP) + [c("destroy", "b3")]
    assert r == downloads("b3") and extras(out) == KEYS
    refusal(TypeError, "register_batch_generalized: unknown option(s) ['metric', 'normals']", sctx.register_batch_generalized, clouds(), metric=GICP, normals=None)


def test_register_batch_generalized_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_estimate_covariances", sctx.register_batch_generalized, clouds()) == ["b1"]


def test_register_batch_colored(pkg, sctx, stub):
    im, iq = [a[:, 0].copy() for a in per_moving()], [a[:, 0].copy() for a in per_model()]
    lam = c("set_color_weight", "b1", (0.968, 0.968, 0.968))
    w, r, out = drive(stub, sctx.register_batch_colored, clouds(), (im, iq))
    assert w == [CREATE, c("estimate_normals", "b1", "ptr", None), c("set_intensities", "b1", flat(im), flat(iq)),
                 c("estimate_intensity_gradients", "b1", (8, 8, 8), None), lam, NO_GATE, NO_INIT] + loop("b1", 50, COLORED) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    nq = per_model()
    w, r, out = drive(stub, sctx.register_batch_colored, clouds(), (im, iq), [3, 4, 5], [0.5, 0.75, 1.0], nq, max_iter=6, max_distance=2.0, trim=0.5,
                      reciprocal=True, init=np.eye(4), tol=0.5, fixed_iterations=True)
    assert w == [CREATE, c("set_model_normals", "b2", flat(nq)), c("set_intensities", "b2", flat(im), flat(iq)),
                 c("estimate_intensity_gradients", "b2", (3, 4, 5), None), c("set_color_weight", "b2", (0.5, 0.75, 1.0)),
                 c("set_max_distance", "b2", (2.0, 2.0, 2.0)), c("set_initial_transforms", "b2", EYE * 3), c("set_trim", "b2", (0.5, 0.5, 0.5)),
                 c("set_reciprocal", "b2", (1, 1, 1))] + loop("b2", 6, COLORED, 0.5, 1) + [c("destroy", "b2")]
    assert r == downloads("b2") and extras(out) == KEYS
    w, r, out = drive(stub, sctx.register_batch_colored, clouds(), (im, iq), lam=None)   # None: the library's default, a NULL
    assert w[4] == c("set_color_weight", "b3", None)
    refusal(TypeError, "register_batch_colored: unknown option(s) ['metric']", sctx.register_batch_colored, clouds(), (im, iq), metric=COLORED)


def test_register_batch_colored_failure(pkg, sctx, stub):
    im, iq = [a[:, 0].copy() for a in per_moving()], [a[:, 0].copy() for a in per_model()]
    assert failing(pkg, stub, "icp_batch_estimate_intensity_gradients", sctx.register_batch_colored, clouds(), (im, iq)) == ["b1"]


def test_register_batch_symmetric(pkg, sctx, stub):
    w, r, out = drive(stub, sctx.register_batch_symmetric, clouds())
    assert w == [CREATE, c("estimate_covariances", "b1", K20, K20, 1, 1e-3, None, None), c("estimate_point_normals", "b1", 2, None, None, None, None),
                 NO_GATE, NO_INIT] + loop("b1", 50, SYMMETRIC) + [c("destroy", "b1")]
    assert r == downloads("b1") and extras(out) == KEYS
    w, r, out = drive(stub, sctx.register_batch_symmetric, clouds(), [5, 6, 7], "none", max_iter=8, max_distance=1.0, reciprocal=False)
    assert w == [CREATE, c("estimate_covariances", "b2", (5, 6, 7), (5, 6, 7), 1, 1e-3, None, None), c("estimate_point_normals", "b2", 0, None, None, None, None),
                 c("set_max_distance", "b2", (1.0, 1.0, 1.0)), c("set_initial_transforms", "b2", None), c("set_reciprocal", "b2", (0, 0, 0))] + loop(
        "b2", 8, SYMMETRIC) + [c("destroy", "b2")]
    nm, nq = per_moving(), per_model()
    w, r, out = drive(stub, sctx.register_batch_symmetric, clouds(), normals=(nm, nq), trim=0.5, init=np.eye(4), tol=0.5, fixed_iterations=True)
    assert w == [CREATE, c("set_point_normals", "b3", flat(nm), flat(nq)), c("set_max_distance", "b3", None), c("set_initial_transforms", "b3", EYE * 3),
                 c("set_trim", "b3", (0.5, 0.5, 0.5))] + loop("b3", 50, SYMMETRIC, 0.5, 1) + [c("destroy", "b3")]
    assert r == downloads("b3") and extras(out) == KEYS
    refusal(TypeError, "register_batch_symmetric: unknown option(s) ['lam']", sctx.register_batch_symmetric, clouds(), lam=0.5)


def test_register_batch_symmetric_failure(pkg, sctx, stub):
    assert failing(pkg, stub, "icp_batch_estimate_point_normals", sctx.register_batch_symmetric, clouds()) == ["b1"]


ZERO_T = (0.0,) * 48   # the poses a level hands to the next: the stub's state() leaves T at zero
HALF = (0.5, 0.5, 0.5)


def thin(src, voxel):
    return c("downsample", src, (voxel,) * 3, (voxel,) * 3, None, None, "out")


def test_register_batch_multiscale(pkg, sctx, stub):
    # point-to-point, the coarse level thinned, one gate per level (a list as long as voxels), a start pose
    w, r, out = drive(stub, sctx.register_batch_multiscale, clouds(), [0.5, 0], max_distance=[0.5, 0.25], init=np.eye(4))
    assert w == [CREATE, thin("b1", 0.5), c("set_max_distance", "b2", HALF), c("set_initial_transforms", "b2", EYE * 3)] + loop("b2", 40, P2P) + [
        c("destroy", "b2"), c("set_max_distance", "b1", (0.25, 0.25, 0.25)), c("set_initial_transforms", "b1", ZERO_T)] + loop("b1", 40, P2P) + [c("destroy", "b1")]
    assert r == {("get_offsets", "b2"): 1, ("state", "b2"): 3, **downloads("b1")}   # indices, inliers and clouds come down at the last level alone
    assert extras(out) == ["fitness", "inliers", "levels", "status"]
    for b, (n, m) in enumerate(SHAPES):
        lv = out[b].extra["levels"]
        assert [sorted(x) for x in lv] == [["T", "iterations", "m", "n", "status", "voxel"]] * 2
        assert [(x["voxel"], x["n"], x["m"], x["status"], x["iterations"], x["T"].shape) for x in lv] == [(0.5, n, m, 0, 0, (4, 4)), (0.0, n, m, 0, 0, (4, 4))]
    # point-to-plane with a kernel, the fine level thinned, one gate per pair (an array), trim and reciprocity at every level
    w, r, out = drive(stub, sctx.register_batch_multiscale, clouds(), [None, 2.0], metric=PLANE, max_distance=np.array([1.0, 2.0, 3.0]), kernel="cauchy",
                      scale=1.5, trim=0.5, reciprocal=True, tol=0.5, fixed_iterations=True)

    def level(h, T):
        return [c("estimate_normals", h, "ptr", None), c("set_max_distance", h, (1.0, 2.0, 3.0)), c("set_initial_transforms", h, T),
                c("set_trim", h, HALF), c("set_reciprocal", h, (1, 1, 1)), c("set_robust", h, (2, 2, 2), (1.5, 1.5, 1.5))] + loop(h, 50, PLANE, 0.5, 1)

    assert w == [c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, F32, "out")] + level("b3", None) + [thin("b3", 2.0)] + level("b4", ZERO_T) + [
        c("destroy", "b4"), c("destroy", "b3")]
    assert r == {("state", "b3"): 3, ("get_offsets", "b4"): 1, **downloads("b4", weights=True)}
    assert extras(out) == ["fitness", "inliers", "levels", "status", "weights"]
    # a list of per-pair length is not per level; a kernel without a scale hands a NULL scale on; caller's normals where no level thins
    nq = per_model()
    w, r, out = drive(stub, sctx.register_batch_multiscale, clouds(), [0, 0], metric=PLANE, normals=nq, max_distance=[1.0, 2.0, 3.0], kernel=["huber", None, 3])

    def level(T):
        return [c("set_model_normals", "b5", flat(nq)), c("set_max_distance", "b5", (1.0, 2.0, 3.0)), c("set_initial_transforms", "b5", T),
                c("set_robust", "b5", (1, 0, 3), None)] + loop("b5", 50, PLANE)

    assert w == [CREATE] + level(None) + level(ZERO_T) + [c("destroy", "b5")]
    assert r == downloads("b5", weights=True, states=6)
    # the generalized metric: every level estimates its own covariances; one gate for all
    w, r, out = drive(stub, sctx.register_batch_multiscale, clouds(), [1.0, 0.0], metric=GICP, k=(5, [6, 7, 8]), regularisation="none", lam=0.5, max_distance=2.0)

    def level(h, T):
        return [c("estimate_covariances", h, K5, (6, 7, 8), 0, 0.5, None, None), c("set_max_distance", h, (2.0, 2.0, 2.0)),
                c("set_initial_transforms", h, T)] + loop(h, 50, GICP)

    assert w == [CREATE, thin("b6", 1.0)] + level("b7", None) + [c("destroy", "b7")] + level("b6", ZERO_T) + [c("destroy", "b6")]
    assert r == {("get_offsets", "b7"): 1, ("state", "b7"): 3, **downloads("b6")} and extras(out) == ["fitness", "inliers", "levels", "status"]
    w, r, out = drive(stub, sctx.register_batch_multiscale, clouds(), [0], metric=GICP)
    assert w == [CREATE, c("estimate_covariances", "b8", K20, K20, 1, 1e-3, None, None), c("set_max_distance", "b8", None),
                 c("set_initial_transforms", "b8", None)] + loop("b8", 50, GICP) + [c("destroy", "b8")]
    refusal(TypeError, "register_batch_multiscale: unknown option(s) ['voxel']", sctx.register_batch_multiscale, clouds(), [0], voxel=1)
    refusal(ValueError, "register_batch_multiscale needs at least one level", sctx.register_batch_multiscale, clouds(), [])
    refusal(ValueError, "caller-given normals cannot follow a downsampled model: every level estimates its own", sctx.register_batch_multiscale, clouds(),
            [0.5, 0], metric=PLANE, normals=nq)


def test_register_batch_multiscale_failure(pkg, sctx, stub):
    """the second level's thinned batch goes first, then the uploaded one"""
    assert failing(pkg, stub, "icp_batch_set_trim", sctx.register_batch_multiscale, clouds(), [0, 0.5], trim=0.5, skip=1) == ["b2", "b1"]


def test_register_batch_global(pkg, sctx, stub):
    # RANSAC, the default normals route (covariances and clouds down, numpy's normals up: that upload is seen as non-NULL only)
    w, r, out = drive(stub, sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25)
    assert w == [CREATE, thin("b1", 0.5), c("estimate_covariances", "b2", K5, K5, 0, 1e-3, "ptr", "ptr"),
                 c("compute_features", "b2", K5, K5, "ptr", "ptr", None, None), c("match_features", "b2", 1, "ptr", "ptr", "ptr"),
                 c("ransac", "b2", ("icp_ransac_params", 100, 0.25, 0.9), (0, 0, 0), "ptr", "ptr", "ptr", "ptr"), c("destroy", "b2"), c("destroy", "b1"),
                 c("create", "ctx", 3, "ptr", MOFF, "ptr", QOFF, F32, "out"), c("set_max_distance", "b3", None),
                 c("set_initial_transforms", "b3", EYE * 3)] + loop("b3", 40, P2P) + [c("destroy", "b3")]
    assert r == {("get_offsets", "b2"): 1, ("get_clouds", "b2"): 1, **downloads("b3")}
    assert extras(out) == ["fitness", "global", "inliers", "status"]
    assert [sorted(o.extra["global"]) for o in out] == [["T", "correspondences", "inliers", "status"]] * 3
    # FGR on the uploaded clouds (no voxel), normals on the device facing a viewpoint, the local loop's options handed on
    w, r, out = drive(stub, sctx.register_batch_global, clouds(), None, 5, 0, 0.25, method="fgr", device_normals=True, viewpoint=(1.0, 2.0, 3.0),
                      iterations=8, mutual=False, gate=1.0, metric=PLANE, max_iter=6, trim=0.5, reciprocal=True, tol=0.5, fixed_iterations=True)
    assert w == [CREATE, c("estimate_covariances", "b4", K5, K5, 0, 1e-3, None, None), c("estimate_point_normals", "b4", 1, "ptr", "ptr", None, None),
                 c("compute_features_stored", "b4", K5, K5, None, None), c("match_features", "b4", 0, "ptr", "ptr", "ptr"),
                 c("fgr", "b4", ("icp_fgr_params", 8, 0.25, 1.4, 4, 0, 0.95), None, "ptr", "ptr", "ptr", "ptr", "ptr"), c("destroy", "b4"),
                 CREATE, c("estimate_normals", "b5", "ptr", None), c("set_max_distance", "b5", (1.0, 1.0, 1.0)), c("set_initial_transforms", "b5", EYE * 3),
                 c("set_trim", "b5", HALF), c("set_reciprocal", "b5", (1, 1, 1))] + loop("b5", 6, PLANE, 0.5, 1) + [c("destroy", "b5")]
    assert r == downloads("b5") and extras(out) == ["fitness", "global", "inliers", "status"]
    assert [sorted(o.extra["global"]) for o in out] == [["T", "objective", "status", "used", "weights"]] * 3
    # RANSAC on the keypoints of the thinned clouds without their planes, normals on the device: kb, bt, cut, full go in that order
    zero = (0.0, 0.0, 0.0)
    planes, iss = [(2, 1000, 0.02, zero, 0.0)] * 3, [(1, 5, 0.5, 0.25, 0.975, 0.975)] * 3
    w, r, out = drive(stub, sctx.register_batch_global, clouds(), 0.5, [5, 6, 7], 100, 0.25, planes=("remove", 0.02), keypoints=(0.5, 0.25),
                      device_normals=True, seed=9, edge_similarity=0.8)
    assert w == [CREATE, c("segment_plane", "b6", planes, planes, (9, 9, 9), "ptr", "ptr", "ptr", None, None, None, None, "out"), thin("b7", 0.5),
                 c("estimate_covariances", "b8", (5, 6, 7), (5, 6, 7), 0, 1e-3, None, None), c("estimate_point_normals", "b8", 2, None, None, None, None),
                 c("compute_features_stored", "b8", (5, 6, 7), (5, 6, 7), None, None),
                 c("select_keypoints", "b8", iss, iss, None, None, None, None, "ptr", "out"), c("match_features", "b9", 1, "ptr", "ptr", "ptr"),
                 c("ransac", "b9", ("icp_ransac_params", 100, 0.25, 0.8), (9, 9, 9), "ptr", "ptr", "ptr", "ptr"),
                 c("destroy", "b9"), c("destroy", "b8"), c("destroy", "b7"), c("destroy", "b6"),
                 CREATE, c("set_max_distance", "b10", None), c("set_initial_transforms", "b10", EYE * 3)] + loop("b10", 40, P2P) + [c("destroy", "b10")]
    assert r == {("get_offsets", "b7"): 1, ("get_offsets", "b8"): 1, ("get_offsets", "b9"): 1, **downloads("b10")}
    assert [sorted(o.extra["global"]) for o in out] == [["T", "correspondences", "inliers", "keypoints", "plane_inliers", "planes", "status"]] * 3
    assert out[0].extra["global"]["planes"].shape == (2, 4)
    # FGR on tuples with seeds per pair, planes and keypoints per pair, the default normals route, no voxel
    per_planes = [{"kind": "keep", "distance": 1.0}, None, ("detect", 0.5, 7)]
    rules = [(3, 1000, 1.0, zero, 0.0), (0, 0, 0.0, zero, 0.0), (1, 7, 0.5, zero, 0.0)]
    per_iss = [(0.5, 0.25), None, {"salient_radius": 1.0, "non_max_radius": 2.0}]
    kp = [(1, 5, 0.5, 0.25, 0.975, 0.975), (0, 0, 0.0, 0.0, 0.0, 0.0), (1, 5, 1.0, 2.0, 0.975, 0.975)]
    w, r, out = drive(stub, sctx.register_batch_global, clouds(), 0, 5, 50, 0.25, method="fgr", planes=per_planes, keypoints=per_iss, seed=[1, 2, 3],
                      division_factor=2.0, decrease_every=3, tuple_similarity=0.5)
    assert w == [CREATE, c("segment_plane", "b11", rules, rules, (1, 2, 3), "ptr", "ptr", "ptr", None, None, None, None, "out"),
                 c("estimate_covariances", "b12", K5, K5, 0, 1e-3, "ptr", "ptr"), c("compute_features", "b12", K5, K5, "ptr", "ptr", None, None),
                 c("select_keypoints", "b12", kp, kp, None, None, None, None, "ptr", "out"), c("match_features", "b13", 1, "ptr", "ptr", "ptr"),
                 c("fgr", "b13", ("icp_fgr_params", 64, 0.25, 2.0, 3, 50, 0.5), (1, 2, 3), "ptr", "ptr", "ptr", "ptr", "ptr"),
                 c("destroy", "b13"), c("destroy", "b12"), c("destroy", "b11"),
                 CREATE, c("set_max_distance", "b14", None), c("set_initial_transforms", "b14", EYE * 3)] + loop("b14", 40, P2P) + [c("destroy", "b14")]
    assert r == {("get_offsets", "b12"): 1, ("get_clouds", "b12"): 1, ("get_offsets", "b13"): 1, **downloads("b14")}
    assert [sorted(o.extra["global"]) for o in out] == [["T", "keypoints", "objective", "plane_inliers", "planes", "status", "used", "weights"]] * 3
    refusal(TypeError, "register_batch_global: unknown option(s) ['init', 'kernel']", sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25,
            kernel="huber", init=np.eye(4))
    refusal(ValueError, "register_batch_global: method must be 'ransac' or 'fgr', not 'teaser'", sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25,
            method="teaser")


def test_register_batch_global_failure(pkg, sctx, stub):
    """kb, then bt, then cut, then full -- also when a call in the middle fails, and when the thinning itself does"""
    go = dict(planes=("remove", 0.02), keypoints=(0.5, 0.25), device_normals=True)
    assert failing(pkg, stub, "icp_batch_match_features", sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25, **go) == ["b4", "b3", "b2", "b1"]
    stub.label, stub.layout = {1: "ctx"}, {}
    assert failing(pkg, stub, "icp_batch_compute_features_stored", sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25, **go) == ["b3", "b2", "b1"]
    stub.label, stub.layout = {1: "ctx"}, {}
    assert failing(pkg, stub, "icp_batch_downsample", sctx.register_batch_global, clouds(), 0.5, 5, 100, 0.25, **go) == ["b2", "b1"]


# ---- the effective max_iter where the caller gives none ---------------------------------------------------------------------------
def _colored(ctx, pairs):
    return ctx.register_batch_colored(pairs, ([a[:, 0].copy() for a in per_moving()], [a[:, 0].copy() for a in per_model()]))


@pytest.mark.parametrize("name, entry, want", [
    ("point_to_point_batch", lambda ctx, p: ctx.point_to_point_batch(p, trim=0.5), [40]),
    ("point_to_plane_batch_gated", lambda ctx, p: ctx.point_to_plane_batch_gated(p, 0.5), [50]),
    ("register_batch", lambda ctx, p: ctx.register_batch(p), [40]),
    ("register_batch point-to-point", lambda ctx, p: ctx.register_batch(p, metric=P2P, max_iter=None), [40]),
    ("register_batch point-to-plane", lambda ctx, p: ctx.register_batch(p, metric=PLANE), [50]),
    ("register_batch_robust", lambda ctx, p: ctx.register_batch_robust(p, "huber", 1.0), [40]),
    ("register_batch_robust point-to-point", lambda ctx, p: ctx.register_batch_robust(p, "huber", 1.0, metric=P2P, max_iter=None), [40]),
    ("register_batch_robust point-to-plane", lambda ctx, p: ctx.register_batch_robust(p, "huber", 1.0, metric=PLANE), [50]),
    ("register_batch_generalized", lambda ctx, p: ctx.register_batch_generalized(p), [50]),
    ("register_batch_generalized None", lambda ctx, p: ctx.register_batch_generalized(p, max_iter=None), [50]),
    ("register_batch_colored", _colored, [50]),
    ("register_batch_symmetric", lambda ctx, p: ctx.register_batch_symmetric(p), [50]),
    ("register_batch_multiscale", lambda ctx, p: ctx.register_batch_multiscale(p, [0.5, 0]), [40, 40]),
    ("register_batch_multiscale point-to-point", lambda ctx, p: ctx.register_batch_multiscale(p, [0.5, 0], metric=P2P, max_iter=None), [40, 40]),
    ("register_batch_multiscale point-to-plane", lambda ctx, p: ctx.register_batch_multiscale(p, [0.5, 0], metric=PLANE), [50, 50]),
    # multiscale's rule is "40 for point-to-point, else 50", register_batch's "50 for point-to-plane, else 40": they part at this metric
    ("register_batch_multiscale generalized", lambda ctx, p: ctx.register_batch_multiscale(p, [0.5, 0], metric=GICP), [50, 50]),
    ("register_batch_global", lambda ctx, p: ctx.register_batch_global(p, 0.5, 5, 100, 0.25, device_normals=True), [40]),
    ("register_batch_global point-to-plane", lambda ctx, p: ctx.register_batch_global(p, 0.5, 5, 0, 0.25, method="fgr", device_normals=True, metric=PLANE), [50]),
])
def test_default_max_iter(sctx, stub, name, entry, want):
    calls, _ = rec(stub, entry, sctx, clouds())
    assert [x[1][1][1] for x in calls if x[0] == "icp_batch_begin"] == want, name


def test_ransac_and_fgr_seeds(bt, stub):
    """one seed for every pair or one per pair; fgr reads them only where it draws tuples"""
    ransac = lambda seeds: c("ransac", "b1", ("icp_ransac_params", 10, 0.5, 0.9), seeds, "ptr", "ptr", "ptr", "ptr")
    fgr = lambda tuples, seeds: c("fgr", "b1", ("icp_fgr_params", 64, 0.5, 1.4, 4, tuples, 0.95), seeds, "ptr", "ptr", "ptr", "ptr", "ptr")
    assert rec(stub, bt.ransac, 10, 0.5)[0] == [ransac((0, 0, 0))]
    assert rec(stub, bt.ransac, 10, 0.5, seed=2 ** 40)[0] == [ransac((2 ** 40,) * 3)]
    assert rec(stub, bt.ransac, 10, 0.5, seed=np.array([3, 2, 1], dtype=np.int32))[0] == [ransac((3, 2, 1))]
    refusal(ValueError, "one seed per pair (or a scalar)", bt.ransac, 10, 0.5, seed=[1, 2])
    assert rec(stub, bt.fgr, 0.5, seed=7)[0] == [fgr(0, None)]
    assert rec(stub, bt.fgr, 0.5, tuples=20, seed=7)[0] == [fgr(20, (7, 7, 7))]
    assert rec(stub, bt.fgr, 0.5, tuples=20, seed=[1, 2, 3])[0] == [fgr(20, (1, 2, 3))]
    refusal(ValueError, "one seed per pair (or a scalar)", bt.fgr, 0.5, tuples=20, seed=[1, 2, 3, 4])
    bt.fgr(0.5, seed=[1, 2, 3, 4])   # ... so no tuples, no check
