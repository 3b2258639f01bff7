"""Host-side mirror of the reference's ICP interface on top of the C ABI (numpy in / numpy out).

The reference exposes its path only through `main()` programs; the seams are its kernel
signatures and loops.  `Context` wraps one `icp_ctx` (one HIP device) and offers those seams with
the reference's names and argument meaning:

    Matching(P, Q) -> idx                 src/CUDA/GPU_point_to_point_real.cu:38-79 / src/ICP_CPU.c:220-234
    point_to_point(D, M, ...) -> Result   src/ICP_point_to_point.cu:295-423 / src/ICP_CPU.c:217-271
    point_to_plane(D, M, ...) -> Result   src/ICP_point_to_plane.cu:517-631

Clouds are (N, 3) arrays, float32 or float64 (the dtype selects the device arithmetic), i.e. the
reference's AoS "xyzxyz" GPU layout.  No arithmetic happens here.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi


@dataclass
class Result:
    T: np.ndarray            # (4, 4) composed transform, moving -> model
    iterations: int          # the reference's loop counter at exit
    passes: int              # matching passes that contributed to T
    err: np.ndarray          # err[0] = 0, err[k] = RMS error after pass k-1 (length passes + 1)
    idx: np.ndarray          # (N,) int32 correspondences of the last contributing pass
    moved: np.ndarray        # (N, 3) final moving cloud
    seconds_total: float = 0.0
    seconds_nn: float = 0.0
    seconds_host: float = 0.0    # host half of the iterations (error, stop rule, solve), summed; 0 unless profiling is on
    seconds_setup: float = 0.0   # icp_set_model (+ normals) + icp_set_moving inside the call
    extra: dict = field(default_factory=dict)


def _as_cloud(a, dtype=None):
    a = np.asarray(a)
    if dtype is None:
        dtype = a.dtype if a.dtype in (np.float32, np.float64) else np.float32
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("a cloud is an (N, 3) array")
    return a


def _prec(dtype):
    return capi.ICP_F64 if np.dtype(dtype) == np.float64 else capi.ICP_F32


class Context:
    """One `icp_ctx`: a HIP device, its stream and the HBM-resident clouds."""

    def __init__(self, device=0):
        self._lib = capi.load()
        h = C.c_void_p()
        capi.check(self._lib.icp_create(int(device), C.byref(h)), "icp_create")
        self._h = h
        self._dtype = None
        self._n = 0
        self._m = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- plumbing ------------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        capi.check(self._lib.icp_set_stream(self._h, C.c_void_p(hip_stream or 0)), "icp_set_stream")

    def set_exclusive(self, on=True):
        """the caller owns the device: hall-sized clouds run 16-wave blocks, one to a CU (same bits, ~4 % faster)"""
        capi.check(self._lib.icp_set_exclusive(self._h, 1 if on else 0), "icp_set_exclusive")

    def set_profiling(self, every_nth=1):
        """time every n-th matching launch of the loop with HIP events (0 / False = off)"""
        capi.check(self._lib.icp_set_profiling(self._h, int(every_nth)), "icp_set_profiling")

    # ---- multi-GPU: library-issued RCCL all-reduce ----------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * 128)()
        capi.check(capi.load().icp_comm_unique_id(buf), "icp_comm_unique_id")
        return bytes(buf)

    def comm_init(self, id_bytes, rank, world):
        buf = (C.c_ubyte * 128).from_buffer_copy(id_bytes)
        capi.check(self._lib.icp_comm_init(self._h, buf, int(rank), int(world)), "icp_comm_init")

    def comm_destroy(self):
        capi.check(self._lib.icp_comm_destroy(self._h), "icp_comm_destroy")

    @staticmethod
    def comm_random_id():
        buf = (C.c_ubyte * 128)()
        capi.check(capi.load().icp_comm_random_id(buf), "icp_comm_random_id")
        return bytes(buf)

    def comm_init_local(self, id_bytes, rank, world):
        """ranks of ONE node: the loop's vector is exchanged through shared host memory (the resident loop stays on)"""
        buf = (C.c_ubyte * 128).from_buffer_copy(id_bytes)
        capi.check(self._lib.icp_comm_init_local(self._h, buf, int(rank), int(world)), "icp_comm_init_local")

    # ---- matching seam -------------------------------------------------------------------------
    def Matching(self, P, Q):
        """idx[i] = argmin_j |P_i - Q_j|^2, lowest j on ties (reference `Matching` kernel)."""
        P = _as_cloud(P)
        Q = _as_cloud(Q, P.dtype)
        idx = np.empty(P.shape[0], dtype=np.int32)
        fn = self._lib.icp_nn_match_f64 if P.dtype == np.float64 else self._lib.icp_nn_match_f32
        capi.check(fn(self._h, P.ctypes.data, P.shape[0], Q.ctypes.data, Q.shape[0], idx.ctypes.data), "icp_nn_match")
        self._dtype, self._n, self._m = P.dtype, P.shape[0], Q.shape[0]
        return idx

    nn_match = Matching

    # ---- resident clouds -----------------------------------------------------------------------
    def set_model(self, Q):
        Q = _as_cloud(Q)
        capi.check(self._lib.icp_set_model(self._h, Q.ctypes.data, Q.shape[0], _prec(Q.dtype)), "icp_set_model")
        self._dtype, self._m = Q.dtype, Q.shape[0]

    def set_moving(self, P):
        P = _as_cloud(P, self._dtype)
        capi.check(self._lib.icp_set_moving(self._h, P.ctypes.data, P.shape[0], _prec(P.dtype)), "icp_set_moving")
        self._dtype, self._n = P.dtype, P.shape[0]

    def set_model_normals(self, Nrm):
        Nrm = _as_cloud(Nrm, self._dtype)
        capi.check(self._lib.icp_set_model_normals(self._h, Nrm.ctypes.data, Nrm.shape[0]), "icp_set_model_normals")

    def reset_moving(self):
        capi.check(self._lib.icp_reset_moving(self._h), "icp_reset_moving")

    def get_moving(self):
        out = np.empty((self._n, 3), dtype=self._dtype)
        capi.check(self._lib.icp_get_moving(self._h, out.ctypes.data), "icp_get_moving")
        return out

    def get_indices(self):
        out = np.empty(self._n, dtype=np.int32)
        capi.check(self._lib.icp_get_indices(self._h, out.ctypes.data), "icp_get_indices")
        return out

    def nn_match_resident(self, timed=False):
        ms = C.c_float(0)
        capi.check(self._lib.icp_nn_match_resident(self._h, C.byref(ms) if timed else None), "icp_nn_match_resident")
        return ms.value

    def nn_match_bench(self, reps, seeded=True):
        ms = C.c_float(0)
        capi.check(self._lib.icp_nn_match_bench_ex(self._h, int(reps), 1 if seeded else 0, C.byref(ms)), "icp_nn_match_bench_ex")
        return ms.value

    def nn_match_bench_launches(self, reps=10, warmups=2, mode=0):
        """per-launch hipEvent durations [ms] of the matching kernel (reference method: Matching_opt.cu:213-226);
        mode 0 seeded, 1 cold, 2 the dense packed kernel that executes every pair"""
        out = np.zeros(int(reps), dtype=np.float32)
        capi.check(self._lib.icp_nn_match_bench_launches(self._h, int(reps), int(warmups), int(mode),
                                                         out.ctypes.data_as(C.POINTER(C.c_float))), "icp_nn_match_bench_launches")
        return out

    def nn_launch_info_ex(self, dense=False):
        v = [C.c_int(0) for _ in range(5)]
        capi.check(self._lib.icp_nn_launch_info_ex(self._h, 1 if dense else 0, *[C.byref(x) for x in v]), "icp_nn_launch_info_ex")
        return dict(zip(("splits", "blocks", "threads", "n_pad", "m_pad"), (x.value for x in v)))

    WORK_SLOTS = ("find_boxes", "upper_boxes", "hits_box", "hits_xy", "hits_full", "sample_groups", "block_passes", "block_transforms",
                  "spec_lists", "spec_covered", "spec_hits", "list_hits")

    def set_work_counting(self, enable=True):
        capi.check(self._lib.icp_set_work_counting(self._h, 1 if enable else 0), "icp_set_work_counting")

    def get_work_counters(self, reset=True):
        out = np.zeros(12, dtype=np.uint64)
        capi.check(self._lib.icp_get_work_counters(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if reset else 0),
                   "icp_get_work_counters")
        return dict(zip(self.WORK_SLOTS, (int(x) for x in out)))

    def diag_row_roles(self, hits, min_part=2048, total_div=4096, control=True):
        """the roles of an ordered launch's blocks from its rows' hit counters, by the device kernels the loop uses (icp_diag_row_roles)"""
        h = np.ascontiguousarray(hits, dtype=np.uint32).copy()
        roles = np.zeros(h.size + 4096, dtype=np.int32)
        capi.check(self._lib.icp_diag_row_roles(self._h, h.ctypes.data_as(C.POINTER(C.c_uint32)), int(h.size), int(min_part), int(total_div), 1 if control else 0,
                                                roles.ctypes.data_as(C.POINTER(C.c_int32))), "icp_diag_row_roles")
        return roles, h

    def diag_loop_moments(self):
        """(the ICP_NMOM vector the loop's host half last received, its ROUTE_* bits): icp_diag_loop_moments"""
        mom = np.zeros(capi.ICP_NMOM, dtype=np.float64)
        route = C.c_int(0)
        capi.check(self._lib.icp_diag_loop_moments(self._h, mom.ctypes.data_as(C.POINTER(C.c_double)), C.byref(route)), "icp_diag_loop_moments")
        return mom, route.value

    def diag_knn4_geometry(self, m):
        """the launch shape of the fp32 neighbour search of an m-point model on this context (icp_diag_knn4_geometry): dict of
        n_pad, blocks_x, splits, seg_len and tiles (LDS tiles per wave); arithmetic alone, nothing is launched"""
        out = (C.c_int * 5)()
        capi.check(self._lib.icp_diag_knn4_geometry(self._h, int(m), out), "icp_diag_knn4_geometry")
        return dict(zip(("n_pad", "blocks_x", "splits", "seg_len", "tiles"), (int(x) for x in out)))

    def nn_launch_info(self):
        v = [C.c_int(0) for _ in range(5)]
        capi.check(self._lib.icp_nn_launch_info(self._h, *[C.byref(x) for x in v]), "icp_nn_launch_info")
        return dict(zip(("splits", "blocks", "threads", "n_pad", "m_pad"), (x.value for x in v)))

    def estimate_normals(self, want_neighbours=False):
        nrm = np.empty((self._m, 3), dtype=self._dtype)
        nbr = np.empty((self._m, 4), dtype=np.int32) if want_neighbours else None
        capi.check(self._lib.icp_estimate_normals(self._h, nrm.ctypes.data, nbr.ctypes.data if want_neighbours else None),
                   "icp_estimate_normals")
        return (nrm, nbr) if want_neighbours else nrm

    # ---- full loops ----------------------------------------------------------------------------
    def _run(self, metric, D, M, normals, max_iter, tol, fixed_iterations):
        D = _as_cloud(D)
        M = _as_cloud(M, D.dtype)
        n, m = D.shape[0], M.shape[0]
        prm = capi.icp_params(int(max_iter), float(tol), 1 if fixed_iterations else 0, _prec(D.dtype), metric)
        err = np.zeros(int(max_iter) + 1, dtype=np.float64)
        idx = np.zeros(n, dtype=np.int32)
        moved = np.zeros((n, 3), dtype=D.dtype)
        res = capi.icp_result()
        res.err = err.ctypes.data_as(C.POINTER(C.c_double))
        res.idx = idx.ctypes.data_as(C.POINTER(C.c_int32))
        res.moved = moved.ctypes.data
        if metric == capi.ICP_POINT_TO_PLANE:
            nptr = None
            if normals is not None:
                normals = _as_cloud(normals, D.dtype)
                nptr = normals.ctypes.data
            rc = self._lib.icp_point_to_plane(self._h, D.ctypes.data, n, M.ctypes.data, m, nptr, C.byref(prm), C.byref(res))
            capi.check(rc, "icp_point_to_plane")
        else:
            rc = self._lib.icp_point_to_point(self._h, D.ctypes.data, n, M.ctypes.data, m, C.byref(prm), C.byref(res))
            capi.check(rc, "icp_point_to_point")
        self._dtype, self._n, self._m = D.dtype, n, m
        return Result(T=np.array(res.T[:], dtype=np.float64).reshape(4, 4), iterations=res.iterations,
                      passes=res.passes, err=err[: res.passes + 1].copy(), idx=idx, moved=moved,
                      seconds_total=res.seconds_total, seconds_nn=res.seconds_nn,
                      seconds_host=res.seconds_host, seconds_setup=res.seconds_setup)

    def point_to_point(self, D, M, max_iter=40, tol=1e-6, fixed_iterations=False):
        return self._run(capi.ICP_POINT_TO_POINT, D, M, None, max_iter, tol, fixed_iterations)

    def point_to_plane(self, D, M, normals=None, max_iter=50, tol=1e-6, fixed_iterations=False):
        return self._run(capi.ICP_POINT_TO_PLANE, D, M, normals, max_iter, tol, fixed_iterations)

    # ---- batched ICP (icp_batch_*): many independent pairs, one launch per step -----------------------
    def batch(self, pairs):
        """a Batch of (D, M) pairs of one dtype, uploaded once (see Batch)"""
        return Batch(self, pairs)

    def point_to_point_batch(self, pairs, max_iter=40, tol=1e-6, fixed_iterations=False, max_distance=None, init=None, trim=None):
        """point_to_point for every (D, M) of `pairs` (one dtype) in one batched registration; a list of Result in pair order,
        each exactly what point_to_point gives for that pair alone (extra["status"]: ICP_OK or the code that ended its loop).
        max_distance (a scalar or one value per pair, inf = that pair is not gated): a match farther away than that pulls on
        nothing (Batch.set_max_distance); extra["inliers"] is then the mask of the last contributing pass and extra["fitness"]
        the share of the points it kept.
        init (one (4, 4) for every pair, or (count, 4, 4)): the pose every pair starts from (Batch.set_initial_transforms); the
        gate then acts on distances measured after it, and Result.T includes it.  Runs through a Batch as max_distance does.
        trim (a scalar or one value per pair, each in (0, 1]; 1.0 = that pair is not trimmed): the share of every moving cloud to
        keep -- the closest matches of every pass, ties with the last one included (Batch.set_trim); extra["inliers"] and
        extra["fitness"] as for max_distance.  Runs through a Batch too."""
        if max_distance is not None or init is not None or trim is not None:
            return self._run_batch_gated(capi.ICP_POINT_TO_POINT, pairs, None, max_iter, tol, fixed_iterations, max_distance, init, trim)
        return self._run_batch(capi.ICP_POINT_TO_POINT, pairs, None, max_iter, tol, fixed_iterations)

    def point_to_plane_batch(self, pairs, normals=None, max_iter=50, tol=1e-6, fixed_iterations=False):
        """point_to_plane for every (D, M) of `pairs` in one batched registration, as point_to_point_batch; normals: one (m, 3)
        array per pair, or None (then estimated on the device: one neighbour launch + one normals launch for all pairs)"""
        return self._run_batch(capi.ICP_POINT_TO_PLANE, pairs, normals, max_iter, tol, fixed_iterations)

    def point_to_plane_batch_gated(self, pairs, max_distance, normals=None, max_iter=50, tol=1e-6, fixed_iterations=False, init=None, trim=None):
        """point_to_plane_batch with a maximum correspondence distance (a scalar or one value per pair, or None; the gate is on the
        Euclidean distance to the matched point), as point_to_point_batch(max_distance=...): extra["inliers"], extra["fitness"];
        init and trim as there.
        (point_to_plane_batch itself keeps its parameter list, which tests/test_batch_plane_abi.py holds fixed.)"""
        return self._run_batch_gated(capi.ICP_POINT_TO_PLANE, pairs, normals, max_iter, tol, fixed_iterations, max_distance, init, trim)

    def register_batch(self, pairs, metric=capi.ICP_POINT_TO_POINT, normals=None, max_iter=None, tol=1e-6, fixed_iterations=False,
                       max_distance=None, init=None, trim=None, reciprocal=None):
        """the one-call entry that takes every option of a batch: metric (ICP_POINT_TO_POINT, or ICP_POINT_TO_PLANE with normals --
        one (m, 3) array per pair, or None: estimated on the device), max_iter (None: 40 for point-to-point, 50 for
        point-to-plane, the defaults of point_to_point_batch / point_to_plane_batch), max_distance, init and trim as
        point_to_point_batch takes them, and reciprocal (None: off; a bool for every pair; or one flag per pair): a reciprocal
        pair keeps only mutual nearest neighbours (Batch.set_reciprocal).  Always runs through a Batch; a list of Result in pair
        order with extra["status"], extra["inliers"] (the mask of the last contributing pass) and extra["fitness"]."""
        max_iter = _default_max_iter("register_batch", metric, max_iter)
        return self._run_batch_gated(metric, pairs, normals, max_iter, tol, fixed_iterations, max_distance, init, trim, reciprocal)

    def register_batch_robust(self, pairs, kernel, scale, **options):
        """register_batch with a robust kernel: kernel ("huber", "cauchy", "tukey", None or an ICP_ROBUST_* integer) and scale (the
        kernel's k, in the clouds' unit) for every pair, or one of each per pair (Batch.set_robust).  Every kept match pulls with a
        weight in [0, 1] that falls smoothly with its residual; the loop is iteratively re-weighted least squares.  options:
        register_batch's, by keyword.  The same list of Result, with extra["weights"] added: the (n,) float64 weights of each
        pair's most recent matching pass (0.0 where the match was rejected)."""
        _known_options("register_batch_robust", options)
        return self._run_batch_keywords("register_batch_robust", options.get("metric", capi.ICP_POINT_TO_POINT), pairs, options, (kernel, scale))

    def register_batch_generalized(self, pairs, k=20, regularisation="frobenius", lam=1e-3, covariances=None, **options):
        """register_batch with the generalized (plane-to-plane) metric: every kept match pulls with the inverse of the summed
        local covariances of both clouds at the match (Batch.begin with ICP_GENERALIZED).  The covariances are estimated on the
        device from the k nearest neighbours of every point (k: one value, or (k_moving, k_model), each a scalar or one per pair;
        regularisation and lam as Batch.estimate_covariances takes them), or given: covariances = (moving, model), one (n, 6) and
        one (m, 6) float64 array per pair (Batch.set_covariances; covariances_from_normals makes them from good normals).
        options: register_batch's, by keyword, without metric and normals; robust kernels are not combined with this metric.  The
        same list of Result as register_batch."""
        _known_options("register_batch_generalized", options)

        def prepare(bt):
            if covariances is not None:
                moving, model = covariances
                bt.set_covariances(moving, model)
            else:
                bt._estimate_covariances_k(k, regularisation, lam)

        return self._run_batch_keywords("register_batch_generalized", capi.ICP_GENERALIZED, pairs, options, prepare=prepare)

    def register_batch_colored(self, pairs, intensities, k=8, lam=capi.ICP_COLOR_LAMBDA_DEFAULT, normals=None, **options):
        """register_batch with the colored metric (Park, Zhou, Koltun, ICCV 2017; Batch.begin with ICP_COLORED): every kept match
        pulls with its point-to-plane residual, weighed by lam, and with the difference between the moving point's intensity and
        the model's intensity field at the point's foot in the tangent plane, weighed by 1 - lam -- what registers flat or gently
        curved textured surfaces, which geometry alone leaves free to slide.  intensities = (moving, model): per side one (points,)
        float64 array per pair (intensity_from_rgb makes them from colours); k: the neighbours of the gradient estimate, a scalar
        or one per pair; lam: a scalar or one per pair, in [0, 1]; normals: one (m, 3) array per pair, or None: estimated on the
        device.  options: register_batch's, by keyword, without metric and normals; robust kernels are not combined with this
        metric.  The same list of Result as register_batch."""
        _known_options("register_batch_colored", options)
        moving, model = intensities

        def prepare(bt):
            bt._model_normals(normals)
            bt.set_intensities(moving, model)
            bt.estimate_intensity_gradients(k)
            bt.set_color_weight(lam)

        return self._run_batch_keywords("register_batch_colored", capi.ICP_COLORED, pairs, options, prepare=prepare)

    def register_batch_symmetric(self, pairs, k=20, orient="centroid", normals=None, **options):
        """register_batch with the symmetric metric (Rusinkiewicz, SIGGRAPH 2019; Batch.begin with ICP_SYMMETRIC): every kept match
        pulls along the sum of the two points' own normals and the step is split into two half rotations, so the residual vanishes
        wherever the two points lie on a common second-order patch -- a wider basin than point-to-plane's after a rough start, and
        no bias from the two clouds sampling the surface differently.  normals = (moving, model): per side one (points, 3) float64
        array of unit normals per pair (Batch.set_point_normals; their signs need not agree), or None: estimated on the device
        from the covariances of k neighbours (Batch.estimate_covariances(k): a scalar or one value per pair, both sides) and
        oriented by orient (Batch.estimate_point_normals).  options: register_batch's, by keyword, without metric and normals;
        robust kernels are not combined with this metric.  The same list of Result as register_batch."""
        _known_options("register_batch_symmetric", options)

        def prepare(bt):
            if normals is not None:
                moving, model = normals
                bt.set_point_normals(moving, model)
            else:
                bt.estimate_covariances(k)
                bt.estimate_point_normals(orient)

        return self._run_batch_keywords("register_batch_symmetric", capi.ICP_SYMMETRIC, pairs, options, prepare=prepare)

    def register_batch_global(self, pairs, voxel, k, hypotheses, max_distance, **options):
        """register_batch for pairs in unknown relative pose: a start pose from descriptors first, then the local loop from it.
        The pairs are uploaded once; a copy thinned at voxel (Batch.downsample; 0 or None: the clouds themselves) gets raw
        covariances from k neighbours (ICP_COV_NONE), normals from them (oriented_normals, facing viewpoint -- None: each cloud's
        own centroid, which no rigid motion changes), FPFH descriptors from the same k (Batch.compute_features), mutual matches
        (Batch.match_features) and a RANSAC pose (Batch.ransac with hypotheses, max_distance and the options edge_similarity,
        0.9, and seed, 0); register_batch then runs on the full pairs with init = those poses.  options: besides viewpoint,
        edge_similarity, seed and mutual (True), register_batch's by keyword without init; gate is handed on as its max_distance.
        The same list of Result, with extra["global"] added: the dict Batch.ransac returned for the pair.
        method="fgr" (the default is "ransac") runs Batch.fgr in RANSAC's place: hypotheses is read as tuples (0: every
        correspondence) and max_distance as delta; the options iterations, division_factor, decrease_every and tuple_similarity are
        handed on where given, seed too; extra["global"] is then the dict Batch.fgr returned.
        keypoints=rule (Batch.keypoints' rule, one for all pairs or one per pair; the default is None) matches and solves on the
        ISS keypoints of the thinned clouds alone: the descriptors are computed on the whole thinned clouds as before, then
        Batch.keypoints(moving=rule, model=rule) keeps the salient points with their descriptors, and matching and RANSAC or FGR
        run on that batch; extra["global"] gains "keypoints": (n_kept, m_kept).
        device_normals=True (the default is False) makes the normals on the device from the covariances
        (Batch.estimate_point_normals, facing the centroids, or viewpoint where given) and describes from them
        (Batch.compute_features_stored): no clouds and no covariances come down, no normals go up.  The Jacobi's and LAPACK's
        vectors differ in the last bits, so descriptors and poses can differ from the default route's.
        planes=rule (Batch.segment_plane's rule, one for all pairs or one per pair; the default is None) applies the rule to both
        clouds of every pair before downsampling -- ("remove", distance) takes the dominant plane out, so that a floor or a wall
        neither fills the match list with ties nor lets the pose slide; seed is handed on.  The start pose is found on those
        clouds; the local loop runs on the full pairs as before.  extra["global"] gains "planes": the (2, 4) planes of the pair's
        moving cloud and model, and "plane_inliers": their two counts."""
        _known_options("register_batch_global", options)
        method = options.get("method", "ransac")
        if method not in ("ransac", "fgr"):
            raise ValueError(f"register_batch_global: method must be 'ransac' or 'fgr', not {method!r}")
        pairs = list(pairs)
        v = 0.0 if voxel is None else float(voxel)
        with Batch(self, pairs) as full:
            cut, cut_info = full, None
            if options.get("planes") is not None:
                cut, cut_info = full.segment_plane(moving=options["planes"], model=options["planes"], seed=options.get("seed", 0))
            try:
                bt = cut if v == 0.0 else cut.downsample(v)
            except Exception:
                if cut is not full:
                    cut.close()
                raise
            try:
                view = options.get("viewpoint")
                if options.get("device_normals", False):   # nothing comes down, nothing goes up
                    bt.estimate_covariances(k, None, regularisation="none", want=False)
                    bt.estimate_point_normals("centroid" if view is None else "viewpoint", viewpoints=view)
                    bt.compute_features_stored(k)
                else:
                    cm, cq = bt.estimate_covariances(k, None, regularisation="none", want=True)
                    clouds = bt.get_clouds()
                    eye = lambda X: X.astype(np.float64).mean(0) if view is None else view
                    nm = [oriented_normals(D, c, eye(D)) for (D, _), c in zip(clouds, cm)]
                    nq = [oriented_normals(M, c, eye(M)) for (_, M), c in zip(clouds, cq)]
                    bt.compute_features(k, (nm, nq))
                kb, kept = bt, None
                if options.get("keypoints") is not None:   # match and solve on the salient points alone, with their descriptors
                    kb, info = bt.keypoints(moving=options["keypoints"], model=options["keypoints"])
                    kept = [(int(info["counts"][b]), int(info["counts"][bt.count + b])) for b in range(bt.count)]
                try:
                    kb.match_features(mutual=options.get("mutual", True))
                    if method == "fgr":
                        more = {o: options[o] for o in ("iterations", "division_factor", "decrease_every", "tuple_similarity") if o in options}
                        start = kb.fgr(max_distance, tuples=hypotheses, seed=options.get("seed", 0), **more)
                    else:
                        start = kb.ransac(hypotheses, max_distance, edge_similarity=options.get("edge_similarity", 0.9), seed=options.get("seed", 0))
                finally:
                    if kb is not bt:
                        kb.close()
                if kept is not None:
                    for r, c in zip(start, kept):
                        r["keypoints"] = c
                if cut_info is not None:
                    for b, r in enumerate(start):
                        r["planes"] = cut_info["planes"][[b, full.count + b]].copy()
                        r["plane_inliers"] = (int(cut_info["inliers"][b]), int(cut_info["inliers"][full.count + b]))
            finally:
                if bt is not cut:
                    bt.close()
                if cut is not full:
                    cut.close()
        T0 = np.stack([r["T"] for r in start])
        rest = {o: options[o] for o in ("metric", "normals", "max_iter", "tol", "fixed_iterations", "trim", "reciprocal") if o in options}
        out = self.register_batch(pairs, max_distance=options.get("gate"), init=T0, **rest)
        for res, r in zip(out, start):
            res.extra["global"] = r
        return out

    def register_batch_multiscale(self, pairs, voxels, **options):
        """coarse-to-fine register_batch on a voxel pyramid made on the device: the pairs are uploaded once, and level l runs on
        that batch thinned at voxels[l] (Batch.downsample; 0 or None: full resolution, the uploaded batch itself).  voxels:
        coarsest first.  Level 0 starts from init, level l + 1 from the T every pair's state reported at level l, whatever its
        status.  options: register_batch's, by keyword, plus kernel and scale as register_batch_robust takes them.
        max_distance: one value or one per pair (every level), or a list or tuple of len(voxels) such values, one per level (a
        list of that length always reads per level: give per-pair values as an array).
        Point-to-plane levels estimate their own normals on the device; normals given together with a level that downsamples is
        a ValueError.  Returns the last level's list of Result; each carries extra["levels"]: per level a dict of voxel, n, m,
        status, iterations and T.
        metric ICP_GENERALIZED: every level estimates the covariances of its own clouds on the device; the options k,
        regularisation and lam are then read as register_batch_generalized takes them."""
        _known_options("register_batch_multiscale", options)
        voxels = [0.0 if v is None else float(v) for v in voxels]
        if not voxels:
            raise ValueError("register_batch_multiscale needs at least one level")
        metric = options.get("metric", capi.ICP_POINT_TO_POINT)
        normals = options.get("normals")
        if normals is not None and any(v != 0.0 for v in voxels):
            raise ValueError("caller-given normals cannot follow a downsampled model: every level estimates its own")
        max_iter = _default_max_iter("register_batch_multiscale", metric, options.get("max_iter"))
        gate = options.get("max_distance")
        per_level = isinstance(gate, (list, tuple)) and len(gate) == len(voxels)
        robust = (options["kernel"], options.get("scale")) if options.get("kernel") is not None else None
        with Batch(self, pairs) as full:
            T = options.get("init")
            levels = [[] for _ in range(full.count)]
            out = None
            for l, v in enumerate(voxels):
                bt = full if v == 0.0 else full.downsample(v)
                try:
                    if metric == capi.ICP_POINT_TO_PLANE:
                        bt._model_normals(normals)
                    if metric == capi.ICP_GENERALIZED:
                        bt._estimate_covariances_k(options.get("k", 20), options.get("regularisation", "frobenius"), options.get("lam", 1e-3))
                    states = bt._drive(metric, max_iter, options.get("tol", 1e-6), options.get("fixed_iterations", False),
                                       gate[l] if per_level else gate, T, options.get("trim"), options.get("reciprocal"), robust)
                    T = np.stack([st["T"] for st in states])
                    for b, st in enumerate(states):
                        levels[b].append({"voxel": v, "n": int(bt._moff[b + 1] - bt._moff[b]), "m": int(bt._qoff[b + 1] - bt._qoff[b]),
                                          "status": st["status"], "iterations": st["iterations"], "T": st["T"].copy()})
                    if l == len(voxels) - 1:
                        out = bt._results(states, robust is not None)
                        for b, res in enumerate(out):
                            res.extra["levels"] = levels[b]
                finally:
                    if bt is not full:
                        bt.close()
            return out

    def _run_batch_gated(self, metric, pairs, normals, max_iter, tol, fixed_iterations, max_distance, init=None, trim=None, reciprocal=None):
        """the one-call functions have neither a gate nor initial transforms nor trimming nor reciprocity: create, [normals],
        set_max_distance, set_initial_transforms, set_trim, set_reciprocal, begin, run to the end, results"""
        return self._run_batch_options(metric, pairs, normals, max_iter, tol, fixed_iterations, max_distance, init, trim, reciprocal, None)

    def _run_batch_options(self, metric, pairs, normals, max_iter, tol, fixed_iterations, max_distance, init, trim, reciprocal, robust, prepare=None):
        """... and robust: None, or (kernel, scale) for set_robust -- the results then carry extra["weights"]; prepare: None, or a
        callable that gives the new Batch what its metric needs beyond normals (the colored metric's intensities and gradients, the
        symmetric metric's point normals)"""
        with Batch(self, pairs) as bt:
            if prepare is not None:
                prepare(bt)
            if metric == capi.ICP_POINT_TO_PLANE:
                bt._model_normals(normals)
            states = bt._drive(metric, max_iter, tol, fixed_iterations, max_distance, init, trim, reciprocal, robust)
            return bt._results(states, robust is not None)

    def _run_batch_keywords(self, where, metric, pairs, options, robust=None, prepare=None):
        """_run_batch_options from the **options of the entry point `where`, with that entry point's default max_iter"""
        return self._run_batch_options(metric, pairs, options.get("normals"), _default_max_iter(where, metric, options.get("max_iter")),
                                       options.get("tol", 1e-6), options.get("fixed_iterations", False), options.get("max_distance"),
                                       options.get("init"), options.get("trim"), options.get("reciprocal"), robust, prepare=prepare)

    def _run_batch(self, metric, pairs, normals, max_iter, tol, fixed_iterations):
        Ds, Ms, moff, qoff, dtype = _batch_arrays(pairs)
        count, cap = len(Ds), int(max_iter) + 1
        prm = capi.icp_params(int(max_iter), float(tol), 1 if fixed_iterations else 0, _prec(dtype), metric)
        T = np.zeros((count, 16))
        it, ps, st = (np.zeros(count, dtype=np.int32) for _ in range(3))
        err = np.zeros((count, cap))
        idx = np.zeros(int(moff[-1]), dtype=np.int32)
        moved = np.zeros((int(moff[-1]), 3), dtype=dtype)
        D, M = np.concatenate(Ds), np.concatenate(Ms)
        pi, pd, p64 = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        outs = (T.ctypes.data_as(pd), it.ctypes.data_as(pi), ps.ctypes.data_as(pi), err.ctypes.data_as(pd),
                idx.ctypes.data_as(C.POINTER(C.c_int32)), moved.ctypes.data, st.ctypes.data_as(pi))
        if metric == capi.ICP_POINT_TO_PLANE:
            N = _batch_normals(normals, [M.shape for M in Ms], dtype) if normals is not None else None
            rc = self._lib.icp_point_to_plane_batch(self._h, count, D.ctypes.data, moff.ctypes.data_as(p64), M.ctypes.data, qoff.ctypes.data_as(p64),
                                                    N.ctypes.data if N is not None else None, C.byref(prm), *outs)
            capi.check(rc, "icp_point_to_plane_batch")
        else:
            rc = self._lib.icp_point_to_point_batch(self._h, count, D.ctypes.data, moff.ctypes.data_as(p64), M.ctypes.data, qoff.ctypes.data_as(p64),
                                                    C.byref(prm), *outs)
            capi.check(rc, "icp_point_to_point_batch")
        return [Result(T=T[b].reshape(4, 4).copy(), iterations=int(it[b]), passes=int(ps[b]), err=err[b, : ps[b] + 1].copy(),
                       idx=idx[moff[b]:moff[b + 1]].copy(), moved=moved[moff[b]:moff[b + 1]].copy(), extra={"status": int(st[b])})
                for b in range(count)]

    # ---- step-wise loop (multi-GPU driver, per-iteration parity tests) -------------------------
    def loop_begin(self, metric=capi.ICP_POINT_TO_POINT, max_iter=40, tol=1e-6, fixed_iterations=False):
        prm = capi.icp_params(int(max_iter), float(tol), 1 if fixed_iterations else 0, _prec(self._dtype), metric)
        capi.check(self._lib.icp_loop_begin(self._h, C.byref(prm)), "icp_loop_begin")
        self._max_iter = int(max_iter)

    def loop_enqueue(self):
        capi.check(self._lib.icp_loop_enqueue(self._h), "icp_loop_enqueue")

    def loop_moments_dev(self):
        return self._lib.icp_loop_moments_dev(self._h)

    def loop_set_moments_dev(self, dev_ptr):
        capi.check(self._lib.icp_loop_set_moments_dev(self._h, C.c_void_p(dev_ptr or 0)), "icp_loop_set_moments_dev")

    def loop_complete(self):
        done = C.c_int(0)
        capi.check(self._lib.icp_loop_complete(self._h, C.byref(done)), "icp_loop_complete")
        return bool(done.value)

    def loop_run(self, max_steps):
        """up to max_steps iterations inside the library; returns (steps_done, done)"""
        k, d = C.c_int(0), C.c_int(0)
        capi.check(self._lib.icp_loop_run(self._h, int(max_steps), C.byref(k), C.byref(d)), "icp_loop_run")
        return k.value, bool(d.value)

    def recoveries(self):
        """registrations this context finished step-wise after a resident / armed pass never delivered its rows"""
        return int(self._lib.icp_recoveries(self._h))

    def loop_state(self):
        it, ps = C.c_int(0), C.c_int(0)
        err = np.zeros(self._max_iter + 1, dtype=np.float64)
        T = np.zeros(16, dtype=np.float64)
        capi.check(self._lib.icp_loop_state(self._h, C.byref(it), C.byref(ps), err.ctypes.data_as(C.POINTER(C.c_double)),
                                            err.size, T.ctypes.data_as(C.POINTER(C.c_double))), "icp_loop_state")
        return dict(iterations=it.value, passes=ps.value, err=err[: ps.value + 1].copy(), T=T.reshape(4, 4))

    def loop_timing(self):
        sec, cnt = C.c_double(0), C.c_int(0)
        capi.check(self._lib.icp_loop_timing(self._h, C.byref(sec), C.byref(cnt)), "icp_loop_timing")
        return sec.value, cnt.value

    def loop_phase_seconds(self):
        """(matching-kernel seconds, host-solve seconds) of the current / last loop; both 0 unless profiling is on"""
        a, b = C.c_double(0), C.c_double(0)
        capi.check(self._lib.icp_loop_phase_seconds(self._h, C.byref(a), C.byref(b)), "icp_loop_phase_seconds")
        return a.value, b.value

    def loop_timing_passes(self):
        n = C.c_longlong(0)
        capi.check(self._lib.icp_loop_timing_passes(self._h, C.byref(n)), "icp_loop_timing_passes")
        return n.value

    def loop_indices(self):
        out = np.empty(self._n, dtype=np.int32)
        capi.check(self._lib.icp_loop_indices(self._h, out.ctypes.data), "icp_loop_indices")
        return out

    # ---- hall ingest ---------------------------------------------------------------------------
    def os1_to_cartesian(self, ranges, encoder_count0, altitude16, azimuth16):
        r = np.ascontiguousarray(ranges, dtype=np.uint32)
        alt = np.ascontiguousarray(altitude16, dtype=np.float32)
        az = np.ascontiguousarray(azimuth16, dtype=np.float32)
        out = np.empty((r.size, 3), dtype=np.float32)
        pf = C.POINTER(C.c_float)
        capi.check(self._lib.icp_os1_to_cartesian(self._h, r.ctypes.data, r.size, int(encoder_count0),
                                                  alt.ctypes.data_as(pf), az.ctypes.data_as(pf), out.ctypes.data),
                   "icp_os1_to_cartesian")
        return out


    def os1_packets_to_cartesian(self, packets, altitude16, azimuth16):
        """raw packet bytes (uint8, n_packets * 12608) -> (xyz [mm] (N,3) float32, ranges (N,) uint32), decoded on the device"""
        pk = np.ascontiguousarray(packets, dtype=np.uint8).reshape(-1)
        assert pk.size % 12608 == 0
        npk = pk.size // 12608
        alt = np.ascontiguousarray(altitude16, dtype=np.float32)
        az = np.ascontiguousarray(azimuth16, dtype=np.float32)
        xyz = np.empty((npk * 256, 3), dtype=np.float32)
        rng = np.empty(npk * 256, dtype=np.uint32)
        pf = C.POINTER(C.c_float)
        capi.check(self._lib.icp_os1_packets_to_cartesian(self._h, pk.ctypes.data, npk, alt.ctypes.data_as(pf), az.ctypes.data_as(pf),
                                                          xyz.ctypes.data, rng.ctypes.data), "icp_os1_packets_to_cartesian")
        return xyz, rng


def _batch_arrays(pairs):
    """(D, M) pairs -> the clouds as contiguous arrays of one dtype and the int64 offsets of their concatenation"""
    pairs = list(pairs)
    if not pairs:
        raise ValueError("a batch needs at least one pair")
    dtype = _as_cloud(pairs[0][0]).dtype
    Ds = [_as_cloud(D, dtype) for D, _ in pairs]
    Ms = [_as_cloud(M, dtype) for _, M in pairs]
    moff = np.concatenate([[0], np.cumsum([D.shape[0] for D in Ds])]).astype(np.int64)
    qoff = np.concatenate([[0], np.cumsum([M.shape[0] for M in Ms])]).astype(np.int64)
    return Ds, Ms, moff, qoff, dtype


def _ptr(a, ctype=C.c_double):
    """an optional array -> a pointer to its first element, or None (NULL)"""
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _batch_normals(normals, shapes, dtype):
    """one (m, 3) array of normals per pair -> their concatenation in the layout of the models, whose shapes are `shapes`"""
    normals = list(normals)
    if len(normals) != len(shapes):
        raise ValueError("one array of normals per pair")
    Ns = [_as_cloud(N, dtype) for N in normals]
    for N, shape in zip(Ns, shapes):
        if N.shape != shape:
            raise ValueError("a pair's normals must have the shape of its model")
    return np.concatenate(Ns)


# the batch entry points that take **options: the names each accepts ...
_LOOP_OPTIONS = {"max_iter", "tol", "fixed_iterations", "max_distance", "init", "trim", "reciprocal"}
_OPTIONS = {
    "register_batch_robust": _LOOP_OPTIONS | {"metric", "normals"},
    "register_batch_generalized": _LOOP_OPTIONS,
    "register_batch_colored": _LOOP_OPTIONS,
    "register_batch_symmetric": _LOOP_OPTIONS,
    "register_batch_multiscale": _LOOP_OPTIONS | {"metric", "normals", "kernel", "scale", "k", "regularisation", "lam"},
    "register_batch_global": (_LOOP_OPTIONS - {"max_distance", "init"}) | {
        "metric", "normals", "gate", "planes", "viewpoint", "edge_similarity", "seed", "mutual", "method", "iterations", "division_factor",
        "decrease_every", "tuple_similarity", "keypoints", "device_normals"},
}
# ... and the max_iter of a caller who gives none: by metric, under None for every other metric.  register_batch follows the
# one-call functions (50 is point_to_plane_batch's), the multiscale runs read it the other way round: they part at ICP_GENERALIZED
_MAX_ITER = {
    "register_batch": {capi.ICP_POINT_TO_PLANE: 50, None: 40},
    "register_batch_robust": {capi.ICP_POINT_TO_PLANE: 50, None: 40},
    "register_batch_multiscale": {capi.ICP_POINT_TO_POINT: 40, None: 50},
    "register_batch_generalized": {None: 50},
    "register_batch_colored": {None: 50},
    "register_batch_symmetric": {None: 50},
}


def _known_options(where, options):
    unknown = set(options) - _OPTIONS[where]
    if unknown:
        raise TypeError(f"{where}: unknown option(s) {sorted(unknown)}")


def _default_max_iter(where, metric, max_iter):
    if max_iter is not None:
        return max_iter
    return _MAX_ITER[where].get(metric, _MAX_ITER[where][None])


_ROBUST_KINDS = {None: capi.ICP_ROBUST_NONE, "none": capi.ICP_ROBUST_NONE, "huber": capi.ICP_ROBUST_HUBER,
                 "cauchy": capi.ICP_ROBUST_CAUCHY, "tukey": capi.ICP_ROBUST_TUKEY}


def _plane_rule(r):
    if r[0] not in _PLANE_KINDS:
        raise ValueError(f"unknown plane rule kind {r[0]!r}: 'detect', 'remove', 'keep' or None")
    ax = [float(x) for x in r[3]]
    if len(ax) != 3:
        raise ValueError("a plane rule's axis has three components")
    return capi.icp_plane_rule(_PLANE_KINDS[r[0]], int(r[2]), float(r[1]), (C.c_double * 3)(*ax), float(r[4]))


def _keypoint_rule(r):
    return capi.icp_keypoint_rule(capi.ICP_KEYPOINT_ISS, int(r[4]), float(r[0]), float(r[1]), float(r[2]), float(r[3]))


_PLANE_KINDS = {"detect": capi.ICP_PLANE_DETECT, "remove": capi.ICP_PLANE_REMOVE, "keep": capi.ICP_PLANE_KEEP}
# Batch._coded_rules: the struct, its NONE kind, what the first element of a single rule's tuple is, the fields of a rule as the
# caller writes it -- (name, default), the first two are required -- and the struct of such a tuple
_RULES = {
    "plane": (capi.icp_plane_rule, capi.ICP_PLANE_NONE, lambda x: isinstance(x, str),
              (("kind", None), ("distance", None), ("hypotheses", 1000), ("axis", (0, 0, 0)), ("min_cos", 0.0)), _plane_rule),
    "keypoint": (capi.icp_keypoint_rule, capi.ICP_KEYPOINT_NONE, np.isscalar,
                 (("salient_radius", None), ("non_max_radius", None), ("gamma_21", 0.975), ("gamma_32", 0.975), ("min_neighbours", 5)), _keypoint_rule),
}


class Batch:
    """icp_batch: (D, M) pairs of one dtype resident on the context's device; every step runs the pass of every pair still
    running in one launch.  Each pair's loop is the one Context.point_to_point (point_to_plane, with the batch's normals) runs
    for it alone.  Outputs are split per pair."""

    def __init__(self, ctx, pairs):
        Ds, Ms, moff, qoff, dtype = _batch_arrays(pairs)
        D, M = np.concatenate(Ds), np.concatenate(Ms)
        h = C.c_void_p()
        capi.check(ctx._lib.icp_batch_create(ctx._h, len(Ds), D.ctypes.data, _ptr(moff, C.c_int64), M.ctypes.data, _ptr(qoff, C.c_int64),
                                             _prec(dtype), C.byref(h)), "icp_batch_create")
        self._adopt(ctx, h, dtype, moff, qoff)

    @classmethod
    def _from_handle(cls, ctx, h, count, dtype):
        """a Batch around a ready icp_batch handle (Batch.downsample): its layout is read back with icp_batch_get_offsets"""
        self = cls.__new__(cls)
        moff, qoff = np.zeros(int(count) + 1, dtype=np.int64), np.zeros(int(count) + 1, dtype=np.int64)
        capi.check(ctx._lib.icp_batch_get_offsets(h, _ptr(moff, C.c_int64), _ptr(qoff, C.c_int64)), "icp_batch_get_offsets")
        self._adopt(ctx, h, dtype, moff, qoff)
        return self

    def _adopt(self, ctx, h, dtype, moff, qoff):
        """the fields of a Batch around the handle h, whose clouds lie at the int64 offsets moff and qoff"""
        self._ctx = ctx   # (keeps the context alive: a batch must go before it)
        self._lib = ctx._lib
        self._h = h
        self._max_iter = 0
        self._dtype = dtype
        self._moff, self._qoff = moff, qoff
        self.count = len(moff) - 1
        self._model_shapes = [(int(qoff[b + 1] - qoff[b]), 3) for b in range(self.count)]

    def _per_pair(self, v, what, dtype=np.float64):
        """a scalar for every pair, or one value per pair -> a contiguous (count,) array of dtype; None stays None (NULL)"""
        if v is None:
            return None
        a = np.asarray(v, dtype=dtype)
        if a.ndim == 0:
            a = np.full(self.count, a, dtype=dtype)
        a = np.ascontiguousarray(a)
        if a.shape != (self.count,):
            raise ValueError(f"one {what} per pair (or a scalar)")
        return a

    def downsample(self, voxel, voxel_model=None, want_maps=False):
        """a new Batch on the same context whose clouds are this batch's clouds as uploaded, thinned on a voxel grid on the
        device (icp_batch_downsample): one point per occupied cell, cells in first-occurrence order, a cell's point the mean of
        its members added in source order in double (a lone point: its own bytes).  voxel: the grid's edge, a scalar or one
        value per pair, 0 = copy that cloud; voxel_model: the same for the models (None: as voxel).  This batch is only read,
        and its loop does not notice.  want_maps: also return, per pair, the (n,) and (m,) int32 maps from every source point
        to its output point: (Batch, moving_maps, model_maps)."""
        vm = self._per_pair(voxel, "voxel edge")
        vq = vm if voxel_model is None else self._per_pair(voxel_model, "model voxel edge")
        out, info = self._thin("icp_batch_downsample", (_ptr(vm), _ptr(vq)), [("map", C.c_int32, want_maps)])
        return (out, info["moving_map"], info["model_map"]) if want_maps else out

    def _thin(self, name, lead, outputs, tail=()):
        """what downsample, remove_outliers, keypoints and segment_plane share: the C call `name`(handle, *lead, the optional
        per-point outputs, *tail, &new handle) -> (the new Batch, info).  outputs: (key, element type, wanted) in the call's
        order; a wanted one is a flat array per side, the moving clouds' before the models', cut per pair into
        info["moving_" + key] and info["model_" + key]; one not wanted goes as two NULLs"""
        flat, ptrs = [], []
        for _, ctype, wanted in outputs:
            for off in (self._moff, self._qoff):
                flat.append(np.empty(int(off[-1]), dtype=ctype) if wanted else None)
                ptrs.append(_ptr(flat[-1], ctype))
        h = C.c_void_p()
        capi.check(getattr(self._lib, name)(self._h, *lead, *ptrs, *tail, C.byref(h)), name)
        out = Batch._from_handle(self._ctx, h, self.count, self._dtype)
        info = {}
        for (key, _, wanted), a, q in zip(outputs, flat[0::2], flat[1::2]):
            if wanted:
                info["moving_" + key], info["model_" + key] = self._split(a), self._cut(q, self._qoff)
        return out, info

    def _rule_list(self, rules, what, one):
        """one rule (then `one` is true) or one per pair -> a list of count rules; what: "moving", "model plane", ..."""
        rules = [rules] * self.count if one else list(rules)
        if len(rules) != self.count:
            raise ValueError(f"one {what} rule per pair (or a single rule)")
        return rules

    def _outlier_rules(self, rules, what):
        """one rule or one per pair -> a ctypes array of count icp_outlier_rule (None: NULL, copy that side)"""
        if rules is None:
            return None
        arr = (capi.icp_outlier_rule * self.count)()
        for b, r in enumerate(self._rule_list(rules, what, isinstance(rules, tuple) and len(rules) == 3 and isinstance(rules[0], str))):
            if r is None:
                arr[b] = capi.icp_outlier_rule(capi.ICP_OUTLIER_NONE, 0, 0.0)
            elif r[0] == "statistical":   # ("statistical", k, ratio)
                arr[b] = capi.icp_outlier_rule(capi.ICP_OUTLIER_STATISTICAL, int(r[1]), float(r[2]))
            elif r[0] == "radius":        # ("radius", r, min_neighbours)
                arr[b] = capi.icp_outlier_rule(capi.ICP_OUTLIER_RADIUS, int(r[2]), float(r[1]))
            else:
                raise ValueError(f"unknown outlier rule {r[0]!r}: 'statistical', 'radius' or None")
        return arr

    def remove_outliers(self, moving=None, model=None, want_maps=False, want_scores=False):
        """a new Batch on the same context whose clouds are this batch's clouds as uploaded without their isolated points, made
        on the device (icp_batch_remove_outliers; the rules are stated in include/icp_mi355x.h).  moving, model: one rule or one
        per pair -- ("statistical", k, ratio): keep a point iff the mean distance to its k nearest neighbours is at most the
        cloud's mean + ratio * its sample deviation; ("radius", r, min_neighbours): keep a point iff at least min_neighbours
        other points lie within r; None: copy.  Kept points are copied, in the source order.  This batch is only read, and its
        loop does not notice.  Returns (Batch, info): info["stats"] is a (2 * count, 4) array of [mean, std, thr, kept], the
        moving clouds first; want_maps adds "moving_map" and "model_map" (per pair, int32: the new index of a kept point, -1 for
        a removed one), want_scores "moving_score" and "model_score" (per pair, float64: the mean neighbour distance, or the
        neighbour count of a radius rule)."""
        stats = np.empty((2 * self.count, 4), dtype=np.float64)
        out, info = self._thin("icp_batch_remove_outliers", (self._outlier_rules(moving, "moving"), self._outlier_rules(model, "model")),
                               [("map", C.c_int32, want_maps), ("score", C.c_double, want_scores)], (_ptr(stats),))
        return out, {"stats": stats, **info}

    def _coded_rules(self, rules, what, label):
        """the codec of the plane and the keypoint rules (_RULES[label]): one rule or one per pair -> a ctypes array of count rule
        structs (None: NULL, copy that side).  A rule is None (the NONE rule), a tuple of the table's first two fields or more, the
        rest padded with the table's defaults, or a dict of the table's names; a single rule is a dict, or a tuple whose first
        element passes the table's test"""
        if rules is None:
            return None
        struct, none, first, fields, make = _RULES[label]
        names = tuple(name for name, _ in fields)
        one = isinstance(rules, dict) or (isinstance(rules, tuple) and len(rules) > 0 and first(rules[0]))
        arr = (struct * self.count)()
        for b, r in enumerate(self._rule_list(rules, f"{what} {label}", one)):
            if r is None:
                arr[b] = struct(none)   # (every other field 0)
                continue
            if isinstance(r, dict):
                if set(r) - set(names) or names[0] not in r or names[1] not in r:
                    raise ValueError(f"a {label} rule needs {names[0]} and {names[1]}, and may hold {names[2:]}")
                r = tuple(r.get(name, default) for name, default in fields)
            r = tuple(r)
            if not 2 <= len(r) <= len(fields):
                raise ValueError(f"a {label} rule is ({', '.join(names[:2] + tuple(f'{n}={d}' for n, d in fields[2:]))})")
            arr[b] = make(r + tuple(default for _, default in fields[len(r):]))
        return arr

    def segment_plane(self, moving=None, model=None, seed=0, want_masks=False, want_maps=False):
        """a new Batch on the same context whose clouds are this batch's clouds as uploaded without their dominant plane, or
        reduced to it, found by RANSAC on the device (icp_batch_segment_plane; the rule is stated in include/icp_mi355x.h).  moving,
        model: one rule or one per pair -- (kind, distance, hypotheses=1000, axis=(0, 0, 0), min_cos=0.0) or a dict of those
        names; kind "detect" copies the cloud and reports its plane, "remove" keeps the points farther than distance from the
        plane, "keep" those within; a non-zero axis admits only planes whose normal n has |n . axis| / |axis| >= min_cos; None:
        copy, nothing is searched.  seed: a scalar for every pair, or one per pair.  Kept points are copied, in the source order.
        Zero lidar returns are the caller's to drop: a plane through the origin counts every one of them.  This batch is only
        read, and its loop does not notice.  Returns (Batch, info): info["planes"] (2 * count, 4) float64 -- nx, ny, nz, d, the
        moving clouds first -- info["inliers"] (2 * count,) int32 and info["status"] (2 * count,) (ICP_OK; ICP_ERR_EMPTY where a
        cloud has no valid hypothesis: it is copied); want_masks adds "moving_mask" and "model_mask" (per pair, uint8: 1 = on
        the plane), want_maps "moving_map" and "model_map" (per pair, int32: the new index of a kept point, -1 for a removed one)."""
        rm, rq = self._coded_rules(moving, "moving", "plane"), self._coded_rules(model, "model", "plane")
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, dtype=np.uint64), (self.count,)))
        planes = np.zeros((2 * self.count, 4), dtype=np.float64)
        inl = np.zeros(2 * self.count, dtype=np.int32)
        st = np.zeros(2 * self.count, dtype=np.intc)
        out, info = self._thin("icp_batch_segment_plane", (rm, rq, _ptr(sd, C.c_uint64), _ptr(planes), _ptr(inl, C.c_int32), _ptr(st, C.c_int)),
                               [("mask", C.c_uint8, want_masks), ("map", C.c_int32, want_maps)])
        self._segment_hyp = [0 if side is None else side[b].hypotheses for side in (rm, rq) for b in range(self.count)]   # (diag_segment)
        return out, {"planes": planes, "inliers": inl, "status": st, **info}

    def diag_segment(self, b, side):
        """the last segment_plane call's hypotheses of pair b, side 0 (the moving cloud) or 1 (the model)
        (icp_diag_batch_segment): dict of triples (H, 3) int32 -- point indices, -1 for an empty slot -- valid (H,) uint8, planes
        (H, 4) and counts (H,) int32 (-1: invalid)"""
        hyp = getattr(self, "_segment_hyp", None)
        H = int(hyp[int(side) * self.count + int(b)]) if hyp is not None and 0 <= int(b) < self.count and int(side) in (0, 1) else 0
        tr, va = np.zeros((max(H, 1), 3), dtype=np.int32), np.zeros(max(H, 1), dtype=np.uint8)
        pl, cn = np.zeros((max(H, 1), 4)), np.zeros(max(H, 1), dtype=np.int32)
        p32 = C.POINTER(C.c_int32)
        capi.check(self._lib.icp_diag_batch_segment(self._h, int(b), int(side), tr.ctypes.data_as(p32), va.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                    pl.ctypes.data_as(C.POINTER(C.c_double)), cn.ctypes.data_as(p32)), "icp_diag_batch_segment")
        return dict(triples=tr[:H], valid=va[:H], planes=pl[:H], counts=cn[:H])

    def keypoints(self, moving=None, model=None, want_maps=False, want_saliency=False):
        """a new Batch on the same context whose clouds are the ISS keypoints of this batch's clouds as uploaded, made on the
        device (icp_batch_select_keypoints; the rule is stated in include/icp_mi355x.h).  moving, model: one rule or one per pair
        -- (salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbours=5) or a dict of those names: a point's
        saliency is the smallest eigenvalue of the covariance of the points within salient_radius, where the eigenvalue ratios are
        below the gammas and at least min_neighbours points lie within; it is kept iff no point within non_max_radius has a
        higher saliency; None: copy.  Kept points are copied, in the source order.  Where this batch holds descriptors
        (compute_features) the new one holds those of the kept points, so match_features, ransac and fgr run on it as they
        are.  This batch is only read, and its loop does not notice.  Returns (Batch, info): info["counts"] is a (2 * count,) int32
        array of the kept points, the moving clouds first; want_maps adds "moving_map" and "model_map" (per pair, int32: the new
        index of a kept point, -1 for a dropped one), want_saliency "moving_saliency" and "model_saliency" (per pair, float64)."""
        counts = np.empty(2 * self.count, dtype=np.int32)
        out, info = self._thin("icp_batch_select_keypoints", (self._coded_rules(moving, "moving", "keypoint"), self._coded_rules(model, "model", "keypoint")),
                               [("map", C.c_int32, want_maps), ("saliency", C.c_double, want_saliency)], (_ptr(counts, C.c_int32),))
        return out, {"counts": counts, **info}

    def get_clouds(self):
        """the clouds the batch holds as uploaded (or as Batch.downsample made them; never the moved cloud): a list of (D, M)"""
        D = np.empty((int(self._moff[-1]), 3), dtype=self._dtype)
        M = np.empty((int(self._qoff[-1]), 3), dtype=self._dtype)
        capi.check(self._lib.icp_batch_get_clouds(self._h, D.ctypes.data, M.ctypes.data), "icp_batch_get_clouds")
        return [(D[self._moff[b]:self._moff[b + 1]].copy(), M[self._qoff[b]:self._qoff[b + 1]].copy()) for b in range(self.count)]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _split(self, flat):
        return self._cut(flat, self._moff)

    def set_model_normals(self, normals):
        """the unit normals of every pair's model points (one (m, 3) array per pair): what a point-to-plane begin needs"""
        N = _batch_normals(normals, self._model_shapes, self._dtype)
        capi.check(self._lib.icp_batch_set_model_normals(self._h, N.ctypes.data), "icp_batch_set_model_normals")

    def _model_normals(self, normals):
        """the caller's model normals, or None: estimated on the device"""
        if normals is not None:
            self.set_model_normals(normals)
        else:
            self.estimate_normals()

    def estimate_normals(self, want_neighbours=False):
        """kNN(4) + PCA normals of every pair's model on the device (one neighbour launch + one normals launch for all pairs);
        a per-pair list of normals, and a per-pair list of (m, 4) neighbours (indices within that pair's model) when asked"""
        total = int(self._qoff[-1])
        nrm = np.empty((total, 3), dtype=self._dtype)
        nbr = np.empty((total, 4), dtype=np.int32) if want_neighbours else None
        capi.check(self._lib.icp_batch_estimate_normals(self._h, nrm.ctypes.data, _ptr(nbr, C.c_int32)),
                   "icp_batch_estimate_normals")
        return (self._cut(nrm, self._qoff), self._cut(nbr, self._qoff)) if want_neighbours else self._cut(nrm, self._qoff)

    def _side(self, arrays, off, width, what):
        """one float64 array per pair, (points, width) or (points,) for width None -> their concatenation in that side's layout
        (None: NULL); what: "moving covariances", "model normals", ..."""
        if arrays is None:
            return None
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
        if len(arrays) != self.count:
            raise ValueError(f"one array of {what} per pair")
        for b, a in enumerate(arrays):
            points = int(off[b + 1] - off[b])
            if a.shape != ((points,) if width is None else (points, width)):
                raise ValueError(f"a pair's {what} must be (points,{'' if width is None else ' ' + str(width)})")
        return np.ascontiguousarray(np.concatenate(arrays))

    def _cut(self, flat, off):
        return [flat[off[b]:off[b + 1]].copy() for b in range(self.count)]

    def set_covariances(self, moving=None, model=None):
        """the covariance of every point, what a generalized begin needs on both sides: per side one (points, 6) float64 array per
        pair -- xx, xy, xz, yy, yz, zz, symmetric positive semi-definite (the caller's duty; only finiteness is checked) -- or
        None: that side is left as it is.  The moving covariances belong to the clouds as uploaded, in their own frame.  Discards
        a loop under way."""
        a, q = self._side(moving, self._moff, 6, "moving covariances"), self._side(model, self._qoff, 6, "model covariances")
        capi.check(self._lib.icp_batch_set_covariances(self._h, _ptr(a), _ptr(q)), "icp_batch_set_covariances")

    def _estimate_covariances_k(self, k, regularisation, lam):
        """estimate_covariances as the entry points take k: one value for both sides, or (k_moving, k_model)"""
        km, kq = k if isinstance(k, tuple) else (k, None)
        self.estimate_covariances(km, kq, regularisation=regularisation, lam=lam)

    def estimate_covariances(self, k=20, k_model=None, regularisation="frobenius", lam=1e-3, want=False):
        """the covariance of every point from its k nearest neighbours, on the device in one launch (icp_batch_estimate_covariances):
        the neighbourhood of point i is every point of its cloud no farther than its k-th nearest other point (ties included, i
        itself included), the covariance the neighbourhood's, in double.  k: a scalar or one value per pair, each in [3, 32], for
        the moving clouds, or None (that side is left as it is); k_model: the same for the models, None: as k.
        regularisation "frobenius": C / ||C||_F + lam I (lam > 0); "none" or None: the raw covariance.  want: also return
        (moving, model), per pair the (points, 6) float64 arrays of the sides estimated (None for a side left as it is).
        Discards a loop under way."""
        reg = {"frobenius": capi.ICP_COV_FROBENIUS, "none": capi.ICP_COV_NONE, None: capi.ICP_COV_NONE}[regularisation] if (
            regularisation is None or isinstance(regularisation, str)) else int(regularisation)
        km, kq = self._per_pair(k, "k", np.intc), self._per_pair(k if k_model is None else k_model, "model k", np.intc)
        om = np.empty((int(self._moff[-1]), 6)) if want and km is not None else None
        oq = np.empty((int(self._qoff[-1]), 6)) if want and kq is not None else None
        capi.check(self._lib.icp_batch_estimate_covariances(self._h, _ptr(km, C.c_int), _ptr(kq, C.c_int), reg, float(lam), _ptr(om), _ptr(oq)),
                   "icp_batch_estimate_covariances")
        if want:
            return (self._cut(om, self._moff) if om is not None else None, self._cut(oq, self._qoff) if oq is not None else None)

    def get_covariances(self):
        """(moving, model): per pair the (points, 6) float64 covariances the batch holds (icp_batch_get_covariances)"""
        om, oq = np.empty((int(self._moff[-1]), 6)), np.empty((int(self._qoff[-1]), 6))
        capi.check(self._lib.icp_batch_get_covariances(self._h, _ptr(om), _ptr(oq)), "icp_batch_get_covariances")
        return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def set_intensities(self, moving=None, model=None):
        """the intensity of every point, what a colored begin needs on both sides: per side one (points,) float64 array per pair,
        or None: that side is left as it is.  New model intensities discard the gradients.  Discards a loop under way."""
        a, q = self._side(moving, self._moff, None, "moving intensities"), self._side(model, self._qoff, None, "model intensities")
        capi.check(self._lib.icp_batch_set_intensities(self._h, _ptr(a), _ptr(q)), "icp_batch_set_intensities")

    def estimate_intensity_gradients(self, k=8, want=False):
        """the intensity gradient of every model point from its k nearest neighbours, on the device in one launch
        (icp_batch_estimate_intensity_gradients): a least-squares fit of the intensity differences over the neighbourhood -- every
        other point no farther than the k-th nearest, ties included -- in the tangent plane of the point's normal.  The batch
        must hold model intensities and model normals.  k: a scalar or one value per pair, each in [3, 32].  want: also return
        the per-pair list of (m, 3) float64 gradients.  Discards a loop under way."""
        kq = self._per_pair(k, "k", np.intc)
        out = np.empty((int(self._qoff[-1]), 3)) if want else None
        capi.check(self._lib.icp_batch_estimate_intensity_gradients(self._h, _ptr(kq, C.c_int), _ptr(out)), "icp_batch_estimate_intensity_gradients")
        if want:
            return self._cut(out, self._qoff)

    def set_intensity_gradients(self, grads):
        """the caller's own intensity gradients: one (m, 3) float64 array per pair, in the models' frame"""
        g = self._side(list(grads), self._qoff, 3, "model gradients")
        capi.check(self._lib.icp_batch_set_intensity_gradients(self._h, _ptr(g)), "icp_batch_set_intensity_gradients")

    def get_intensity_gradients(self):
        """per pair the (m, 3) float64 gradients the batch holds (icp_batch_get_intensity_gradients)"""
        out = np.empty((int(self._qoff[-1]), 3))
        capi.check(self._lib.icp_batch_get_intensity_gradients(self._h, _ptr(out)), "icp_batch_get_intensity_gradients")
        return self._cut(out, self._qoff)

    def set_color_weight(self, lam=None):
        """lambda, the weight of the geometric term of the colored metric (1 - lambda weighs the photometric term): a scalar for
        every pair, one value per pair, each in [0, 1], or None: ICP_COLOR_LAMBDA_DEFAULT.  Discards a loop under way."""
        capi.check(self._lib.icp_batch_set_color_weight(self._h, _ptr(self._per_pair(lam, "lambda"))), "icp_batch_set_color_weight")

    def diag_rotation(self, b):
        """(3, 3): the rotation pair b's most recent matching pass of a generalized loop rotated its moving covariances by, or of
        a symmetric loop its moving point normals (icp_diag_batch_rotation)"""
        R = np.zeros(9)
        capi.check(self._lib.icp_diag_batch_rotation(self._h, int(b), R.ctypes.data_as(C.POINTER(C.c_double))), "icp_diag_batch_rotation")
        return R.reshape(3, 3)

    def compute_features(self, k, normals, k_model=None, want=False):
        """a 33-bin FPFH descriptor of every point of both clouds of every pair, on the device in two launches
        (icp_batch_compute_features): k neighbours per point (a scalar or one value per pair, each in [3, 32]; k_model: the same
        for the models, None: as k) and normals = (moving, model), per side one (points, 3) float64 array of unit normals per pair,
        consistently oriented (the caller's duty; oriented_normals makes them from covariances).  The clouds are those the batch
        holds as uploaded, never the moved ones; a loop under way is left alone.  want: also return (moving, model), per pair the
        (points, 33) float64 descriptors."""
        moving, model = normals
        km, kq = self._per_pair(k, "k", np.intc), self._per_pair(k if k_model is None else k_model, "model k", np.intc)
        nm, nq = self._side(list(moving), self._moff, 3, "moving normals"), self._side(list(model), self._qoff, 3, "model normals")
        om = np.empty((int(self._moff[-1]), capi.ICP_FEATURE_BINS)) if want else None
        oq = np.empty((int(self._qoff[-1]), capi.ICP_FEATURE_BINS)) if want else None
        capi.check(self._lib.icp_batch_compute_features(self._h, _ptr(km, C.c_int), _ptr(kq, C.c_int), _ptr(nm), _ptr(nq), _ptr(om), _ptr(oq)),
                   "icp_batch_compute_features")
        if want:
            return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def _viewpoints(self, viewpoints):
        """(moving, model), each (count, 3) float64: one (3,) viewpoint for every cloud, or a (moving, model) pair of per-pair arrays"""
        if isinstance(viewpoints, (tuple, list)) and len(viewpoints) == 2 and np.ndim(viewpoints[0]) == 2:
            vm, vq = (np.ascontiguousarray(v, dtype=np.float64) for v in viewpoints)
        else:
            one = np.asarray(viewpoints, dtype=np.float64)
            if one.shape != (3,):
                raise ValueError("viewpoints must be one (3,) point or a (moving, model) pair of (count, 3) arrays")
            vm = vq = np.ascontiguousarray(np.tile(one, (self.count, 1)))
        if vm.shape != (self.count, 3) or vq.shape != (self.count, 3):
            raise ValueError("one (3,) viewpoint per pair and side")
        return vm, vq

    def estimate_point_normals(self, orient="centroid", viewpoints=None, want=False):
        """the normal of every point of both clouds of every pair from the covariances the batch holds, on the device
        (icp_batch_estimate_point_normals): the eigenvector of the smallest eigenvalue by icp_eigh3's Jacobi, exactly (0, 0, 0) where
        it is not finite, kept on the device for compute_features_stored.  orient: "centroid" faces each cloud's own centroid,
        "viewpoint" faces viewpoints -- one (3,) point for every cloud, or a (moving, model) pair of (count, 3) arrays, each in that
        cloud's own frame -- "none" or None leaves the eigenvector as it is.  want: also return (moving, model), per pair the
        (points, 3) float64 normals.  One launch, two for "centroid"; a host wait only with want.  A loop under way is left alone."""
        mode = {"none": capi.ICP_ORIENT_NONE, None: capi.ICP_ORIENT_NONE, "viewpoint": capi.ICP_ORIENT_VIEWPOINT,
                "centroid": capi.ICP_ORIENT_CENTROID}[orient] if (orient is None or isinstance(orient, str)) else int(orient)
        vm = vq = None
        if mode == capi.ICP_ORIENT_VIEWPOINT and viewpoints is not None:
            vm, vq = self._viewpoints(viewpoints)
        om = np.empty((int(self._moff[-1]), 3)) if want else None
        oq = np.empty((int(self._qoff[-1]), 3)) if want else None
        capi.check(self._lib.icp_batch_estimate_point_normals(self._h, mode, _ptr(vm), _ptr(vq), _ptr(om), _ptr(oq)), "icp_batch_estimate_point_normals")
        if want:
            return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def set_point_normals(self, moving=None, model=None):
        """point normals of the caller's own (icp_batch_set_point_normals): per side one (points, 3) float64 array per pair, or
        None: that side is left as it is.  Only finiteness is checked."""
        a, q = self._side(moving, self._moff, 3, "moving normals"), self._side(model, self._qoff, 3, "model normals")
        capi.check(self._lib.icp_batch_set_point_normals(self._h, _ptr(a), _ptr(q)), "icp_batch_set_point_normals")

    def get_point_normals(self):
        """(moving, model): per pair the (points, 3) float64 point normals the batch holds (icp_batch_get_point_normals)"""
        om, oq = np.empty((int(self._moff[-1]), 3)), np.empty((int(self._qoff[-1]), 3))
        capi.check(self._lib.icp_batch_get_point_normals(self._h, _ptr(om), _ptr(oq)), "icp_batch_get_point_normals")
        return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def compute_features_stored(self, k, k_model=None, want=False):
        """compute_features from the point normals the batch holds (estimate_point_normals, set_point_normals): the same two
        launches, nothing uploaded (icp_batch_compute_features_stored)"""
        km, kq = self._per_pair(k, "k", np.intc), self._per_pair(k if k_model is None else k_model, "model k", np.intc)
        om = np.empty((int(self._moff[-1]), capi.ICP_FEATURE_BINS)) if want else None
        oq = np.empty((int(self._qoff[-1]), capi.ICP_FEATURE_BINS)) if want else None
        capi.check(self._lib.icp_batch_compute_features_stored(self._h, _ptr(km, C.c_int), _ptr(kq, C.c_int), _ptr(om), _ptr(oq)),
                   "icp_batch_compute_features_stored")
        if want:
            return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def diag_centroids(self):
        """(moving, model), each (count, 3) float64: the centroids of the last estimate_point_normals("centroid")
        (icp_diag_batch_centroids)"""
        out = np.empty((2 * self.count, 3))
        capi.check(self._lib.icp_diag_batch_centroids(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "icp_diag_batch_centroids")
        return out[:self.count].copy(), out[self.count:].copy()

    def get_features(self):
        """(moving, model): per pair the (points, 33) float64 descriptors the batch holds (icp_batch_get_features)"""
        om = np.empty((int(self._moff[-1]), capi.ICP_FEATURE_BINS))
        oq = np.empty((int(self._qoff[-1]), capi.ICP_FEATURE_BINS))
        capi.check(self._lib.icp_batch_get_features(self._h, _ptr(om), _ptr(oq)), "icp_batch_get_features")
        return self._cut(om, self._moff), self._cut(oq, self._qoff)

    def diag_set_features(self, moving, model):
        """descriptors of the caller's own, per side one (points, 33) float64 array per pair (icp_diag_batch_set_features): for tests"""
        a = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, capi.ICP_FEATURE_BINS) for x in moving]))
        q = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, capi.ICP_FEATURE_BINS) for x in model]))
        if a.shape[0] != int(self._moff[-1]) or q.shape[0] != int(self._qoff[-1]):
            raise ValueError("one (points, 33) array of descriptors per cloud")
        capi.check(self._lib.icp_diag_batch_set_features(self._h, _ptr(a), _ptr(q)), "icp_diag_batch_set_features")

    def match_features(self, mutual=True):
        """the nearest descriptor of the other cloud for every point, both ways (icp_batch_match_features): (fwd, rev, kept), per
        pair fwd (n,) int32 -- the model point whose descriptor is nearest to moving point i's, the lowest index on ties -- rev
        (m,) int32 the same from the models, kept (n,) uint8 = not mutual or rev[fwd[i]] == i.  A pair's correspondence list, what
        score_transforms and ransac work on, is its kept i in ascending order, each with fwd[i]."""
        p32 = C.POINTER(C.c_int32)
        fwd = np.zeros(int(self._moff[-1]), dtype=np.int32)
        rev = np.zeros(int(self._qoff[-1]), dtype=np.int32)
        kept = np.zeros(int(self._moff[-1]), dtype=np.uint8)
        capi.check(self._lib.icp_batch_match_features(self._h, 1 if mutual else 0, fwd.ctypes.data_as(p32), rev.ctypes.data_as(p32),
                                                      kept.ctypes.data_as(C.POINTER(C.c_uint8))), "icp_batch_match_features")
        return self._split(fwd), self._cut(rev, self._qoff), self._split(kept)

    def score_transforms(self, T, max_distance):
        """(count, per_pair) int32: how many correspondences of every pair lie within max_distance (a scalar, one value per pair,
        or None: no limit) of their match once the pair's moving cloud as uploaded is moved by each of its candidate poses
        (icp_batch_score_transforms).  T: (count, per_pair, 4, 4), or (count, 4, 4) for one candidate per pair."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim == 3:
            T = T[:, None]
        if T.ndim != 4 or T.shape[0] != self.count or T.shape[2:] != (4, 4) or T.shape[1] < 1:
            raise ValueError("candidate transforms must be (count, per_pair, 4, 4)")
        T = np.ascontiguousarray(T)
        md = self._per_pair(max_distance, "maximum distance")
        pd = C.POINTER(C.c_double)
        out = np.zeros((self.count, T.shape[1]), dtype=np.int32)
        capi.check(self._lib.icp_batch_score_transforms(self._h, int(T.shape[1]), T.ctypes.data_as(pd), _ptr(md),
                                                        out.ctypes.data_as(C.POINTER(C.c_int32))), "icp_batch_score_transforms")
        return out

    def ransac(self, hypotheses, max_distance, edge_similarity=0.9, seed=0):
        """a start pose for every pair from its correspondence list (icp_batch_ransac): hypotheses three-match samples per pair,
        drawn by a counter-based generator from seed (a scalar for every pair, or one per pair), screened by the edge-length
        check, solved on the host and scored on the device; the best is refitted on its inliers.  Per pair a dict of T (4, 4: maps
        the moving cloud as uploaded into the model's frame -- what set_initial_transforms takes), inliers, correspondences and
        status (ICP_OK, or ICP_ERR_EMPTY where fewer than three correspondences or no valid hypothesis exist: T is then the identity)."""
        sd = self._per_pair(seed, "seed", np.uint64)
        prm = capi.icp_ransac_params(int(hypotheses), float(max_distance), float(edge_similarity))
        T = np.zeros((self.count, 4, 4))
        inl, cor = np.zeros(self.count, dtype=np.int32), np.zeros(self.count, dtype=np.int32)
        st = np.zeros(self.count, dtype=np.intc)
        p32 = C.POINTER(C.c_int32)
        capi.check(self._lib.icp_batch_ransac(self._h, C.byref(prm), _ptr(sd, C.c_uint64), T.ctypes.data_as(C.POINTER(C.c_double)),
                                              inl.ctypes.data_as(p32), cor.ctypes.data_as(p32), st.ctypes.data_as(C.POINTER(C.c_int))), "icp_batch_ransac")
        self._ransac_hyp = int(hypotheses)
        return [dict(T=T[b].copy(), inliers=int(inl[b]), correspondences=int(cor[b]), status=int(st[b])) for b in range(self.count)]

    def diag_ransac(self, b):
        """the last ransac run's hypotheses of pair b (icp_diag_batch_ransac): dict of triples (H, 3) int32 -- positions in the
        pair's correspondence list, -1 for an empty slot -- valid (H,) uint8, T (H, 4, 4) and counts (H,) int32 (-1: invalid)"""
        H = int(getattr(self, "_ransac_hyp", 0))
        tr, va = np.zeros((max(H, 1), 3), dtype=np.int32), np.zeros(max(H, 1), dtype=np.uint8)
        T, cn = np.zeros((max(H, 1), 4, 4)), np.zeros(max(H, 1), dtype=np.int32)
        p32 = C.POINTER(C.c_int32)
        capi.check(self._lib.icp_diag_batch_ransac(self._h, int(b), tr.ctypes.data_as(p32), va.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   T.ctypes.data_as(C.POINTER(C.c_double)), cn.ctypes.data_as(p32)), "icp_diag_batch_ransac")
        return dict(triples=tr[:H], valid=va[:H], T=T[:H], counts=cn[:H])

    def fgr(self, max_distance, iterations=64, division_factor=1.4, decrease_every=4, tuples=0, tuple_similarity=0.95, seed=0):
        """a start pose for every pair from its correspondence list by Fast Global Registration (icp_batch_fgr): no hypotheses --
        iterations weighted Gauss-Newton steps on the Geman-McClure objective, whose scale mu starts at the squared extent of the
        used points and is divided by division_factor every decrease_every iterations, never below max_distance squared.
        tuples 0: every correspondence is used and the result needs no seed; tuples > 0: the correspondences that occur in a
        triple of ransac's generator (seed: a scalar for every pair, or one per pair) that passes the edge check at
        tuple_similarity.  Per pair a dict of T (4, 4: maps the moving cloud as uploaded into the model's frame -- what
        set_initial_transforms takes), weights (n,) float64 -- the soft inlier weight of every moving point at T, 0 for a point
        that was not used -- used (how many correspondences were), objective and status (ICP_OK; ICP_ERR_EMPTY where fewer than
        three correspondences are used: T is then the identity; ICP_ERR_SINGULAR where a step's system was not positive definite:
        T is then the pose reached so far)."""
        sd = self._per_pair(seed, "seed", np.uint64) if int(tuples) > 0 else None
        prm = capi.icp_fgr_params(int(iterations), float(max_distance), float(division_factor), int(decrease_every), int(tuples), float(tuple_similarity))
        T = np.zeros((self.count, 4, 4))
        w = np.zeros(int(self._moff[-1]))
        used = np.zeros(self.count, dtype=np.int32)
        obj = np.zeros(self.count)
        st = np.zeros(self.count, dtype=np.intc)
        pd = C.POINTER(C.c_double)
        capi.check(self._lib.icp_batch_fgr(self._h, C.byref(prm), _ptr(sd, C.c_uint64), T.ctypes.data_as(pd),
                                           w.ctypes.data_as(pd), used.ctypes.data_as(C.POINTER(C.c_int32)), obj.ctypes.data_as(pd),
                                           st.ctypes.data_as(C.POINTER(C.c_int))), "icp_batch_fgr")
        self._fgr_iter, self._fgr_used = int(iterations), used.copy()
        return [dict(T=T[b].copy(), weights=w[self._moff[b]:self._moff[b + 1]].copy(), used=int(used[b]), objective=float(obj[b]), status=int(st[b]))
                for b in range(self.count)]

    def diag_fgr(self, b):
        """the last fgr run's history of pair b (icp_diag_batch_fgr): dict of used_pos (U,) int32 -- positions in the pair's
        correspondence list -- mu_hist (I,), mom_hist (I, 32) and T_hist (I, 4, 4), the pose every iteration's terms were formed
        at; the iterations the pair did not run hold zeros"""
        I = int(getattr(self, "_fgr_iter", 0))
        U = int(self._fgr_used[int(b)]) if I else 0
        up = np.zeros(max(U, 1), dtype=np.int32)
        mu, mom, T = np.zeros(max(I, 1)), np.zeros((max(I, 1), capi.ICP_NMOM)), np.zeros((max(I, 1), 4, 4))
        pd = C.POINTER(C.c_double)
        capi.check(self._lib.icp_diag_batch_fgr(self._h, int(b), up.ctypes.data_as(C.POINTER(C.c_int32)), mu.ctypes.data_as(pd), mom.ctypes.data_as(pd),
                                                T.ctypes.data_as(pd)), "icp_diag_batch_fgr")
        return dict(used_pos=up[:U], mu_hist=mu[:I], mom_hist=mom[:I], T_hist=T[:I])

    def diag_fgr_times(self):
        """where the host's time went in the iterations of the last fgr run (icp_diag_batch_fgr_times): dict of enqueue_s, wait_s
        and solve_s, summed over the iterations, and iterations, how many ran"""
        t = np.zeros(4)
        capi.check(self._lib.icp_diag_batch_fgr_times(self._h, t.ctypes.data_as(C.POINTER(C.c_double))), "icp_diag_batch_fgr_times")
        return dict(enqueue_s=float(t[0]), wait_s=float(t[1]), solve_s=float(t[2]), iterations=int(t[3]))

    def set_max_distance(self, v):
        """the maximum correspondence distance: a scalar for every pair, one value per pair (inf: that pair is not gated), or
        None (no gate).  A match farther away than that enters no sum of its pass.  Discards a loop under way."""
        capi.check(self._lib.icp_batch_set_max_distance(self._h, _ptr(self._per_pair(v, "maximum distance"))), "icp_batch_set_max_distance")

    def set_trim(self, v):
        """the share of every moving cloud to keep: a scalar for every pair, one value per pair (1.0: that pair is not trimmed), or
        None (no trimming).  Each in (0, 1].  A pair keeps the K = ceil(share * n) closest matches of every pass and every match
        tied with the K-th; the others enter no sum.  Discards a loop under way."""
        capi.check(self._lib.icp_batch_set_trim(self._h, _ptr(self._per_pair(v, "share to keep"))), "icp_batch_set_trim")

    def diag_trim(self, b):
        """(tau_sq, K) of pair b (icp_diag_batch_trim): the squared-distance threshold of its most recent matching pass (inf for a
        pair that is not trimmed) and its rank"""
        tau, k = C.c_double(0.0), C.c_int(0)
        capi.check(self._lib.icp_diag_batch_trim(self._h, int(b), C.byref(tau), C.byref(k)), "icp_diag_batch_trim")
        return tau.value, k.value

    def set_reciprocal(self, v):
        """reciprocal (mutual nearest neighbour) matches: None (off), a bool for every pair, or one flag per pair.  A reciprocal
        pair keeps, in every matching pass, only the matches i -> idx[i] whose model point's own nearest moving point is i; with
        a gate or a trim all tests must pass.  Discards a loop under way."""
        if v is None:
            capi.check(self._lib.icp_batch_set_reciprocal(self._h, None), "icp_batch_set_reciprocal")
            return
        if isinstance(v, (bool, np.bool_)):
            a = np.full(self.count, 1 if v else 0, dtype=np.uint8)
        else:
            a = np.ascontiguousarray(np.asarray(v).astype(bool).astype(np.uint8))
            if a.shape != (self.count,):
                raise ValueError("one reciprocity flag per pair (or a bool, or None)")
        capi.check(self._lib.icp_batch_set_reciprocal(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8))), "icp_batch_set_reciprocal")

    def diag_reverse(self):
        """per pair, (m,) int32: for a reciprocal pair each model point's nearest moving point (the lowest index on ties) of the
        pair's most recent matching pass (icp_diag_batch_reverse); -1 throughout for a pair whose flag is off or that has not
        matched since begin"""
        out = np.empty(int(self._qoff[-1]), dtype=np.int32)
        capi.check(self._lib.icp_diag_batch_reverse(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "icp_diag_batch_reverse")
        return self._cut(out, self._qoff)

    def set_robust(self, kind, scale=None):
        """robust kernels: kind None (none), one kernel for every pair, or one per pair -- "huber", "cauchy", "tukey", None or the
        ICP_ROBUST_* integers; scale: the kernel's k, one value for every pair or one per pair (not read where the kind is None).
        Every kept match of a robust pair enters the sums of a pass with the kernel's weight of its residual (point-to-point: the
        distance to the match; point-to-plane: the distance along the match's normal); gate, trim and reciprocity decide as ever.
        Discards a loop under way."""
        if kind is None:
            capi.check(self._lib.icp_batch_set_robust(self._h, None, None), "icp_batch_set_robust")
            return
        kinds = [kind] * self.count if isinstance(kind, (str, int, np.integer)) else list(kind)
        if len(kinds) != self.count:
            raise ValueError("one robust kernel per pair (or one for every pair, or None)")
        k = np.ascontiguousarray([_ROBUST_KINDS[x] if (x is None or isinstance(x, str)) else int(x) for x in kinds], dtype=np.intc)
        capi.check(self._lib.icp_batch_set_robust(self._h, _ptr(k, C.c_int), _ptr(self._per_pair(scale, "scale"))), "icp_batch_set_robust")

    def get_weights(self):
        """per pair, (n,) float64: the weight of every moving point's match in the pair's most recent matching pass
        (icp_batch_get_weights): 0.0 where the match was rejected, 1.0 for a kept match of a pair without a kernel"""
        out = np.empty(int(self._moff[-1]), dtype=np.float64)
        capi.check(self._lib.icp_batch_get_weights(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "icp_batch_get_weights")
        return self._split(out)

    def set_initial_transforms(self, T):
        """the pose every pair's registration starts from: one (4, 4) for every pair, (count, 4, 4), or None (none).  Rounded once
        to the batch's dtype and applied to the uploaded clouds by every begin (they do not compound); state()["T"] includes
        it.  Every value finite, every bottom row 0 0 0 1.  Discards a loop under way."""
        if T is None:
            capi.check(self._lib.icp_batch_set_initial_transforms(self._h, None), "icp_batch_set_initial_transforms")
            return
        a = np.asarray(T, dtype=np.float64)
        if a.shape == (4, 4):
            a = np.broadcast_to(a, (self.count, 4, 4))
        if a.shape != (self.count, 4, 4):
            raise ValueError("one (4, 4) initial transform for every pair, or (count, 4, 4)")
        a = np.ascontiguousarray(a)
        capi.check(self._lib.icp_batch_set_initial_transforms(self._h, a.ctypes.data_as(C.POINTER(C.c_double))), "icp_batch_set_initial_transforms")

    def begin(self, max_iter=40, tol=1e-6, fixed_iterations=False, metric=capi.ICP_POINT_TO_POINT):
        """start every pair's registration from the uploaded clouds, moved by the pair's initial transform where the batch holds
        any (ICP_POINT_TO_PLANE: the batch must hold normals; ICP_GENERALIZED: covariances on both sides and no robust kernel;
        ICP_COLORED: normals, intensities on both sides, intensity gradients and no robust kernel; ICP_SYMMETRIC: point normals on
        both sides -- estimate_point_normals or set_point_normals -- and no robust kernel; new point normals discard such a loop)"""
        prm = capi.icp_params(int(max_iter), float(tol), 1 if fixed_iterations else 0, _prec(self._dtype), int(metric))
        capi.check(self._lib.icp_batch_begin(self._h, C.byref(prm)), "icp_batch_begin")
        self._max_iter = int(max_iter)

    def run(self, steps):
        """up to `steps` passes of every running pair; returns (steps_done, pairs still running)"""
        k, a = C.c_int(0), C.c_int(0)
        capi.check(self._lib.icp_batch_run(self._h, int(steps), C.byref(k), C.byref(a)), "icp_batch_run")
        return k.value, a.value

    def _drive(self, metric, max_iter, tol, fixed_iterations, max_distance, init, trim, reciprocal, robust):
        """what every batch entry point does with a prepared batch: the per-pair options (the gate and the start poses always, None
        too, which clears them; trim, reciprocity and robust -- (kernel, scale) -- only where given), begin, run to the end.
        Returns every pair's state"""
        self.set_max_distance(max_distance)
        self.set_initial_transforms(init)
        if trim is not None:
            self.set_trim(trim)
        if reciprocal is not None:
            self.set_reciprocal(reciprocal)
        if robust is not None:
            self.set_robust(*robust)
        self.begin(max_iter=max_iter, tol=tol, fixed_iterations=fixed_iterations, metric=metric)
        while self.run(1 << 20)[1] > 0:
            pass
        return [self.state(b) for b in range(self.count)]

    def _results(self, states, weights):
        """the list of Result of a finished loop from _drive's states; weights: also extra["weights"] (a robust run)"""
        idx, inl, moved = self.loop_indices(), self.loop_inliers(), self.get_moving()
        wts = self.get_weights() if weights else None
        out = []
        for b, st in enumerate(states):
            out.append(Result(T=st["T"].copy(), iterations=st["iterations"], passes=st["passes"], err=st["err"], idx=idx[b], moved=moved[b],
                              extra={"status": st["status"], "inliers": inl[b], "fitness": float(inl[b].sum()) / inl[b].size}))
            if wts is not None:
                out[-1].extra["weights"] = wts[b]
        return out

    def state(self, b):
        st, it, ps = C.c_int(0), C.c_int(0), C.c_int(0)
        err = np.zeros(self._max_iter + 1)
        T = np.zeros(16)
        pd = C.POINTER(C.c_double)
        capi.check(self._lib.icp_batch_state(self._h, int(b), C.byref(st), C.byref(it), C.byref(ps), err.ctypes.data_as(pd), err.size,
                                             T.ctypes.data_as(pd)), "icp_batch_state")
        return dict(status=st.value, iterations=it.value, passes=ps.value, err=err[: ps.value + 1].copy(), T=T.reshape(4, 4))

    def diag_moments(self, b):
        """the ICP_NMOM vector pair b's loop last advanced on (icp_diag_batch_moments)"""
        mom = np.zeros(capi.ICP_NMOM, dtype=np.float64)
        capi.check(self._lib.icp_diag_batch_moments(self._h, int(b), mom.ctypes.data_as(C.POINTER(C.c_double))), "icp_diag_batch_moments")
        return mom

    def done(self):
        """(count,) bool: the pairs whose loop has ended"""
        out = np.zeros(self.count, dtype=np.int32)
        capi.check(self._lib.icp_batch_done(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "icp_batch_done")
        return out.astype(bool)

    def get_moving(self):
        out = np.empty((int(self._moff[-1]), 3), dtype=self._dtype)
        capi.check(self._lib.icp_batch_get_moving(self._h, out.ctypes.data), "icp_batch_get_moving")
        return self._split(out)

    def _indices(self, fn, where):
        out = np.empty(int(self._moff[-1]), dtype=np.int32)
        capi.check(fn(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), where)
        return self._split(out)

    def get_indices(self):
        """each pair's matches of its most recent matching pass"""
        return self._indices(self._lib.icp_batch_get_indices, "icp_batch_get_indices")

    def loop_indices(self):
        """each pair's matches of the last pass that contributed to its T"""
        return self._indices(self._lib.icp_batch_loop_indices, "icp_batch_loop_indices")

    def _inliers(self, fn, where):
        out = np.empty(int(self._moff[-1]), dtype=np.uint8)
        capi.check(fn(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))), where)
        return self._split(out.astype(bool))

    def get_inliers(self):
        """per pair, a bool per moving point: its match of the most recent matching pass was kept (all True without a gate)"""
        return self._inliers(self._lib.icp_batch_get_inliers, "icp_batch_get_inliers")

    def loop_inliers(self):
        """per pair, a bool per moving point: its match of the last pass that contributed to T was kept"""
        return self._inliers(self._lib.icp_batch_loop_inliers, "icp_batch_loop_inliers")

    def evaluate(self, max_distance=None, metric=capi.ICP_POINT_TO_POINT, want_matches=False):
        """how well every pair is registered where its moving cloud stands (icp_batch_evaluate: after begin the start cloud, after
        run the moved one; the loop does not notice).  max_distance: a scalar for every pair, one value per pair (inf: every match of
        that pair counts), or None (every match counts) -- the evaluation's own distance, not the batch's gate.  One dict per pair:
        status, inliers, fitness (inliers / n), rmse (over the inliers), information (6 x 6 float64, order rx ry rz tx ty tz: the
        metric's Gauss-Newton matrix over the inliers); with want_matches also idx and inliers_mask (bool)."""
        md = self._per_pair(max_distance, "evaluation distance")
        total = int(self._moff[-1])
        status, inl = np.zeros(self.count, dtype=np.intc), np.zeros(self.count, dtype=np.int32)
        fit, rmse, info = np.zeros(self.count), np.zeros(self.count), np.zeros((self.count, 6, 6))
        idx = np.zeros(total, dtype=np.int32) if want_matches else None
        mask = np.zeros(total, dtype=np.uint8) if want_matches else None
        pd, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        capi.check(self._lib.icp_batch_evaluate(self._h, int(metric), _ptr(md),
                                                status.ctypes.data_as(C.POINTER(C.c_int)), inl.ctypes.data_as(pi32), fit.ctypes.data_as(pd),
                                                rmse.ctypes.data_as(pd), info.ctypes.data_as(pd),
                                                _ptr(idx, C.c_int32), _ptr(mask, C.c_uint8)), "icp_batch_evaluate")
        out = [dict(status=int(status[b]), inliers=int(inl[b]), fitness=float(fit[b]), rmse=float(rmse[b]), information=info[b].copy())
               for b in range(self.count)]
        if want_matches:
            for b, (i, m) in enumerate(zip(self._split(idx), self._split(mask.astype(bool)))):
                out[b]["idx"], out[b]["inliers_mask"] = i, m
        return out

    def diag_eval_moments(self, b):
        """the ICP_NMOM evaluation vector of pair b from the latest evaluate() (icp_diag_batch_eval_moments; slots capi.EVAL_*)"""
        mom = np.zeros(capi.ICP_NMOM, dtype=np.float64)
        capi.check(self._lib.icp_diag_batch_eval_moments(self._h, int(b), mom.ctypes.data_as(C.POINTER(C.c_double))), "icp_diag_batch_eval_moments")
        return mom


# ---- host-only helpers (no device) -------------------------------------------------------------
def intensity_from_rgb(rgb):
    """(n,) float64: the mean of the three channels of an (n, 3) colour array, (r + g) + b over 3.0 in double -- the intensity
    Open3D's colored ICP takes (Batch.set_intensities)"""
    c = np.asarray(rgb, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("rgb must be (n, 3)")
    return np.ascontiguousarray(((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0)


def covariances_from_normals(normals, eps=1e-3):
    """(n, 6) float64: I - (1 - eps) n n^T per point as xx, xy, xz, yy, yz, zz -- the plane regularisation of the Generalized-ICP
    paper (variance eps along the normal, 1 across it) for callers who have good unit normals (Batch.set_covariances)"""
    N = np.asarray(normals, dtype=np.float64)
    if N.ndim != 2 or N.shape[1] != 3:
        raise ValueError("normals must be (n, 3)")
    s = 1.0 - float(eps)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.ascontiguousarray(np.stack([1.0 - s * x * x, -s * x * y, -s * x * z, 1.0 - s * y * y, -s * y * z, 1.0 - s * z * z], axis=1))


def oriented_normals(points, covariances, viewpoint):
    """(n, 3) float64 unit normals from per-point covariances ((n, 6): xx, xy, xz, yy, yz, zz, as Batch.estimate_covariances
    returns them): the eigenvector of the smallest eigenvalue, flipped to face viewpoint (3,) -- what Batch.compute_features takes"""
    C6 = np.ascontiguousarray(covariances, dtype=np.float64)
    P = np.asarray(points, dtype=np.float64)
    if C6.ndim != 2 or C6.shape[1] != 6 or P.shape != (C6.shape[0], 3):
        raise ValueError("points must be (n, 3) and covariances (n, 6)")
    _, Z = np.linalg.eigh(C6[:, np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])])
    N = Z[:, :, 0]
    flip = (N * (np.asarray(viewpoint, dtype=np.float64)[None, :] - P)).sum(1) < 0
    return np.ascontiguousarray(np.where(flip[:, None], -N, N))


def solve_rigid(mom):
    """icp_solve_rigid: the point-to-point solve with the determinant fix -- R is always a rotation"""
    lib = capi.load()
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    R, t = np.zeros(9), np.zeros(3)
    pd = C.POINTER(C.c_double)
    capi.check(lib.icp_solve_rigid(mom.ctypes.data_as(pd), R.ctypes.data_as(pd), t.ctypes.data_as(pd)), "icp_solve_rigid")
    return R.reshape(3, 3), t


def solve_point_to_point(mom):
    lib = capi.load()
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    R, t = np.zeros(9), np.zeros(3)
    pd = C.POINTER(C.c_double)
    capi.check(lib.icp_solve_point_to_point(mom.ctypes.data_as(pd), R.ctypes.data_as(pd), t.ctypes.data_as(pd)),
               "icp_solve_point_to_point")
    return R.reshape(3, 3), t


def solve_point_to_plane(mom):
    lib = capi.load()
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    R, t, x = np.zeros(9), np.zeros(3), np.zeros(6)
    pd = C.POINTER(C.c_double)
    capi.check(lib.icp_solve_point_to_plane(mom.ctypes.data_as(pd), R.ctypes.data_as(pd), t.ctypes.data_as(pd),
                                            x.ctypes.data_as(pd)), "icp_solve_point_to_plane")
    return R.reshape(3, 3), t, x


def solve_symmetric(mom):
    """the symmetric metric's step from a pass's vector (icp_solve_symmetric): (R, t, x), x = (a, tt) as solved, R = Ra Ra and
    t = Ra (c tt) with Ra the rotation by atan(|a|) about a"""
    lib = capi.load()
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    R, t, x = np.zeros(9), np.zeros(3), np.zeros(6)
    pd = C.POINTER(C.c_double)
    capi.check(lib.icp_solve_symmetric(mom.ctypes.data_as(pd), R.ctypes.data_as(pd), t.ctypes.data_as(pd),
                                       x.ctypes.data_as(pd)), "icp_solve_symmetric")
    return R.reshape(3, 3), t, x


def shard_range(n, rank, world):
    lib = capi.load()
    b, c = C.c_int64(0), C.c_int64(0)
    capi.check(lib.icp_shard_range(int(n), int(rank), int(world), C.byref(b), C.byref(c)), "icp_shard_range")
    return b.value, c.value


def share_rows_plan(hits, blocks, model_points, min_hits=64):
    """how a launch of `blocks` matching blocks deals itself to the rows whose hit counts of the previous launch are `hits`
    (icp_share_rows_plan): returns (parts per row, target hits per block)"""
    lib = capi.load()
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    parts = np.zeros(hits.shape[0], dtype=np.int32)
    target = C.c_uint32(0)
    capi.check(lib.icp_share_rows_plan(hits.ctypes.data_as(C.POINTER(C.c_uint32)), int(hits.shape[0]), int(blocks), int(model_points), int(min_hits),
                                       parts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(target)), "icp_share_rows_plan")
    return parts, int(target.value)


def eigh3(A):
    lib = capi.load()
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(9)
    w, Z = np.zeros(3), np.zeros(9)
    pd = C.POINTER(C.c_double)
    capi.check(lib.icp_eigh3(A.ctypes.data_as(pd), w.ctypes.data_as(pd), Z.ctypes.data_as(pd)), "icp_eigh3")
    return w, Z.reshape(3, 3)


def plane_from_points(abc):
    """the plane (nx, ny, nz, d) of three points (3, 3) by icp_batch_segment_plane's rule (icp_plane_from_points), or None where
    the hypothesis is invalid: coincident or collinear points, or a cross product outside the double range"""
    lib = capi.load()
    abc = np.ascontiguousarray(abc, dtype=np.float64).reshape(9)
    out = np.zeros(4)
    pd = C.POINTER(C.c_double)
    rc = lib.icp_plane_from_points(abc.ctypes.data_as(pd), out.ctypes.data_as(pd))
    if rc == capi.ICP_ERR_EMPTY:
        return None
    capi.check(rc, "icp_plane_from_points")
    return out


def plane_from_moments(centroid, cov6):
    """the plane (nx, ny, nz, d) through centroid (3,) whose normal is the eigenvector of the smallest eigenvalue of the second
    moments cov6 (xx, xy, xz, yy, yz, zz): the last step of icp_batch_segment_plane's refit (icp_plane_from_moments), or None where
    that vector is zero or not finite"""
    lib = capi.load()
    c = np.ascontiguousarray(centroid, dtype=np.float64).reshape(3)
    v = np.ascontiguousarray(cov6, dtype=np.float64).reshape(6)
    out = np.zeros(4)
    pd = C.POINTER(C.c_double)
    rc = lib.icp_plane_from_moments(c.ctypes.data_as(pd), v.ctypes.data_as(pd), out.ctypes.data_as(pd))
    if rc == capi.ICP_ERR_EMPTY:
        return None
    capi.check(rc, "icp_plane_from_moments")
    return out


class LocalComm:
    """icp_lcomm_*: the host-memory communicator on its own (no device): sum of <= 32 doubles over the ranks of a node,
    added in rank order on every rank."""

    def __init__(self, id_bytes, rank, world):
        self._lib = capi.load()
        self._h = C.c_void_p()
        buf = (C.c_ubyte * 128).from_buffer_copy(id_bytes)
        capi.check(self._lib.icp_lcomm_create(buf, int(rank), int(world), C.byref(self._h)), "icp_lcomm_create")

    def allreduce(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64).copy()
        capi.check(self._lib.icp_lcomm_allreduce(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), int(v.size)), "icp_lcomm_allreduce")
        return v

    def close(self):
        if self._h:
            self._lib.icp_lcomm_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
