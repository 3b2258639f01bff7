/*
 * icp_mi355x.h -- C ABI of libicp_mi355x.so, the MI355X (gfx950) ICP registration hot path.
 *
 * The reference (Carlos310197/Fast-Point-Cloud-Registration-with-GPUs) has no library, plugin or
 * FFI interface: the path sits behind three main() programs (CMakeLists.txt:26, README.md:12).
 * The narrowest seams that exist are its kernel signatures and its driver loops; every entry
 * point below names the reference statement group it replaces (file:line relative to the
 * reference root).  Plain C: opaque handle, caller-owned buffers, int return codes, no
 * exceptions, no exit().  Nothing here takes or returns a torch type.
 *
 * Conventions
 *   - clouds cross the boundary in the reference GPU layout: AoS "xyzxyz..." (column-major 3xN,
 *     src/ICP_point_to_point.cu:139-152), float or double, HOST pointers unless a name says _dev.
 *   - correspondence semantics are those of the CPU path (src/ICP_CPU.c:227-232): squared
 *     distance (dx*dx + dy*dy) + dz*dz with every operation rounded separately (no FMA), the
 *     LOWEST model index wins ties, every idx[i] is always written.  Finite coordinates can square to +inf (around 1e20 in
 *     float, 1e160 in double): a point whose every distance overflowed matches model point 0 -- what an ascending scan with
 *     a strict `<` keeps -- in both precisions, in every kernel, and the moment sums carry point 0's coordinates for it.
 *   - rotation matrices are row-major 3x3 (R maps moving -> model), transforms row-major 4x4.
 *   - non-finite input -- a DELIBERATE DEVIATION from the reference, listed in INTEGRATION.md under "entry points that change
 *     behaviour": a cloud (or normal set) with a NaN or an infinite coordinate is REFUSED -- icp_set_model, icp_set_moving,
 *     icp_set_model_normals and everything built on them (icp_nn_match_*, icp_point_to_*) return ICP_ERR_INVALID and the
 *     context keeps no such cloud.  The reference does not check its input: its distances come from vdSub / vdSqr / vdAdd
 *     (src/ICP_CPU.c:227-231) and the match from cblas_idamin (:232), whose answer for a vector that holds NaN is whatever
 *     the BLAS at hand does (MKL documents none); whichever index comes back, the centroid sums (:342-366) then turn the
 *     whole transform into NaN.  There is nothing usable to reproduce, so the library says so at the door.
 *   - a context is bound to one HIP device; calls on one context are not re-entrant, distinct
 *     contexts are independent.  Every device entry point fails with ICP_ERR_NO_DEVICE when no
 *     gfx950 device is usable -- there is no CPU fallback.
 */
#ifndef ICP_MI355X_H
#define ICP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICP_ABI_VERSION 2 /* 2: icp_result gained seconds_host / seconds_setup, icp_loop_phase_seconds; later the icp_batch_* entry
                           * points were added, icp_batch_evaluate, icp_batch_downsample and icp_batch_remove_outliers among them (new symbols only: nothing that existed changed) */

/* return codes */
#define ICP_OK 0
#define ICP_ERR_INVALID (-1)   /* bad argument (NULL pointer, negative size, unknown enum) */
#define ICP_ERR_NO_DEVICE (-2) /* no usable HIP device / device index out of range */
#define ICP_ERR_HIP (-3)       /* a HIP runtime call or kernel launch failed (see icp_last_error) */
#define ICP_ERR_EMPTY (-4)     /* no model point (m == 0) where a match is required, or no correspondence within the maximum
                                * distance (a gated pair of a batch whose matching pass kept no point) */
#define ICP_ERR_SINGULAR (-5)  /* 6x6 point-to-plane system not positive definite */
#define ICP_ERR_IO (-6)        /* dataset file missing / malformed */
#define ICP_ERR_STATE (-7)     /* call sequence error (e.g. step before begin, clouds not set) */
#define ICP_ERR_NOMEM (-8)

typedef enum { ICP_F32 = 0, ICP_F64 = 1 } icp_precision;
typedef enum { ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1 } icp_metric;

typedef struct icp_ctx icp_ctx; /* opaque: owns device buffers, stream, pinned staging */

/* number of doubles in the per-iteration moment vector (the only data that ever crosses ranks) */
#define ICP_NMOM 32
/* moment vector slots (doubles).  Point-to-point uses [0..18], point-to-plane [0..1] + [2..28]. */
#define ICP_MOM_ERR 0  /* sum |p_new - q[idx_prev]|^2 of the transform applied in this enqueue */
#define ICP_MOM_CNT 1  /* number of moving points that contributed */
#define ICP_MOM_SP 2   /* sum p (3) */
#define ICP_MOM_SQ 5   /* sum q[idx] (3) */
#define ICP_MOM_SQP 8  /* sum q_a * p_b, a-major (9) */
#define ICP_MOM_SPP 17 /* sum |p|^2   (informational: nothing on the path reads these two; the single-GPU point-to-point */
#define ICP_MOM_SQQ 18 /* sum |q[idx]|^2  fast path, whose rows the host adds itself, leaves them 0)                         */
#define ICP_MOM_C 2    /* point-to-plane: upper triangle of C, row-major (21) */
#define ICP_MOM_B 23   /* point-to-plane: b (6) */
#define ICP_MOM_W 29   /* sum of the weights of the kept matches (robust batches; both metrics) */

typedef struct icp_params {
    int max_iter;         /* MAX_ITER: 200 src/ICP_CPU.c:17, 40 src/ICP_point_to_point.cu:24, 50 ICP_point_to_plane.cu:23 */
    double tol;           /* 1e-5 src/ICP_CPU.c:267, 1e-6 src/ICP_point_to_point.cu:420 */
    int fixed_iterations; /* != 0: no tolerance test, run exactly max_iter passes (src/ICP_standard.cu:369) */
    int precision;        /* icp_precision of the device arithmetic */
    int metric;           /* icp_metric */
} icp_params;

typedef struct icp_result {
    double T[16];        /* composed transform, row-major 4x4: T = [R_k|t_k] * ... * [R_0|t_0] */
    int iterations;      /* the reference's `iteration` / `num_iterations` at loop exit */
    int passes;          /* matching passes that contributed to T */
    double* err;         /* caller-allocated max_iter+1 doubles (or NULL); err[0] = 0, err[k] = RMS after pass k-1 */
    int32_t* idx;        /* caller-allocated n int32 (or NULL): correspondences of the last contributing pass */
    void* moved;         /* caller-allocated 3n values of the run's precision, AoS (or NULL): final moving cloud */
    double seconds_total;   /* wall-clock of the loop (upload/download excluded) */
    double seconds_nn;      /* device time of the matching kernels, summed (0 unless profiling enabled) */
    /* per-phase seconds (the reference's match_time / minimization_time / transf_time / error_time,
     * src/CUDA/GPU_point_to_point_real.cu:241,386-403).  Transformation and error estimation have no time of their own
     * here: they are the front end of the matching kernel (same launch) and are inside seconds_nn. */
    double seconds_host;    /* host half of the iterations, summed: error + stop rule + 3x3 SVD / 6x6 solve (0 unless profiling enabled) */
    double seconds_setup;   /* icp_point_to_*: icp_set_model (+ normals) + icp_set_moving of this call -- upload, layout, order, boxes */
} icp_result;

/* ---- library / context ------------------------------------------------------------------- */
int icp_abi_version(void);
const char* icp_strerror(int code);
/* last error text of the calling thread (HIP error strings etc.), never NULL */
const char* icp_last_error(void);
/* number of usable HIP devices, or a negative error code */
int icp_device_count(void);
/* The loop is a host-thread <-> GPU conversation and every message from the other socket costs ~0.5 us more, so the entry
 * points that hold that conversation (icp_create while it allocates its pinned buffers, icp_loop_run, icp_loop_complete,
 * icp_point_to_*) narrow the calling thread's CPU affinity to the device's NUMA node (sysfs local_cpulist) if the thread
 * currently runs elsewhere -- and put the caller's mask back before they return.  ICP_PIN=0 never touches the affinity;
 * ICP_PIN=2 narrows once in icp_create and keeps it (a thread dedicated to the context). */
int icp_create(int device, icp_ctx** out);
void icp_destroy(icp_ctx* ctx);
/* run all work of this context on an externally owned hipStream_t (e.g. torch's current stream);
 * NULL restores the context's own stream */
int icp_set_stream(icp_ctx* ctx, void* hip_stream);
/* hipEvent timing of the matching kernel inside the loop: 0 = off, n > 0 = time every n-th launch
 * (two event records + a stream synchronisation on the timed launches only; with a resident registration
 * kernel the launch is the whole registration).  The call restarts the stride and the accumulators: the first
 * launch after it is a timed one. */
int icp_set_profiling(icp_ctx* ctx, int every_nth);

/* ---- matching seam: replaces  Matching<<<>>>(n, P, Q, q_points, idx)
 *      src/CUDA/GPU_point_to_point_real.cu:38-79, src/ICP_point_to_point.cu:31-57 (fp32) and the
 *      MKL loop src/ICP_CPU.c:220-234 (fp64).  Host pointers, AoS.  idx[i] in [0, m). --------- */
int icp_nn_match_f32(icp_ctx* ctx, const float* P_aos, int n, const float* Q_aos, int m, int32_t* idx);
int icp_nn_match_f64(icp_ctx* ctx, const double* P_aos, int n, const double* Q_aos, int m, int32_t* idx);

/* ---- resident clouds (data stays in HBM between calls) ------------------------------------- */
/* upload + convert to the internal padded SoA layout.  precision: ICP_F32 / ICP_F64 selects the
 * element type of `xyz_aos` AND of the device arithmetic. */
int icp_set_model(icp_ctx* ctx, const void* xyz_aos, int m, int precision);
int icp_set_moving(icp_ctx* ctx, const void* xyz_aos, int n, int precision);
/* unit normals of the model points, AoS, same precision as the model (point-to-plane) */
int icp_set_model_normals(icp_ctx* ctx, const void* nxyz_aos, int m);
/* put the moving cloud back to the state icp_set_moving uploaded (device-to-device copy of a resident pristine
 * copy): lets a caller register the same pair repeatedly without touching PCIe */
int icp_reset_moving(icp_ctx* ctx);
int icp_get_moving(icp_ctx* ctx, void* xyz_aos_out);        /* 3n values, precision of the cloud */
int icp_get_indices(icp_ctx* ctx, int32_t* idx_out);        /* n int32: the most recent matching pass */
/* one matching pass over the resident clouds; indices stay on the device.  kernel_ms (optional)
 * receives the hipEvent time of the matching kernel(s) alone. */
int icp_nn_match_resident(icp_ctx* ctx, float* kernel_ms);
/* geometry of the last matching launch (the programs print it as the reference prints its Grid Size / Block Size,
 * src/CUDA/GPU_point_to_point_real.cu:237).  threads: the block of a steady pass of the loop, not exclusive.  For ICP_F64 clouds
 * on rows of 64 points it reports 512 although the launch takes 1024 wherever the rows do not outnumber the CUs (a value kept
 * as callers have seen it). */
int icp_nn_launch_info(icp_ctx* ctx, int* splits, int* blocks, int* threads, int* n_pad, int* m_pad);
/* The caller owns the device (no other context of this or any other process keeps kernels resident on it): clouds of up to
 * 16 384 moving points (one row of 64 per CU) then run their rows as 16-wave blocks, one to a CU, instead of 8-wave blocks that
 * leave room for a second resident context -- hall pair 9.5 -> 9.15 us per iteration (profiles/r2/r2_02_waves_8_vs_16.txt).
 * The results are the same bits.  Off by default: the library cannot see who else is on the device.  (The reference's
 * programs own their GPU implicitly, src/ICP_point_to_point.cu:90.) */
int icp_set_exclusive(icp_ctx* ctx, int on);

/* ---- model normals: replaces knn + Normals + host ssyev loop
 *      src/CUDA/GPU_point_to_plane_real.cu:54-188,391-423 (k = 4 neighbours, self excluded).
 *      Works on the resident model; results stay resident and are optionally returned.
 *      Neighbours, mean and covariance are formed in the model's own precision: an ICP_F64 model (survey coordinates,
 *      a small patch far from the origin) gets its normals from double arithmetic throughout.
 *      The rule, over the whole range of the model's precision F (tests/knn_ref.py states it in numpy):
 *      Neighbours.  d(i, j) = (dx*dx + dy*dy) + dz*dz, every operation rounded separately in F.  The candidates of query i
 *      are all j in [0, m), i included, with d(i, j) < +inf, ordered by (d, j) ascending; rank 0 is dropped, ranks 1-4 are the
 *      neighbours.  A rank that does not exist (fewer than five candidates: the points are so far apart that the squared
 *      distances overflow) holds index 0: every index returned, and every index the normals read, lies in [0, m).  The rule
 *      has no sentinel; it is the reference's k+1 passes of first-arg-min with overwrite-by-10000 exactly where every query's
 *      fifth-smallest distance is below 10000.
 *      Normals.  bar = (sum of the four neighbours) * 0.25, then the six sums A += (x - bar)(y - bar) over them, in F.  If
 *      an entry of that covariance is not finite, the normal is exactly (+0, +0, +0) -- the rule of
 *      icp_batch_estimate_point_normals -- and the point adds nothing to the sums of a point-to-plane pass.  Otherwise it
 *      is the unit eigenvector of the eigenvalue of smallest magnitude (magnitudes compared in F, the first of the ascending
 *      eigenvalues on ties); a zero covariance gives the first axis. ------- */
int icp_estimate_normals(icp_ctx* ctx, void* nxyz_aos_out /*3m or NULL*/, int32_t* neighbours_out /*4m or NULL*/);

/* ---- the ICP loops: replace main()'s while-loops
 *      point-to-point  src/ICP_CPU.c:217-271, src/ICP_point_to_point.cu:295-423
 *      point-to-plane  src/ICP_point_to_plane.cu:517-631, src/CUDA/CPU_ICP_point_to-plane.cpp:309-428
 *      Clouds are host AoS arrays of prm->precision.  For point-to-plane the model normals are
 *      estimated on the device first unless `normals_aos` is given. ---------------------------- */
int icp_point_to_point(icp_ctx* ctx, const void* data_aos, int n, const void* model_aos, int m,
                       const icp_params* prm, icp_result* out);
int icp_point_to_plane(icp_ctx* ctx, const void* data_aos, int n, const void* model_aos, int m,
                       const void* normals_aos /*may be NULL*/, const icp_params* prm, icp_result* out);

/* ---- step-wise loop over the resident clouds (what the loops above are built from; used by the
 *      multi-GPU driver, which all-reduces the moment vector between enqueue and complete) ---- */
int icp_loop_begin(icp_ctx* ctx, const icp_params* prm);
/* enqueue (asynchronously): [transform + error of the previous pass] -> matching -> fused
 * gather/moments -> finalize into the ICP_NMOM-double device vector. */
int icp_loop_enqueue(icp_ctx* ctx);
/* device address of that vector (valid until icp_destroy); to be summed across ranks in place */
void* icp_loop_moments_dev(icp_ctx* ctx);
/* optional: make the loop write its moments into caller-owned device memory (e.g. a torch tensor) */
int icp_loop_set_moments_dev(icp_ctx* ctx, void* dev_ptr_32_doubles);
/* copy the (reduced) vector back, evaluate the stop rule, solve R,t for the next pass.
 * *done != 0 when the loop has ended. */
int icp_loop_complete(icp_ctx* ctx, int* done);
/* up to max_steps x (enqueue + complete) without returning to the caller in between (single GPU, or a
 * communicator attached with icp_comm_init); stops early when the loop ends */
int icp_loop_run(icp_ctx* ctx, int max_steps, int* steps_done, int* done);
/* A pass of icp_loop_run's resident / armed conversation that never delivers its rows (a lost message, blocks that another
 * process kept off the machine) does not end the registration when the loop started from the cloud icp_set_moving uploaded
 * (or icp_reset_moving restored) and no communicator is attached: the kernel is withdrawn and the same registration is run
 * again from the copy with plain launches, one per pass -- every loop form yields the same bits.  ICP_ERR_HIP is returned
 * only if that fails as well.  icp_recoveries: how often this context has done so (the reference's loops,
 * src/ICP_point_to_point.cu:308-421, are plain launches throughout and have nothing to recover from). */
int icp_recoveries(icp_ctx* ctx);
/* current state: iterations so far, error series (count doubles), composed transform.
 * After a FAILED icp_loop_run / icp_loop_complete: a numeric failure (degenerate correspondences: ICP_ERR_SINGULAR /
 * ICP_ERR_INVALID from the minimisation) ends the loop but keeps its state readable -- this call, icp_loop_indices and
 * icp_get_moving answer for the passes that completed.  A device failure (ICP_ERR_HIP, a pass that never delivered its rows)
 * discards the loop: this call then returns ICP_ERR_STATE and icp_get_moving the cloud as icp_set_moving uploaded it. */
int icp_loop_state(icp_ctx* ctx, int* iterations, int* passes, double* err, int err_cap, double* T16);
/* summed hipEvent time and count of the matching-kernel launches timed since icp_set_profiling was last called
 * (cumulative over loops; the bench's roofline leg reads the timed region through this) */
int icp_loop_timing(icp_ctx* ctx, double* seconds_nn, int* nn_launches);
/* matching passes executed by those timed launches: equal to their count when every pass is its own launch, larger
 * when icp_loop_run keeps ONE resident kernel for a whole registration (that kernel is then the timed launch, every
 * n-th one, host round trips between its passes included) */
int icp_loop_timing_passes(icp_ctx* ctx, long long* passes);
/* the current (or last) loop's own phase sums: matching-kernel seconds and host-solve seconds, as icp_result reports them
 * (both 0 unless icp_set_profiling is on); either pointer may be NULL */
int icp_loop_phase_seconds(icp_ctx* ctx, double* seconds_nn, double* seconds_host);
/* correspondences of the last pass that contributed to T (ping-pong buffer), n int32 */
int icp_loop_indices(icp_ctx* ctx, int32_t* idx_out);

/* ---- batched ICP: many independent small pairs, one launch of every pair's pass per step -----------------------------
 * The reference registers one pair per program run (src/ICP_point_to_point.cu:295-423, src/ICP_point_to_plane.cu:517-631); a
 * loop of icp_point_to_point / icp_point_to_plane over many small pairs pays a whole iteration's launch and round trip (and,
 * for point-to-plane, a neighbour search of its own) per pair.  A batch keeps all its pairs on the device and
 * runs ONE matching launch + ONE reduction launch + ONE 32-double-per-pair download per step for every pair still running.  It
 * offers both metrics, and per pair a maximum correspondence distance, an initial transform, trimmed rejection and an evaluation
 * of the pose it stands at (fitness, inlier RMSE, information matrix).
 *   - pair b = moving points [moving_off[b], moving_off[b+1]) and model points [model_off[b], model_off[b+1]) of the
 *     concatenated AoS arrays, element type = precision (as icp_set_model).  Offsets: count+1 int64, starting at 0, strictly
 *     increasing (every cloud >= 1 point, <= ICP_BATCH_MAX_POINTS).  Anything else, a NaN or an infinite coordinate
 *     anywhere or count < 1 is refused with ICP_ERR_INVALID, and no batch is made.
 *   - each pair's loop is exactly what icp_point_to_point (icp_point_to_plane with the same normals) computes for that pair
 *     alone (same stop rule, iterations, passes,
 *     err series, composed T, idx of the last contributing pass, final cloud), and a pair's bits do not depend on the other
 *     pairs of the batch or their order: work is cut relative to each pair's first point, partial sums are added per pair
 *     in a fixed order, there are no floating-point atomics.  Pairs finish independently; a numeric failure of one pair's
 *     minimisation ends that pair only (its status: ICP_ERR_SINGULAR where a pair's 6x6 point-to-plane system is not
 *     positive definite), the others go on.
 *   - a batch uses the context's device and stream and nothing else of it (resident clouds, loop, counters stay as they
 *     were).  It must be destroyed before its context.  While the context has an enqueued pass that is not completed
 *     (icp_loop_enqueue without icp_loop_complete) the batch calls return ICP_ERR_STATE.
 *   - icp_batch_begin starts every pair's registration from the clouds icp_batch_create uploaded (moved by the pair's initial
 *     transform, where the batch holds any: below).
 *   - point-to-plane needs the unit normals of every pair's model points.  The batch holds one set: the caller's
 *     (icp_batch_set_model_normals) or the one icp_batch_estimate_normals makes on the device -- kNN(4) + PCA exactly as
 *     icp_estimate_normals does for one model (src/CUDA/GPU_point_to_plane_real.cu:54-188,391-423), with ONE neighbour launch
 *     and ONE normals launch for all pairs; every pair's neighbours and normals are those of icp_estimate_normals on that
 *     model alone, bit for bit.  Either call may come at any time after icp_batch_create and replaces the set; a loop under
 *     way is discarded (icp_batch_run returns ICP_ERR_STATE until the next icp_batch_begin).  A refused call leaves the batch's
 *     normals as they were (none, or the previous set).  icp_batch_begin accepts ICP_POINT_TO_PLANE only on a batch that holds
 *     normals (else ICP_ERR_INVALID); a batch that holds normals still begins ICP_POINT_TO_POINT, with the bits of one that
 *     holds none.
 *   - maximum correspondence distance (icp_batch_set_max_distance): one double per pair, each > 0 or +INFINITY (that pair is
 *     not gated); NULL removes the gate.  Without it every moving point pulls on its nearest model point however far away,
 *     which is the reference's behaviour.
 *       threshold: thr_p = (F)(max_dist[p] * max_dist[p]) -- the product formed in double and rounded once to the batch's
 *         precision F; +INFINITY gives thr = +inf.  A NaN, a value <= 0 or -INFINITY anywhere: ICP_ERR_INVALID, the message
 *         names the pair, and the batch keeps the thresholds it had (or none).
 *       the call may come at any time after icp_batch_create; like the normals calls it discards a loop under way
 *         (icp_batch_run returns ICP_ERR_STATE until the next icp_batch_begin).
 *       gate: a match is kept iff d <= thr_p, where d is the winning squared distance the matching already holds --
 *         (dx*dx + dy*dy) + dz*dz, every operation rounded separately in F; nothing is recomputed in double, and a point
 *         exactly on the threshold is kept.  For point-to-plane the gate is on the same Euclidean d.
 *       idx is unchanged: every index is the bit-exact nearest neighbour in [0, m), kept or not.
 *       sums: only kept points contribute to ICP_MOM_CNT and to every sum of the pass, for both metrics.  ICP_MOM_ERR of a
 *         pass is the sum of |p_new - q[idx_prev]|^2 over the points kept by the matching pass those indices came from, and
 *         err[k] = sqrt(ERR_k) / sqrt(CNT_{k-1}), CNT_{k-1} being the kept count of that same matching pass.
 *       a matching pass that keeps no point ends that pair with status ICP_ERR_EMPTY (unless the stop rule ended its loop on
 *         that very pass): err[k] of the pass is recorded; T, iterations, passes and the cloud are those of the passes
 *         completed; the other pairs go on.  One or two kept points in point-to-point behave as a one- or two-point cloud
 *         does; a 6x6 system that is not positive definite ends the pair with ICP_ERR_SINGULAR.
 *       a batch with no gate, or with every value +INFINITY, produces the bits of a batch that never heard of the gate, and a
 *         gated pair's bits depend on that pair and its threshold alone (no atomics, fixed order).
 *       icp_batch_get_inliers / icp_batch_loop_inliers: one byte per moving point, 1 = that point's match was kept, for the
 *         pass icp_batch_get_indices / icp_batch_loop_indices report, with their errors and ordering (ICP_ERR_STATE before
 *         the first pass and during the context's pending pass).  An ungated batch answers all ones.
 *   - initial transforms (icp_batch_set_initial_transforms): one row-major 4x4 of doubles per pair (the layout of icp_result.T),
 *     the pose each pair's registration starts from -- an odometry guess, a coarse registration's result, the T of an earlier
 *     run of this very batch (coarse-to-fine gating without another upload); NULL removes them.
 *       validation: every value finite (and finite once rounded to the batch's precision), every bottom row 0 0 0 1; anything
 *         else is ICP_ERR_INVALID, the message names the first offending pair, and the batch keeps the transforms it had (or
 *         none).  The upper 3x4 is applied as given: no orthogonality or determinant check (the library's own R carries no
 *         reflection fix either).
 *       rounding: the 12 values of a pair are rounded once to the batch's precision F; T0F is that matrix read back in double.
 *       the call may come at any time after icp_batch_create; like the normals and gate calls it discards a loop under way
 *         (icp_batch_run returns ICP_ERR_STATE until the next icp_batch_begin).
 *       icp_batch_begin: pair p starts from apply(T0F_p, p0), p0 the point as uploaded, in the arithmetic every pass moves
 *         points with: ((r0 x + r1 y) + r2 z) + t, every operation rounded separately in F.  The uploaded clouds are never
 *         modified: every begin starts from them, transforms do not compound over repeated begins.  A pair whose 16 doubles are
 *         the identity bit for bit is copied, not multiplied (its start cloud has the bytes of the upload, a -0.0 included).
 *         All pairs' start clouds come from ONE launch in icp_batch_begin, in place of the device-to-device copy; a batch that
 *         holds no transforms begins with that copy, as it always did, and the steps are the same either way.
 *       results: from the start cloud on, a pair's loop is that of a batch without initial transforms created from that start
 *         cloud -- status, iterations, passes, the err series (err[0] = 0: the initial transform is not a pass), idx, inlier
 *         masks, moment vectors and the final cloud, bit for bit, whatever the other pairs and their order.  The gate therefore
 *         acts on distances measured after the initial transform.  icp_batch_state reports T = T_loop . T0F, T_loop being what
 *         that plain batch reports and the product formed in double, s = 0; s += T_loop[a][k] * T0F[k][b] for k = 0..3; a
 *         copied (identity) pair reports T_loop untouched.
 *       overflow: a finite transform can carry a finite cloud out of F's range.  A pair whose start cloud holds a NaN or an
 *         infinite coordinate begins ended: status ICP_ERR_INVALID, passes 0, iterations 0, T = T0F.  icp_batch_begin still
 *         returns ICP_OK and the other pairs run.  (One int per pair comes back from the launch: icp_batch_begin waits for it
 *         when, and only when, the batch holds transforms.)
 *   - trimmed rejection (icp_batch_set_trim): one double per pair, the share rho of the moving cloud to keep -- the share that
 *     overlaps the model, which a user usually knows where a fitting distance is not known (Chetverikov's TrICP); NULL removes
 *     trimming.
 *       validation: each value must satisfy 0 < rho <= 1.  A NaN, a value <= 0 or a value > 1 anywhere: ICP_ERR_INVALID, the
 *         message names the first offending pair, and the batch keeps the shares it had (or none).
 *       the call may come at any time after icp_batch_create; like the normals, gate and initial-transform calls it discards
 *         a loop under way (icp_batch_run returns ICP_ERR_STATE until the next icp_batch_begin), and it returns ICP_ERR_STATE
 *         while the context has a pending pass.
 *       rank: K_p = ceil(rho_p * (double)n_p), the product formed in double, clamped to [1, n_p]; fixed at the call, because
 *         n_p never changes.  rho_p == 1.0 exactly means the pair is not trimmed.
 *       threshold: in every matching pass of a trimmed pair tau_p is the K_p-th smallest of the pair's n_p winning squared
 *         distances d_i, where d_i is the value the matching already holds -- (dx*dx + dy*dy) + dz*dz, every operation
 *         rounded separately in the batch's precision F; nothing is recomputed.  tau_p is therefore one of the d_i, bit for
 *         bit.  A pair that is not trimmed has tau = +inf.
 *       a match is kept iff d_i <= tau_p -- and also d_i <= thr_p where the batch holds a gate.  Every point tied with the K-th
 *         is kept: the kept count is then >= K_p, and the answer depends on no ordering of equal values.  The selection
 *         ignores the gate: the rank counts all n_p points.  For point-to-plane the test is on the same Euclidean d.
 *       everything else follows the gate's rules.  idx is unchanged: every index is the bit-exact nearest neighbour in [0, m),
 *         kept or not.  Only kept points contribute to ICP_MOM_CNT and to every sum of the pass, for both metrics.
 *         ICP_MOM_ERR of a pass is the sum of |p_new - q[idx_prev]|^2 over the points kept by the matching pass those indices
 *         came from, and err[k] = sqrt(ERR_k) / sqrt(CNT_{k-1}).  icp_batch_get_inliers / icp_batch_loop_inliers report the
 *         kept mask.  Trimming alone always keeps at least one point, so ICP_ERR_EMPTY can arise only together with a gate.
 *       bits: a batch with no trim, or with every value 1.0, produces the bits of a batch that never heard of trimming and
 *         runs the same two launches per step.  In a batch that trims some pairs, a pair with rho = 1.0 still has the bits
 *         of that pair in a plain batch: every mask, idx, cloud, err, T and moment vector.  A trimmed pair's bits depend on
 *         that pair, its rho and its gate alone, not on the other pairs or their order (no floating-point atomics, fixed
 *         summation order).  Trimming works with initial transforms as the gate does: distances are measured after the
 *         transform.
 *       cost: a pair's tau is known only when every one of its points has been matched, so a step of a batch that trims at
 *         least one pair runs four launches in place of two (matching, selection, sums, reduction) and still one download.
 *   - reciprocal matches (icp_batch_set_reciprocal): one byte per pair, non-zero = that pair keeps only mutual nearest neighbours
 *     (PCL's reciprocal correspondences): the remedy where many moving points collapse onto one model point at the border of a
 *     partial overlap or next to clutter.  NULL switches reciprocity off for the whole batch.
 *       the call may come at any time after icp_batch_create; like the other icp_batch_set_* calls it discards a loop under way
 *         (icp_batch_run returns ICP_ERR_STATE until the next icp_batch_begin).  A null batch is ICP_ERR_INVALID, a context with
 *         a pending pass ICP_ERR_STATE; a refused call leaves the batch as it was.
 *       rule, in every matching pass of a reciprocal pair: idx[i] is the forward match as ever, the lowest j that minimises
 *         dist2(p_i, q_j) = (dx*dx + dy*dy) + dz*dz, every operation rounded separately in the batch's precision F.  rev[j] is
 *         the lowest i that minimises the same dist2 over the pair's n moving points, on the cloud this pass matched on (the
 *         cloud after the pass's front end has applied the previous motion).  The match of i is mutual iff rev[idx[i]] == i.
 *         dist2 squares its differences, so the reverse distance of (j, i) is the forward distance of (i, j) bit for bit:
 *         both searches compare the same numbers, and only the order among equal ones (lowest index first, both ways) differs.
 *       combination: kept = mutual && d <= tau_p && d <= thr_p -- three independent tests.  tau_p stays the K_p-th smallest of
 *         ALL n_p winning distances of the pair, exactly as without reciprocity (the selection ignores the mutual rule as it
 *         ignores the gate): a reciprocal, trimmed pair may therefore keep fewer than ceil(rho n) points.  (Ranking only the
 *         mutual matches is not offered.)
 *       everything else follows the gate's rules.  idx is unchanged, kept or not; only kept points contribute to ICP_MOM_CNT
 *         and to every sum of the pass, for both metrics; the next pass's ICP_MOM_ERR covers kept points only and err[k] =
 *         sqrt(ERR_k) / sqrt(CNT_{k-1}); icp_batch_get_inliers / icp_batch_loop_inliers report the kept mask.  The mutual rule
 *         alone always keeps at least one point -- the lowest i that attains the pair's smallest distance is mutual -- so
 *         ICP_ERR_EMPTY can still arise only together with a gate.
 *       bits: a batch with no flags, or with every flag 0, runs exactly the steps it runs without them, with the same bits.  In
 *         a batch with a reciprocal pair, a pair whose flag is 0 still has the bits of that pair in a batch without flags, and a
 *         reciprocal pair's bits depend on that pair, its flag, its rho and its gate alone.  Initial transforms: reciprocity
 *         acts on the start cloud.
 *       cost: the reverse search is a second scan of m x n distances in a launch of its own (one block per 64 model points),
 *         so a step of a batch with a reciprocal pair runs four launches (matching, reverse search, decision and sums,
 *         reduction), five when it also trims, and still one download.
 *   - robust kernels (icp_batch_set_robust): one kind (ICP_ROBUST_*) and one scale k per pair.  Every kept match of a robust pair
 *     pulls with a weight w(r) in [0, 1] that falls smoothly with its residual r -- M-estimator weighting, solved as iteratively
 *     re-weighted least squares (Open3D's RobustKernel): the remedy that needs no keep-or-drop decision.  kind == NULL, or every
 *     kind ICP_ROBUST_NONE: the batch is not robust; it runs the steps and produces the bits of a batch that never heard of this.
 *       validation: every kind is one of the four constants; for a kind other than NONE, scale[p] = k must be finite and > 0 and
 *         k * k (formed in double) finite and > 0; the scale of a NONE pair is not read, and scale == NULL is allowed only if
 *         every kind is NONE.  Anything else is ICP_ERR_INVALID, the message names the first offending pair, and the batch keeps
 *         what it had.  A null batch is ICP_ERR_INVALID, a context with a pending pass ICP_ERR_STATE.  Like the other
 *         icp_batch_set_* calls it may come at any time after icp_batch_create and discards a loop under way.
 *       residual, every term formed in double from the widened coordinates of the match (p, q = Q[idx], n = N[idx]):
 *         point-to-point r2 = dx*dx + dy*dy + dz*dz with d = q - p (the front end's error arithmetic); point-to-plane r2 = bi *
 *         bi with bi = (px-qx)*nx + (py-qy)*ny + (pz-qz)*nz, the bi the plane terms form.
 *       weight, in double, k2 = k * k formed once on the host:  ICP_ROBUST_HUBER  r2 <= k2 ? 1 : k / sqrt(r2);
 *         ICP_ROBUST_CAUCHY  1 / (1 + r2 / k2);  ICP_ROBUST_TUKEY  r2 <= k2 ? (1 - r2/k2)^2 : 0;  ICP_ROBUST_NONE  exactly 1.0.
 *         All three are continuous in r: no decision hangs on a rounding.  An overflowed r2 = +inf gives 0, never a NaN.
 *       combination: kept is decided exactly as without kernels -- gate, trim (tau still ranks all n distances) and the mutual
 *         rule.  Weights change no mask and no idx, and nothing icp_batch_get_inliers reports; a kept point whose weight is 0 is
 *         still kept.
 *       sums: ICP_MOM_CNT stays the kept count; ICP_MOM_W = sum w over the kept points; every other slot of the pass is the term
 *         it always was times the point's w (point-to-point SP, SQ, SQP, SPP, SQQ; point-to-plane C, B).  ICP_MOM_ERR is
 *         unchanged: unweighted, over the points the previous matching pass kept; err[k] = sqrt(ERR_k) / sqrt(CNT_{k-1}), the stop
 *         rule and the iteration counting are untouched.
 *       solve: on a copy of the vector whose ICP_MOM_CNT slot holds ICP_MOM_W (icp_host_loop_set_weighted): the point-to-point
 *         solve divides by that slot -- the weighted Kabsch solve -- and the plane solve never reads it.  A matching pass whose
 *         ICP_MOM_W is not > 0 ends the pair with ICP_ERR_EMPTY (unless the stop rule ended the loop on that very pass).
 *       bits: in a robust batch a pair of kind NONE has the bits of that pair in the same batch without kernels (w = 1.0
 *         multiplies exactly; the rows are added in the same block shape and order), and a robust pair's bits depend on that
 *         pair, its kernel, its scale and its other options alone: no floating-point atomics, fixed summation order.  Initial
 *         transforms: weights act on residuals measured after the transform.  icp_batch_evaluate neither reads nor changes
 *         kernels or weights.
 *       icp_batch_get_weights: one double per moving point, each pair's most recent matching pass, with the errors and ordering
 *         of icp_batch_get_indices: 0.0 for a rejected point, 1.0 for a kept point of a NONE pair; a batch without kernels
 *         answers the kept mask as 1.0 / 0.0.  The device buffer behind it exists only once a batch is given kernels.
 *       cost: a step of a robust batch always runs deferred -- matching, [reverse search,] [selection,] batch_robust_moments
 *         (decision, residual, weight, weighted terms), reduction: three launches with nothing else, up to five with reciprocity
 *         and trimming, still one download.
 *   - evaluation (icp_batch_evaluate): did pair p register, and how well is it constrained?  Per pair the fitness (the share of
     its moving points with a model point within a distance of the caller's choosing), the inlier RMSE and the 6 x 6
     information matrix a pose-graph optimiser takes beside T -- measured where the pair's moving cloud stands on the device,
     exactly the cloud icp_batch_get_moving returns: after icp_batch_begin the start cloud (initial transform included: K
     candidate poses of one pair, uploaded K times, are scored with no ICP iteration), after icp_batch_run the cloud moved by
     the `passes` motions icp_batch_state's T describes, for an ended pair the final cloud.
       matching: the batch's own search.  idx is the bit-exact nearest neighbour in [0, m), the lowest index on ties; d is the
         winning squared distance the matching holds -- (dx*dx + dy*dy) + dz*dz, every operation rounded separately in the
         batch's precision F; nothing is recomputed.
       gate: max_dist follows icp_batch_set_max_distance's rules -- count doubles, each > 0 or +INFINITY, thr = (F)(max_dist *
         max_dist) with the product formed in double and rounded once, a match kept iff d <= thr (a point on the threshold is
         kept); a NaN, a value <= 0 or -INFINITY is ICP_ERR_INVALID, the message names the pair, and nothing is launched.  NULL:
         every match is kept.  The batch's own gate, its trim shares and tau are neither read nor changed, and neither are its reciprocity
         flags: an evaluation scores forward matches at a distance, whatever icp_batch_set_reciprocal was told.
       evaluation vector: ICP_NMOM doubles per pair (slots ICP_EVAL_*, icp_mi355x_diag.h), every term formed in double from
         the widened coordinates of the kept matches, added per work item and then per pair in a fixed order, no
         floating-point atomics: a pair's bits depend on that pair and its threshold alone.  Both metrics: SD = sum |q[idx] -
         p|^2 (differences in double) and CNT.  ICP_POINT_TO_POINT: sum q and the upper triangle of sum q q^T, q the matched
         model point.  ICP_POINT_TO_PLANE: sum cn cn^T, cn = (p x n[idx], n[idx]), the statements and slots of a plane pass's
         C; it needs the batch's normals (ICP_ERR_INVALID without them).
       outputs, formed on the host in double from that vector and nothing else (every pointer may be NULL; per pair):
         status_out 1, inliers_out = (int)CNT, fitness_out = CNT / (double)n, rmse_out = sqrt(SD / CNT) or 0.0 where CNT = 0,
         info_out 36 doubles: the symmetric row-major 6 x 6 in the order (rx, ry, rz, tx, ty, tz) of icp_solve_point_to_plane's
         x, written in full.  Point-to-plane: C, mirrored.  Point-to-point: sum over the kept q = (x, y, z) of g1 g1^T + g2 g2^T
         + g3 g3^T with g1 = (0, z, -y, 1, 0, 0), g2 = (-z, 0, x, 0, 1, 0), g3 = (y, -x, 0, 0, 0, 1) -- I00 = Syy + Szz, I11 =
         Sxx + Szz, I22 = Sxx + Syy, I01 = -Sxy, I02 = -Sxz, I12 = -Syz, I04 = -Sz, I05 = Sy, I13 = Sz, I15 = -Sx, I23 = -Sy,
         I24 = Sx, I03 = I14 = I25 = 0, I33 = I44 = I55 = CNT, the rest of the lower-right block 0: each entry at most one
         addition of two slots.  idx_out (always in [0, m)) and mask_out (1 = the match was kept) are concatenated as the
         moving clouds.
       pair status: a pair whose start cloud icp_batch_begin refused (not finite after its initial transform) is not evaluated:
         status ICP_ERR_INVALID and zeros throughout.  Every other pair is evaluated and gets ICP_OK, ended pairs and pairs that
         failed with ICP_ERR_SINGULAR or ICP_ERR_EMPTY included.
       errors: ICP_ERR_STATE before icp_batch_begin, after any call that discards the loop and while the context has a pending
         pass; ICP_ERR_INVALID for a null batch or an unknown metric.
       the loop does not notice: the call neither discards nor advances it, and every later icp_batch_run, _state, _get_*,
         _loop_*, icp_diag_batch_moments and icp_diag_batch_trim answers with the bytes it would have given without the call.
       cost: three launches (the loop's deferred matching with nothing applied, the decision and the terms, the reduction) and
         one download of 32 doubles per pair, plus the indices when idx_out or mask_out is given.
 *   - voxel-grid downsampling (icp_batch_downsample): a new, thinner batch made on the device from the clouds a batch already
 *     holds -- same context, same count, same precision, every cloud reduced to one point per occupied cell of a voxel grid of
 *     its own.  The rule is deterministic and can be reproduced bit for bit in numpy (tests/batch_voxel_ref.py does).
 *       inputs: voxel_moving and voxel_model hold count doubles each.  A value that is finite and > 0 is the edge v of that
 *         cloud's grid; exactly 0.0 copies that cloud unchanged, its bytes and its order; a NULL array means every value is 0.0.
 *         A NaN, a negative or an infinite value: ICP_ERR_INVALID, the message names the first offending pair.  A null src or a
 *         null out: ICP_ERR_INVALID.  A context with a pending pass: ICP_ERR_STATE.  On any refusal *out is NULL and nothing of
 *         src changes.
 *       source: the clouds src holds as uploaded (or as made by an earlier icp_batch_downsample), P0 and Q -- never the moved
 *         cloud.  The options, the normals and the loop of src are not read.  The loop does not notice: the call neither
 *         discards nor advances it, and every later icp_batch_run, _state, _get_*, _loop_*, icp_diag_batch_moments and
 *         icp_diag_batch_trim of src answers with the bytes it would have given without the call.
 *       cell of a point: lo = the component-wise minimum of the cloud's points (comparisons only: exact in the batch's
 *         precision F).  For each axis c = floor(((double)x - (double)lo) / v): the subtraction, the division and the floor are
 *         each one IEEE operation in double, v is the caller's double as given, and nothing is multiplied by a reciprocal.
 *       range: every cell index must be <= 2097151 (21 bits per axis).  The largest index of an axis is
 *         floor(((double)hi - (double)lo) / v), hi the component-wise maximum (every step of the expression is monotonic); the
 *         call checks that value per cloud and axis.  A grid too fine for the cloud's extent: ICP_ERR_INVALID, the message names
 *         the pair and the side.  How the three indices are packed into a key is internal: only equality of cells is observable.
 *       output cloud: one point per occupied cell, the cells ordered by the lowest source index they contain (first occurrence).
 *         Output points therefore keep the order of the input, and a grid so fine that every point is alone returns the input
 *         cloud byte for byte, in its order.
 *       output point: a cell with one point outputs that point's bytes -- copied, not computed: a -0.0 survives.  A cell with
 *         c >= 2 points, per axis: s = 0.0; s += (double)x_i over the members in ascending source index; the output is
 *         (F)(s / (double)c), one division and one rounding to F.  Nothing is fused, nothing is reordered, and there are no
 *         floating-point atomics.
 *       maps: moving_map_out and model_map_out are optional (NULL: not wanted).  Each holds one int32 per source point,
 *         concatenated in src's layout: the index, within its pair's new cloud, of the output point that source point went into
 *         (for a copied cloud 0 .. n-1).  What a caller needs to carry colours or labels along.
 *       independence: a pair's output clouds and maps depend on that pair's cloud and its v alone -- not on the other pairs,
 *         their order or the batch size.
 *       new batch: *out is a complete batch, as if icp_batch_create had been called with the output clouds: its own offsets
 *         (icp_batch_get_offsets), the library's usual alignment and work items, no options, no normals
 *         (icp_batch_estimate_normals on it estimates from the thinned model and refuses a model left with fewer than 5 points,
 *         as it always does), no loop under way.  Every cloud keeps at least one point.  It is destroyed on its own, before the
 *         context; src may be destroyed first.  icp_batch_get_clouds downloads its clouds (or any batch's: P0 and Q).
 *       cost: four launches (bounds + range check + keys, one block per cloud; grouping and centroids, one wave per 64 points;
 *         ranks and maps, one block per cloud; compaction into the new batch's planes) and two host waits: one for the cell
 *         count of every cloud (2 x count int32, with the range flags), which the new batch's layout needs, one at the end (with
 *         the maps where they are asked for).  The grouping is brute force -- every point compares its key with its cloud's keys,
 *         n^2 / 64 tile steps per cloud -- and the longest chain is the sequential sum of the most populated cell.
 *   - statistical and radius outlier removal (icp_batch_remove_outliers): a new batch made on the device from the clouds a
 *     batch already holds -- same context, same count, same precision, every cloud without its isolated points.  Each cloud
 *     has a rule of its own (icp_outlier_rule).  The rules are deterministic and can be reproduced bit for bit in numpy
 *     (tests/batch_outlier_ref.py does).  Where the two overlap the call behaves as icp_batch_downsample.
 *       inputs: moving and model hold count rules each; a NULL array copies that side.  kind ICP_OUTLIER_NONE copies the
 *         cloud, its bytes and its order.  ICP_OUTLIER_STATISTICAL: neighbours = k, value = the ratio a.  ICP_OUTLIER_RADIUS:
 *         value = the radius r, neighbours = min, the least number of other points within r.
 *       source: the clouds src holds as uploaded (or as made by an earlier call), P0 and Q -- never the moved cloud.  The
 *         options, the normals and the loop of src are not read.  The loop does not notice: every later icp_batch_run, _state,
 *         _get_*, _loop_* and icp_diag_batch_* of src answers with the bytes it would have given without the call.
 *       distance: d2(i, j) is the matching's squared distance (dx*dx + dy*dy) + dz*dz, every operation rounded separately in
 *         the batch's precision F.  j runs over the other points of the same cloud, j != i by index: a coincident point
 *         counts, at distance 0.
 *       statistical rule: take the k smallest d2(i, .) as a multiset (ties cannot change a multiset); widen each to double and
 *         take a correctly rounded double sqrt; add them from the smallest to the largest, starting at 0.0; divide once by
 *         (double)k: this is dbar_i.  Per cloud every sum is formed in one order: a granule is 64 consecutive points from the
 *         cloud's first point; each granule is added from 0.0 in ascending index; the granule sums are added from 0.0 in
 *         ascending granule order.  S = the sum of dbar_i, mean = S / (double)n; dev_i = dbar_i - mean, q_i = dev_i * dev_i,
 *         Qsum = the sum of q_i; std = sqrt(Qsum / (double)(n - 1)), the sample deviation; thr = mean + a * std, one
 *         multiplication then one addition.  Keep iff dbar_i <= thr: a point on the threshold is kept, so a lattice with
 *         std == 0 keeps everything.  Nothing is fused, nothing is multiplied by a reciprocal, and there are no floating-point
 *         atomics.
 *       radius rule: thr2 = (F)(r * r), the product formed in double and rounded once (the gate's rule);
 *         c_i = #{ j != i : d2(i, j) <= thr2 }; keep iff c_i >= min.
 *       output cloud: the kept points, copied, not computed, in the source order: a -0.0 survives.
 *       outputs, all optional (NULL: not wanted): the maps hold one int32 per source point in src's layout -- the index of a
 *         kept point within its new cloud, -1 for a removed point, 0 .. n-1 for a copied cloud.  The scores hold one double per
 *         source point: dbar_i, or (double)c_i for the radius rule, for kept and removed points alike; 0.0 for a copied cloud.
 *         stats_out holds four doubles per cloud, [mean, std, thr, kept], the moving clouds first (2 * count x 4): a radius
 *         cloud has [0, 0, (double)thr2, kept], a copied cloud [0, 0, 0, n].
 *       refusals: on any refusal *out is NULL, nothing of src changes and no output array is written; where a pair is at fault
 *         the message names the first offending pair and the side.  ICP_ERR_INVALID: a null src or a null out; an unknown kind;
 *         a statistical k outside [1, ICP_OUTLIER_MAX_NEIGHBOURS] or a cloud of n < k + 1 points; a ratio that is negative, NaN
 *         or infinite; a radius that is not finite or not > 0; a radius min outside [1, 65535]; a cloud whose mean or std comes
 *         out not finite.  ICP_ERR_STATE: a pass pending on the context.  ICP_ERR_EMPTY: a cloud would keep no point (known at
 *         the first host wait, before the new batch exists).
 *       independence: a pair's outputs depend on that pair's cloud and its rule alone -- not on the other pairs, their order
 *         or the batch size.
 *       new batch: *out is a complete batch, as if icp_batch_create had been called with the output clouds: no options, no
 *         normals, no loop under way; it can go straight into icp_batch_downsample, icp_batch_estimate_normals or
 *         icp_batch_begin, and it is destroyed on its own.
 *       cost: three launches (the neighbour scan, one block per 64 points; the statistic, the decision and the maps, one
 *         block per cloud; compaction into the new batch's planes) and two host waits: one for the kept count of every cloud,
 *         which the new batch's layout needs, one at the end with the optional outputs.  The scan is brute force, n^2 distances
 *         per cloud.
 *   - the generalized metric (ICP_GENERALIZED, plane-to-plane; Segal et al., RSS 2009, in the fast_gicp formulation): every kept
 *     match (p_i, q_j) pulls with the inverse of S = Cq_j + Rc Cp_i Rc^T, the local shape of BOTH clouds at the match.  The batch
 *     holds one covariance per point of either side, given (icp_batch_set_covariances) or estimated on the device from a
 *     neighbourhood of the caller's size (icp_batch_estimate_covariances); icp_batch_get_covariances reads them back.
 *       storage: a covariance is 6 doubles per point, xx, xy, xz, yy, yz, zz -- always double, whatever the batch's precision --
 *         concatenated in the layout of the clouds (moving_off, model_off).  The moving covariances belong to the cloud as
 *         uploaded, in its own frame: the loop rotates them, the caller never does.
 *       both calls follow icp_batch_set_model_normals / icp_batch_estimate_normals: any time after icp_batch_create; they replace
 *         that side's set; a loop under way is discarded; a refused call leaves the batch as it was.  A pending pass on the
 *         context: ICP_ERR_STATE.  A null batch: ICP_ERR_INVALID.  A NULL array on one side leaves that side untouched; both NULL
 *         is ICP_ERR_INVALID.
 *       icp_batch_set_covariances checks finiteness only: a NaN or an infinite value is ICP_ERR_INVALID and the message names the
 *         pair and the side.  That every matrix is symmetric positive semi-definite is the caller's duty.
 *       icp_batch_estimate_covariances: k_moving and k_model hold count ints each, every k within [ICP_COV_MIN_NEIGHBOURS,
 *         ICP_COV_MAX_NEIGHBOURS]; a cloud of fewer than k + 1 points is ICP_ERR_INVALID (the message names the pair and the
 *         side), and so is an unknown regularisation.  With ICP_COV_FROBENIUS lambda must be finite and > 0; with ICP_COV_NONE
 *         it is not read.  The outputs are optional.  The rule for point i of a cloud, reproducible bit for bit in numpy
 *         (tests/batch_gicp_ref.py does):
 *           d2(i, j) is the matching's squared distance (dx*dx + dy*dy) + dz*dz in the batch's precision F.
 *           tau_i is the k-th smallest d2(i, j) over j != i by index -- the statistical outlier rule's multiset: a coincident
 *             point counts, at 0.
 *           the neighbourhood is every j of the cloud with d2(i, j) <= tau_i, i itself included: all ties with the k-th are in,
 *             the count c >= k + 1, and the set depends on no ordering of equal values.
 *           sums, in double, from 0.0, over the neighbourhood in ascending j: e = ((double)x_j - (double)x_i, ...) -- differences
 *             against the query, so a cloud far from the origin loses nothing; s_a += e_a; S_ab += e_a * e_b for the six a <= b.
 *           C_ab = (S_ab - (s_a * s_b) / (double)c) / (double)c: each operation rounded on its own, nothing fused.
 *           ICP_COV_FROBENIUS: f = sqrt(((xx*xx + yy*yy) + zz*zz) + 2.0 * ((xy*xy + xz*xz) + yz*yz)); f > 0: C'_ab = C_ab / f,
 *             plus lambda on the diagonal; f == 0: C' = lambda I exactly.  ICP_COV_NONE: the raw covariance.  f and the quotients
 *             are formed on the matrix icp_eigh3's range rule leaves (below): with amax the largest magnitude of the six entries,
 *             all finite, amax > 2^400 multiplies the six by 2^-600 first and 0 < amax < 2^-400 by 2^+600 -- no square leaves
 *             the double range, the quotients are scale-free, and f == 0 is left to the zero matrix alone.  Within 2^+-400
 *             nothing is multiplied.
 *           a cloud's result depends on that cloud, its k and the two parameters alone.
 *         cost: one launch for all clouds of the sides asked for (one block per 64 points: the k-th distance in a register list,
 *           then the sums in one pass over the cloud), no atomics, and one host wait only when an output array is wanted.
 *       icp_batch_begin with ICP_GENERALIZED needs covariances on both sides (ICP_ERR_INVALID without), and a batch that holds
 *         robust kernels refuses this metric with ICP_ERR_INVALID: weights on a Mahalanobis residual are a later change.
 *         icp_batch_evaluate, the single-pair loops (icp_loop_begin, icp_point_to_*) and the one-call icp_point_to_*_batch
 *         refuse the value as any unknown metric; icp_host_loop_create accepts it and solves as for point-to-plane.
 *       a step always runs deferred: the point-to-point matching launch, [the reverse search,] [the trim's selection,]
 *         batch_gicp_moments, the reduction up to ICP_MOM_B + 5 -- three launches, up to five, one download.  The kept decision is
 *         the one of every deferred batch: gate, tau over all n distances, the mutual rule.  Front end, ICP_MOM_ERR (Euclidean,
 *         over the points the previous matching pass kept), the err series, the stop rule, idx, masks, initial transforms and
 *         the ICP_ERR_EMPTY / ICP_ERR_SINGULAR handling are those of the other metrics.
 *       terms of a kept match of moving point i to model point j, every one in double from the widened coordinates p (the moved
 *         point) and q:  Rc = the rotation part of the product of every motion applied to the cloud this pass matched on, the
 *         initial transform as rounded to the batch's precision included, composed on the host in double as icp_batch_state
 *         composes T (icp_diag_batch_rotation reads it).  Tm = Rc Cp_i, the full 3 x 3, each entry (r0*c0 + r1*c1) + r2*c2;
 *         B_ab = (Tm_a0*Rc_b0 + Tm_a1*Rc_b1) + Tm_a2*Rc_b2 for a <= b; S = Cq_j + B.  Cofactors c00 = S11*S22 - S12*S12,
 *         c01 = S02*S12 - S01*S22, c02 = S01*S12 - S02*S11, c11 = S00*S22 - S02*S02, c12 = S01*S02 - S00*S12, c22 = S00*S11 -
 *         S01*S01; det = (S00*c00 + S01*c01) + S02*c02; M_ab = c_ab / det.  A match whose det is not finite or not > 0 is
 *         rejected: it counts as not kept in mask, count and sums, like a gate rejection.  e = p - q; J columns j0 = (0, -pz,
 *         py), j1 = (pz, 0, -px), j2 = (-py, px, 0), j3, j4, j5 the unit vectors; u_a = M j_a.  Slot C(a, c) += j_a . u_c for
 *         a <= c; slot B(a) -= u_a . e; ICP_MOM_CNT = 1.  Every dot product is (x*x' + y*y') + z*z'.  With M = n n^T these are
 *         the plane pass's statements.  A pair's bits depend on that pair and its options alone.
 *   - global registration (icp_batch_compute_features, icp_batch_match_features, icp_batch_score_transforms, icp_batch_ransac):
 *     a start pose for pairs in unknown relative pose -- describe every point, match the descriptors, RANSAC over the matches; the
 *     pose that comes out goes straight into icp_batch_set_initial_transforms.  One launch per stage for every pair of the batch;
 *     every rule below is restated in numpy, bit for bit (tests/batch_feature_ref.py); a pair's bits depend on that pair alone.
 *       descriptors (icp_batch_compute_features): a 33-bin FPFH (Rusu et al., ICRA 2009) per point, both clouds of every pair.
 *         k_moving and k_model hold count ints each, every k within [ICP_COV_MIN_NEIGHBOURS, ICP_COV_MAX_NEIGHBOURS]; a cloud of
 *         fewer than k + 1 points is ICP_ERR_INVALID, the message names the pair and the side.  moving_normals and model_normals
 *         hold three doubles per point, laid out as the clouds -- always double, whatever the batch's precision; both sides are
 *         required; a NaN or an infinite value is ICP_ERR_INVALID.  Unit length and a consistent orientation of the normals are
 *         the caller's duty.  The batch does not keep the normals.  A descriptor is ICP_FEATURE_BINS doubles per point; the
 *         outputs are optional, the batch keeps the descriptors on the device and icp_batch_get_features reads them back
 *         (ICP_ERR_STATE where a side that is asked for holds none).  Source: the clouds as uploaded or as made by
 *         icp_batch_downsample / icp_batch_remove_outliers, P0 and Q -- never the moved cloud.  The loop does not notice: the call
 *         neither discards nor advances it.  A pending pass on the context: ICP_ERR_STATE.  A null batch: ICP_ERR_INVALID.  A
 *         refused call leaves the batch as it was.  New descriptors discard the matches of icp_batch_match_features.
 *         Every operation below is one IEEE double operation, nothing is fused, and the only functions used are
 *         + - * / sqrt fabs floor.
 *           neighbourhood: the covariance rule's.  d2(i, j) is the matching's squared distance in the batch's precision F; tau_i is
 *             the k-th smallest over j != i by index; the neighbourhood of i is every j != i with d2(i, j) <= tau_i: all ties are in.
 *           pair term of (i, j), from the widened coordinates: d = p_j - p_i, r2 = (dx*dx + dy*dy) + dz*dz; the pair is skipped if
 *             r2 == 0 or r2 is not finite.  r = sqrt(r2); a1 = dot(n_i, d) / r; a2 = dot(n_j, d) / r.  If fabs(a1) < fabs(a2) the
 *             roles swap: n1 = n_j, n2 = n_i, d = -d, f3 = -a2; otherwise n1 = n_i, n2 = n_j, f3 = a1.  v = d x n1, each component
 *             a*b - c*d; vv = dot(v, v); the pair is skipped if vv == 0 or vv is not finite.  v = v / sqrt(vv), three divisions.
 *             w = n1 x v; f2 = dot(v, n2); x = dot(n1, n2); y = dot(w, n2).  Every dot is (x*x' + y*y') + z*z'.
 *           the third angle is binned in the diamond angle, not in atan2 -- a deliberate deviation from PCL: s = fabs(x) + fabs(y);
 *             if s == 0 then t = 0, otherwise q = y / s and t = q if x >= 0, t = 2 - q if y >= 0, else t = -2 - q.  t is monotone
 *             in atan2(y, x) and lies in [-2, 2]; it needs no transcendental, so no bin decision hangs on a libm.
 *           bin(val, lo, width) = clamp((int)floor((11.0 * (val - lo)) / width), 0, 10), the clamp taken before the conversion (a
 *             NaN lands in bin 0).  t uses (-2, 4) into bins 0-10, f2 uses (-1, 2) into bins 11-21, f3 uses (-1, 2) into bins 22-32.
 *           SPFH: the bins are integer counts, so no summation order exists; c is the number of pair terms not skipped;
 *             S_i[b] = (100.0 * (double)cnt_b) / (double)c, or all zeros where c == 0.
 *           FPFH: A[b] = 0.0; for the neighbourhood of i in ascending j, skipping d2(i, j) == 0: wgt = 1.0 / (double)d2(i, j);
 *             A[b] += S_j[b] * wgt.  Per sub-histogram of 11 bins: s is the sequential sum from 0.0 in ascending b;
 *             F_i[b] = (A[b] * 100.0) / s, or 0.0 where s is not > 0 or not finite.
 *           a cloud's descriptors depend on that cloud, its k and its normals alone.
 *         cost: two launches for all clouds of both sides (batch_spfh_kernel, batch_fpfh_kernel: one block per 64 points), no
 *           atomics, one host wait.
 *       point normals (icp_batch_estimate_point_normals, icp_batch_set_point_normals, icp_batch_get_point_normals,
 *         icp_batch_compute_features_stored): the normals the descriptors are computed from, made on the device from the
 *         covariances the batch holds and kept there -- what Open3D's estimate_normals + orient_normals_towards_camera_location
 *         give.  Three planes of doubles per side, laid out as the clouds; always double, whatever the batch's precision; separate
 *         from the model normals of point-to-plane (icp_batch_set_model_normals), which are not touched.
 *           icp_batch_estimate_point_normals computes both sides, always.  It needs covariances on both sides, given or estimated,
 *             with any regularisation (ICP_ERR_STATE otherwise; the message names the side).  orient: ICP_ORIENT_NONE,
 *             ICP_ORIENT_VIEWPOINT or ICP_ORIENT_CENTROID; an unknown value is ICP_ERR_INVALID.  With ICP_ORIENT_VIEWPOINT
 *             moving_viewpoints and model_viewpoints are both required: 3 doubles per pair, each in that cloud's own frame; a NULL
 *             array, a NaN or an infinite value is ICP_ERR_INVALID and the message names the pair and the side.  In the other
 *             modes the arrays are not read.  The outputs are optional: 3 doubles per point, laid out as the clouds, as
 *             icp_batch_compute_features takes them; there is a host wait only when one is given.  A pending pass on the
 *             context: ICP_ERR_STATE.  A null batch: ICP_ERR_INVALID.  A refused call leaves the previous normals and everything
 *             else as they were.  The loop does not notice: the call neither discards nor advances it.  The normals are a
 *             snapshot: later covariance calls leave them in place.  The batches icp_batch_downsample, icp_batch_remove_outliers
 *             and icp_batch_select_keypoints make hold none.
 *           the rule for point i of a cloud, reproducible bit for bit in numpy (tests/batch_normals_ref.py does).  Every operation
 *             is one IEEE double operation, nothing is fused, and the only functions used are + - * / sqrt fabs copysign.
 *               eigenvector: icp_eigh3's statements (below) on the symmetric matrix built from the stored xx, xy, xz, yy, yz, zz,
 *                 the updates of v included -- cyclic Jacobi over (0,1), (0,2), (1,2) from v = I; at most 64 sweeps; the stop test
 *                 off <= 1e-34 * dia || off == 0.0; the same theta, t, c, s; the same three compare-and-swaps of the order with the
 *                 strict <.  n is column ord[0] of v, not renormalised.  A zero matrix gives (1, 0, 0); equal smallest
 *                 eigenvalues give whatever these statements give.  icp_eigh3's range rule comes first: a matrix of six finite
 *                 entries whose largest magnitude lies beyond 2^+-400 is solved times 2^-+600 -- the same rotations, so n does
 *                 not depend on a power of two in C.
 *               non-finite rule: if any component of n is not finite, n is exactly (0.0, 0.0, 0.0) -- the kept normals are always
 *                 finite, which is what icp_batch_compute_features demands of the caller's.
 *               orientation: to_a = v_a - (double)x_a for the cloud's viewpoint v; dt = (n_x*to_x + n_y*to_y) + n_z*to_z; n is
 *                 negated iff dt < 0: dt == 0 and a NaN keep it.  With ICP_ORIENT_NONE nothing is negated.
 *               centroid (ICP_ORIENT_CENTROID: v is the cloud's own centroid, which no rigid motion changes), per cloud and axis:
 *                 s_t = 0.0 and s_t += (double)x_j for j = t, t + 256, ... below n, for t = 0 .. 255; total = 0.0 and
 *                 total += s_t for t ascending; v = total / (double)n.
 *             A cloud's normals depend on that cloud, its covariances and its viewpoint alone.
 *           icp_batch_set_point_normals and icp_batch_get_point_normals follow icp_batch_set_covariances and
 *             icp_batch_get_covariances: a NULL side is left untouched, both NULL is ICP_ERR_INVALID; the setter checks finiteness
 *             only (ICP_ERR_INVALID, the message names the pair and the side); get on a side without normals is ICP_ERR_STATE.
 *             Neither touches the loop.
 *           icp_batch_compute_features_stored is icp_batch_compute_features with the kept normals in place of the host arrays:
 *             the same two launches and the one wait, no upload of normals; a side without normals is ICP_ERR_STATE.
 *           cost: one launch for all clouds of both sides (batch_point_normals_kernel: one wave per 64 points, one point per
 *             lane), two with ICP_ORIENT_CENTROID (batch_centroid_kernel first: one block of 256 per cloud, 6 KiB of LDS); no
 *             atomics; a host wait only when an output is wanted.
 *       matching (icp_batch_match_features): D(i, j) = the sum of (F_i[b] - G_j[b])^2 from 0.0 over b = 0..32 in ascending b, in
 *         double, each operation rounded on its own; F the moving cloud's descriptors, G the model's.  fwd[i] is the lowest j that
 *         minimises D, rev[j] the lowest i (a NaN never wins; where no D is below +INFINITY the answer is 0).
 *         kept[i] = !mutual || rev[fwd[i]] == i.  The batch keeps fwd, rev and kept on the device; a pair's correspondence list
 *         is its kept i in ascending order, paired with fwd[i]; C_p is its length.  fwd_out and kept_out are concatenated as the
 *         moving clouds, rev_out as the models; each may be NULL.  It needs descriptors on both sides (ICP_ERR_STATE otherwise).
 *         Two launches of batch_feature_match (the sides swapped), n x m x 33 differences per pair, and one host wait.  The loop
 *         does not notice.
 *       scoring (icp_batch_score_transforms): per_pair in [1, 65536] candidate 4 x 4 matrices per pair (count x per_pair x 16 doubles,
 *         row-major, bottom row 0 0 0 1, validated as icp_batch_set_initial_transforms validates).  Each is rounded once to F and
 *         applied to P0 in the front end's arithmetic, ((r0 x + r1 y) + r2 z) + t, every operation rounded separately in F;
 *         d = the matching's squared distance in F against Q[fwd[i]]; a correspondence counts iff d <= thr, thr = (F)(max_dist *
 *         max_dist) by the gate's rule (max_dist: count doubles, each > 0 or +INFINITY; NULL: +INFINITY for every pair); a moved
 *         point that is not finite is a miss.  count_out holds count x per_pair int32; integers have no summation order, so the
 *         result is exact.  ICP_ERR_STATE without matches.  One launch of batch_score_transforms, one host wait.  The loop does
 *         not notice.
 *       RANSAC (icp_batch_ransac): hypotheses in [1, 65536]; max_distance finite and > 0; edge_similarity e in [0, 1), 0 switches
 *         the edge check off; one seed per pair: a pair's result depends on that pair, its seed and the parameters alone.
 *           draws: mix(x) is the splitmix64 finaliser on z = x + 0x9E3779B97F4A7C15: z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9,
 *             z = (z ^ (z >> 27)) * 0x94D049BB133111EB, mix = z ^ (z >> 31), all modulo 2^64.
 *             draw(h, r) = mix(mix(mix(seed_p) + h) + r) % C_p; the modulo bias is accepted.
 *           hypothesis h: slots 0, 1 and 2 take the draws r = 0, 1, 2, ...; a draw equal to an earlier slot is skipped; at most 16
 *             draws are used; fewer than three distinct picks make the hypothesis invalid.  A pick is a position in the
 *             correspondence list.
 *           edge check: for the three point pairs (0, 1), (1, 2) and (0, 2), la and lb are sqrt of the double squared distance
 *             (dx*dx + dy*dy) + dz*dz between the widened moving points, and between the model points; the hypothesis is valid
 *             iff la >= e*lb && lb >= e*la for all three.
 *           solve: the 32-double moment vector of the three matches, added in slot order, goes through icp_solve_rigid (below).
 *           score: every valid hypothesis through batch_score_transforms, a fixed number of hypotheses per launch.  Winner: the largest
 *             count, the lowest h among equals.  Refit: the moments over the winner's inliers in ascending list order,
 *             icp_solve_rigid, one more scoring launch; the refit is returned if its count is at least the winner's, else the winner.
 *           per pair: status ICP_ERR_EMPTY where C_p < 3 or no hypothesis is valid -- then T is the identity and inliers is 0 --
 *             otherwise ICP_OK.  T16_out (16 doubles per pair) maps P0 into the model's frame; inliers_out and
 *             correspondences_out (C_p) hold one int32 per pair, status_out one int; every output may be NULL.
 *         ICP_ERR_STATE without matches; ICP_ERR_INVALID for a null batch, null parameters, null seeds or a value out of range.
 *         The loop does not notice.
 *       Fast Global Registration (icp_batch_fgr; Zhou, Park, Koltun, ECCV 2016; Open3D's
 *         registration_fgr_based_on_feature_matching): no hypotheses -- one robust objective (Geman-McClure, by graduated
 *         non-convexity) over the correspondence list, minimised by `iterations` weighted Gauss-Newton steps.  iterations in
 *         [1, 1024]; max_distance (delta) finite and > 0; division_factor finite and > 1; decrease_every >= 1; tuples in [0, 65536];
 *         tuple_similarity in [0, 1), read only where tuples > 0; one seed per pair, read only where tuples > 0 (seed may be NULL
 *         iff tuples == 0).  With tuples == 0 the call is deterministic without a seed.  Everything is in double, from coordinates
 *         widened once; every operation is one IEEE double operation, nothing is fused; the only functions used are + - * /.
 *           used list: tuples == 0: every correspondence, in list order.  tuples > 0: hypotheses h = 0 .. tuples-1 by RANSAC's own
 *             draw, triple and edge check with e = tuple_similarity (a hypothesis is valid iff it has three distinct picks and
 *             passes the edge check; nothing is solved); a list position is used iff it occurs in a valid triple, each position is
 *             used once, however often it occurs -- a deliberate deviation from Open3D, which repeats them -- and the order is
 *             ascending list position.  U_p is the length of the used list.  U_p < 3: status ICP_ERR_EMPTY, T the identity, every
 *             weight 0, objective 0.
 *           scale: pbar and qbar are the sequential sums of the used moving and model points, in list order, divided by U_p; D2 is
 *             the largest of (dx*dx + dy*dy) + dz*dz over the used points of both sides, each against its own mean; mu = D2.
 *             D2 == 0 or not finite: ICP_ERR_EMPTY, as above.
 *           iteration it = 0 .. iterations-1, from T = the identity: if it % decrease_every == 0 and mu > delta*delta then
 *             mu = max(mu / division_factor, delta*delta) -- mu is never lowered below delta^2.  Per used correspondence (p0, q):
 *             p_a = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]; e_a = p_a - q_a; r2 = (ex*ex + ey*ey) + ez*ez;
 *             s = mu / (mu + r2); l = s*s (s stands for sqrt(l): no sqrt is needed).  The three residual rows are
 *             cn_x = (0, pz, -py, 1, 0, 0), cn_y = (-pz, 0, px, 0, 1, 0), cn_z = (py, -px, 0, 0, 0, 1); w_a[r] = l * cn_a[r].
 *             The sums go into a plane pass's slots: C(r, c) += (w_x[r]*cn_x[c] + w_y[r]*cn_y[c]) + w_z[r]*cn_z[c] for r <= c;
 *             B(r) -= (w_x[r]*ex + w_y[r]*ey) + w_z[r]*ez; ICP_MOM_CNT += 1; ICP_MOM_W += l;
 *             ICP_MOM_ERR += l*r2 + mu*((1 - s)*(1 - s)); the slots behind ICP_MOM_W are 0.  A correspondence whose p or r2 is not
 *             finite adds nothing and counts 0 (its weight is reported as 0.0).
 *           solve: the vector goes through icp_solve_point_to_plane (below): R = Rz Ry Rx, unknowns (rx, ry, rz, tx, ty, tz);
 *             T = S T with S = [R t; 0 1], every entry (s0 a + s1 b) + s2 c, the translation + t.  A system that is not positive
 *             definite, or a product that is not finite, ends that pair with ICP_ERR_SINGULAR at the pose reached so far; the
 *             other pairs go on.
 *           results: T16_out maps P0 into the model's frame and goes straight into icp_batch_set_initial_transforms, as RANSAC's
 *             pose does.  objective_out is ICP_MOM_ERR of the pair's last iteration.  A last weights-only launch at the final T
 *             and the last mu gives weights_out, laid out as the moving clouds: a used point gets its l, every other point 0.0.
 *             used_out is U_p.  Every output pointer may be NULL.
 *           sums: per work item of 64 list entries, then per pair, in a fixed order; no floating-point atomics.  A pair's bits
 *             depend on that pair, its seed and the parameters alone -- not on its neighbours or its position in the batch.
 *           cost: per iteration one upload of 14 doubles per pair (T, mu, a flag), two launches (batch_fgr_terms, one block per 64
 *             list entries; batch_fgr_finalize, one block per pair), one download, one host wait and the host's 6 x 6 solve.
 *         ICP_ERR_STATE without matches or with a pending pass on the context; ICP_ERR_INVALID for a null batch, null parameters,
 *         null seeds with tuples > 0 or a value out of range; a refused call leaves the batch as it was.  The loop does not notice:
 *         the call reads P0 and Q, never the moved cloud, and neither discards nor advances a registration under way.
 *       keypoints (icp_batch_select_keypoints): the descriptor scan of icp_batch_match_features grows with the product of both cloud
 *         sizes; the answer (Open3D's, too) is to describe the whole cloud but to match only its salient points, chosen by ISS
 *         (Intrinsic Shape Signatures; Zhong, ICCV Workshops 2009; Open3D's compute_iss_keypoints).  The call makes a new batch
 *         on the device from the clouds a batch already holds -- same context, same count, same precision, every cloud reduced
 *         to its keypoints -- and carries the descriptors of the kept points along.  Each cloud has a rule of its own
 *         (icp_keypoint_rule).  Where the two overlap the call behaves as icp_batch_remove_outliers.
 *           inputs: moving and model hold count rules each; a NULL array copies that side; kind ICP_KEYPOINT_NONE copies the
 *             cloud, its bytes and its order.  ICP_KEYPOINT_ISS reads salient_radius, non_max_radius, gamma_21, gamma_32 and
 *             min_neighbours.
 *           source: P0 and Q, the clouds as uploaded or as made by an earlier call -- never the moved cloud.  The options, the
 *             normals and the loop of src are not read.  The loop does not notice.
 *           the rule for point i of a cloud, reproducible bit for bit in numpy (tests/batch_keypoint_ref.py does).  Every operation
 *             is one IEEE operation, nothing is fused, nothing is multiplied by a reciprocal, and the only functions used are
 *             + - * / sqrt fabs copysign.
 *               distance: d2(i, j) is the matching's squared distance (dx*dx + dy*dy) + dz*dz in the batch's precision F;
 *                 ts = (F)(salient_radius * salient_radius) and tn = (F)(non_max_radius * non_max_radius), each product formed in
 *                 double and rounded once (the gate's rule).
 *               salient neighbourhood: every j of the cloud with d2(i, j) <= ts, i itself included at distance 0; c is its size.
 *                 A point exactly on the radius is in.
 *               sums: the covariance rule's statements -- in double, from 0.0, over the neighbourhood in ascending j:
 *                 e = (double)x_j - (double)x_i, s_a += e_a, S_ab += e_a * e_b for the six a <= b;
 *                 C_ab = (S_ab - (s_a * s_b) / (double)c) / (double)c.
 *               eigenvalues: icp_eigh3's statements (below) on the symmetric matrix built from C -- cyclic Jacobi over (0,1),
 *                 (0,2), (1,2); at most 64 sweeps; the stop test off <= 1e-34 * dia || off == 0.0; the same theta, t, c, s and
 *                 update statements; the same ascending order w0 <= w1 <= w2.  The eigenvectors are not formed: the eigenvalues do
 *                 not depend on them.  icp_eigh3's range rule comes first, and w0, w1, w2 are the scaled-back eigenvalues: a
 *                 matrix of six finite entries whose largest magnitude lies beyond 2^+-400 is solved times 2^-+600, and each
 *                 eigenvalue is multiplied by 2^+-600 once the order is fixed -- the saliency of a cloud times 2^e is 2^(2e)
 *                 times the cloud's own.
 *               saliency: sal_i = w0 iff c >= min_neighbours && (w1 / w2) < gamma_21 && (w0 / w1) < gamma_32 && w0 > 0, else
 *                 sal_i is exactly 0.0.  A NaN fails every comparison.  The divisions are Open3D's.
 *               selection: M_i is every j with d2(i, j) <= tn, i included.  i is a keypoint iff sal_i > 0 &&
 *                 |M_i| >= min_neighbours && sal_j <= sal_i for every j in M_i.  Equal saliencies keep each other, as Open3D's
 *                 IsLocalMaxima does: coincident points are kept or dropped together.
 *           output cloud: the keypoints, copied, not computed, in the source order: a -0.0 survives.
 *           outputs, all optional (NULL: not wanted): the maps hold one int32 per source point in src's layout -- the index of a
 *             kept point within its new cloud, -1 for a dropped point, 0 .. n-1 for a copied cloud.  The saliencies hold one
 *             double per source point, sal_i for kept and dropped points alike; 0.0 for a copied cloud.  count_out holds the
 *             kept points of every cloud, the moving clouds first (2 * count int32).
 *           refusals: on any refusal *out is NULL, nothing of src changes and no output array is written; where a pair is at
 *             fault the message names the first offending pair and the side.  ICP_ERR_INVALID: a null src or a null out; an
 *             unknown kind; min_neighbours outside [1, 65535]; a radius that is not finite or not > 0; a gamma that is not
 *             finite or not > 0.  ICP_ERR_STATE: a pass pending on the context.  ICP_ERR_EMPTY: a cloud would keep no point
 *             (known at the first host wait, before the new batch exists).
 *           independence: a cloud's outputs depend on that cloud and its rule alone -- not on the other pairs, their order or
 *             the batch size.
 *           new batch: *out is a complete batch, as if icp_batch_create had been called with the output clouds: no options, no
 *             normals, no loop under way, no matches.  Descriptors: where src holds descriptors on a side
 *             (icp_batch_compute_features), the new batch holds the descriptors of the kept points of that side, copied on the
 *             device byte for byte, in the kept order; icp_batch_match_features, icp_batch_ransac, icp_batch_fgr and
 *             icp_batch_get_features work on it unchanged.  A side of src without descriptors gives a side without.
 *           cost: four launches (batch_iss_saliency and batch_iss_select, one block per 64 points: the sums in one pass over the
 *             cloud by one wave, then the neighbourhood count and the comparison by four; batch_keypoint_rank, one block per
 *             cloud: maps and counts; batch_keypoint_compact: coordinates and descriptors into the new batch) and two host waits:
 *             one for the kept count of every cloud, which the new batch's layout needs, one at the end with the optional
 *             outputs.  Both scans are brute force, n^2 distances per cloud.  LDS per block: 24 KiB (saliency), 42 KiB in fp32
 *             and 34 KiB in fp64 (selection), 16 bytes (rank), none (compaction).  No atomics.
 *   - plane segmentation (icp_batch_segment_plane; Open3D's segment_plane, PCL's SACSegmentation): a floor or a wall holds a large
 *     share of a scan's points, fixes only three of the six unknowns and gives descriptors that are all alike.  The call finds the
 *     dominant plane of every cloud by RANSAC -- points x hypotheses plane tests per cloud, counted on the device -- and makes a new
 *     batch without it, or of it alone.  Each cloud has a rule of its own (icp_plane_rule).  Where the two overlap the call behaves
 *     as icp_batch_remove_outliers.  The rule is restated in numpy, bit for bit (tests/batch_segment_ref.py).
 *       inputs: moving and model hold count rules each; a NULL array copies that side; kind ICP_PLANE_NONE copies the cloud, its
 *         bytes and its order, and nothing is searched (its status is ICP_OK, its plane four zeros).  The other kinds read
 *         hypotheses, distance, axis and min_cos.  seed holds one word per pair.
 *       source: P0 and Q, the clouds as uploaded or as made by an earlier call -- never the moved cloud.  The options, the normals
 *         and the loop of src are not read.  The loop does not notice.
 *       the rule for a cloud of n points whose kind is not ICP_PLANE_NONE.  Everything is in IEEE double on coordinates widened
 *         once; every operation is rounded on its own, nothing is fused, nothing is multiplied by a reciprocal, and the only
 *         functions used are + - * / sqrt fabs.
 *           draws: icp_batch_ransac's generator, unchanged: draw(h, r) = mix(mix(mix(seed_p + side) + h) + r) % n, side 0 for the
 *             moving cloud and 1 for the model, sums modulo 2^64.  Slots 0, 1, 2 take the draws r = 0, 1, ...; a draw equal to an
 *             earlier slot is skipped; at most 16 draws are used; fewer than three distinct indices make the hypothesis invalid.
 *           plane of three points a, b, c (icp_plane_from_points): u = b - a, v = c - a;
 *             w = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx); l = sqrt((wx*wx + wy*wy) + wz*wz).  The hypothesis is invalid unless
 *             l > 0 and l is finite: coincident and collinear picks end here, and so do the zero returns of a lidar -- a triple
 *             out of the heap at the origin is invalid, while a plane through the origin still counts every point of the heap;
 *             dropping zero returns is the caller's job.  n = w / l, three divisions.  sign rule: all three components are
 *             negated iff the component of largest magnitude is negative; the lowest index decides among equal magnitudes.
 *             d = -((nx*ax + ny*ay) + nz*az).
 *           range: the products of w are squares of the cloud's extent and l squares them again: l leaves the double range
 *             (overflows to +INFINITY) once the triangle's edges pass about 2^255, and is exactly 0 once they fall below about
 *             2^-269.  Such hypotheses are invalid, not wrong.  (Between 2^-269 and 2^-255 the squares are subnormal and n is
 *             what these statements give.)
 *           axis constraint: axis == (0, 0, 0) means none.  Otherwise ahat = axis / sqrt((ax*ax + ay*ay) + az*az), three divisions,
 *             and the hypothesis is valid iff fabs((nx*ahx + ny*ahy) + nz*ahz) >= min_cos (PCL's perpendicular-plane model without
 *             its trigonometry: what lets a caller ask for the floor and not the larger wall).
 *           score: s_i = ((nx*x + ny*y) + nz*z) + d; point i is an inlier iff fabs(s_i) <= distance.  A point on the threshold is
 *             in, a NaN is out.  Counts are integers: exact whatever order the device adds them in.
 *           winner: the largest count, the lowest h among equals.  With no valid hypothesis the cloud's status is ICP_ERR_EMPTY, its
 *             plane four zeros, its count 0, its mask all 0; under ICP_PLANE_DETECT and ICP_PLANE_REMOVE such a cloud is copied.
 *           refit over the winner's k >= 3 inliers (k < 3: no refit): S = the sum of the inlier coordinates in the outlier call's
 *             order -- granules of 64 consecutive points from the cloud's first point, each granule added from 0.0 in ascending
 *             index, the granule sums added from 0.0 in ascending order; c = S / (double)k; the six sums of ex*ex, ex*ey, ex*ez,
 *             ey*ey, ey*ez, ez*ez with e = x - c in the same order, each divided once by (double)k.  icp_plane_from_moments:
 *             icp_eigh3's eigenvector of the smallest eigenvalue (column 0 of Z, as icp_batch_estimate_point_normals chooses it,
 *             not renormalised); the refit is dropped if that vector is zero or not finite; the sign rule;
 *             d = -((nx*cx + ny*cy) + nz*cz); the axis test again -- a refit that fails it is dropped.  The refit is scored once
 *             more, and the call returns the refit if its count is at least the winner's, else the winner (icp_batch_ransac's
 *             rule).  The mask is the returned plane's.
 *       outputs, all optional (NULL: not wanted): planes_out 4 doubles per cloud (nx, ny, nz, d), inliers_out and status_out
 *         (ICP_OK or ICP_ERR_EMPTY) one per cloud -- 2 * count clouds, the moving clouds first.  The masks hold one byte per source
 *         point in src's layout: 1 = the point lies on its cloud's plane.  The maps follow the outlier call: the index of a kept
 *         point within its new cloud, -1 for a removed point, 0 .. n-1 for a copied cloud.  Kept points are copied, not computed,
 *         in the source order: a -0.0 survives.  ICP_PLANE_DETECT copies the cloud; ICP_PLANE_REMOVE keeps the points off the
 *         plane, ICP_PLANE_KEEP those on it.
 *       refusals: on any refusal *out is NULL, nothing of src changes and no output array is written; where a pair is at fault
 *         the message names the first offending pair and the side.  ICP_ERR_INVALID: a null src or a null out; null seeds where
 *         any rule searches; an unknown kind; hypotheses outside [1, 65536]; a distance that is not finite or not >= 0; an axis
 *         that is not finite; min_cos outside [0, 1]; a searched cloud of n < 3.  ICP_ERR_STATE: a pass pending on the context.
 *         ICP_ERR_EMPTY for the whole call (known at the first host wait of the new batch's layout, before the new batch exists):
 *         an ICP_PLANE_REMOVE cloud whose every point is an inlier; an ICP_PLANE_KEEP cloud with no plane, or with no inlier.
 *       independence: a cloud's outputs depend on that cloud, its rule, its pair's seed and its side alone -- not on the other
 *         pairs, their order or the batch size.
 *       new batch: *out is a complete batch, as if icp_batch_create had been called with the output clouds: no options, no
 *         normals, no descriptors, no loop under way.  Several planes are peeled by calling again on the result.
 *       cost: the host draws and solves the hypotheses (three points each); the device scores them, 4096 per cloud and launch
 *         (batch_plane_score: one block of 256 threads per 4096 points of a cloud and per 32 hypotheses, the planes read at a
 *         uniform address, one integer counter per hypothesis and lane, integer adds of the blocks' counts), then
 *         batch_plane_refit and batch_plane_decide (one block per cloud each; 48 KiB and 16 bytes of LDS) and the outlier call's
 *         compaction.  Host waits: one for the clouds the host draws from, one per scoring launch (ceil(H / 4096)), one for the
 *         refit's moments, and the outlier call's two around the layout of the new batch -- five for up to 4096 hypotheses; two
 *         when nothing is searched.  No floating-point atomics.
 *   - the colored metric (ICP_COLORED; Park, Zhou, Koltun, ICCV 2017; Open3D's registration_colored_icp): a flat or gently curved
 *     textured surface leaves geometry alone three unknowns free; a scalar intensity per point (a reflectivity, the mean of an
 *     RGB colour) fixes them.  Every kept match pulls with two residuals, the point-to-plane distance weighed by lambda and the
 *     difference between the moving point's intensity and the model's intensity field at the point's foot in the tangent plane,
 *     weighed by 1 - lambda.  The batch holds one intensity per point on both sides (icp_batch_set_intensities), one intensity
 *     gradient per model point, estimated on the device (icp_batch_estimate_intensity_gradients) or given
 *     (icp_batch_set_intensity_gradients; icp_batch_get_intensity_gradients reads them back), and one weight lambda per pair
 *     (icp_batch_set_color_weight).
 *       storage: an intensity is one double per point, a gradient three doubles per model point -- always double, whatever the
 *         batch's precision -- concatenated in the layout of the clouds (moving_off, model_off).
 *       the calls follow icp_batch_set_covariances: any time after icp_batch_create; a NULL side is left untouched, both NULL is
 *         ICP_ERR_INVALID; a NaN or an infinite value is ICP_ERR_INVALID and the message names the pair and the side; a loop
 *         under way is discarded; a refused call leaves the batch as it was.  A pending pass on the context: ICP_ERR_STATE.  A
 *         null batch: ICP_ERR_INVALID.
 *       gradients depend on the model's intensities and normals: new model intensities and new model normals
 *         (icp_batch_set_model_normals, icp_batch_estimate_normals) discard them.
 *       icp_batch_estimate_intensity_gradients needs model intensities and model normals (ICP_ERR_STATE otherwise); k_model holds
 *         count ints within [ICP_COV_MIN_NEIGHBOURS, ICP_COV_MAX_NEIGHBOURS]; a model of fewer than k + 1 points is
 *         ICP_ERR_INVALID, the message names the pair.  grad_out may be NULL: there is a host wait only when it is given.
 *       icp_batch_set_color_weight takes count doubles in [0, 1]; NULL means ICP_COLOR_LAMBDA_DEFAULT for every pair, which is
 *         also what a batch holds before the first call.
 *       the gradient rule for model point i, reproducible bit for bit in numpy (tests/batch_color_ref.py does).  Every operation
 *         is one IEEE double operation, nothing is fused, and the only functions used are + - * /.
 *           neighbourhood: the FPFH rule's.  d2(i, j) is the matching's squared distance in the batch's precision F; tau_i is the
 *             k-th smallest over j != i by index; every j != i with d2(i, j) <= tau_i is in; c is their number.
 *           inputs, per neighbour j: n is the model normal of i, widened; e = q_j - q_i from the widened coordinates;
 *             h = dot(e, n); u_a = e_a - h*n_a; g = I_j - I_i.
 *           sums, from 0.0 in ascending j: A_ab += u_a*u_b for the six a <= b; r_a += u_a*g.
 *           tangent constraint: w = (double)c * (double)c; A_ab += w*(n_a*n_b): the gradient has no part along the normal.
 *           solve: the generalized metric's cofactor statements on A -- c00 = A11*A22 - A12*A12, c01 = A02*A12 - A01*A22,
 *             c02 = A01*A12 - A02*A11, c11 = A00*A22 - A02*A02, c12 = A01*A02 - A00*A12, c22 = A00*A11 - A01*A01;
 *             det = (A00*c00 + A01*c01) + A02*c02; M_ab = c_ab / det; d_a = (M_a0*r_0 + M_a1*r_1) + M_a2*r_2.
 *           fallback: the gradient is exactly (0, 0, 0) where det is not finite or not > 0, or a component of d is not finite.
 *           Every dot is (x*x' + y*y') + z*z'.  A model's gradients depend on that model, its normals, its intensities and its k alone.
 *         cost: one launch for all models (batch_intensity_gradient_kernel: one block per 64 points, the k-th distance in a register
 *           list, then the nine sums in one pass over the model), no atomics.
 *       icp_batch_begin with ICP_COLORED needs model normals, intensities on both sides and gradients (ICP_ERR_INVALID without;
 *         the message names what is missing), and a batch that holds robust kernels refuses this metric with ICP_ERR_INVALID, as
 *         it refuses ICP_GENERALIZED.  Every pair's host loop solves as for point-to-plane.  icp_host_loop_create,
 *         icp_batch_evaluate, the single-pair loops (icp_loop_begin, icp_point_to_*) and the one-call icp_point_to_*_batch refuse
 *         the value as any unknown metric.  icp_batch_downsample and icp_batch_remove_outliers make batches that hold no
 *         intensities: the caller carries them over with the maps.
 *       a step always runs deferred: the point-to-point matching launch, [the reverse search,] [the trim's selection,]
 *         batch_color_moments, the reduction up to ICP_MOM_B + 5 -- three launches, up to five, one download.  The kept decision
 *         is the one of every deferred batch: gate, tau over all n distances, the mutual rule.  Front end, ICP_MOM_ERR (Euclidean,
 *         over the points the previous matching pass kept), the err series, the stop rule, idx, masks, initial transforms and
 *         the ICP_ERR_EMPTY / ICP_ERR_SINGULAR handling are those of the other metrics.
 *       terms of a kept match of moving point i to model point j, every one in double from the widened moved point p, the model
 *         point q, the normal n and the gradient d of j and the two intensities: e = p - q, h = dot(e, n); s = dot(d, n),
 *         m_a = d_a - s*n_a; u_a = e_a - h*n_a; rI = (Iq_j + dot(d, u)) - Ip_i.  J columns j0 = (0, -pz, py), j1 = (pz, 0, -px),
 *         j2 = (-py, px, 0), j3, j4, j5 the unit vectors; G_a = dot(j_a, n), K_a = dot(j_a, m).  lg = lambda[pair], lp = 1.0 - lg.
 *         Slot C(a, c) += lg*(G_a*G_c) + lp*(K_a*K_c) for a <= c; slot B(a) -= lg*(G_a*h) + lp*(K_a*rI); ICP_MOM_CNT = 1.
 *         With lg == 1 these are the plane pass's statements.  A pair's bits depend on that pair and its options alone.
 *   - the symmetric metric (ICP_SYMMETRIC; Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019; PCL's
 *     TransformationEstimationSymmetricPointToPlaneLLS): the point-to-plane objective made symmetric in the two clouds.  Every kept
 *     match pulls along n_p + n_q, the sum of the two points' own normals, and the step is split into two half rotations.  The
 *     residual then vanishes wherever the two points lie on a common second-order patch, not only on a common plane: a wider
 *     basin after a rough global pose, and no bias from the two clouds sampling the surface differently.  It reads the point
 *     normals the batch holds on both sides (icp_batch_estimate_point_normals, icp_batch_set_point_normals: three doubles per
 *     point, in the frame of the cloud as uploaded) and nothing else.
 *       icp_batch_begin with ICP_SYMMETRIC needs point normals on both sides (ICP_ERR_INVALID without; the message names the side
 *         and the two calls that provide them), and a batch that holds robust kernels refuses this metric with ICP_ERR_INVALID,
 *         as it refuses ICP_GENERALIZED and ICP_COLORED.  It combines with gate, trim, reciprocity and initial transforms.  Every
 *         pair's host loop is a point-to-plane loop that solves by icp_solve_symmetric (icp_host_loop_set_symmetric).
 *         icp_host_loop_create, icp_batch_evaluate, the single-pair loops (icp_loop_begin, icp_point_to_*) and the one-call
 *         icp_point_to_*_batch refuse the value as any unknown metric.
 *       while a symmetric loop is under way icp_batch_set_point_normals and icp_batch_estimate_point_normals discard it
 *         (icp_batch_run: ICP_ERR_STATE until the next icp_batch_begin); under any other loop they leave it running, as before.
 *       a step always runs deferred: the point-to-point matching launch, [the reverse search,] [the trim's selection,]
 *         batch_sym_moments, the reduction up to ICP_MOM_B + 5 -- three launches, up to five, one download.  The kept decision
 *         is the one of every deferred batch: gate, tau over all n distances, the mutual rule.  Front end, ICP_MOM_ERR (Euclidean,
 *         over the points the previous matching pass kept), the err series, the stop rule, idx, masks, initial transforms and
 *         the ICP_ERR_EMPTY / ICP_ERR_SINGULAR handling are those of the other metrics.  A rejected point's idx entry carries
 *         the rejection in its top bit.
 *       terms of a kept match of moving point i to model point j.  Every operation is one IEEE double operation, nothing is
 *         fused, and the only functions used are + - *.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  p is the widened moved point, q
 *         the widened model point; m0 the stored point normal of i, in the frame of the cloud as uploaded; nq the stored point
 *         normal of j; Rc = the 3 x 3 of the pair's composed T at this pass, what the generalized step uploads
 *         (icp_diag_batch_rotation reads it).  np_a = dot(Rc[a], m0): on the first pass of a pair without an initial transform Rc
 *         is the identity and np == m0 bit for bit.  s = dot(np, nq); n_a = s < 0 ? nq_a - np_a : nq_a + np_a -- the sign rule
 *         is always on: PCA normals have no sign of their own, and ICP_ORIENT_NONE is allowed (PCL's
 *         enforce_same_direction_normals).  e = p - q, g = p + q componentwise, h = dot(e, n).  v0 = g1*n2 - g2*n1,
 *         v1 = g2*n0 - g0*n2, v2 = g0*n1 - g1*n0, v3..5 = n.  Slot C(a, c) += v_a*v_c for a <= c; slot B(a) -= v_a*h;
 *         ICP_MOM_CNT = 1.  A kept match whose n is exactly zero counts and adds zeros: the stored fallback normal (0, 0, 0) on
 *         both sides gives such a match.  The points are not centred: the cosine and sine terms of the linearization are exact
 *         about any origin, and the dropped term depends only on p - q.  A pair's bits depend on that pair and its options
 *         alone: no atomics, the fixed summation order of the other metrics.
 *       solve (icp_solve_symmetric, below): x from icp_solve_point_to_plane's Cholesky of the same slots, with the same
 *         ICP_ERR_SINGULAR; a solution that is not finite, or whose l2 is not finite, is ICP_ERR_SINGULAR too.  a = x[0..2] is the
 *         axis times tan(theta), tt = x[3..5] the translation over cos(theta).  With no trigonometry and no division by |a|:
 *         l2 = (a0*a0 + a1*a1) + a2*a2, c = 1.0 / sqrt(1.0 + l2), k = (c*c) / (1.0 + c); Ra_ab = c*E_ab + k*(a_a*a_b), where
 *         E = I + [a]x holds 1, 0 or a signed component of a (E01 = -a2, E02 = a1, E10 = a2, E12 = -a0, E20 = -a1, E21 = a0);
 *         t'_a = c*tt_a; R = Ra Ra and t = Ra t', each entry a dot of a row with a column.  Ra is the exact rotation by
 *         theta = atan(|a|) about a: the motion is p -> Ra (Ra p + t'), and a = 0 gives the identity.
     Not gated, not trimmed and without an initial transform: the single-pair loops (icp_point_to_*, icp_loop_*) and the
 *     multi-GPU sums -- a single pair that needs any of them is a batch of one; nor do they weigh matches by a robust kernel.  Trimming is the only rejection by rank: there
 *     is no other percentile rejection (none by a multiple of the median or of the standard deviation of the distances). */
typedef struct icp_batch icp_batch;
#define ICP_BATCH_MAX_POINTS 65536 /* per cloud of one pair */
int icp_batch_create(icp_ctx* ctx, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                     const int64_t* model_off, int precision, icp_batch** out);
void icp_batch_destroy(icp_batch* b);
/* unit normals of every pair's model points, concatenated exactly as model_aos was (model_off layout), element type = the
 * batch's precision.  NULL, a NaN or an infinite component anywhere: ICP_ERR_INVALID */
int icp_batch_set_model_normals(icp_batch* b, const void* nxyz_aos);
/* kNN(4) + PCA normals of every pair's model on the device: one neighbour launch + one normals launch for the whole batch.
 * nxyz_aos_out (3 per model point) and neighbours_out (4 per model point, indices WITHIN that pair's model) may be NULL.
 * Neighbours and normals follow the rule stated at icp_estimate_normals -- a rank that does not exist holds index 0, a
 * covariance that is not finite gives (+0, +0, +0) -- and are that call's on each model alone, bit for bit, over the whole range.
 * A pair's model of fewer than 5 points (k = 4 neighbours + self, as icp_estimate_normals): ICP_ERR_INVALID, the message
 * names the pair */
int icp_batch_estimate_normals(icp_batch* b, void* nxyz_aos_out, int32_t* neighbours_out);
/* prm->precision must be the batch's; prm->metric ICP_POINT_TO_POINT, or ICP_POINT_TO_PLANE on a batch that holds normals, or
 * ICP_GENERALIZED on a batch that holds covariances on both sides and no robust kernel, or ICP_COLORED on a batch that holds model
 * normals, intensities on both sides, intensity gradients and no robust kernel, or ICP_SYMMETRIC on a batch that holds point
 * normals on both sides and no robust kernel */
int icp_batch_begin(icp_batch* b, const icp_params* prm);
/* up to max_steps passes for every pair still running; *active (optional) = pairs not yet done */
int icp_batch_run(icp_batch* b, int max_steps, int* steps_done, int* active);
/* per pair: status = ICP_OK or the rc that ended this pair's loop; the rest as icp_loop_state */
int icp_batch_state(icp_batch* b, int pair, int* status, int* iterations, int* passes, double* err, int err_cap, double* T16);
/* count int32: 1 where that pair's loop has ended (stop rule, max_iter, or a failed minimisation), else 0 */
int icp_batch_done(icp_batch* b, int32_t* done_out);
int icp_batch_get_moving(icp_batch* b, void* aos_out);      /* all pairs, concatenated as uploaded, as icp_get_moving */
int icp_batch_get_indices(icp_batch* b, int32_t* idx_out);  /* each pair's most recent matching pass, as icp_get_indices */
int icp_batch_loop_indices(icp_batch* b, int32_t* idx_out); /* each pair's last contributing pass, as icp_loop_indices */
/* per-pair gate: count doubles, or NULL = no gate.  Each value > 0, or +INFINITY (that pair is not gated). */
int icp_batch_set_max_distance(icp_batch* b, const double* max_dist);
/* per-pair share of the moving cloud to keep: count doubles, or NULL = no trimming.  Each value in (0, 1]; exactly 1.0: that
 * pair is not trimmed. */
int icp_batch_set_trim(icp_batch* b, const double* keep_ratio);
/* per-pair reciprocity: count bytes, non-zero = that pair keeps only mutual nearest neighbours; NULL = off for the whole batch */
int icp_batch_set_reciprocal(icp_batch* b, const uint8_t* on);
/* per-pair robust kernel: count ints (ICP_ROBUST_*) + count doubles (the scale k of every pair whose kind is not NONE), or
 * kind == NULL: no robust kernels */
#define ICP_ROBUST_NONE 0
#define ICP_ROBUST_HUBER 1
#define ICP_ROBUST_CAUCHY 2
#define ICP_ROBUST_TUKEY 3
int icp_batch_set_robust(icp_batch* b, const int* kind, const double* scale);
/* 1 double per moving point, concatenated as the moving clouds: the weight of each pair's most recent matching pass (0.0 = the
 * match was rejected; as icp_batch_get_indices) */
int icp_batch_get_weights(icp_batch* b, double* w_out);
/* count x 16 doubles, one row-major 4x4 per pair (the layout of icp_result.T), or NULL = no initial transforms */
int icp_batch_set_initial_transforms(icp_batch* b, const double* T16);
/* per-pair fitness, inlier RMSE and information matrix where the moving clouds stand (above); max_dist: count doubles or NULL;
 * every output pointer may be NULL: status / inliers / fitness / rmse 1 per pair, info 36 per pair, idx / mask 1 per moving point */
int icp_batch_evaluate(icp_batch* b, int metric, const double* max_dist, int* status_out, int32_t* inliers_out, double* fitness_out,
                       double* rmse_out, double* info_out, int32_t* idx_out, uint8_t* mask_out);
/* 1 byte per moving point, concatenated as the moving clouds: 1 = that point's match was kept */
int icp_batch_get_inliers(icp_batch* b, uint8_t* mask_out);   /* each pair's most recent matching pass (as icp_batch_get_indices) */
int icp_batch_loop_inliers(icp_batch* b, uint8_t* mask_out);  /* each pair's last contributing pass (as icp_batch_loop_indices) */
/* a new batch on src's context: same count and precision, every pair's clouds thinned on a voxel grid (the rule: above).
 * voxel_moving / voxel_model: count doubles each (0.0 = copy that cloud), or NULL = copy that side; the maps (1 int32 per source
 * point, src's layout) may be NULL */
int icp_batch_downsample(icp_batch* src, const double* voxel_moving, const double* voxel_model, int32_t* moving_map_out,
                         int32_t* model_map_out, icp_batch** out);
/* the layout of a batch: count+1 int64 each, as icp_batch_create takes them; either pointer may be NULL */
int icp_batch_get_offsets(icp_batch* b, int64_t* moving_off_out, int64_t* model_off_out);
/* the clouds as uploaded / as made by icp_batch_downsample (P0 and Q, never the moved cloud), AoS, concatenated by the offsets
 * above; either pointer may be NULL */
int icp_batch_get_clouds(icp_batch* b, void* moving_aos_out, void* model_aos_out);
/* a new batch on src's context: same count and precision, every pair's clouds without their outliers (the rules: above) */
#define ICP_OUTLIER_NONE 0         /* copy the cloud: its bytes, its order */
#define ICP_OUTLIER_STATISTICAL 1  /* neighbours = k, value = std_ratio */
#define ICP_OUTLIER_RADIUS 2       /* neighbours = the least number of other points within value = radius */
#define ICP_OUTLIER_MAX_NEIGHBOURS 32
typedef struct icp_outlier_rule { int kind; int neighbours; double value; } icp_outlier_rule;
int icp_batch_remove_outliers(icp_batch* src,
        const icp_outlier_rule* moving, const icp_outlier_rule* model,      /* count each; NULL = copy that side */
        int32_t* moving_map_out, int32_t* model_map_out,                    /* 1 per source point, src's layout; may be NULL */
        double* moving_score_out, double* model_score_out,                  /* 1 per source point; may be NULL */
        double* stats_out,                                                  /* 2*count x 4, moving clouds first; may be NULL */
        icp_batch** out);
/* a new batch on src's context: same count and precision, every pair's clouds without their dominant plane, or reduced to it (the
 * rule: above).  seed: one word per pair (may be NULL where no rule searches); every output may be NULL */
#define ICP_PLANE_NONE   0   /* copy the cloud: its bytes, its order; nothing is searched */
#define ICP_PLANE_DETECT 1   /* copy the cloud; report its plane and inlier mask */
#define ICP_PLANE_REMOVE 2   /* new cloud = the points off the plane */
#define ICP_PLANE_KEEP   3   /* new cloud = the points on the plane */
typedef struct icp_plane_rule { int kind; int hypotheses; double distance; double axis[3]; double min_cos; } icp_plane_rule;   /* 48 bytes */
int icp_batch_segment_plane(icp_batch* src, const icp_plane_rule* moving, const icp_plane_rule* model, const uint64_t* seed /*count*/,
                            double* planes_out /*2*count x 4, moving clouds first*/, int32_t* inliers_out /*2*count*/, int* status_out /*2*count*/,
                            uint8_t* moving_mask_out, uint8_t* model_mask_out, int32_t* moving_map_out, int32_t* model_map_out,
                            icp_batch** out);
/* host: three points (9 doubles: a, b, c) -> plane4 = (nx, ny, nz, d) by the rule above.  ICP_ERR_EMPTY, and four zeros, where the
 * hypothesis is invalid (l is not > 0 or not finite); ICP_ERR_INVALID on a NULL pointer */
int icp_plane_from_points(const double* abc9, double* plane4);
/* host: the refit's last step -- the centroid and the six second moments (xx, xy, xz, yy, yz, zz) -> plane4.  ICP_ERR_EMPTY, and
 * four zeros, where the eigenvector is zero or not finite; ICP_ERR_INVALID on a NULL pointer */
int icp_plane_from_moments(const double* centroid3, const double* cov6, double* plane4);
/* the generalized metric (above): prm->metric of icp_batch_begin on a batch that holds covariances on both sides */
#define ICP_GENERALIZED 2                 /* third value of icp_metric */
#define ICP_COV_NONE 0                    /* the raw covariance */
#define ICP_COV_FROBENIUS 1               /* C / ||C||_F + lambda I */
#define ICP_COV_MIN_NEIGHBOURS 3
#define ICP_COV_MAX_NEIGHBOURS 32
/* 6 doubles per point (xx, xy, xz, yy, yz, zz), concatenated as the clouds; a NULL side is left untouched, both NULL: ICP_ERR_INVALID */
int icp_batch_set_covariances(icp_batch* b, const double* moving_cov, const double* model_cov);
/* k_moving / k_model: count ints each (NULL: that side is left untouched; both NULL: ICP_ERR_INVALID); lambda: read with
 * ICP_COV_FROBENIUS only; the outputs (6 doubles per point) may be NULL */
int icp_batch_estimate_covariances(icp_batch* b, const int* k_moving, const int* k_model, int regularisation, double lambda,
                                   double* moving_cov_out, double* model_cov_out);
/* the covariances the batch holds; either pointer may be NULL; ICP_ERR_STATE where a side that is asked for holds none */
int icp_batch_get_covariances(icp_batch* b, double* moving_cov_out, double* model_cov_out);
/* the colored metric (above): prm->metric of icp_batch_begin on a batch that holds model normals, intensities and gradients */
#define ICP_COLORED 3                         /* fourth value of icp_metric */
#define ICP_COLOR_LAMBDA_DEFAULT 0.968
/* 1 double per point, concatenated as the clouds; a NULL side is left untouched, both NULL: ICP_ERR_INVALID */
int icp_batch_set_intensities(icp_batch* b, const double* moving_I, const double* model_I);
/* k_model: count ints; grad_out (3 doubles per model point) may be NULL */
int icp_batch_estimate_intensity_gradients(icp_batch* b, const int* k_model, double* grad_out);
/* 3 doubles per model point, concatenated as the models */
int icp_batch_set_intensity_gradients(icp_batch* b, const double* grad);
/* the gradients the batch holds; ICP_ERR_STATE where it holds none */
int icp_batch_get_intensity_gradients(icp_batch* b, double* grad_out);
/* count doubles in [0, 1]: the weight of the geometric term; NULL: ICP_COLOR_LAMBDA_DEFAULT for every pair */
int icp_batch_set_color_weight(icp_batch* b, const double* lambda);
/* the symmetric metric (above): prm->metric of icp_batch_begin on a batch that holds point normals on both sides */
#define ICP_SYMMETRIC 4                       /* fifth value of icp_metric */
/* global registration (above).  k_*: count ints each; *_normals: 3 doubles per point, laid out as the clouds; the outputs
 * (ICP_FEATURE_BINS doubles per point) may be NULL */
#define ICP_FEATURE_BINS 33
int icp_batch_compute_features(icp_batch* b, const int* k_moving, const int* k_model, const double* moving_normals,
                               const double* model_normals, double* moving_feat_out, double* model_feat_out);
/* point normals on the device (above).  *_viewpoints: 3 doubles per pair, read with ICP_ORIENT_VIEWPOINT only; the normals:
 * 3 doubles per point, laid out as the clouds; the outputs may be NULL */
#define ICP_ORIENT_NONE 0        /* the eigenvector as the Jacobi leaves it */
#define ICP_ORIENT_VIEWPOINT 1   /* facing the caller's viewpoint of each cloud */
#define ICP_ORIENT_CENTROID 2    /* facing each cloud's own centroid */
int icp_batch_estimate_point_normals(icp_batch* b, int orient, const double* moving_viewpoints, const double* model_viewpoints,
                                     double* moving_normals_out, double* model_normals_out);
int icp_batch_set_point_normals(icp_batch* b, const double* moving_normals, const double* model_normals);
int icp_batch_get_point_normals(icp_batch* b, double* moving_normals_out, double* model_normals_out);
/* icp_batch_compute_features from the point normals the batch holds */
int icp_batch_compute_features_stored(icp_batch* b, const int* k_moving, const int* k_model, double* moving_feat_out, double* model_feat_out);
/* the descriptors the batch holds; either pointer may be NULL; ICP_ERR_STATE where a side that is asked for holds none */
int icp_batch_get_features(icp_batch* b, double* moving_feat_out, double* model_feat_out);
/* fwd_out / kept_out: 1 per moving point; rev_out: 1 per model point; each may be NULL */
int icp_batch_match_features(icp_batch* b, int mutual, int32_t* fwd_out, int32_t* rev_out, uint8_t* kept_out);
/* T16: count x per_pair x 16 doubles; max_dist: count doubles or NULL; count_out: count x per_pair int32 */
int icp_batch_score_transforms(icp_batch* b, int per_pair, const double* T16, const double* max_dist, int32_t* count_out);
typedef struct icp_ransac_params { int hypotheses; double max_distance; double edge_similarity; } icp_ransac_params;
int icp_batch_ransac(icp_batch* b, const icp_ransac_params* prm, const uint64_t* seed /*count*/,
                     double* T16_out, int32_t* inliers_out, int32_t* correspondences_out, int* status_out);
/* Fast Global Registration over the correspondence lists (above) */
typedef struct icp_fgr_params {
    int iterations;           /* [1, 1024]; Open3D's default is 64 */
    double max_distance;      /* delta: finite, > 0; mu is never lowered below delta^2 */
    double division_factor;   /* finite, > 1; 1.4 */
    int decrease_every;       /* >= 1; 4 */
    int tuples;               /* [0, 65536]; 0 = use every correspondence */
    double tuple_similarity;  /* [0, 1); read only where tuples > 0; 0.95 */
} icp_fgr_params;
int icp_batch_fgr(icp_batch* b, const icp_fgr_params* prm, const uint64_t* seed /* count; may be NULL iff tuples == 0 */,
                  double* T16_out, double* weights_out /* 1 per moving point */, int32_t* used_out /* 1 per pair */,
                  double* objective_out /* 1 per pair */, int* status_out);
/* a new batch on src's context: same count and precision, every pair's clouds reduced to their keypoints, with the descriptors
 * of the kept points where src holds descriptors (the rule: above) */
#define ICP_KEYPOINT_NONE 0   /* copy the cloud: its bytes, its order */
#define ICP_KEYPOINT_ISS  1
typedef struct icp_keypoint_rule { int kind; int min_neighbours; double salient_radius; double non_max_radius; double gamma_21; double gamma_32; } icp_keypoint_rule;   /* 40 bytes */
int icp_batch_select_keypoints(icp_batch* src,
        const icp_keypoint_rule* moving, const icp_keypoint_rule* model,   /* count each; NULL = copy that side */
        int32_t* moving_map_out, int32_t* model_map_out,                   /* 1 per source point, src's layout; may be NULL */
        double* moving_saliency_out, double* model_saliency_out,           /* 1 per source point; may be NULL */
        int32_t* count_out,                                                /* 2 * count, moving clouds first; may be NULL */
        icp_batch** out);
/* one call: create + begin + run to the end + results, then destroy.  Every output pointer may be NULL; per pair:
 * T16_out 16, iterations_out / passes_out / status_out 1, err_out max_iter+1 doubles; idx_out and moved_out (3 values per
 * point, precision of the run) concatenated as the moving clouds.  A failed pair is reported in status_out, not in the
 * return code.  prm->metric must be ICP_POINT_TO_POINT. */
int icp_point_to_point_batch(icp_ctx* ctx, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                             const int64_t* model_off, const icp_params* prm, double* T16_out, int* iterations_out,
                             int* passes_out, double* err_out, int32_t* idx_out, void* moved_out, int* status_out);
/* as icp_point_to_point_batch; normals_aos may be NULL (then estimated on the device); prm->metric must be ICP_POINT_TO_PLANE */
int icp_point_to_plane_batch(icp_ctx* ctx, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                             const int64_t* model_off, const void* normals_aos, const icp_params* prm, double* T16_out,
                             int* iterations_out, int* passes_out, double* err_out, int32_t* idx_out, void* moved_out, int* status_out);

/* ---- multi-GPU: the loop's single collective issued by the library (RCCL over xGMI, bound at run time) ----
 * One process per GPU.  Rank 0 obtains an id (icp_comm_unique_id), the host application distributes those
 * ICP_COMM_ID_BYTES bytes by any means (MPI, a torch.distributed broadcast, a file), every rank calls
 * icp_comm_init on its context.  From then on icp_loop_enqueue all-reduces (sum, in place) the ICP_NMOM vector
 * right behind the finalize kernel on the loop's stream; icp_loop_complete sees the global sums.  Shard the
 * MOVING cloud with icp_shard_range and give every rank the full model. */
#define ICP_COMM_ID_BYTES 128
int icp_comm_unique_id(void* out_id_bytes);
int icp_comm_init(icp_ctx* ctx, const void* id_bytes, int rank, int world);
int icp_comm_destroy(icp_ctx* ctx);
/* The same exchange for ranks on ONE node, through POSIX shared memory instead of a device collective: in the
 * single-node fast path the loop's vector is already in host memory when the rows have been added, and 256 bytes
 * between processes of a node take ~1 us (RCCL: ~15-20 us, more than the iteration).  Every rank adds the ranks'
 * vectors in rank order, so all ranks continue from bit-identical sums; the resident-kernel loop stays available.
 * id_bytes: ICP_COMM_ID_BYTES random bytes from rank 0 (icp_comm_random_id), distributed by the application. */
int icp_comm_random_id(void* out_id_bytes);
int icp_comm_init_local(icp_ctx* ctx, const void* id_bytes, int rank, int world);
/* the host-memory communicator on its own (no device needed: multi-process CPU tests, custom drivers);
 * icp_lcomm_allreduce: v[0..count) <- sum over ranks in rank order, count <= ICP_NMOM */
typedef struct icp_lcomm icp_lcomm;
int icp_lcomm_create(const void* id_bytes, int rank, int world, icp_lcomm** out);
int icp_lcomm_allreduce(icp_lcomm* comm, double* v, int count);
void icp_lcomm_destroy(icp_lcomm* comm);

/* ---- host-only pieces (no device needed; exercised by the CPU test-suite) ------------------- */
/* 3x3 cross-covariance solve from raw moments: replaces cublasSgemm + cusolverDnSgesvd + 2 gemm
 * (src/ICP_point_to_point.cu:356-397) / dgemm + LAPACKE_dgesvd (src/ICP_CPU.c:239-248).
 * R = U*Vt with NO reflection fix (the reference has none).  Returns ICP_OK. */
int icp_solve_point_to_point(const double* mom /*ICP_NMOM*/, double* R9, double* t3);
/* icp_solve_point_to_point with the determinant fix: the last column of U is flipped when det(U Vt) < 0, so R is always a
 * rotation (det = +1) -- what a minimal sample needs: three points give a rank-2 cross-covariance, and without the fix about
 * half the hypotheses of icp_batch_ransac would come out as reflections.  ICP_ERR_INVALID where ICP_MOM_CNT is not > 0. */
int icp_solve_rigid(const double* mom /*ICP_NMOM*/, double* R9, double* t3);
/* 6x6 normal equations: replaces cusolverDnSpotrf/Spotrs UPPER (src/ICP_point_to_plane.cu:576-581)
 * and LAPACKE_ssysv (CPU_ICP_point_to-plane.cpp:371); x = (alpha,beta,gamma,tx,ty,tz), then the
 * full (non-linearised) R = Rz(gamma) Ry(beta) Rx(alpha) (src/ICP_point_to_plane.cu:585-593). */
int icp_solve_point_to_plane(const double* mom /*ICP_NMOM*/, double* R9, double* t3, double* x6);
/* the symmetric metric's step (the rule: "the symmetric metric" above): the same Cholesky of the same slots, x = (a, tt) into x6
 * (may be NULL) as solved, then R = Ra Ra and t = Ra (c tt) with Ra the rotation by atan(|a|) about a.  ICP_ERR_SINGULAR as
 * icp_solve_point_to_plane, and where x or |a|^2 is not finite; ICP_ERR_INVALID where mom, R9 or t3 is NULL. */
int icp_solve_symmetric(const double* mom /*ICP_NMOM*/, double* R9, double* t3, double* x6);
/* The host half of the loops above as a device-free state machine (the device loop runs this very
 * code): feed it the rank-reduced ICP_NMOM vector of each pass, it returns the stop decision and the
 * next R, t; tell it when that motion has been applied.  Sequence per pass:
 *   advance(mom_k) -> [done?] -> apply R,t to the shard -> note_applied() -> (next pass' moments) ... */
typedef struct icp_host_loop icp_host_loop;
int icp_host_loop_create(const icp_params* prm, icp_host_loop** out);
void icp_host_loop_destroy(icp_host_loop* h);
int icp_host_loop_advance(icp_host_loop* h, const double* mom /*ICP_NMOM*/, int* done, double* R9, double* t3);
int icp_host_loop_note_applied(icp_host_loop* h);
/* on != 0: the vectors are those of a robust pass -- every advance from now on solves on a copy of the vector whose ICP_MOM_CNT slot
 * holds mom[ICP_MOM_W] (the weighted Kabsch solve; the plane solve never reads the slot), and a matching pass whose ICP_MOM_W is
 * not > 0 ends the loop with ICP_ERR_EMPTY.  The error, its divisor (the kept count), the stop rule and the iteration counting
 * do not change.  Off (the default): the loop is the one it always was. */
int icp_host_loop_set_weighted(icp_host_loop* h, int on);
/* on != 0: the vectors are those of a symmetric pass -- every advance of a point-to-plane loop from now on solves by
 * icp_solve_symmetric where it solved by icp_solve_point_to_plane.  Everything else is unchanged.  Off (the default): the loop is
 * the one it always was. */
int icp_host_loop_set_symmetric(icp_host_loop* h, int on);
int icp_host_loop_state(icp_host_loop* h, int* iterations, int* passes, double* err, int err_cap, double* T16);
/* contiguous shard [begin, begin+count) of n moving points for `rank` of `world`.  Any partition of the moving points is the same
 * registration, and a registration is as slow as its slowest rank: where the work per point varies over a LARGE cloud (BASELINE
 * configs[4]: contiguous eighths take 16 to 30 ms) deal compact blocks of the cloud to the ranks instead (distributed.curve_order +
 * shard_cyclic_index of the Python mirror) -- every rank simply passes its own points to icp_set_moving. */
int icp_shard_range(int64_t n, int rank, int world, int64_t* begin, int64_t* count);
/* symmetric 3x3 eigen-solve used for the normals (upper triangle of row-major A read);
 * w ascending, Z[i*3+k] = component i of eigenvector k.  The range rule: the stop test of the cyclic Jacobi squares the entries, so
 * with amax the largest magnitude of the six entries read, all of them finite, amax > 2^400 multiplies them by 2^-600 and
 * 0 < amax < 2^-400 by 2^+600 before the first sweep -- an exact power of two, which changes no rotation -- and the three
 * eigenvalues are multiplied by 2^+600 or 2^-600 after the ascending order is fixed: w is the scaled-back eigenvalues, and one that
 * leaves the double range on the way back is what IEEE makes of the product (inf, a subnormal, 0).  Every matrix with amax within
 * [2^-400, 2^400], the zero matrix, and every matrix with an entry that is not finite go through as they are, bit for bit. */
int icp_eigh3(const double* A9, double* w3, double* Z9);

/* ---- datasets: the reference's input formats --------------------------------- */
/* synthetic z = x^2 - y^2 grid, fp32 AoS: src/ICP_point_to_point.cu:103-152 (W*W points) */
int icp_synthetic_grid_f32(int W, float xy_min, float xy_max, float* D_aos);
/* fp64 AoS variant of src/ICP_CPU.c:51-95 */
int icp_synthetic_grid_f64(int W, double xy_min, double xy_max, double* D_aos);
/* model = R*D + t with the closed-form column-major rotation of the GPU programs
 * (src/ICP_point_to_point.cu:157-190), fp32 */
int icp_make_model_f32(const float* D_aos, int n, const float angles_xyz[3], const float t[3], float* M_aos);
/* model of src/ICP_CPU.c:100-149 (r = rx*ry*rz, +sin above the diagonal), fp64 */
int icp_make_model_cpu_f64(const double* D_aos, int n, const double angles_xyz[3], const double t[3], double* M_aos);
/* the hard-coded rotation of src/ICP_standard.cu:247-249 */
int icp_make_model_standard_f32(const float* D_aos, int n, float* M_aos);
/* "x y z" / "x;y;z" text (Bunny_res.csv / Bunny.csv): src/CUDA/GPU_point_to_point_bunny.cu:463-497.
 * Returns the number of POINTS read (>= 0) or a negative error; at most cap_points are stored. */
int icp_read_xyz_text(const char* path, float* out_aos, int cap_points);
/* Ouster OS1-16 dump, one byte value per text line (Donut_1024x16.csv) or raw binary packets
 * (12608 B each): src/CUDA/GPU_point_to_point_real.cu:432-488.  16 beams x 16 azimuth blocks per
 * packet; ranges in mm.  Returns the number of ranges or a negative error. */
int icp_read_os1_ranges(const char* path, uint32_t* ranges_out, int cap, uint32_t* encoder_count0);
/* beam_intrinsics.csv: 64 altitude + 64 azimuth angles (deg), the 16 used beams selected as the
 * reference does (every 4th from the 3rd): src/CUDA/GPU_point_to_point_real.cu:503-527 */
int icp_read_os1_intrinsics(const char* path, float altitude16[16], float azimuth16[16]);
/* polar -> Cartesian on the device, replaces Conversion<<<>>> src/CUDA/GPU_point_to_point_real.cu:20-36.
 * Output AoS fp32 in mm (host). */
int icp_os1_to_cartesian(icp_ctx* ctx, const uint32_t* ranges, int n, uint32_t encoder_count0,
                         const float altitude16[16], const float azimuth16[16], float* xyz_aos_mm);

/* raw OS1-16 packets (n_packets x 12608 bytes, as captured from the sensor) -> ranges + Cartesian points in one
 * device pass: replaces the host parse loop + H2D + Conversion<<<>>> of
 * src/CUDA/GPU_point_to_point_real.cu:457-487,538-563.  256 points per packet; ranges_out may be NULL. */
int icp_os1_packets_to_cartesian(icp_ctx* ctx, const uint8_t* packets, int n_packets, const float altitude16[16],
                                 const float azimuth16[16], float* xyz_aos_mm, uint32_t* ranges_out);

#ifdef __cplusplus
}
#endif
#endif /* ICP_MI355X_H */
