/*
 * icp_mi355x_diag.h -- measurement and diagnostic entry points of libicp_mi355x.so: what bench.py, the sweep program
 * and the tests use to time the matching kernel alone, to count the work it executes and to inspect launch geometry.
 * None of this is on the registration path and nothing here replaces a reference statement other than the reference's
 * own timing harness (src/CUDA/Matching_opt.cu:213-226).  Same conventions as icp_mi355x.h.
 */
#ifndef ICP_MI355X_DIAG_H
#define ICP_MI355X_DIAG_H

#include "icp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `reps` back-to-back launches of the matching kernel alone between two hipEvents on the context's
 * stream; total_ms / reps is the kernel's average launch duration (bench.py roofline leg) */
int icp_nn_match_bench(icp_ctx* ctx, int reps, float* total_ms);
/* same; seeded != 0 hands the kernel the most recent correspondences as its starting bound (what the ICP
 * loop does from its second pass on), seeded == 0 starts it cold (what icp_nn_match_* does).  Behind the timed span the last
 * launch's results are merged: icp_get_indices then returns the correspondences of that launch */
int icp_nn_match_bench_ex(icp_ctx* ctx, int reps, int seeded, float* total_ms);
/* The reference's own kernel-timing method (src/CUDA/Matching_opt.cu:213-226: cudaEventRecord around every launch,
 * minimum of 10 after warm-up): `warmups` untimed launches, then `reps` launches with a hipEvent pair around each one;
 * each_ms[r] receives the duration of launch r.  mode 0: the matching kernel as the loop launches it (seeded with the
 * most recent correspondences), 1: cold (no seed), 2: the dense packed kernel, which EXECUTES every one of the
 * n_pad x m_pad pairs (fp32 only; no boxes, no early-out) -- the brute-force scan the roofline arithmetic is about. */
int icp_nn_match_bench_launches(icp_ctx* ctx, int reps, int warmups, int mode, float* each_ms);
/* ... of the launch the resident clouds get from the production plan (dense == 0) or from the dense packed kernel */
int icp_nn_launch_info_ex(icp_ctx* ctx, int dense, int* splits, int* blocks, int* threads, int* n_pad, int* m_pad);
/* the launch shape icp_estimate_normals gives the fp32 neighbour search (knn4_f32_v2) of a model of m >= 5 points on this context's
 * CU count: out = { n_pad (queries, padded to blocks of 128), blocks_x (query blocks), splits (model segments = grid.y),
 * seg_len (model points per segment; wave w of a block scans the points [s * seg_len + w * seg_len / 4, + seg_len / 4) of segment
 * s), tiles (LDS tiles each wave streams its quarter through) }.  Arithmetic alone: nothing is launched, no cloud need be
 * resident.  What lets a test put equal distances on both sides of every border at which two lists are merged. */
int icp_diag_knn4_geometry(icp_ctx* ctx, int m, int out[5]);
/* Executed-work accounting of the sparse matching kernel (it returns the brute-force answer of Matching<<<>>> without
 * evaluating most pairs, so the roofline of EXECUTED arithmetic needs a count).  enable != 0: every following sparse
 * launch of this context runs its instrumented instantiation and adds wave-level tallies to 8 device counters;
 * icp_get_work_counters reads them (uint64 x ICP_WORK_SLOTS) and optionally zeroes them.  Slots:
 *   0 chunk boxes tested against a block's group box (one lane each)      1 upper-level boxes (large models)
 *   2 hits = (wave, 8-point chunk) pairs through the per-point box test   3 ... through the xy half of the distances
 *   4 ... evaluated in full (each hit: 64 lanes x 2 moving points x 8 model points)
 *   5 cold-start sample groups scanned (128 x 8 pairs each)   6 (block, pass) pairs   7 ... that applied a transform
 * Timing with counting on is not representative (atomics, extra registers): count in a separate run. */
#define ICP_WORK_SLOTS 12 /* 8..11: speculative lists entered / that covered the pass / their hits / hits of ordinarily built lists */
int icp_set_work_counting(icp_ctx* ctx, int enable);
int icp_get_work_counters(icp_ctx* ctx, uint64_t* out_slots, int reset);

/* shared rows (clouds of 33-57 k moving points): how a matching launch of `blocks` blocks deals itself to `rows`
 * rows of 128 moving points, given the hit chunks every row listed in the launch before -- parts[r] blocks search row r
 * (>= 1 each, their sum <= blocks whatever the counts hold), *target = hits per block the split aims at.  The kernel computes
 * exactly this in every block; no device is involved here (no reference counterpart: its kernels are thread-per-point). */
int icp_share_rows_plan(const uint32_t* hits, int rows, int blocks, int model_points, int min_hits, int32_t* parts, uint32_t* target);
/* ordered + split rows (large clouds): the roles a launch's blocks get from the hit counters of the launch before,
 * computed ON THE DEVICE by the kernels the loop uses -- control != 0: the single-workgroup launch (rows <= 16 384: quantised
 * counting sort + roles), else keys + rocPRIM radix sort + roles.  roles_out: rows + ICP_ROLES_EXTRA entries, each
 * row | part << 21 | log2(parts) << 27, or -1 for a block nothing needs; hits_io is read AND zeroed, as by the loop.
 * min_part / total_div: the smallest part of a split row in hits, and what the counters' sum is divided by for the target. */
#define ICP_ROLES_EXTRA 4096
int icp_diag_row_roles(icp_ctx* ctx, uint32_t* hits_io, int rows, int min_part, int total_div, int control, int32_t* roles_out);

/* The ICP_NMOM-double moment vector the loop's host half (HostLoop::advance: error, stop rule, solve) last received -- after the
 * rows were added up by whoever adds them for this plan and after any exchange between the ranks of a node communicator -- and,
 * in *route (may be NULL), how it came about: the ICP_ROUTE_* bits below.  Everything a pass gives the host is in this vector;
 * tests/test_gpu_moments.py holds it against exact sums over (moving cloud, model, correspondences) of the same pass.  Reading it
 * costs the loop nothing: the flags are set where the pass is issued and completed, the vector is the one the loop keeps anyway.
 * ICP_ERR_STATE before the first completed pass of a loop, and between icp_loop_enqueue and icp_loop_complete (the vector would
 * be the previous pass's, the route the pending one's).  (The reference has no such seam: its sums are cublas calls between
 * the kernels, src/ICP_point_to_point.cu:308-357.) */
#define ICP_ROUTE_HOST_ROWS 0x001      /* the host added the pass's rows from pinned memory (sum_host_rows) */
#define ICP_ROUTE_COMPACT 0x002        /* ... rows in the compact 16-double format (tag in the low mantissa bits of slots 0/4/8/12) */
#define ICP_ROUTE_AVX 0x004            /* ... with the AVX adder (else the scalar loop: ICP_MAILBOX=plain, or no AVX) */
#define ICP_ROUTE_FIN_LAUNCH 0x008     /* the matching launch added its rows up itself (fin_close) */
#define ICP_ROUTE_FIN_PINNED 0x010     /* ... and left the vector in pinned memory (else in the device vector, copied back) */
#define ICP_ROUTE_FIN_KERNEL 0x020     /* rows left on the device and added by finalize_kernel, the vector copied back */
#define ICP_ROUTE_FIN_TWO_STAGE 0x040  /* ... through finalize_ranges_kernel first (more than 2048 rows) */
#define ICP_ROUTE_FUSED_TAIL 0x080     /* the rows come from the matching kernel's fused tail */
#define ICP_ROUTE_MOMENTS_KERNEL 0x100 /* ... or from moments_kernel (the two-kernel form) */
#define ICP_ROUTE_ERROR_ONLY 0x200     /* the loop's last pass: a transform and its error, nothing matched (only ICP_MOM_ERR means anything) */
#define ICP_ROUTE_ARMED 0x400          /* the pass was an armed launch released through its mailbox */
#define ICP_ROUTE_RESIDENT 0x800       /* the pass was a message to the resident kernel */
int icp_diag_loop_moments(icp_ctx* ctx, double* out32, int* route);
/* the same for pair `pair` of a batch: the row of the step's download that pair's loop last advanced on (the rows are always
 * added by batch_finalize_kernel; they come from nn_match_batch's fused tail, or from batch_trim_moments in a batch that trims
 * or holds a reciprocal pair, or from batch_robust_moments in a batch with a robust kernel: there slot ICP_MOM_W = 29 holds the sum
 * of the kept matches' weights, ICP_MOM_CNT stays the kept count and every other slot behind ICP_MOM_ERR is weighted; in every
 * other batch slot 29 is 0).
 * ICP_ERR_STATE before the pair's first completed pass. */
int icp_diag_batch_moments(icp_batch* b, int pair, double* out32);
/* trimmed rejection of pair `pair` (icp_batch_set_trim): *tau_sq = the threshold of the pair's most recent matching pass -- the
 * K-th smallest winning squared distance, in the batch's precision, read back in double; +inf for a pair that is not trimmed --
 * and *rank = K (n for a pair that is not trimmed).  Either pointer may be NULL.  The per-pair threshold buffer is copied down
 * on demand: nothing is added to a step's download.  ICP_ERR_STATE before the pair's first completed matching pass. */
int icp_diag_batch_trim(icp_batch* b, int pair, double* tau_sq, int* rank);
/* reciprocal matches (icp_batch_set_reciprocal): the reverse search, one int32 per model point, concatenated as the models were
 * (model_off[count] entries).  For every reciprocal pair: rev[j] of that pair's most recent matching pass, the lowest i in [0, n)
 * that minimises dist2(p_i, q_j).  -1 throughout for a pair whose flag is 0, or that has completed no matching pass since
 * icp_batch_begin.  Downloaded on demand: nothing is added to a step.  ICP_ERR_STATE before the first step of a loop. */
int icp_diag_batch_reverse(icp_batch* b, int32_t* rev_out);
/* The evaluation vector of pair `pair` from the latest icp_batch_evaluate (icp_mi355x.h): ICP_NMOM doubles, the only data the
 * call's per-pair outputs (inliers, fitness, rmse, information) are formed from.  Every term is formed in double from the widened
 * coordinates of the kept matches, added per work item and then per pair in a fixed order.  Slots, q = the matched model point,
 * p = the moving point, n = the model normal at the match:
 *   ICP_EVAL_SD   sum |q - p|^2, the differences formed in double        ICP_EVAL_CNT  the kept count
 *   ICP_POINT_TO_POINT:  ICP_EVAL_SQ (3) sum q;  ICP_EVAL_SQQ (6) sum q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z, q_z q_z
 *   ICP_POINT_TO_PLANE:  ICP_MOM_C .. ICP_MOM_C + 20  sum cn cn^T, upper triangle row-major, cn = (p x n, n): a plane pass's C
 * Every other slot is 0; a pair that was not evaluated (status ICP_ERR_INVALID) has an all-zero vector.  ICP_ERR_STATE before the
 * batch's first evaluation; a refused icp_batch_evaluate leaves the vectors of the evaluation before it. */
#define ICP_EVAL_SD 0
#define ICP_EVAL_CNT 1
#define ICP_EVAL_SQ 2
#define ICP_EVAL_SQQ 5
int icp_diag_batch_eval_moments(icp_batch* b, int pair, double* out32);
/* the generalized metric (ICP_GENERALIZED): the 9 doubles, row-major, of the rotation Rc that pair `pair`'s most recent matching
 * pass rotated the moving covariances by -- the rotation part of the product of every motion applied to the cloud that pass
 * matched on, the initial transform included (the upper left 3 x 3 of icp_batch_state's T at that pass).  A host copy of what
 * the step uploaded: nothing is downloaded.  A symmetric loop (ICP_SYMMETRIC) answers too: its passes rotate the moving point
 * normals by the same Rc.  ICP_ERR_STATE unless a generalized or a symmetric loop is under way and the pair has completed
 * a matching pass. */
int icp_diag_batch_rotation(icp_batch* b, int pair, double* R9);

/* descriptors of the caller's own in place of icp_batch_compute_features' (ICP_FEATURE_BINS doubles per point, both sides, laid
 * out as icp_batch_get_features returns them; nothing is checked): what lets a test match clouds too small to describe, or
 * descriptors with planted ties.  Discards the matches. */
int icp_diag_batch_set_features(icp_batch* b, const double* moving_feat, const double* model_feat);
/* the last icp_batch_ransac run's hypotheses of pair `pair`, H = that run's prm->hypotheses of each: triples 3 x H int32 (the
 * positions in the pair's correspondence list that slots 0, 1, 2 took; -1 for a slot left empty), valid H bytes (three distinct
 * picks, the edge check passed and the solve succeeded), T16 16 x H doubles (the pose icp_solve_rigid gave, in double, before it
 * is rounded to the batch's precision for scoring; the identity for an invalid hypothesis), counts H int32 (the inliers
 * batch_score_transforms counted; -1 for an invalid hypothesis).  Host copies: nothing is downloaded.  Every output may be NULL.
 * ICP_ERR_STATE before the first run. */
int icp_diag_batch_ransac(icp_batch* b, int pair, int32_t* triples, uint8_t* valid, double* T16, int32_t* counts);
/* the last icp_batch_fgr run's history of pair `pair`, I = that run's prm->iterations: used_pos U_p int32 (the positions in the
 * pair's correspondence list that were used, ascending; U_p is the call's used_out), mu_hist I doubles (mu of every iteration),
 * mom_hist I x ICP_NMOM doubles (the vector every iteration's solve read), T_hist I x 16 doubles (the pose that iteration's terms
 * were formed at: the identity for iteration 0).  The iterations a pair did not run -- after ICP_ERR_SINGULAR, or all of them for
 * ICP_ERR_EMPTY -- hold zeros.  Host copies: nothing is downloaded.  Every output may be NULL.  ICP_ERR_STATE before the first run. */
int icp_diag_batch_fgr(icp_batch* b, int pair, int32_t* used_pos, double* mu_hist, double* mom_hist, double* T_hist);
/* where the host's time went in the iterations of the last icp_batch_fgr run, summed over them, in seconds: [0] enqueue (the
 * control block, its upload, the two launches, the download), [1] the wait for the vectors, [2] the solves of all pairs; [3] is
 * the number of iterations that ran.  Three clock reads per iteration.  ICP_ERR_STATE before the first run. */
int icp_diag_batch_fgr_times(icp_batch* b, double* seconds4);
/* the centroids batch_centroid_kernel made in the last icp_batch_estimate_point_normals call with ICP_ORIENT_CENTROID: 3 doubles
 * per cloud, 2 * count clouds, the moving clouds first.  One download, one wait.  ICP_ERR_STATE after no such call. */
int icp_diag_batch_centroids(icp_batch* b, double* out /* 2 * count * 3 */);
/* the last icp_batch_segment_plane call's hypotheses of one cloud of src -- pair `pair`, side 0 (the moving cloud) or 1 (the
 * model) -- H = that cloud's rule's hypotheses: triples 3 x H int32 (the point indices that slots 0, 1, 2 took; -1 for a slot left
 * empty), valid H bytes (three distinct picks, l > 0 and finite, the axis test passed), planes 4 x H doubles (nx, ny, nz, d; zeros
 * for an invalid hypothesis), counts H int32 (the inliers batch_plane_score counted; -1 for an invalid hypothesis).  Host copies:
 * nothing is downloaded.  Every output may be NULL.  ICP_ERR_STATE before the first call and for a cloud whose kind was
 * ICP_PLANE_NONE; a refused call leaves the hypotheses of the call before it. */
int icp_diag_batch_segment(icp_batch* b, int pair, int side, int32_t* triples, uint8_t* valid, double* planes, int32_t* counts);
#ifdef __cplusplus
}
#endif
#endif /* ICP_MI355X_DIAG_H */
