// icp_batch.cpp -- batched ICP (icp_batch_*, icp_point_to_point_batch, icp_point_to_plane_batch): many independent pairs, and per
// step ONE matching launch + ONE reduction launch + ONE download of ICP_NMOM doubles per pair for every pair still running.
//
//   step k:  [R, t + mode of every pair: H2D]  ->  nn_match_batch (icp_k_batch.hip: transform + error, match, moments per work item)
//            [a batch that trims or holds a reciprocal or a robust pair: nn_match_batch<DEFER>  ->  nn_match_batch_rev (reciprocal)
//             ->  batch_trim_select (trims)  ->  batch_trim_moments / batch_robust_moments -- see the table below]
//            ->  batch_finalize_kernel (per pair, fixed order)  ->  D2H count x ICP_NMOM  ->  sync
//            ->  HostLoop::advance per pair that took part (error, stop rule, 3x3 solve or 6x6 solve)
//
// A batch may hold a maximum correspondence distance per pair (icp_batch_set_max_distance).  Its passes then run the gated
// instantiations of nn_match_batch: a match farther than that enters no sum, the point's idx entry carries the rejection in
// its top bit for the next pass's error (and for the mask downloads), and a pass that keeps nothing ends its pair with
// ICP_ERR_EMPTY.  Launches and downloads per step stay as above; a batch without thresholds runs the ungated kernels.
//
// A batch may hold an initial transform per pair (icp_batch_set_initial_transforms).  icp_batch_begin then makes every pair's
// start cloud with ONE launch (batch_init_kernel: apply_rt of the transform rounded to the batch's precision, T0F, on the
// clouds as uploaded) in place of the P0 -> P copy, and reads one flag per pair back: a pair whose start cloud left the
// precision's range begins ended (ICP_ERR_INVALID).  The loops know nothing of it -- from the start cloud on a pair runs as
// in a batch created from that cloud -- and icp_batch_state composes T_loop . T0F when it is read.  The steps are unchanged.
//
// A batch may hold a share to keep per pair (icp_batch_set_trim): a pair then keeps the K = ceil(rho n) closest of its n matches in
// every matching pass, and every match tied with the K-th.  The K-th distance is known only when all of the pair's points are
// matched, so the steps of such a batch run deferred: nn_match_batch<.., DEFER> (matching, no decision)  ->  batch_trim_select
// (tau = the K-th smallest distance, per pair)  ->  batch_trim_moments (the decision, with the gate's where there is one, and the
// sums)  ->  batch_finalize_kernel: four launches, still one download.  A batch whose shares are all 1.0 runs the steps above.
//
// A batch may hold a reciprocity flag per pair (icp_batch_set_reciprocal): a reciprocal pair keeps a match only if the model
// point's own nearest moving point, on the cloud the pass matched on, is that very point (rev[idx[i]] == i).  That decision needs
// the reverse search of the whole pair, so the steps of such a batch run deferred as well: nn_match_batch<.., DEFER>  ->
// nn_match_batch_rev (one block per model work item: rev)  ->  batch_trim_select (only if the batch also trims)  ->
// batch_trim_moments<.., MUTUAL> (mutual && trim && gate, and the sums)  ->  batch_finalize_kernel: four launches, five with
// trimming, still one download.  rev is consumed inside the step that wrote it (no ping-pong), and a pair's rows of it are
// rewritten only when that pair matches.  A batch whose flags are all 0 runs the steps it ran without them.
//
// A batch may hold a robust kernel per pair (icp_batch_set_robust: Huber, Cauchy or Tukey weights at a scale k): every kept match
// of such a pair enters the sums with a weight in [0, 1] that falls with its residual, and the pair's HostLoop solves on the
// weighted vector (HostLoop::weighted: CNT <- W).  The weight needs nothing the deferred decision does not have, so the steps of a
// batch with a robust pair always run deferred, with batch_robust_moments in batch_trim_moments' place: the same decision, then
// residual, weight and weighted terms, the weight of every point into a buffer of its own (icp_batch_get_weights), and the
// reduction up to slot ICP_MOM_W.  Three launches with nothing else, up to five, still one download.  A batch whose kinds are all
// NONE runs the steps it ran without them.
//
// A batch may hold a covariance per point on both sides (icp_batch_set_covariances; icp_batch_estimate_covariances: ONE launch of
// batch_cov_kernel, icp_k_gicp.hip, for all clouds of the sides asked for -- the rule, which numpy reproduces bit for bit, is stated
// in include/icp_mi355x.h).  icp_batch_begin then takes a third metric, ICP_GENERALIZED (plane-to-plane): the steps always run
// deferred with the point-to-point matching launch and batch_gicp_moments in batch_trim_moments' place -- the same decision, a match
// whose det(Cq + Rc Cp Rc^T) is not finite and > 0 rejected too, then the terms of the 6 x 6 system into a plane pass's slots --
// and every pair's HostLoop solves as for point-to-plane.  Rc, the rotation of every motion applied to the cloud a pass matches
// on, is composed on the host as icp_batch_state composes T and travels with the step's control words (9 doubles per pair).
// Three launches, up to five, one download.  The other metrics of such a batch run the steps they ran without covariances.
//
// A batch may also hold one intensity per point on both sides, one intensity gradient per model point and one weight per pair
// (icp_batch_set_intensities, icp_batch_estimate_intensity_gradients: ONE launch of batch_intensity_gradient_kernel, icp_k_color.hip,
// for all models -- the rule is stated in include/icp_mi355x.h and reproduced bit for bit in numpy).  icp_batch_begin then takes a
// fourth metric, ICP_COLORED: the generalized metric's route with batch_color_moments in batch_gicp_moments' place -- the same
// decision, then the geometric and the photometric terms of the 6 x 6 system into a plane pass's slots; every pair's HostLoop is
// begun as a point-to-plane loop.  The other metrics of such a batch run the steps they ran without intensities.
//
// And it may hold a unit normal per point on both sides (icp_batch_estimate_point_normals, icp_batch_set_point_normals: what the
// descriptors are computed from).  icp_batch_begin then takes a fifth metric, ICP_SYMMETRIC (Rusinkiewicz, SIGGRAPH 2019): the
// generalized metric's route with batch_sym_moments (icp_k_sym.hip) in batch_gicp_moments' place -- the same decision, then the
// terms of the symmetrized point-to-plane system along n_p + n_q into a plane pass's slots, the moving normal turned by the step's
// Rc as the generalized metric turns the covariances; every pair's HostLoop is begun as a point-to-plane loop that solves by
// icp::solve_symmetric (HostLoop::symmetric: two half rotations).  New point normals discard a symmetric loop, and no other.
//
//   batch kind             launches of a step
//   symmetric metric       nn_match_batch<DEFER>, [nn_match_batch_rev,] [batch_trim_select,] batch_sym_moments<MUTUAL?>, batch_finalize_kernel
//   colored metric         nn_match_batch<DEFER>, [nn_match_batch_rev,] [batch_trim_select,] batch_color_moments<MUTUAL?>, batch_finalize_kernel
//   generalized metric     nn_match_batch<DEFER>, [nn_match_batch_rev,] [batch_trim_select,] batch_gicp_moments<MUTUAL?>, batch_finalize_kernel
//   any robust pair        nn_match_batch<DEFER>, [nn_match_batch_rev,] [batch_trim_select,] batch_robust_moments<MUTUAL?>, batch_finalize_kernel
//   any reciprocal pair    nn_match_batch<DEFER>, nn_match_batch_rev, [batch_trim_select,] batch_trim_moments<MUTUAL>, batch_finalize_kernel
//   trims only             nn_match_batch<DEFER>, batch_trim_select, batch_trim_moments, batch_finalize_kernel
//   gates only / plain     nn_match_batch, batch_finalize_kernel
//
// A batch answers how well every pair is registered where it stands (icp_batch_evaluate): the loop's own matching -- the deferred
// instantiation with mode BATCH_MATCH alone, which only reads P -- into buffers of the evaluation's own, batch_eval_moments (the
// decision at the caller's distance and the ICP_EVAL_* terms), batch_finalize_kernel, and one download of ICP_NMOM doubles per
// pair: three launches, none of which writes idx, mom, tau, thr or ctl of the loop.  Fitness, inlier RMSE and the 6 x 6 information
// matrix are assembled on the host from that vector alone.  The loop does not notice the call.
//
// A batch is thinned on the device into a new batch on the same context, whose clouds are P0 and Q of the source reduced by a rule
// per cloud (the rules, which numpy reproduces bit for bit, are stated in include/icp_mi355x.h).  The three calls share one sequence
// (the thin_* functions below; the clouds and their work items: icp_batch_clouds.h):  the 2 x count clouds, their work items and
// their rules go up  ->  the call's select launches (every cloud's count, every point's output index)  ->  [D2H: 2 x count counts
// and flags, the first wait; the data-dependent refusals; the new batch is laid out and allocated as icp_batch_create does it:
// lay_out + allocate]  ->  the call's compact launch into the new, zeroed planes  ->  P0 -> P  ->  the second wait, which brings
// the optional outputs.  Two waits; the source is only read, its loop does not notice, the temporaries live for the call, and no
// output array is written before the call can no longer be refused.
//   icp_batch_downsample        one point per occupied voxel: batch_voxel_keys, _group, _rank  ->  batch_voxel_compact (the centroids)
//   icp_batch_remove_outliers   a statistical or a radius rule: batch_outlier_scan, _decide  ->  batch_outlier_compact (the kept points' bytes)
//   icp_batch_select_keypoints  ISS keypoints (icp_k_keypoint.hip): batch_iss_saliency, batch_iss_select, batch_keypoint_rank  ->
//                               batch_keypoint_compact (coordinates, and the kept points' descriptors where the source holds descriptors,
//                               so that matching and RANSAC or FGR run on a few hundred points per cloud)
//   icp_batch_segment_plane     the dominant plane of every cloud, removed or kept (icp_k_segment.hip): the hypotheses are drawn and solved
//                               on the host from the downloaded clouds, as the RANSAC's are, and scored by batch_plane_score, kPlaneChunk
//                               per cloud and launch; batch_plane_refit, the eigenvector on the host, batch_plane_decide  ->  the outlier
//                               call's compaction.  Three more waits than the others: the clouds, the counts, the refit's moments
//
// A start pose for pairs in unknown relative pose (global registration; the rules, which numpy reproduces bit for bit, are stated in
// include/icp_mi355x.h; kernels: icp_k_feat.hip): icp_batch_compute_features (batch_spfh_kernel -> batch_fpfh_kernel, one block
// per 64 points of every cloud of both sides: a 33-bin FPFH per point, kept on the device)  ->  icp_batch_match_features
// (batch_feature_match twice, the sides swapped; fwd and rev come down, kept and every pair's correspondence list are made on
// the host and go back up)  ->  icp_batch_ransac (the hypotheses are drawn, screened and solved on the host -- icp::solve_rigid --
// and scored by batch_score_transforms, kRansacChunk hypotheses of every pair per launch; the winner is refitted on its inliers and
// scored once more)  ->  icp_batch_set_initial_transforms.  icp_batch_score_transforms scores the caller's own candidates.
// icp_batch_fgr takes RANSAC's place without hypotheses: the used list of every pair is made once on the host (with the tuple test:
// RANSAC's draws and edge check) and uploaded; then per iteration FGR_CTL doubles per pair go up (T, mu, a flag), batch_fgr_terms +
// batch_fgr_finalize run over the pairs still running, the vectors come down (the one wait) and the host solves every pair's 6 x 6
// system (icp::solve_point_to_plane); a last launch at the final poses writes the weights.  All
// of them read P0 and Q and buffers of their own: the loop does not notice.
//
// The normals the descriptors are computed from are made on the device from the covariances the batch holds and kept there
// (icp_batch_estimate_point_normals; kernels: icp_k_normals.hip): [batch_centroid_kernel, ICP_ORIENT_CENTROID only]  ->
// batch_point_normals_kernel  ->  [D2H + one wait, only where an output is wanted].  icp_batch_compute_features_stored then
// describes from them: icp_batch_compute_features' host body without the upload.  The loop does not notice either call.
//
// Point-to-plane needs the model normals of every pair, in planes laid out as the models: given by the caller
// (icp_batch_set_model_normals) or made on the device by ONE neighbour launch + ONE normals launch for the whole batch
// (icp_batch_estimate_normals: knn4_batch + normals_batch_kernel, icp_k_plane.hip).  The reference estimates them once per
// program, before its loop (src/ICP_point_to_plane.cu:391-438).
//
// Whatever a batch holds per point -- covariances, intensities, gradients, point normals, descriptors, the model normals -- is a
// PointAttr, and every set and get call goes one way: attr_reserve (scan, allocate; a refusal leaves the batch untouched), the
// call's own invalidations, attr_commit (encode, copy, one wait); attr_get (the refusals, then fetch: download, one wait, decode).
// The packing is icp_batch_clouds.h's encode / decode, the clouds' own included.  Everything the batch owns -- DevBuf, PinnedBuf,
// Event, Staged (icp_ctx.h) -- frees itself: icp_batch_destroy is `delete`.
//
// Every pair runs its own icp::HostLoop, the single-pair loop's host half (icp_host_loop.cpp): the same stop rule, the same
// composition of T, the same err series.  A pass of a pair is what loop_enqueue_body (icp_loop.cpp) makes of it: the motion
// solved by the previous pass is applied in the front of the launch (note_applied when it is enqueued), and the loop's last,
// error-only pass matches nothing.  The reference runs that loop once per program (src/ICP_point_to_point.cu:295-423,
// src/ICP_CPU.c:217-271; point-to-plane src/ICP_point_to_plane.cu:517-631).
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/icp_mi355x_diag.h"
#include "icp_batch_clouds.h"
#include "icp_ctx.h"
#include "icp_host_math.h"

// a value per point that a batch holds for one or both sides (0: the moving clouds, 1: the models)
struct __attribute__((visibility("hidden"))) PointAttr {
    const char* noun;                        // what a refusal calls the values
    icp::Format fmt;                         // how the device holds them
    bool zero_new = false;                   // new room is zeroed, so that the padding between the clouds is never random
    DevBuf buf[2];
    bool have[2] = {false, false};
    PointAttr(const char* n, icp::Format f, bool z = false) : noun(n), fmt(f), zero_new(z) {}
};

struct __attribute__((visibility("hidden"))) icp_batch {   // (the public header only names it, as icp_ctx)
    icp_ctx* ctx = nullptr;
    int count = 0;
    int prec = ICP_F32;
    size_t esize = sizeof(float);
    std::vector<int64_t> moff;               // the caller's moving offsets: the layout of get_moving / get_indices
    std::vector<int64_t> qoff;               // the caller's model offsets: the layout of the normals and the neighbours
    std::vector<icp::BatchPair> pairs;       // where each pair lives on the device
    int n_items = 0;
    long long p_plane = 0, q_plane = 0;      // elements per SoA plane of the moving / model clouds
    DevBuf P, P0, Q, items, pairs_d, ctl, idx[2], partials, mom;   // P0: the moving clouds as uploaded (icp_batch_begin)
    // a value per point of one or both sides (PointAttr: the two buffers, whether each side holds the values, the packed format).
    // N: point-to-plane's model normals, 3 planes in the batch's precision (model-only, as grad: side 0 is never used)
    PointAttr N{"model normals", {3, icp::PLANES, sizeof(float)}};
    DevBuf q_items, nbr;                     // the model's work items, 4 neighbours per model point (icp_batch_estimate_normals)
    int n_q_items = 0;
    DevBuf thr;                              // the gate: every pair's squared maximum correspondence distance, in the batch's precision
    bool gated = false;                      // the batch holds thresholds (icp_batch_set_max_distance): the passes run the gated kernels
    DevBuf trim_rank, tau, dist;             // trimming: every pair's rank K (0: not trimmed), its K-th smallest squared distance of the latest matching pass, every point's winning squared distance (laid out as idx)
    bool trimmed = false;                    // a pair keeps a share < 1 (icp_batch_set_trim): the passes run the deferred route
    std::vector<double> rho;                 // the shares as given (empty: none)
    std::vector<int> rank;                   // K_p = ceil(rho_p n_p) in [1, n_p]
    std::vector<char> tau_seen;              // the pair has completed a matching pass since icp_batch_begin
    DevBuf recip_d, rev;                     // reciprocity: every pair's flag (uint8), every model point's nearest moving point of its pair's most recent matching pass (q_plane int32, laid out as the models; with trimming's dist)
    bool reciprocal = false;                 // a pair's flag is set (icp_batch_set_reciprocal): the passes run the deferred route with the reverse search
    std::vector<uint8_t> recip;              // the flags as given (empty: none)
    DevBuf rob_kind, rob_k, rob_k2, weights; // robust kernels: every pair's kind (int), k and k * k (double); every moving point's weight of its pair's most recent matching pass (p_plane doubles, laid out as idx; allocated with the first kernel)
    bool robust = false;                     // a pair's kind is not NONE (icp_batch_set_robust): the passes run the deferred route with batch_robust_moments
    std::vector<int> rkind;                  // the kinds as given (empty: none)
    std::vector<double> rscale;              // the scales (0 for a NONE pair)
    DevBuf rt0, init_kind, init_flag;        // initial transforms: R, t of every pair in the batch's precision, BATCH_INIT_APPLY / _COPY, the start cloud is not finite
    bool have_init = false;                  // the batch holds initial transforms (icp_batch_set_initial_transforms)
    std::vector<double> T0F;                 // count x 16: every pair's transform as rounded to the batch's precision, read back in double
    std::vector<char> init_copy;             // the pair's 16 doubles were exactly the identity: its cloud is copied, its T is the loop's
    PointAttr cov{"covariances", {6, icp::PLANES, sizeof(double)}};   // the generalized metric: 6 planes of doubles (xx, xy, xz, yy, yz, zz), laid out as the clouds (icp_batch_set_covariances, icp_batch_estimate_covariances)
    Staged cov_args;                         // icp_batch_estimate_covariances: the clouds, their work items and their k of the latest call, as one buffer; recorded behind the call's launch
    std::vector<double> rot;                 // count x 9: the rotation every pair's most recent matching pass of a generalized loop rotated its moving covariances by
    size_t rot_off = 0;                      // where those rotations sit in ctl and h_ctl, behind the modes (copied by a generalized step only)
    PointAttr inten{"intensities", {1, icp::PLANES, sizeof(double)}};   // the colored metric: one plane of doubles, laid out as the clouds (icp_batch_set_intensities)
    PointAttr grad{"intensity gradients", {3, icp::PLANES, sizeof(double)}};   // ... of the models: 3 planes of doubles (icp_batch_set_intensity_gradients, icp_batch_estimate_intensity_gradients); new model intensities or normals discard them
    Staged grad_k;                           // icp_batch_estimate_intensity_gradients: every model's k of the latest call; recorded behind the call's launch
    DevBuf color_w;                          // every pair's lambda (double), uploaded by icp_batch_set_color_weight or by the first colored begin
    std::vector<double> lambda;              // the weights as given (empty: ICP_COLOR_LAMBDA_DEFAULT for every pair)
    bool color_w_set = false;                // color_w holds what lambda says
    int metric = ICP_POINT_TO_POINT;         // of the loop under way
    PinnedBuf h_ctl;                         // R, t of every pair (12 values of the precision), then its mode (int)
    PinnedBuf h_mom;                         // count x ICP_NMOM doubles
    size_t rt_bytes = 0, ctl_bytes = 0;
    bool begun = false;                      // a loop is under way (or has ended) and its state is readable
    long long steps = 0;                     // steps since icp_batch_begin: step k matches into idx[k & 1]
    std::vector<icp::HostLoop> H;
    std::vector<int> status;                 // ICP_OK, or the rc that ended the pair's loop
    std::vector<int> last_match;             // idx buffer of the pair's most recent matching pass
    std::vector<int> applied_buf;            // idx buffer of the pass whose motion the pair applied last
    std::vector<char> mom_seen;              // the pair's HostLoop has advanced on its row of h_mom since icp_batch_begin
    std::vector<char> refused;               // icp_batch_begin refused the pair's start cloud (not finite): it is not evaluated
    // icp_batch_evaluate: buffers of its own, allocated by the first call (the loop's are never written)
    DevBuf e_mode, e_thr, e_idx, e_dist, e_partials, e_mom;
    PinnedBuf h_eval;                        // count x ICP_NMOM doubles, the vectors of the latest evaluation
    bool eval_seen = false;                  // h_eval holds an evaluation
    // global registration (icp_batch_compute_features, _match_features, _score_transforms, _ransac)
    PointAttr feat{"descriptors", {ICP_FEATURE_BINS, icp::ROWS, sizeof(double)}};   // ICP_FEATURE_BINS doubles at (the cloud's offset + i) * ICP_FEATURE_BINS
    PointAttr pnrm{"point normals", {3, icp::PLANES, sizeof(double)}, true};   // what the descriptors are computed from: 3 planes of doubles, laid out as the clouds (icp_batch_estimate_point_normals, icp_batch_set_point_normals; not the model normals N)
    Staged nrm_args, nrm_view;               // icp_batch_estimate_point_normals: the 2 * count clouds and their work items (made once: the layout never changes); 3 doubles per cloud, the viewpoints of the latest call, recorded behind their upload
    DevBuf nrm_cent;                         // ... and the centroids of the latest ICP_ORIENT_CENTROID call
    size_t nrm_off_items = 0;                // where the items start in nrm_args
    int n_nrm_items = 0;                     // 0: nrm_args is not made yet
    bool have_cent = false;                  // nrm_cent holds the centroids of an ICP_ORIENT_CENTROID call
    DevBuf f_fwd, f_rev, f_kept;             // the matches: fwd and kept laid out as idx, rev as the models
    DevBuf f_ci, f_cj, f_cn;                 // every pair's correspondence list (moving index, model index: int32 at p_off + e) and its length (int per pair)
    bool have_match = false;
    std::vector<std::vector<int32_t>> corr_i, corr_j;   // the lists on the host
    DevBuf s_cand, s_valid, s_thr, s_counts; // a scoring launch: candidates, their valid bytes, thresholds, counts
    int rs_hyp = 0;                          // the last icp_batch_ransac run: hypotheses per pair, then per pair and hypothesis ...
    std::vector<int32_t> rs_triples, rs_counts;   // ... the three list positions, the count (-1: invalid)
    std::vector<uint8_t> rs_valid;
    std::vector<double> rs_T;                // ... and the pose, 16 doubles
    // Fast Global Registration (icp_batch_fgr): buffers of its own, allocated by the first call (the loop's are never written)
    DevBuf g_ui, g_uj, g_items, g_item0;     // every pair's used list (int32 at p_off + e), its work items and where each pair's items start (count + 1 ints)
    DevBuf g_ctl, g_partials, g_mom, g_w;    // FGR_CTL doubles per pair, a row per item, a vector per pair, every moving point's weight (p_plane doubles, laid out as idx)
    PinnedBuf h_fgr;                         // count x FGR_CTL doubles (what g_ctl is copied from), then count x ICP_NMOM (what g_mom comes down into)
    int fg_iter = 0;                         // the last icp_batch_fgr run: iterations, then per pair ...
    std::vector<std::vector<int32_t>> fg_used;   // ... the used list positions
    std::vector<double> fg_mu, fg_mom, fg_T; // ... and per iteration mu, the vector (ICP_NMOM) and the pose the terms were formed at (16)
    double fg_sec[4] = {0, 0, 0, 0};         // ... and the host's seconds in the iterations: enqueue (fill, upload, launches, download), wait, solve; the iterations run
    // plane segmentation (icp_batch_segment_plane): the last call's hypotheses per cloud (2 * count, the moving clouds first; empty
    // for a cloud that was not searched), for icp_diag_batch_segment
    bool sg_seen = false;
    std::vector<std::vector<int32_t>> sg_triples, sg_counts;   // 3 per hypothesis: the point indices; the count (-1: invalid)
    std::vector<std::vector<uint8_t>> sg_valid;
    std::vector<std::vector<double>> sg_planes;                // 4 per hypothesis
};

namespace {

// which cloud a refusal speaks of: ": pair 3, model"
std::string where(int p, int side) { return ": pair " + std::to_string(p) + (side ? ", model" : ", moving cloud"); }

// 8, 16 or 32: the register capacity of a neighbour list that holds k entries (the kernels' cap)
int list_cap(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// a cloud's k of a neighbourhood call (covariances, intensity gradients, descriptors): in the range, and the cloud has k + 1
// points; cap grows to the list that holds k.  (A statistical outlier rule's k starts at 1 and a keypoint rule has none: their own.)
int check_k(int kk, int points, const char* one, const char* many, const std::string& at, int& cap)
{
    if (kk < ICP_COV_MIN_NEIGHBOURS || kk > ICP_COV_MAX_NEIGHBOURS)
        return fail(ICP_ERR_INVALID, std::string("the neighbours (k) of ") + one + " must lie in [ICP_COV_MIN_NEIGHBOURS, ICP_COV_MAX_NEIGHBOURS]" + at);
    if (points < kk + 1) return fail(ICP_ERR_INVALID, std::string(many) + " from k neighbours need a cloud of at least k + 1 points" + at);
    cap = std::max(cap, list_cap(kk));
    return ICP_OK;
}

// elements per plane of the moving clouds (sd == 0) / of the models
size_t plane_elems(const icp_batch* b, int sd) { return (size_t)(sd ? b->q_plane : b->p_plane); }

bool running(const icp_batch* b, int p) { return b->begun && !b->H[p].done && b->status[p] == ICP_OK; }

int count_running(const icp_batch* b)
{
    int k = 0;
    for (int p = 0; p < b->count; ++p) k += running(b, p) ? 1 : 0;
    return k;
}

// a batch borrows the context's device and stream -- never in the middle of the context's own pass
int ctx_ready(icp_ctx* c)
{
    if (int rc = use(c)) return rc;
    if (c->loop.pending) return fail(ICP_ERR_STATE, "the context has an enqueued pass that is not completed (icp_loop_complete first)");
    return ICP_OK;
}

int ready(icp_batch* b)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    return ctx_ready(b->ctx);
}

// what icp_batch_begin forgets of the loop before (icp_batch_create: the same, of none)
void reset_loop_state(icp_batch* b)
{
    b->status.assign((size_t)b->count, ICP_OK);
    b->last_match.assign((size_t)b->count, 0);
    b->applied_buf.assign((size_t)b->count, 0);
    b->mom_seen.assign((size_t)b->count, 0);
    b->tau_seen.assign((size_t)b->count, 0);
    b->refused.assign((size_t)b->count, 0);
}

int check_offsets(const int64_t* off, int count, const char* what)
{
    if (off[0] != 0) return fail(ICP_ERR_INVALID, std::string(what) + " offsets must start at 0");
    for (int p = 0; p < count; ++p) {
        const int64_t len = off[p + 1] - off[p];
        if (len < 1) return fail(ICP_ERR_INVALID, std::string(what) + " offsets must be strictly increasing (every cloud has >= 1 point)");
        if (len > ICP_BATCH_MAX_POINTS) return fail(ICP_ERR_INVALID, std::string("a ") + what + " cloud has more than ICP_BATCH_MAX_POINTS points");
    }
    return ICP_OK;
}

template <typename F>
bool all_finite(const void* aos, int64_t points)
{
    const F* a = static_cast<const F*>(aos);
    for (int64_t i = 0; i < 3 * points; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

using icp::Side;

Side side(const icp_batch* b, bool model) { return icp::make_side(b->pairs, model ? b->qoff.data() : b->moff.data(), model ? b->q_plane : b->p_plane, model); }

// the clouds themselves: 3 planes of the batch's precision
icp::Format cloud_format(const icp_batch* b) { return icp::Format{3, icp::PLANES, b->esize}; }

// packed values (icp_batch_clouds.h) on their way down: download enqueues the copies of the sides whose output pointer is given,
// the caller waits, deliver lays them out as the caller's
struct Download {
    std::vector<char> h[2];
};

int download(icp_batch* b, const icp::Format& f, const void* const dev[2], void* const out[2], Download& d)
{
    for (int sd = 0; sd < 2; ++sd)
        if (out[sd]) {
            d.h[sd].resize(f.bytes((long long)plane_elems(b, sd)));
            HIP_TRY(hipMemcpyAsync(d.h[sd].data(), dev[sd], d.h[sd].size(), hipMemcpyDeviceToHost, b->ctx->stream));
        }
    return ICP_OK;
}

void deliver(const icp_batch* b, const icp::Format& f, const Download& d, void* const out[2])
{
    for (int sd = 0; sd < 2; ++sd)
        if (out[sd]) icp::decode(f, side(b, sd != 0), d.h[sd].data(), out[sd]);
}

// ... both, around the one wait
int fetch(icp_batch* b, const icp::Format& f, const void* const dev[2], void* const out[2])
{
    Download d;
    if (int rc = download(b, f, dev, out, d)) return rc;
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    deliver(b, f, d, out);
    return ICP_OK;
}

int fetch(icp_batch* b, const PointAttr& a, void* const out[2])
{
    const void* const dev[2] = {a.buf[0].p, a.buf[1].p};
    return fetch(b, a.fmt, dev, out);
}

int fetch_clouds(icp_batch* b, const void* dev_p, const void* dev_q, void* out_p, void* out_q)
{
    const void* const dev[2] = {dev_p, dev_q};
    void* const out[2] = {out_p, out_q};
    return fetch(b, cloud_format(b), dev, out);
}

// the caller's values of one side -> `host`, packed, and on their way to `dev`.  `host` must outlive the copy: the caller waits
int enqueue_packed(icp_batch* b, const icp::Format& f, const void* own, bool model, void* dev, std::vector<char>& host)
{
    icp::encode(f, side(b, model), own, host);
    HIP_TRY(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, b->ctx->stream));
    return ICP_OK;
}

constexpr const char* kPointNormalsFirst = " (icp_batch_estimate_point_normals or icp_batch_set_point_normals first)";

// ---- a value per point (PointAttr).  A set call is  attr_reserve, [what the call invalidates,] attr_commit;  a get call is attr_get.
size_t attr_bytes(const icp_batch* b, const PointAttr& a, int sd) { return a.fmt.bytes((long long)plane_elems(b, sd)); }

// room for one side's values
int attr_room(icp_batch* b, PointAttr& a, int sd)
{
    const size_t bytes = attr_bytes(b, a, sd);
    if (!a.zero_new) {
        HIP_TRY(a.buf[sd].ensure(bytes));
        return ICP_OK;
    }
    if (a.buf[sd].p && bytes <= a.buf[sd].cap) return ICP_OK;
    HIP_TRY(a.buf[sd].ensure(bytes));
    HIP_TRY(hipMemsetAsync(a.buf[sd].p, 0, bytes, b->ctx->stream));
    return ICP_OK;
}

// the values given (doubles) are finite -- `one`, not NULL, is what the refusal calls a value -- and the sides given have room.
// A refusal leaves the batch as it was
int attr_reserve(icp_batch* b, PointAttr& a, const void* const given[2], const char* one)
{
    for (int sd = 0; one && sd < 2; ++sd) {
        if (!given[sd]) continue;
        const double* v = static_cast<const double*>(given[sd]);
        const int64_t* off = sd ? b->qoff.data() : b->moff.data();
        const int w = a.fmt.width;
        for (int p = 0; p < b->count; ++p)
            for (int64_t i = w * off[p]; i < w * off[p + 1]; ++i)
                if (!std::isfinite(v[i])) return fail(ICP_ERR_INVALID, std::string(one) + " has a NaN or an infinite value" + where(p, sd));
    }
    for (int sd = 0; sd < 2; ++sd)
        if (given[sd])
            if (int rc = attr_room(b, a, sd)) return rc;
    return ICP_OK;
}

// the sides given hold nothing, are encoded and copied; one wait; they hold the values
int attr_commit(icp_batch* b, PointAttr& a, const void* const given[2])
{
    std::vector<char> h[2];
    for (int sd = 0; sd < 2; ++sd) {
        if (!given[sd]) continue;
        a.have[sd] = false;
        if (int rc = enqueue_packed(b, a.fmt, given[sd], sd != 0, a.buf[sd].p, h[sd])) return rc;
    }
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vectors go)
    for (int sd = 0; sd < 2; ++sd)
        if (given[sd]) a.have[sd] = true;
    return ICP_OK;
}

// "the batch holds no point normals of the models (... first)", for the first side asked for that holds none
int attr_held(const PointAttr& a, const bool asked[2], const char* hint)
{
    for (int sd = 0; sd < 2; ++sd)
        if (asked[sd] && !a.have[sd])
            return fail(ICP_ERR_STATE, std::string("the batch holds no ") + a.noun + " of the " + (sd ? "models" : "moving clouds") + hint);
    return ICP_OK;
}

int attr_get(icp_batch* b, const PointAttr& a, void* const out[2], const char* hint)
{
    if (int rc = ready(b)) return rc;
    if (!out[0] && !out[1]) return fail(ICP_ERR_INVALID, "output pointer == NULL");
    const bool asked[2] = {out[0] != nullptr, out[1] != nullptr};
    if (int rc = attr_held(a, asked, hint)) return rc;
    return fetch(b, a, out);
}

// element i of an array in the batch's precision: written from a double (rounded once), read back as a double
void put_scalar(const icp_batch* b, void* dst, size_t i, double v)
{
    const float f = (float)v;
    std::memcpy(static_cast<char*>(dst) + i * b->esize, b->prec == ICP_F64 ? (const void*)&v : (const void*)&f, b->esize);
}

double get_scalar(const icp_batch* b, const void* src, size_t i)
{
    double d = 0.0;
    float f = 0.0f;
    std::memcpy(b->prec == ICP_F64 ? (void*)&d : (void*)&f, static_cast<const char*>(src) + i * b->esize, b->esize);
    return b->prec == ICP_F64 ? d : (double)f;
}

// the work items of the moving clouds (of the models): BATCH_ITEM points of one pair, cut from that pair's first point
std::vector<icp::BatchItem> work_items(const icp_batch* b, bool model)
{
    std::vector<icp::BatchItem> items;
    for (int p = 0; p < b->count; ++p) {
        const int len = model ? b->pairs[p].m : b->pairs[p].n;
        for (int first = 0; first < len; first += icp::BATCH_ITEM)
            items.push_back(icp::BatchItem{p, first, std::min(icp::BATCH_ITEM, len - first), 0});
    }
    return items;
}

// ... of the models, on the device (q_items, n_q_items): made once, by whichever of the normals and the reverse search asks first
int ensure_model_items(icp_batch* b)
{
    if (b->n_q_items != 0) return ICP_OK;
    const std::vector<icp::BatchItem> items = work_items(b, true);
    if (items.size() > (size_t)INT_MAX) return fail(ICP_ERR_INVALID, "too many work items for one batch");
    HIP_TRY(b->q_items.ensure(items.size() * sizeof(icp::BatchItem)));
    HIP_TRY(hipMemcpyAsync(b->q_items.p, items.data(), items.size() * sizeof(icp::BatchItem), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (items: a host vector)
    b->n_q_items = (int)items.size();
    return ICP_OK;
}

template <typename F>
void put_rt(void* dst, const double* R, const double* t)
{
    F* o = static_cast<F*>(dst);
    for (int k = 0; k < 9; ++k) o[k] = (F)R[k];
    for (int k = 0; k < 3; ++k) o[9 + k] = (F)t[k];
}

// a new, empty batch on c: the layout two offset arrays give it -- where every pair's clouds start in the planes, its work items
// (host only; icp_batch_create and icp_batch_downsample both start here)
int lay_out(icp_ctx* c, int count, int precision, const int64_t* moving_off, const int64_t* model_off, icp_batch** out)
{
    icp_batch* b = new (std::nothrow) icp_batch();
    if (!b) return fail(ICP_ERR_NOMEM, "batch");
    b->ctx = c;
    b->count = count;
    b->prec = precision;
    b->esize = precision == ICP_F64 ? sizeof(double) : sizeof(float);
    b->N.fmt.esize = b->esize;
    b->moff.assign(moving_off, moving_off + count + 1);
    b->qoff.assign(model_off, model_off + count + 1);
    b->pairs.resize((size_t)count);
    long long items = 0;
    for (int p = 0; p < count; ++p) {
        icp::BatchPair& pr = b->pairs[p];
        pr.n = (int)(moving_off[p + 1] - moving_off[p]);
        pr.m = (int)(model_off[p + 1] - model_off[p]);
        pr.p_off = b->p_plane;
        pr.q_off = b->q_plane;
        b->p_plane += icp::round_up(pr.n, icp::BATCH_ALIGN);
        b->q_plane += icp::round_up(pr.m, icp::BATCH_ALIGN);
        pr.item0 = (int)std::min<long long>(items, INT_MAX);
        items += (pr.n + icp::BATCH_ITEM - 1) / icp::BATCH_ITEM;
        pr.item1 = (int)std::min<long long>(items, INT_MAX);
    }
    if (items > INT_MAX) {
        delete b;
        return fail(ICP_ERR_INVALID, "too many work items for one batch");
    }
    b->n_items = (int)items;
    b->H.resize((size_t)count);
    reset_loop_state(b);
    *out = b;
    return ICP_OK;
}

// everything of a laid-out batch but its clouds: the planes (not filled), the work items and the pairs on the device, the loop's
// buffers.  Enqueues the copy of `items`, which must outlive it: the caller synchronises.
int allocate(icp_batch* b, std::vector<icp::BatchItem>& items)
{
    icp_ctx* c = b->ctx;
    const size_t pb = 3 * (size_t)b->p_plane * b->esize, qb = 3 * (size_t)b->q_plane * b->esize;
    HIP_TRY(b->P.ensure(pb));
    HIP_TRY(b->P0.ensure(pb));
    HIP_TRY(b->Q.ensure(qb));
    items = work_items(b, false);
    HIP_TRY(b->items.ensure(items.size() * sizeof(icp::BatchItem)));
    HIP_TRY(b->pairs_d.ensure(b->pairs.size() * sizeof(icp::BatchPair)));
    HIP_TRY(hipMemcpyAsync(b->items.p, items.data(), items.size() * sizeof(icp::BatchItem), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b->pairs_d.p, b->pairs.data(), b->pairs.size() * sizeof(icp::BatchPair), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(b->idx[k].ensure((size_t)b->p_plane * sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(b->idx[k].p, 0, (size_t)b->p_plane * sizeof(int32_t), c->stream));
    }
    HIP_TRY(b->partials.ensure((size_t)b->n_items * ICP_NMOM * sizeof(double)));
    HIP_TRY(b->mom.ensure((size_t)b->count * ICP_NMOM * sizeof(double)));
    b->rt_bytes = (size_t)b->count * 12 * b->esize;
    b->ctl_bytes = b->rt_bytes + (size_t)b->count * sizeof(int);
    b->rot_off = (b->ctl_bytes + 7) / 8 * 8;   // (room for 9 doubles per pair behind the control words: a generalized step's rotations)
    const size_t ctl_room = b->rot_off + (size_t)b->count * 9 * sizeof(double);
    HIP_TRY(b->ctl.ensure(ctl_room));
    HIP_TRY(b->h_ctl.ensure(ctl_room));
    std::memset(b->h_ctl.p, 0, ctl_room);
    HIP_TRY(b->h_mom.ensure((size_t)b->count * ICP_NMOM * sizeof(double)));
    return ICP_OK;
}

// the caller's clouds into the planes of an allocated batch
int upload(icp_batch* b, const void* moving, const void* model)
{
    icp_ctx* c = b->ctx;
    std::vector<icp::BatchItem> items;
    std::vector<char> ps, qs;
    int rc = allocate(b, items);
    if (rc == ICP_OK) rc = enqueue_packed(b, cloud_format(b), moving, false, b->P0.p, ps);
    if (rc == ICP_OK) rc = enqueue_packed(b, cloud_format(b), model, true, b->Q.p, qs);
    const hipError_t es = hipStreamSynchronize(c->stream);   // (always, a refusal included: before the host vectors go)
    if (rc != ICP_OK) return rc;
    HIP_TRY(es);
    HIP_TRY(hipMemcpyAsync(b->P.p, b->P0.p, 3 * (size_t)b->p_plane * b->esize, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ICP_OK;
}

// the device temporaries of one call: released when the call returns, whichever way -- after what the call enqueued has ended
// (host vectors that its copies read or write are declared before this and so outlive it)
struct Temps {
    hipStream_t st;
    DevBuf buf[16];
    explicit Temps(hipStream_t s) : st(s) {}
    ~Temps()
    {
        (void)hipStreamSynchronize(st);
        for (DevBuf& d : buf) d.release();
    }
    Temps(const Temps&) = delete;
    Temps& operator=(const Temps&) = delete;
};

// ---- thinning a batch into a new batch: what icp_batch_downsample, icp_batch_remove_outliers and icp_batch_select_keypoints share.
// A call runs  thin_begin, [its own temporaries,] thin_upload, thin_args + its select launches, thin_counts, [its refusals,]
// thin_allocate, thin_args + its compact launch, thin_download, [its own downloads,] thin_finish  -- the sequence of the head comment.
enum { T_CLOUDS, T_ITEMS, T_RULES, T_MAP, T_COUNT, T_FLAG, T_VALUE, T_OWN };   // Temps::buf of a thinning call; from T_OWN on: the call's own

struct Thin {
    icp_batch* src;
    hipStream_t st;
    int count;                               // pairs; cloud k < count: the moving cloud of pair k, cloud count + p: the model of pair p
    icp_batch* nb = nullptr;                 // the new batch, once thin_allocate has made it
    icp::CloudList cl;
    std::vector<icp::BatchItem> new_items;
    std::vector<int> flag;                   // per cloud, after thin_counts: the select launches refuse the cloud (T_FLAG; calls that have one)
    std::vector<int32_t> kept, hmap;         // per cloud, after thin_counts: its points in the new batch (T_COUNT); per point: its new index (T_MAP)
    std::vector<double> hvalue;              // per point: the call's score (T_VALUE; calls that have one)
    int32_t* map_out[2] = {nullptr, nullptr};      // the caller's arrays for hmap and hvalue, moving clouds / models (NULL: not wanted)
    double* value_out[2] = {nullptr, nullptr};
    Temps t;                                 // (last: gone first)
    explicit Thin(icp_batch* s) : src(s), st(s->ctx->stream), count(s->count), t(s->ctx->stream) {}
};

// the clouds, the work items and the temporaries every thinning call has (rule_bytes: the call's rules of all clouds; value: the call
// keeps a double per point; flag: an int per cloud)
int thin_begin(Thin& th, size_t rule_bytes, bool value, bool flag)
{
    const bool both[2] = {true, true};
    if (!icp::list_clouds(th.src->pairs, both, th.cl)) return fail(ICP_ERR_INVALID, "too many work items for one batch");
    const size_t n_clouds = th.cl.clouds.size(), tmp = (size_t)th.cl.tmp_plane;
    HIP_TRY(th.t.buf[T_CLOUDS].ensure(n_clouds * sizeof(icp::VoxelCloud)));
    HIP_TRY(th.t.buf[T_ITEMS].ensure(th.cl.items.size() * sizeof(icp::BatchItem)));
    HIP_TRY(th.t.buf[T_RULES].ensure(rule_bytes));
    if (value) HIP_TRY(th.t.buf[T_VALUE].ensure(tmp * sizeof(double)));
    HIP_TRY(th.t.buf[T_MAP].ensure(tmp * sizeof(int32_t)));
    HIP_TRY(th.t.buf[T_COUNT].ensure(n_clouds * sizeof(int32_t)));
    if (flag) HIP_TRY(th.t.buf[T_FLAG].ensure(n_clouds * sizeof(int)));
    return ICP_OK;
}

int thin_upload(Thin& th, const void* rules, size_t rule_bytes)
{
    HIP_TRY(hipMemcpyAsync(th.t.buf[T_CLOUDS].p, th.cl.clouds.data(), th.cl.clouds.size() * sizeof(icp::VoxelCloud), hipMemcpyHostToDevice, th.st));
    HIP_TRY(hipMemcpyAsync(th.t.buf[T_ITEMS].p, th.cl.items.data(), th.cl.items.size() * sizeof(icp::BatchItem), hipMemcpyHostToDevice, th.st));
    HIP_TRY(hipMemcpyAsync(th.t.buf[T_RULES].p, rules, rule_bytes, hipMemcpyHostToDevice, th.st));
    return ICP_OK;
}

// what BatchVoxelArgs, BatchOutlierArgs and BatchKeypointArgs have in common; dst: once the new batch is there
template <typename Args>
void thin_args(Args& a, const Thin& th)
{
    a.precision = th.src->prec;
    a.clouds = (const icp::VoxelCloud*)th.t.buf[T_CLOUDS].p;
    a.n_clouds = (int)th.cl.clouds.size();
    a.items = (const icp::BatchItem*)th.t.buf[T_ITEMS].p;
    a.n_items = (int)th.cl.items.size();
    a.src[0] = th.src->P0.p;
    a.src[1] = th.src->Q.p;
    a.src_plane[0] = th.src->p_plane;
    a.src_plane[1] = th.src->q_plane;
    a.tmp_plane = th.cl.tmp_plane;
    a.map = (int32_t*)th.t.buf[T_MAP].p;
    a.count = (int32_t*)th.t.buf[T_COUNT].p;
    if (!th.nb) return;
    a.dst[0] = th.nb->P0.p;
    a.dst[1] = th.nb->Q.p;
    a.dst_plane[0] = th.nb->p_plane;
    a.dst_plane[1] = th.nb->q_plane;
}

// the flags (calls that have them) and the counts of the select launches come down: the first wait
int thin_counts(Thin& th)
{
    th.flag.assign(th.cl.clouds.size(), 0);
    th.kept.resize(th.cl.clouds.size());
    if (th.t.buf[T_FLAG].p) HIP_TRY(hipMemcpyAsync(th.flag.data(), th.t.buf[T_FLAG].p, th.flag.size() * sizeof(int), hipMemcpyDeviceToHost, th.st));
    HIP_TRY(hipMemcpyAsync(th.kept.data(), th.t.buf[T_COUNT].p, th.kept.size() * sizeof(int32_t), hipMemcpyDeviceToHost, th.st));
    HIP_TRY(hipStreamSynchronize(th.st));   // the first wait: the new batch's layout needs every cloud's count
    return ICP_OK;
}

// the new batch from the counts (every one in [1, the cloud's points]: the caller has checked), its planes zeroed, and where every
// cloud goes in it on the device; *made: the new batch as far as it got (the caller's caller releases it on failure)
int thin_allocate(Thin& th, icp_batch** made)
{
    const int count = th.count;
    std::vector<int64_t> moff((size_t)count + 1, 0), qoff((size_t)count + 1, 0);
    for (int p = 0; p < count; ++p) {
        moff[p + 1] = moff[p] + th.kept[p];
        qoff[p + 1] = qoff[p] + th.kept[(size_t)count + p];
    }
    if (int rc = lay_out(th.src->ctx, count, th.src->prec, moff.data(), qoff.data(), made)) return rc;
    icp_batch* nb = th.nb = *made;
    if (int rc = allocate(nb, th.new_items)) return rc;
    for (int k = 0; k < 2 * count; ++k) th.cl.clouds[k].dst_off = k < count ? nb->pairs[k].p_off : nb->pairs[k - count].q_off;
    HIP_TRY(hipMemcpyAsync(th.t.buf[T_CLOUDS].p, th.cl.clouds.data(), th.cl.clouds.size() * sizeof(icp::VoxelCloud), hipMemcpyHostToDevice, th.st));
    HIP_TRY(hipMemsetAsync(nb->P0.p, 0, 3 * plane_elems(nb, 0) * nb->esize, th.st));   // (the padding between the clouds: all-zero bytes, as an upload leaves it)
    HIP_TRY(hipMemsetAsync(nb->Q.p, 0, 3 * plane_elems(nb, 1) * nb->esize, th.st));
    return ICP_OK;
}

// behind the compact launch: the new batch's P, and the per-point outputs that are wanted start their way down
int thin_download(Thin& th)
{
    HIP_TRY(hipMemcpyAsync(th.nb->P.p, th.nb->P0.p, 3 * plane_elems(th.nb, 0) * th.nb->esize, hipMemcpyDeviceToDevice, th.st));
    if (th.map_out[0] || th.map_out[1]) {
        th.hmap.resize((size_t)th.cl.tmp_plane);
        HIP_TRY(hipMemcpyAsync(th.hmap.data(), th.t.buf[T_MAP].p, th.hmap.size() * sizeof(int32_t), hipMemcpyDeviceToHost, th.st));
    }
    if (th.value_out[0] || th.value_out[1]) {
        th.hvalue.resize((size_t)th.cl.tmp_plane);
        HIP_TRY(hipMemcpyAsync(th.hvalue.data(), th.t.buf[T_VALUE].p, th.hvalue.size() * sizeof(double), hipMemcpyDeviceToHost, th.st));
    }
    return ICP_OK;
}

// the second wait, then every cloud's stretch of the per-point outputs into the caller's arrays
int thin_finish(Thin& th)
{
    HIP_TRY(hipStreamSynchronize(th.st));   // the second wait: the host vectors go, the temporaries are freed
    for (size_t k = 0; k < th.cl.clouds.size(); ++k) {
        const icp::VoxelCloud& c = th.cl.clouds[k];
        const size_t p = k - (size_t)c.side * th.count;
        const int64_t at = c.side ? th.src->qoff[p] : th.src->moff[p];
        if (th.map_out[c.side]) std::memcpy(th.map_out[c.side] + at, th.hmap.data() + c.tmp_off, (size_t)c.n * sizeof(int32_t));
        if (th.value_out[c.side]) std::memcpy(th.value_out[c.side] + at, th.hvalue.data() + c.tmp_off, (size_t)c.n * sizeof(double));
    }
    return ICP_OK;
}

// icp_batch_downsample after its argument checks
int downsample(icp_batch* src, const std::vector<double>& voxel, int32_t* moving_map_out, int32_t* model_map_out, icp_batch** made)
{
    enum { KEYS = T_OWN, FIRST, CENT, RANK };
    Thin th(src);
    th.map_out[0] = moving_map_out;
    th.map_out[1] = model_map_out;
    if (int rc = thin_begin(th, voxel.size() * sizeof(double), false, true)) return rc;
    const size_t tmp = (size_t)th.cl.tmp_plane;
    HIP_TRY(th.t.buf[KEYS].ensure(tmp * sizeof(unsigned long long)));
    HIP_TRY(th.t.buf[FIRST].ensure(tmp * sizeof(int32_t)));
    HIP_TRY(th.t.buf[CENT].ensure(3 * tmp * src->esize));
    HIP_TRY(th.t.buf[RANK].ensure(tmp * sizeof(int32_t)));
    if (int rc = thin_upload(th, voxel.data(), voxel.size() * sizeof(double))) return rc;
    icp::BatchVoxelArgs a{};
    thin_args(a, th);
    a.voxel = (const double*)th.t.buf[T_RULES].p;
    a.keys = (unsigned long long*)th.t.buf[KEYS].p;
    a.too_fine = (int*)th.t.buf[T_FLAG].p;
    a.first = (int32_t*)th.t.buf[FIRST].p;
    a.cent = th.t.buf[CENT].p;
    a.rank = (int32_t*)th.t.buf[RANK].p;
    HIP_TRY(icp::launch_batch_voxel_group(a, th.st));
    if (int rc = thin_counts(th)) return rc;
    for (int p = 0; p < th.count; ++p)
        for (int side = 0; side < 2; ++side)
            if (th.flag[(size_t)side * th.count + p])
                return fail(ICP_ERR_INVALID, "the voxel grid is too fine for the cloud's extent (a cell index above 2097151)" + where(p, side));
    for (int p = 0; p < th.count; ++p)
        if (th.kept[p] < 1 || th.kept[p] > src->pairs[p].n || th.kept[(size_t)th.count + p] < 1 || th.kept[(size_t)th.count + p] > src->pairs[p].m)
            return fail(ICP_ERR_HIP, "icp_batch_downsample: a cloud's cell count is out of range");   // (cannot happen: every cloud has a point)
    if (int rc = thin_allocate(th, made)) return rc;
    thin_args(a, th);
    HIP_TRY(icp::launch_batch_voxel_compact(a, th.st));
    if (int rc = thin_download(th)) return rc;
    return thin_finish(th);
}

// icp_batch_remove_outliers after its argument checks
int remove_outliers(icp_batch* src, const std::vector<icp::OutlierRule>& rules, int32_t* moving_map_out, int32_t* model_map_out,
                    double* moving_score_out, double* model_score_out, double* stats_out, icp_batch** made)
{
    enum { STATS = T_OWN };
    std::vector<double> hstats;
    Thin th(src);
    th.map_out[0] = moving_map_out;
    th.map_out[1] = model_map_out;
    th.value_out[0] = moving_score_out;
    th.value_out[1] = model_score_out;
    if (int rc = thin_begin(th, rules.size() * sizeof(icp::OutlierRule), true, true)) return rc;
    HIP_TRY(th.t.buf[STATS].ensure(4 * rules.size() * sizeof(double)));
    if (int rc = thin_upload(th, rules.data(), rules.size() * sizeof(icp::OutlierRule))) return rc;
    icp::BatchOutlierArgs a{};
    thin_args(a, th);
    a.cap = 8;
    for (const icp::OutlierRule& r : rules)
        if (r.kind == ICP_OUTLIER_STATISTICAL) a.cap = std::max(a.cap, list_cap(r.neighbours));
    a.rules = (const icp::OutlierRule*)th.t.buf[T_RULES].p;
    a.score = (double*)th.t.buf[T_VALUE].p;
    a.stats = (double*)th.t.buf[STATS].p;
    a.bad = (int*)th.t.buf[T_FLAG].p;
    HIP_TRY(icp::launch_batch_outlier_scan(a, th.st));
    if (int rc = thin_counts(th)) return rc;
    for (int p = 0; p < th.count; ++p)
        for (int side = 0; side < 2; ++side) {
            const size_t k = (size_t)side * th.count + p;
            if (th.flag[k]) return fail(ICP_ERR_INVALID, "the mean or the deviation of a cloud's neighbour distances is not finite" + where(p, side));
            if (th.kept[k] < 1) return fail(ICP_ERR_EMPTY, "the rule keeps no point of the cloud" + where(p, side));
            if (th.kept[k] > th.cl.clouds[k].n) return fail(ICP_ERR_HIP, "icp_batch_remove_outliers: a cloud's kept count is out of range");   // (cannot happen)
        }
    if (int rc = thin_allocate(th, made)) return rc;
    thin_args(a, th);
    HIP_TRY(icp::launch_batch_outlier_compact(a, th.st));
    if (int rc = thin_download(th)) return rc;
    if (stats_out) {
        hstats.resize(4 * rules.size());
        HIP_TRY(hipMemcpyAsync(hstats.data(), th.t.buf[STATS].p, hstats.size() * sizeof(double), hipMemcpyDeviceToHost, th.st));
    }
    if (int rc = thin_finish(th)) return rc;
    if (stats_out) std::memcpy(stats_out, hstats.data(), hstats.size() * sizeof(double));
    return ICP_OK;
}

// icp_batch_select_keypoints after its argument checks
int select_keypoints(icp_batch* src, const std::vector<icp::KeypointRule>& rules, int32_t* moving_map_out, int32_t* model_map_out,
                     double* moving_saliency_out, double* model_saliency_out, int32_t* count_out, icp_batch** made)
{
    Thin th(src);
    th.map_out[0] = moving_map_out;
    th.map_out[1] = model_map_out;
    th.value_out[0] = moving_saliency_out;
    th.value_out[1] = model_saliency_out;
    if (int rc = thin_begin(th, rules.size() * sizeof(icp::KeypointRule), true, false)) return rc;
    if (int rc = thin_upload(th, rules.data(), rules.size() * sizeof(icp::KeypointRule))) return rc;
    HIP_TRY(hipMemsetAsync(th.t.buf[T_VALUE].p, 0, (size_t)th.cl.tmp_plane * sizeof(double), th.st));   // (the padding between the clouds: never read, never random)
    HIP_TRY(hipMemsetAsync(th.t.buf[T_MAP].p, 0, (size_t)th.cl.tmp_plane * sizeof(int32_t), th.st));
    icp::BatchKeypointArgs a{};
    thin_args(a, th);
    a.rules = (const icp::KeypointRule*)th.t.buf[T_RULES].p;
    a.sal = (double*)th.t.buf[T_VALUE].p;
    HIP_TRY(icp::launch_batch_keypoint_select(a, th.st));
    if (int rc = thin_counts(th)) return rc;
    for (int p = 0; p < th.count; ++p)
        for (int side = 0; side < 2; ++side) {
            const size_t k = (size_t)side * th.count + p;
            if (th.kept[k] < 1) return fail(ICP_ERR_EMPTY, "the rule keeps no point of the cloud" + where(p, side));
            if (th.kept[k] > th.cl.clouds[k].n) return fail(ICP_ERR_HIP, "icp_batch_select_keypoints: a cloud's kept count is out of range");   // (cannot happen)
        }
    if (int rc = thin_allocate(th, made)) return rc;
    thin_args(a, th);
    for (int sd = 0; sd < 2; ++sd) {   // the descriptors of the kept points, where the source holds that side's
        if (!src->feat.have[sd]) continue;
        const size_t fb = attr_bytes(th.nb, th.nb->feat, sd);
        HIP_TRY(th.nb->feat.buf[sd].ensure(fb));
        HIP_TRY(hipMemsetAsync(th.nb->feat.buf[sd].p, 0, fb, th.st));   // (the padding, as icp_batch_compute_features leaves it)
        a.src_feat[sd] = (const unsigned long long*)src->feat.buf[sd].p;
        a.dst_feat[sd] = (unsigned long long*)th.nb->feat.buf[sd].p;
    }
    HIP_TRY(icp::launch_batch_keypoint_compact(a, th.st));
    if (int rc = thin_download(th)) return rc;
    if (int rc = thin_finish(th)) return rc;
    th.nb->feat.have[0] = src->feat.have[0];
    th.nb->feat.have[1] = src->feat.have[1];
    if (count_out) std::memcpy(count_out, th.kept.data(), th.kept.size() * sizeof(int32_t));
    return ICP_OK;
}

// T of pair `pair` as icp_batch_state reports it: the loop's T, times the initial transform as rounded to the batch's precision
// where the pair has one (T = T_loop . T0F, the product in HostLoop::note_applied's order)
void composed_T(const icp_batch* b, int pair, double* T16)
{
    const icp::HostLoop& H = b->H[pair];
    if (b->have_init && !b->init_copy[pair]) {
        const double* T0 = b->T0F.data() + (size_t)pair * 16;
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += H.T[a * 4 + k] * T0[k * 4 + c];
                T16[a * 4 + c] = s;
            }
    } else {
        std::memcpy(T16, H.T, sizeof H.T);
    }
}

// one step: enqueue the pass of every running pair, then complete it (loop_enqueue_body + loop_complete_body, per pair)
int step(icp_batch* b)
{
    icp_ctx* c = b->ctx;
    const int cur = (int)(b->steps & 1);
    const bool generalized = b->metric == ICP_GENERALIZED;
    const bool rotates = generalized || b->metric == ICP_SYMMETRIC;   // the step uploads Rc: the moving covariances, or the moving point normals, turn with the cloud
    int* mode = reinterpret_cast<int*>(b->h_ctl.as<char>() + b->rt_bytes);
    for (int p = 0; p < b->count; ++p) {
        mode[p] = 0;
        if (!running(b, p)) continue;
        icp::HostLoop& H = b->H[p];
        const bool apply = H.have_rt;
        const bool final_only = H.next_is_final();   // the loop ends after this error whatever it is: nothing is matched
        if (apply) {
            void* rt = b->h_ctl.as<char>() + (size_t)p * 12 * b->esize;
            if (b->prec == ICP_F64) put_rt<double>(rt, H.R, H.t);
            else put_rt<float>(rt, H.R, H.t);
            b->applied_buf[p] = b->last_match[p];
            H.note_applied();
            mode[p] |= icp::BATCH_APPLY;
        }
        if (!final_only) {
            b->last_match[p] = cur;
            mode[p] |= icp::BATCH_MATCH;
            if (rotates) {   // Rc: the rotation of every motion applied to the cloud this pass matches on
                double T[16];
                composed_T(b, p, T);
                double* R = b->rot.data() + (size_t)p * 9;
                for (int a = 0; a < 3; ++a)
                    for (int k = 0; k < 3; ++k) R[a * 3 + k] = T[a * 4 + k];
            }
        }
    }
    if (rotates) std::memcpy(b->h_ctl.as<char>() + b->rot_off, b->rot.data(), b->rot.size() * sizeof(double));
    HIP_TRY(hipMemcpyAsync(b->ctl.p, b->h_ctl.p, rotates ? b->rot_off + b->rot.size() * sizeof(double) : b->ctl_bytes, hipMemcpyHostToDevice, c->stream));
    icp::BatchPassArgs a{};
    a.precision = b->prec;
    a.metric = b->metric;
    a.items = (const icp::BatchItem*)b->items.p;
    a.n_items = b->n_items;
    a.pairs = (const icp::BatchPair*)b->pairs_d.p;
    a.n_pairs = b->count;
    a.mode = (const int*)(static_cast<char*>(b->ctl.p) + b->rt_bytes);
    a.rt = b->ctl.p;
    a.P_soa = b->P.p;
    a.p_plane = b->p_plane;
    a.Q_soa = b->Q.p;
    a.N_soa = b->metric == ICP_POINT_TO_PLANE || b->metric == ICP_COLORED ? b->N.buf[1].p : nullptr;
    a.q_plane = b->q_plane;
    a.idx_prev = (const int32_t*)b->idx[cur ^ 1].p;
    a.idx_cur = (int32_t*)b->idx[cur].p;
    a.partials = (double*)b->partials.p;
    a.mom = (double*)b->mom.p;
    a.thr = b->gated ? b->thr.p : nullptr;
    a.trim_rank = b->trimmed ? (const int*)b->trim_rank.p : nullptr;
    a.dist = b->dist.p;
    a.tau = b->tau.p;
    a.recip = b->reciprocal ? (const uint8_t*)b->recip_d.p : nullptr;
    a.rev = (int32_t*)b->rev.p;
    a.q_items = (const icp::BatchItem*)b->q_items.p;
    a.n_q_items = b->n_q_items;
    a.robust_kind = b->robust ? (const int*)b->rob_kind.p : nullptr;
    a.robust_k = (const double*)b->rob_k.p;
    a.robust_k2 = (const double*)b->rob_k2.p;
    a.weights = (double*)b->weights.p;
    if (rotates) a.rot = reinterpret_cast<const double*>(static_cast<const char*>(b->ctl.p) + b->rot_off);
    if (generalized) {
        a.cov_p = (const double*)b->cov.buf[0].p;
        a.cov_q = (const double*)b->cov.buf[1].p;
    }
    if (b->metric == ICP_SYMMETRIC) {
        a.nrm_p = (const double*)b->pnrm.buf[0].p;
        a.nrm_q = (const double*)b->pnrm.buf[1].p;
    }
    if (b->metric == ICP_COLORED) {
        a.int_p = (const double*)b->inten.buf[0].p;
        a.int_q = (const double*)b->inten.buf[1].p;
        a.grad_q = (const double*)b->grad.buf[1].p;
        a.color_w = (const double*)b->color_w.p;
    }
    HIP_TRY(icp::launch_batch_pass(a, c->stream));
    HIP_TRY(hipMemcpyAsync(b->h_mom.p, b->mom.p, (size_t)b->count * ICP_NMOM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    b->steps += 1;
    for (int p = 0; p < b->count; ++p) {
        if (mode[p] == 0) continue;
        if (mode[p] & icp::BATCH_MATCH) b->tau_seen[p] = 1;
        b->mom_seen[p] = 1;   // (a pair that takes no part in a later step keeps this row: batch_finalize_kernel skips it)
        const int rc = b->H[p].advance(b->h_mom.as<double>() + (size_t)p * ICP_NMOM);
        if (rc != ICP_OK) {   // a numeric failure ends this pair only; what its completed passes produced stays readable
            b->status[p] = rc;
            b->H[p].done = true;
        }
    }
    return ICP_OK;
}

// every pair's lambda as the batch holds it (ICP_COLOR_LAMBDA_DEFAULT where none was given) -> color_w
int upload_color_weights(icp_batch* b)
{
    std::vector<double> w = b->lambda;
    if (w.empty()) w.assign((size_t)b->count, ICP_COLOR_LAMBDA_DEFAULT);
    HIP_TRY(b->color_w.ensure(w.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(b->color_w.p, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vector goes)
    b->color_w_set = true;
    return ICP_OK;
}

// the buffer each pair's indices are read from: its most recent matching pass, or the pass whose motion it applied last
// (out: the indices; mask: 1 where that pass kept the point's match -- one of the two)
int download_indices(icp_batch* b, bool contributing, int32_t* out, uint8_t* mask = nullptr)
{
    if (int rc = ready(b)) return rc;
    if (!out && !mask) return fail(ICP_ERR_INVALID, "output pointer == NULL");
    if (!b->begun || b->steps == 0) return fail(ICP_ERR_STATE, "no matching pass since icp_batch_begin");
    std::vector<int32_t> h[2];
    for (int k = 0; k < 2; ++k) {
        h[k].resize((size_t)b->p_plane);
        HIP_TRY(hipMemcpyAsync(h[k].data(), b->idx[k].p, (size_t)b->p_plane * sizeof(int32_t), hipMemcpyDeviceToHost, b->ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    for (int p = 0; p < b->count; ++p) {
        const int which = contributing && b->H[p].applied > 0 ? b->applied_buf[p] : b->last_match[p];
        const int32_t* src = h[which].data() + b->pairs[p].p_off;
        for (int i = 0; i < b->pairs[p].n; ++i) {   // (a gated pass marks its rejected matches above the index: see BATCH_IDX_REJECTED)
            if (out) out[b->moff[p] + i] = src[i] & icp::BATCH_IDX_MASK;
            if (mask) mask[b->moff[p] + i] = src[i] >= 0 ? 1 : 0;
        }
    }
    return ICP_OK;
}

// the end of a call that thins src into `made`: the new batch to the caller, or -- src was only read -- what the call enqueued ends
// before its host vectors and the new batch go
int hand_over(icp_batch* src, int rc, icp_batch* made, icp_batch** out)
{
    if (rc != ICP_OK) {
        (void)hipStreamSynchronize(src->ctx->stream);
        (void)hipGetLastError();
        if (made) delete made;
        return rc;
    }
    *out = made;
    return ICP_OK;
}

}  // namespace

#pragma GCC visibility push(default)   // (the C ABI)
extern "C" {

int icp_batch_create(icp_ctx* c, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                     const int64_t* model_off, int precision, icp_batch** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (count < 1) return fail(ICP_ERR_INVALID, "a batch needs at least one pair");
    if (!moving_aos || !moving_off || !model_aos || !model_off) return fail(ICP_ERR_INVALID, "null cloud or offsets");
    if (precision != ICP_F32 && precision != ICP_F64) return fail(ICP_ERR_INVALID, "unknown precision");
    if (int rc = check_offsets(moving_off, count, "moving")) return rc;
    if (int rc = check_offsets(model_off, count, "model")) return rc;
    // (icp_set_* refuse a cloud with a NaN or an infinite coordinate; so does a batch, whichever pair holds it)
    const bool finite = precision == ICP_F64 ? all_finite<double>(moving_aos, moving_off[count]) && all_finite<double>(model_aos, model_off[count])
                                             : all_finite<float>(moving_aos, moving_off[count]) && all_finite<float>(model_aos, model_off[count]);
    if (!finite) return fail(ICP_ERR_INVALID, "a cloud of the batch has a NaN or an infinite coordinate");
    if (int rc = ctx_ready(c)) return rc;
    ScopedPin pin(c);
    icp_batch* b = nullptr;
    if (int rc = lay_out(c, count, precision, moving_off, model_off, &b)) return rc;
    if (int rc = upload(b, moving_aos, model_aos)) {
        (void)hipStreamSynchronize(c->stream);
        delete b;
        return rc;
    }
    *out = b;
    return ICP_OK;
}

int icp_batch_downsample(icp_batch* src, const double* voxel_moving, const double* voxel_model, int32_t* moving_map_out,
                         int32_t* model_map_out, icp_batch** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (int rc = ready(src)) return rc;
    std::vector<double> voxel(2 * (size_t)src->count, 0.0);   // the moving clouds' edges, then the models'
    for (int p = 0; p < src->count; ++p)
        for (int side = 0; side < 2; ++side) {
            const double* given = side ? voxel_model : voxel_moving;
            const double v = given ? given[p] : 0.0;
            if (!(std::isfinite(v) && v >= 0.0))   // (NaN fails both)
                return fail(ICP_ERR_INVALID, "a voxel edge must be finite and > 0, or exactly 0 (copy)" + where(p, side));
            voxel[(size_t)side * src->count + p] = v;
        }
    ScopedPin pin(src->ctx);
    icp_batch* made = nullptr;
    const int rc = downsample(src, voxel, moving_map_out, model_map_out, &made);
    return hand_over(src, rc, made, out);
}

int icp_batch_remove_outliers(icp_batch* src, const icp_outlier_rule* moving, const icp_outlier_rule* model, int32_t* moving_map_out,
                              int32_t* model_map_out, double* moving_score_out, double* model_score_out, double* stats_out,
                              icp_batch** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (int rc = ready(src)) return rc;
    static_assert(sizeof(icp::OutlierRule) == sizeof(icp_outlier_rule) && icp::OUTLIER_MAX_K == ICP_OUTLIER_MAX_NEIGHBOURS, "the kernels read the caller's rules");
    std::vector<icp::OutlierRule> rules(2 * (size_t)src->count, icp::OutlierRule{ICP_OUTLIER_NONE, 0, 0.0});   // the moving clouds', then the models'
    for (int p = 0; p < src->count; ++p)
        for (int side = 0; side < 2; ++side) {
            const icp_outlier_rule* given = side ? model : moving;
            if (!given) continue;
            const icp_outlier_rule& r = given[p];
            const int n = side ? src->pairs[p].m : src->pairs[p].n;
            const std::string at = where(p, side);
            if (r.kind == ICP_OUTLIER_NONE) continue;
            if (r.kind == ICP_OUTLIER_STATISTICAL) {
                if (r.neighbours < 1 || r.neighbours > ICP_OUTLIER_MAX_NEIGHBOURS)
                    return fail(ICP_ERR_INVALID, "a statistical rule's neighbours (k) must lie in [1, ICP_OUTLIER_MAX_NEIGHBOURS]" + at);
                if (n < r.neighbours + 1) return fail(ICP_ERR_INVALID, "a statistical rule needs a cloud of at least k + 1 points" + at);
                if (!(std::isfinite(r.value) && r.value >= 0.0))   // (NaN fails both)
                    return fail(ICP_ERR_INVALID, "a statistical rule's ratio must be finite and >= 0" + at);
            } else if (r.kind == ICP_OUTLIER_RADIUS) {
                if (!(std::isfinite(r.value) && r.value > 0.0)) return fail(ICP_ERR_INVALID, "a radius must be finite and > 0" + at);
                if (r.neighbours < 1 || r.neighbours > 65535)
                    return fail(ICP_ERR_INVALID, "a radius rule's least number of neighbours must lie in [1, 65535]" + at);
            } else {
                return fail(ICP_ERR_INVALID, "unknown outlier rule kind" + at);
            }
            rules[(size_t)side * src->count + p] = icp::OutlierRule{r.kind, r.neighbours, r.value};
        }
    ScopedPin pin(src->ctx);
    icp_batch* made = nullptr;
    const int rc = remove_outliers(src, rules, moving_map_out, model_map_out, moving_score_out, model_score_out, stats_out, &made);
    return hand_over(src, rc, made, out);
}

int icp_batch_select_keypoints(icp_batch* src, const icp_keypoint_rule* moving, const icp_keypoint_rule* model, int32_t* moving_map_out,
                               int32_t* model_map_out, double* moving_saliency_out, double* model_saliency_out, int32_t* count_out,
                               icp_batch** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (int rc = ready(src)) return rc;
    static_assert(sizeof(icp::KeypointRule) == sizeof(icp_keypoint_rule) && sizeof(icp_keypoint_rule) == 40, "the kernels read the caller's rules");
    std::vector<icp::KeypointRule> rules(2 * (size_t)src->count, icp::KeypointRule{ICP_KEYPOINT_NONE, 0, 0.0, 0.0, 0.0, 0.0});   // the moving clouds', then the models'
    for (int p = 0; p < src->count; ++p)
        for (int side = 0; side < 2; ++side) {
            const icp_keypoint_rule* given = side ? model : moving;
            if (!given) continue;
            const icp_keypoint_rule& r = given[p];
            const std::string at = where(p, side);
            if (r.kind == ICP_KEYPOINT_NONE) continue;
            if (r.kind != ICP_KEYPOINT_ISS) return fail(ICP_ERR_INVALID, "unknown keypoint rule kind" + at);
            if (r.min_neighbours < 1 || r.min_neighbours > 65535)
                return fail(ICP_ERR_INVALID, "a keypoint rule's least number of neighbours must lie in [1, 65535]" + at);
            if (!(std::isfinite(r.salient_radius) && r.salient_radius > 0.0) || !(std::isfinite(r.non_max_radius) && r.non_max_radius > 0.0))   // (NaN fails both)
                return fail(ICP_ERR_INVALID, "a radius must be finite and > 0" + at);
            if (!(std::isfinite(r.gamma_21) && r.gamma_21 > 0.0) || !(std::isfinite(r.gamma_32) && r.gamma_32 > 0.0))
                return fail(ICP_ERR_INVALID, "a gamma must be finite and > 0" + at);
            rules[(size_t)side * src->count + p] = icp::KeypointRule{r.kind, r.min_neighbours, r.salient_radius, r.non_max_radius, r.gamma_21, r.gamma_32};
        }
    ScopedPin pin(src->ctx);
    icp_batch* made = nullptr;
    const int rc = select_keypoints(src, rules, moving_map_out, model_map_out, moving_saliency_out, model_saliency_out, count_out, &made);
    return hand_over(src, rc, made, out);
}

int icp_batch_get_offsets(icp_batch* b, int64_t* moving_off_out, int64_t* model_off_out)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (moving_off_out) std::memcpy(moving_off_out, b->moff.data(), b->moff.size() * sizeof(int64_t));
    if (model_off_out) std::memcpy(model_off_out, b->qoff.data(), b->qoff.size() * sizeof(int64_t));
    return ICP_OK;
}

int icp_batch_get_clouds(icp_batch* b, void* moving_aos_out, void* model_aos_out)
{
    if (int rc = ready(b)) return rc;
    return fetch_clouds(b, b->P0.p, b->Q.p, moving_aos_out, model_aos_out);
}

void icp_batch_destroy(icp_batch* b)
{
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    delete b;
}

int icp_batch_begin(icp_batch* b, const icp_params* prm)
{
    if (int rc = ready(b)) return rc;
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (prm->metric != ICP_POINT_TO_POINT && prm->metric != ICP_POINT_TO_PLANE && prm->metric != ICP_GENERALIZED && prm->metric != ICP_COLORED &&
        prm->metric != ICP_SYMMETRIC)
        return fail(ICP_ERR_INVALID, "unknown metric");
    if (prm->metric == ICP_POINT_TO_PLANE && !b->N.have[1])
        return fail(ICP_ERR_INVALID, "a point-to-plane batch needs the model normals: icp_batch_set_model_normals or icp_batch_estimate_normals first");
    if (prm->metric == ICP_GENERALIZED) {
        if (!b->cov.have[0] || !b->cov.have[1])
            return fail(ICP_ERR_INVALID, std::string("a generalized batch needs covariances on both sides (icp_batch_set_covariances or icp_batch_estimate_covariances first): the ") +
                                             (!b->cov.have[0] ? "moving clouds" : "models") + " have none");
        if (b->robust) return fail(ICP_ERR_INVALID, "the generalized metric takes no robust kernels (icp_batch_set_robust(NULL) first)");
        HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));   // (the deferred route's winning distances)
    }
    if (prm->metric == ICP_COLORED) {
        const char* missing = !b->N.have[1] ? "the model normals (icp_batch_set_model_normals or icp_batch_estimate_normals)"
                              : !b->inten.have[0] ? "the intensities of the moving clouds (icp_batch_set_intensities)"
                              : !b->inten.have[1] ? "the intensities of the models (icp_batch_set_intensities)"
                              : !b->grad.have[1] ? "the intensity gradients of the models (icp_batch_estimate_intensity_gradients or icp_batch_set_intensity_gradients)"
                                                : nullptr;
        if (missing) return fail(ICP_ERR_INVALID, std::string("a colored batch needs model normals, intensities on both sides and intensity gradients: it lacks ") + missing);
        if (b->robust) return fail(ICP_ERR_INVALID, "the colored metric takes no robust kernels (icp_batch_set_robust(NULL) first)");
        HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));   // (the deferred route's winning distances)
        if (!b->color_w_set)
            if (int rc = upload_color_weights(b)) return rc;
    }
    if (prm->metric == ICP_SYMMETRIC) {
        if (!b->pnrm.have[0] || !b->pnrm.have[1])
            return fail(ICP_ERR_INVALID, std::string("a symmetric batch needs point normals on both sides (icp_batch_estimate_point_normals or icp_batch_set_point_normals first): the ") +
                                             (!b->pnrm.have[0] ? "moving clouds" : "models") + " have none");
        if (b->robust) return fail(ICP_ERR_INVALID, "the symmetric metric takes no robust kernels (icp_batch_set_robust(NULL) first)");
        HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));   // (the deferred route's winning distances)
    }
    if (prm->precision != b->prec) return fail(ICP_ERR_INVALID, "params precision differs from the batch's clouds");
    if (prm->max_iter < 1) return fail(ICP_ERR_INVALID, "max_iter must be >= 1");
    b->begun = false;
    b->metric = prm->metric;
    icp_params hp = *prm;
    if (hp.metric == ICP_COLORED) hp.metric = ICP_POINT_TO_PLANE;   // (the colored metric fills a plane pass's slots: the host loops are point-to-plane loops)
    if (hp.metric == ICP_SYMMETRIC) hp.metric = ICP_POINT_TO_PLANE;   // (so does the symmetric metric: point-to-plane loops that solve by solve_symmetric)
    for (int p = 0; p < b->count; ++p)
        if (int rc = b->H[p].begin(hp)) return fail(rc, "bad loop parameters");
    for (int p = 0; p < b->count; ++p) b->H[p].symmetric = prm->metric == ICP_SYMMETRIC;
    // (a generalized pass may keep nothing whatever the options: a match whose det(S) is not > 0 is rejected)
    for (int p = 0; p < b->count; ++p) b->H[p].gated = b->gated || b->trimmed || b->reciprocal || prm->metric == ICP_GENERALIZED;
    if (prm->metric == ICP_GENERALIZED || prm->metric == ICP_SYMMETRIC) b->rot.assign((size_t)b->count * 9, 0.0);
    for (int p = 0; p < b->count; ++p) b->H[p].weighted = b->robust;   // (a NONE pair of a robust batch: W == CNT exactly)
    reset_loop_state(b);
    if (b->have_init) {
        // the start cloud of every pair in one launch, and one flag per pair back: a finite transform can carry a finite cloud
        // out of the precision's range, and the library refuses non-finite clouds at the door -- that pair begins ended
        hipStream_t st = b->ctx->stream;
        std::vector<int> flag((size_t)b->count, 0);
        HIP_TRY(hipMemsetAsync(b->init_flag.p, 0, flag.size() * sizeof(int), st));
        HIP_TRY(icp::launch_batch_init(b->prec, (const icp::BatchItem*)b->items.p, b->n_items, (const icp::BatchPair*)b->pairs_d.p,
                                       (const int*)b->init_kind.p, b->rt0.p, b->P0.p, b->P.p, b->p_plane, (int*)b->init_flag.p, st));
        HIP_TRY(hipMemcpyAsync(flag.data(), b->init_flag.p, flag.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int p = 0; p < b->count; ++p)
            if (flag[p]) {
                b->status[p] = ICP_ERR_INVALID;
                b->H[p].done = true;
                b->refused[p] = 1;
            }
    } else {
        HIP_TRY(hipMemcpyAsync(b->P.p, b->P0.p, 3 * (size_t)b->p_plane * b->esize, hipMemcpyDeviceToDevice, b->ctx->stream));
    }
    b->steps = 0;
    b->begun = true;
    return ICP_OK;
}

int icp_batch_run(icp_batch* b, int max_steps, int* steps_done, int* active)
{
    if (int rc = ready(b)) return rc;
    if (max_steps < 0) return fail(ICP_ERR_INVALID, "max_steps < 0");
    if (!b->begun) return fail(ICP_ERR_STATE, "icp_batch_begin first");
    ScopedPin pin(b->ctx);
    int k = 0;
    while (k < max_steps && count_running(b) > 0) {
        if (int rc = step(b)) {
            // a device failure leaves the clouds in an unknown state: the loop is discarded
            (void)hipStreamSynchronize(b->ctx->stream);
            (void)hipGetLastError();
            b->begun = false;
            return rc;
        }
        ++k;
    }
    if (steps_done) *steps_done = k;
    if (active) *active = count_running(b);
    return ICP_OK;
}

int icp_batch_state(icp_batch* b, int pair, int* status, int* iterations, int* passes, double* err, int err_cap, double* T16)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (!b->begun) return fail(ICP_ERR_STATE, "no loop");
    const icp::HostLoop& H = b->H[pair];
    if (status) *status = b->status[pair];
    if (iterations) *iterations = H.iterations;
    if (passes) *passes = H.applied;
    if (err) {
        const int cnt = (int)H.err.size() < err_cap ? (int)H.err.size() : err_cap;
        for (int i = 0; i < cnt; ++i) err[i] = H.err[i];
    }
    if (T16) composed_T(b, pair, T16);
    return ICP_OK;
}

int icp_diag_batch_moments(icp_batch* b, int pair, double* out32)
{
    if (!b || !out32) return fail(ICP_ERR_INVALID, "null argument");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (!b->begun || !b->mom_seen[pair] || !b->h_mom.p) return fail(ICP_ERR_STATE, "no completed pass of this pair");
    std::memcpy(out32, b->h_mom.as<double>() + (size_t)pair * ICP_NMOM, ICP_NMOM * sizeof(double));
    return ICP_OK;
}

int icp_diag_batch_trim(icp_batch* b, int pair, double* tau_sq, int* rank)
{
    if (int rc = ready(b)) return rc;
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (!b->begun || !b->tau_seen[pair]) return fail(ICP_ERR_STATE, "no completed matching pass of this pair");
    if (rank) *rank = b->rank.empty() ? b->pairs[pair].n : b->rank[pair];
    if (tau_sq) {
        *tau_sq = INFINITY;   // (a batch that runs the fused pass keeps no tau buffer up to date: none of its pairs is trimmed)
        if (b->trimmed) {
            double raw = 0.0;   // (room for either precision)
            HIP_TRY(hipMemcpyAsync(&raw, static_cast<const char*>(b->tau.p) + (size_t)pair * b->esize, b->esize, hipMemcpyDeviceToHost, b->ctx->stream));
            HIP_TRY(hipStreamSynchronize(b->ctx->stream));
            *tau_sq = get_scalar(b, &raw, 0);
        }
    }
    return ICP_OK;
}

int icp_batch_evaluate(icp_batch* b, int metric, const double* max_dist, int* status_out, int32_t* inliers_out, double* fitness_out,
                       double* rmse_out, double* info_out, int32_t* idx_out, uint8_t* mask_out)
{
    if (int rc = ready(b)) return rc;
    if (metric != ICP_POINT_TO_POINT && metric != ICP_POINT_TO_PLANE) return fail(ICP_ERR_INVALID, "unknown metric");
    if (!b->begun) return fail(ICP_ERR_STATE, "icp_batch_begin first: an evaluation needs the clouds of a loop");
    const bool plane = metric == ICP_POINT_TO_PLANE;
    if (plane && !b->N.have[1])
        return fail(ICP_ERR_INVALID, "a point-to-plane evaluation needs the model normals: icp_batch_set_model_normals or icp_batch_estimate_normals first");
    if (max_dist)
        for (int p = 0; p < b->count; ++p)   // (icp_batch_set_max_distance's rule: NaN fails the comparison too; -inf is <= 0)
            if (!(max_dist[p] > 0))
                return fail(ICP_ERR_INVALID, "the evaluation distance must be > 0 or +INFINITY: pair " + std::to_string(p));
    icp_ctx* c = b->ctx;
    ScopedPin pin(c);
    const size_t vec_bytes = (size_t)b->count * ICP_NMOM * sizeof(double);
    HIP_TRY(b->e_mode.ensure((size_t)b->count * sizeof(int)));
    HIP_TRY(b->e_thr.ensure((size_t)b->count * b->esize));
    HIP_TRY(b->e_idx.ensure((size_t)b->p_plane * sizeof(int32_t)));
    HIP_TRY(b->e_dist.ensure((size_t)b->p_plane * b->esize));
    HIP_TRY(b->e_partials.ensure((size_t)b->n_items * ICP_NMOM * sizeof(double)));
    HIP_TRY(b->e_mom.ensure(vec_bytes));
    HIP_TRY(b->h_eval.ensure(vec_bytes));
    // every pair is evaluated where its cloud stands -- running, ended or failed -- but one whose start cloud was refused
    std::vector<int> mode((size_t)b->count);
    for (int p = 0; p < b->count; ++p) mode[p] = b->refused[p] ? 0 : icp::BATCH_MATCH;
    std::vector<char> thr;
    HIP_TRY(hipMemcpyAsync(b->e_mode.p, mode.data(), mode.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (max_dist) {   // thr = (F)(max_dist^2): the product in double, rounded once to the batch's precision
        thr.resize((size_t)b->count * b->esize);
        for (int p = 0; p < b->count; ++p) put_scalar(b, thr.data(), (size_t)p, max_dist[p] * max_dist[p]);
        HIP_TRY(hipMemcpyAsync(b->e_thr.p, thr.data(), thr.size(), hipMemcpyHostToDevice, c->stream));
    }
    icp::BatchEvalArgs a{};
    a.precision = b->prec;
    a.metric = metric;
    a.items = (const icp::BatchItem*)b->items.p;
    a.n_items = b->n_items;
    a.pairs = (const icp::BatchPair*)b->pairs_d.p;
    a.n_pairs = b->count;
    a.mode = (const int*)b->e_mode.p;
    a.P_soa = b->P.p;
    a.p_plane = b->p_plane;
    a.Q_soa = b->Q.p;
    a.N_soa = plane ? b->N.buf[1].p : nullptr;
    a.q_plane = b->q_plane;
    a.thr = max_dist ? b->e_thr.p : nullptr;
    a.idx = (int32_t*)b->e_idx.p;
    a.dist = b->e_dist.p;
    a.partials = (double*)b->e_partials.p;
    a.mom = (double*)b->e_mom.p;
    std::vector<int32_t> hidx;
    hipError_t e = icp::launch_batch_evaluate(a, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->h_eval.p, b->e_mom.p, vec_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && (idx_out || mask_out)) {
        hidx.resize((size_t)b->p_plane);
        e = hipMemcpyAsync(hidx.data(), b->e_idx.p, hidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);   // (always: the host vectors above must outlive their copies)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b->eval_seen = false;   // (the pinned vectors are in an unknown state; the loop's buffers were not written)
        return fail(ICP_ERR_HIP, std::string("icp_batch_evaluate: ") + hipGetErrorString(e));
    }
    b->eval_seen = true;
    for (int p = 0; p < b->count; ++p) {
        double* v = b->h_eval.as<double>() + (size_t)p * ICP_NMOM;
        const int n = b->pairs[p].n;
        if (b->refused[p]) std::memset(v, 0, ICP_NMOM * sizeof(double));   // (its row of the device vector was never written)
        const double cnt = v[ICP_EVAL_CNT];
        if (status_out) status_out[p] = b->refused[p] ? ICP_ERR_INVALID : ICP_OK;
        if (inliers_out) inliers_out[p] = (int32_t)cnt;
        if (fitness_out) fitness_out[p] = cnt / (double)n;
        if (rmse_out) rmse_out[p] = cnt > 0.0 ? std::sqrt(v[ICP_EVAL_SD] / cnt) : 0.0;
        if (info_out) {
            double* I = info_out + (size_t)p * 36;
            for (int k = 0; k < 36; ++k) I[k] = 0.0;
            if (b->refused[p]) {
                // (zeros)
            } else if (plane) {   // C, mirrored
                int o = ICP_MOM_C;
                for (int r = 0; r < 6; ++r)
                    for (int s = r; s < 6; ++s) I[r * 6 + s] = I[s * 6 + r] = v[o++];
            } else {   // sum over the kept q = (x, y, z) of g1 g1^T + g2 g2^T + g3 g3^T: g1 = (0, z, -y, 1, 0, 0), g2 = (-z, 0, x, 0, 1, 0), g3 = (y, -x, 0, 0, 0, 1)
                const double sx = v[ICP_EVAL_SQ], sy = v[ICP_EVAL_SQ + 1], sz = v[ICP_EVAL_SQ + 2];
                const double xx = v[ICP_EVAL_SQQ], xy = v[ICP_EVAL_SQQ + 1], xz = v[ICP_EVAL_SQQ + 2];
                const double yy = v[ICP_EVAL_SQQ + 3], yz = v[ICP_EVAL_SQQ + 4], zz = v[ICP_EVAL_SQQ + 5];
                auto sym = [I](int r, int s, double val) { I[r * 6 + s] = I[s * 6 + r] = val; };
                sym(0, 0, yy + zz); sym(1, 1, xx + zz); sym(2, 2, xx + yy);
                sym(0, 1, -xy); sym(0, 2, -xz); sym(1, 2, -yz);
                sym(0, 4, -sz); sym(0, 5, sy);
                sym(1, 3, sz); sym(1, 5, -sx);
                sym(2, 3, -sy); sym(2, 4, sx);
                sym(3, 3, cnt); sym(4, 4, cnt); sym(5, 5, cnt);
            }
        }
        for (int i = 0; i < n && (idx_out || mask_out); ++i) {
            const int32_t raw = b->refused[p] ? 0 : hidx[(size_t)b->pairs[p].p_off + i];
            if (idx_out) idx_out[b->moff[p] + i] = raw & icp::BATCH_IDX_MASK;
            if (mask_out) mask_out[b->moff[p] + i] = (!b->refused[p] && raw >= 0) ? 1 : 0;
        }
    }
    return ICP_OK;
}

int icp_diag_batch_eval_moments(icp_batch* b, int pair, double* out32)
{
    if (!b || !out32) return fail(ICP_ERR_INVALID, "null argument");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (!b->eval_seen || !b->h_eval.p) return fail(ICP_ERR_STATE, "no evaluation of this batch");
    std::memcpy(out32, b->h_eval.as<double>() + (size_t)pair * ICP_NMOM, ICP_NMOM * sizeof(double));
    return ICP_OK;
}

int icp_batch_done(icp_batch* b, int32_t* done_out)
{
    if (!b || !done_out) return fail(ICP_ERR_INVALID, "null argument");
    if (!b->begun) return fail(ICP_ERR_STATE, "no loop");
    for (int p = 0; p < b->count; ++p) done_out[p] = running(b, p) ? 0 : 1;
    return ICP_OK;
}

int icp_batch_get_moving(icp_batch* b, void* aos_out)
{
    if (int rc = ready(b)) return rc;
    if (!aos_out) return fail(ICP_ERR_INVALID, "aos_out == NULL");
    return fetch_clouds(b, b->P.p, nullptr, aos_out, nullptr);
}

int icp_batch_get_indices(icp_batch* b, int32_t* idx_out) { return download_indices(b, false, idx_out); }

int icp_batch_loop_indices(icp_batch* b, int32_t* idx_out) { return download_indices(b, true, idx_out); }

int icp_batch_get_inliers(icp_batch* b, uint8_t* mask_out)
{
    return download_indices(b, false, nullptr, mask_out);
}

int icp_batch_loop_inliers(icp_batch* b, uint8_t* mask_out)
{
    return download_indices(b, true, nullptr, mask_out);
}

int icp_batch_set_max_distance(icp_batch* b, const double* max_dist)
{
    if (int rc = ready(b)) return rc;
    if (max_dist) {
        for (int p = 0; p < b->count; ++p)   // (NaN fails the comparison too; -inf is <= 0)
            if (!(max_dist[p] > 0))
                return fail(ICP_ERR_INVALID, "the maximum correspondence distance must be > 0 or +INFINITY: pair " + std::to_string(p));
        // thr = (F)(max_dist^2): the product in double, rounded once to the batch's precision
        std::vector<char> h((size_t)b->count * b->esize);
        for (int p = 0; p < b->count; ++p) put_scalar(b, h.data(), (size_t)p, max_dist[p] * max_dist[p]);
        HIP_TRY(b->thr.ensure(h.size()));
        b->begun = false;   // a loop under way is discarded: its passes so far used other thresholds (or none)
        b->gated = false;
        HIP_TRY(hipMemcpyAsync(b->thr.p, h.data(), h.size(), hipMemcpyHostToDevice, b->ctx->stream));
        HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vector goes)
        b->gated = true;
    } else {
        b->begun = false;
        b->gated = false;
    }
    return ICP_OK;
}

int icp_batch_set_trim(icp_batch* b, const double* keep_ratio)
{
    if (int rc = ready(b)) return rc;
    if (!keep_ratio) {
        b->begun = false;
        b->trimmed = false;
        b->rho.clear();
        b->rank.clear();
        return ICP_OK;
    }
    for (int p = 0; p < b->count; ++p)   // (NaN fails both comparisons)
        if (!(keep_ratio[p] > 0.0 && keep_ratio[p] <= 1.0))
            return fail(ICP_ERR_INVALID, "the share to keep must satisfy 0 < ratio <= 1: pair " + std::to_string(p));
    // K = ceil(rho * (double)n), the product in double, clamped to [1, n]; exactly 1.0: not trimmed (device rank 0, tau = +inf)
    std::vector<int> rank((size_t)b->count), dev_rank((size_t)b->count);
    std::vector<char> inf((size_t)b->count * b->esize);
    bool any = false;
    for (int p = 0; p < b->count; ++p) {
        const int n = b->pairs[p].n;
        const double k = std::ceil(keep_ratio[p] * (double)n);
        rank[p] = k < 1.0 ? 1 : k > (double)n ? n : (int)k;
        dev_rank[p] = keep_ratio[p] == 1.0 ? 0 : rank[p];
        any = any || dev_rank[p] != 0;
        put_scalar(b, inf.data(), (size_t)p, INFINITY);
    }
    HIP_TRY(b->trim_rank.ensure(dev_rank.size() * sizeof(int)));
    HIP_TRY(b->tau.ensure(inf.size()));
    HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));
    b->begun = false;   // a loop under way is discarded: its passes so far kept other shares (or everything)
    b->trimmed = false;
    HIP_TRY(hipMemcpyAsync(b->trim_rank.p, dev_rank.data(), dev_rank.size() * sizeof(int), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipMemcpyAsync(b->tau.p, inf.data(), inf.size(), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vectors go)
    b->rho.assign(keep_ratio, keep_ratio + b->count);
    b->rank.swap(rank);
    b->trimmed = any;
    return ICP_OK;
}

int icp_batch_set_reciprocal(icp_batch* b, const uint8_t* on)
{
    if (int rc = ready(b)) return rc;
    bool any = false;
    for (int p = 0; on && p < b->count; ++p) any = any || on[p] != 0;
    if (!any) {   // NULL, or every flag 0: the batch runs the steps it ran without flags
        b->begun = false;
        b->reciprocal = false;
        if (on) b->recip.assign((size_t)b->count, 0);
        else b->recip.clear();
        return ICP_OK;
    }
    std::vector<uint8_t> flags((size_t)b->count);
    for (int p = 0; p < b->count; ++p) flags[p] = on[p] ? 1 : 0;
    // the allocations come before the batch changes: a call refused for want of memory leaves it as it was
    if (int rc = ensure_model_items(b)) return rc;
    HIP_TRY(b->recip_d.ensure(flags.size()));
    HIP_TRY(b->rev.ensure((size_t)b->q_plane * sizeof(int32_t)));
    HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));
    b->begun = false;   // a loop under way is discarded: its passes so far kept other matches
    b->reciprocal = false;
    HIP_TRY(hipMemcpyAsync(b->recip_d.p, flags.data(), flags.size(), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipMemsetAsync(b->rev.p, 0xff, (size_t)b->q_plane * sizeof(int32_t), b->ctx->stream));   // (-1: never random, the padding included)
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vector goes)
    b->recip.swap(flags);
    b->reciprocal = true;
    return ICP_OK;
}

int icp_batch_set_robust(icp_batch* b, const int* kind, const double* scale)
{
    if (int rc = ready(b)) return rc;
    bool any = false;
    for (int p = 0; kind && p < b->count; ++p) {
        if (kind[p] != ICP_ROBUST_NONE && kind[p] != ICP_ROBUST_HUBER && kind[p] != ICP_ROBUST_CAUCHY && kind[p] != ICP_ROBUST_TUKEY)
            return fail(ICP_ERR_INVALID, "unknown robust kernel: pair " + std::to_string(p));
        if (kind[p] == ICP_ROBUST_NONE) continue;
        if (!scale) return fail(ICP_ERR_INVALID, "a robust kernel needs a scale (scale == NULL): pair " + std::to_string(p));
        const double k = scale[p], k2 = k * k;   // (NaN fails every comparison; k * k may overflow or underflow)
        if (!(std::isfinite(k) && k > 0 && std::isfinite(k2) && k2 > 0))
            return fail(ICP_ERR_INVALID, "the scale of a robust kernel must be finite and > 0, and so must its square: pair " + std::to_string(p));
        any = true;
    }
    if (!any) {   // NULL, or every kind NONE: the batch runs the steps it ran without kernels
        b->begun = false;
        b->robust = false;
        if (kind) b->rkind.assign((size_t)b->count, ICP_ROBUST_NONE);
        else b->rkind.clear();
        b->rscale.assign(b->rkind.size(), 0.0);
        return ICP_OK;
    }
    std::vector<int> kinds(kind, kind + b->count);
    std::vector<double> k((size_t)b->count, 0.0), k2((size_t)b->count, 0.0);
    for (int p = 0; p < b->count; ++p)
        if (kinds[p] != ICP_ROBUST_NONE) {
            k[p] = scale[p];
            k2[p] = scale[p] * scale[p];
        }
    // the allocations come before the batch changes: a call refused for want of memory leaves it as it was
    const size_t wb = (size_t)b->p_plane * sizeof(double);
    HIP_TRY(b->rob_kind.ensure(kinds.size() * sizeof(int)));
    HIP_TRY(b->rob_k.ensure(k.size() * sizeof(double)));
    HIP_TRY(b->rob_k2.ensure(k2.size() * sizeof(double)));
    HIP_TRY(b->weights.ensure(wb));
    HIP_TRY(b->dist.ensure((size_t)b->p_plane * b->esize));
    b->begun = false;   // a loop under way is discarded: its passes so far weighed the matches otherwise (or not at all)
    b->robust = false;
    hipStream_t st = b->ctx->stream;
    HIP_TRY(hipMemcpyAsync(b->rob_kind.p, kinds.data(), kinds.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->rob_k.p, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->rob_k2.p, k2.data(), k2.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b->weights.p, 0, wb, st));   // (never random, the padding included)
    HIP_TRY(hipStreamSynchronize(st));   // (before the host vectors go)
    b->rkind.swap(kinds);
    b->rscale.swap(k);
    b->robust = true;
    return ICP_OK;
}

int icp_batch_get_weights(icp_batch* b, double* w_out)
{
    if (int rc = ready(b)) return rc;
    if (!w_out) return fail(ICP_ERR_INVALID, "output pointer == NULL");
    if (!b->begun || b->steps == 0) return fail(ICP_ERR_STATE, "no matching pass since icp_batch_begin");
    if (!b->robust) {   // no kernels: the kept mask as 1.0 / 0.0, from the index marks
        std::vector<uint8_t> mask((size_t)b->moff[b->count]);
        if (int rc = download_indices(b, false, nullptr, mask.data())) return rc;
        for (size_t i = 0; i < mask.size(); ++i) w_out[i] = mask[i] ? 1.0 : 0.0;
        return ICP_OK;
    }
    const void* const dev[2] = {b->weights.p, nullptr};
    void* const out[2] = {w_out, nullptr};
    return fetch(b, icp::Format{1, icp::PLANES, sizeof(double)}, dev, out);
}

int icp_diag_batch_reverse(icp_batch* b, int32_t* rev_out)
{
    if (int rc = ready(b)) return rc;
    if (!rev_out) return fail(ICP_ERR_INVALID, "rev_out == NULL");
    if (!b->begun || b->steps == 0) return fail(ICP_ERR_STATE, "no step since icp_batch_begin");
    std::vector<int32_t> h;
    if (b->reciprocal) {
        h.resize((size_t)b->q_plane);
        HIP_TRY(hipMemcpyAsync(h.data(), b->rev.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b->ctx->stream));
        HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    }
    for (int p = 0; p < b->count; ++p) {
        const bool have = b->reciprocal && b->recip[p] && b->tau_seen[p];   // (tau_seen: the pair has completed a matching pass)
        for (int j = 0; j < b->pairs[p].m; ++j) rev_out[b->qoff[p] + j] = have ? h[(size_t)b->pairs[p].q_off + j] : -1;
    }
    return ICP_OK;
}

int icp_batch_set_initial_transforms(icp_batch* b, const double* T16)
{
    if (int rc = ready(b)) return rc;
    if (!T16) {
        b->begun = false;
        b->have_init = false;
        return ICP_OK;
    }
    static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int p = 0; p < b->count; ++p) {
        const double* T = T16 + (size_t)p * 16;
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(T[k]) || (b->prec == ICP_F32 && !std::isfinite((float)T[k])))   // (finite in the batch's precision too)
                return fail(ICP_ERR_INVALID, "an initial transform has a NaN or an infinite value: pair " + std::to_string(p));
        if (!(T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0))
            return fail(ICP_ERR_INVALID, "the bottom row of an initial transform must be exactly 0 0 0 1: pair " + std::to_string(p));
    }
    // the 12 values of a pair, rounded once to the batch's precision (T0F: that matrix read back in double); a pair whose 16
    // doubles are the identity bit for bit is copied, not multiplied
    std::vector<char> rt((size_t)b->count * 12 * b->esize);
    std::vector<int> kind((size_t)b->count);
    std::vector<double> T0F((size_t)b->count * 16);
    std::vector<char> copy((size_t)b->count);
    for (int p = 0; p < b->count; ++p) {
        const double* T = T16 + (size_t)p * 16;
        double* o = T0F.data() + (size_t)p * 16;
        copy[p] = std::memcmp(T, ident, sizeof ident) == 0 ? 1 : 0;
        kind[p] = copy[p] ? icp::BATCH_INIT_COPY : icp::BATCH_INIT_APPLY;
        double R[9], t[3];
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) R[a * 3 + c] = T[a * 4 + c];
            t[a] = T[a * 4 + 3];
        }
        void* dst = rt.data() + (size_t)p * 12 * b->esize;
        if (b->prec == ICP_F64) put_rt<double>(dst, R, t);
        else put_rt<float>(dst, R, t);
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) o[a * 4 + c] = get_scalar(b, dst, (size_t)(a * 3 + c));
            o[a * 4 + 3] = get_scalar(b, dst, (size_t)(9 + a));
        }
        o[12] = o[13] = o[14] = 0.0;
        o[15] = 1.0;
    }
    HIP_TRY(b->rt0.ensure(rt.size()));
    HIP_TRY(b->init_kind.ensure(kind.size() * sizeof(int)));
    HIP_TRY(b->init_flag.ensure(kind.size() * sizeof(int)));
    b->begun = false;   // a loop under way is discarded: it started from another cloud
    b->have_init = false;
    HIP_TRY(hipMemcpyAsync(b->rt0.p, rt.data(), rt.size(), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipMemcpyAsync(b->init_kind.p, kind.data(), kind.size() * sizeof(int), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // (before the host vectors go)
    b->T0F.swap(T0F);
    b->init_copy.swap(copy);
    b->have_init = true;
    return ICP_OK;
}

int icp_batch_set_model_normals(icp_batch* b, const void* nxyz_aos)
{
    if (int rc = ready(b)) return rc;
    if (!nxyz_aos) return fail(ICP_ERR_INVALID, "nxyz_aos == NULL");
    const int64_t points = b->qoff[b->count];
    if (!(b->prec == ICP_F64 ? all_finite<double>(nxyz_aos, points) : all_finite<float>(nxyz_aos, points)))
        return fail(ICP_ERR_INVALID, "a normal of the batch has a NaN or an infinite component");
    const void* const given[2] = {nullptr, nxyz_aos};
    if (int rc = attr_reserve(b, b->N, given, nullptr)) return rc;   // (scanned above: one refusal for the whole batch)
    b->begun = false;   // a loop under way is discarded: its passes so far used other normals (or none)
    b->grad.have[1] = false;   // (intensity gradients lie in the tangent planes of the normals they were made with)
    return attr_commit(b, b->N, given);
}

int icp_batch_estimate_normals(icp_batch* b, void* nxyz_aos_out, int32_t* neighbours_out)
{
    if (int rc = ready(b)) return rc;
    for (int p = 0; p < b->count; ++p)
        if (b->pairs[p].m < 5)
            return fail(ICP_ERR_INVALID, "normals need at least 5 model points (k = 4 neighbours + self): pair " + std::to_string(p) + " has " +
                                             std::to_string(b->pairs[p].m));
    icp_ctx* c = b->ctx;
    const size_t qb = 3 * (size_t)b->q_plane * b->esize, nb = 4 * (size_t)b->q_plane * sizeof(int32_t);
    if (int rc = ensure_model_items(b)) return rc;   // BATCH_ITEM model points of one pair, cut from that pair's first model point
    HIP_TRY(b->nbr.ensure(nb));
    if (int rc = attr_room(b, b->N, 1)) return rc;
    b->begun = false;   // a loop under way is discarded
    b->N.have[1] = false;
    b->grad.have[1] = false;   // (intensity gradients lie in the tangent planes of the normals they were made with)
    HIP_TRY(hipMemsetAsync(b->nbr.p, 0, nb, c->stream));   // (the padding between the clouds: never read, never random)
    HIP_TRY(hipMemsetAsync(b->N.buf[1].p, 0, qb, c->stream));
    HIP_TRY(icp::launch_batch_normals(b->prec, (const icp::BatchItem*)b->q_items.p, b->n_q_items, (const icp::BatchPair*)b->pairs_d.p, b->Q.p,
                                      b->q_plane, (int32_t*)b->nbr.p, b->N.buf[1].p, c->stream));
    const void* const dev[2] = {nullptr, b->N.buf[1].p};
    void* const out[2] = {nullptr, nxyz_aos_out};
    Download d;
    std::vector<int32_t> hn;
    if (int rc = download(b, b->N.fmt, dev, out, d)) return rc;
    if (neighbours_out) {
        hn.resize(4 * (size_t)b->q_plane);
        HIP_TRY(hipMemcpyAsync(hn.data(), b->nbr.p, nb, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    deliver(b, b->N.fmt, d, out);
    if (neighbours_out)
        for (int p = 0; p < b->count; ++p)
            std::memcpy(neighbours_out + 4 * b->qoff[p], hn.data() + 4 * (size_t)b->pairs[p].q_off, 4 * (size_t)b->pairs[p].m * sizeof(int32_t));
    b->N.have[1] = true;
    return ICP_OK;
}

namespace {

// the clouds, the work items and (ks: not NULL) every cloud's k of a launch into one buffer, as lay_out_args places them
void pack_args(void* dst, const icp::ArgsLayout& lay, const icp::CloudList& cl, const std::vector<int>* ks)
{
    char* d = static_cast<char*>(dst);
    std::memcpy(d, cl.clouds.data(), cl.clouds.size() * sizeof(icp::VoxelCloud));
    std::memcpy(d + lay.off_items, cl.items.data(), cl.items.size() * sizeof(icp::BatchItem));
    if (ks) std::memcpy(d + lay.off_ints, ks->data(), ks->size() * sizeof(int));
}

}  // namespace

int icp_batch_set_covariances(icp_batch* b, const double* moving_cov, const double* model_cov)
{
    if (int rc = ready(b)) return rc;
    const void* const given[2] = {moving_cov, model_cov};
    if (!given[0] && !given[1]) return fail(ICP_ERR_INVALID, "moving_cov == NULL and model_cov == NULL");
    if (int rc = attr_reserve(b, b->cov, given, "a covariance")) return rc;
    b->begun = false;   // a loop under way is discarded: its passes so far used other covariances (or none)
    return attr_commit(b, b->cov, given);
}

int icp_batch_estimate_covariances(icp_batch* b, const int* k_moving, const int* k_model, int regularisation, double lambda,
                                   double* moving_cov_out, double* model_cov_out)
{
    if (int rc = ready(b)) return rc;
    const int* given[2] = {k_moving, k_model};
    if (!given[0] && !given[1]) return fail(ICP_ERR_INVALID, "k_moving == NULL and k_model == NULL");
    if (regularisation != ICP_COV_NONE && regularisation != ICP_COV_FROBENIUS) return fail(ICP_ERR_INVALID, "unknown covariance regularisation");
    if (regularisation == ICP_COV_FROBENIUS && !(std::isfinite(lambda) && lambda > 0.0))   // (NaN fails both)
        return fail(ICP_ERR_INVALID, "the lambda of ICP_COV_FROBENIUS must be finite and > 0");
    static_assert(icp::COV_MAX_K == ICP_COV_MAX_NEIGHBOURS, "the kernel's list holds the largest k");
    const int count = b->count;
    std::vector<int> ks(2 * (size_t)count, 0);   // every cloud's k, moving clouds first (0: its side is not asked for)
    int cap = 8;
    for (int side = 0; side < 2; ++side)
        for (int p = 0; given[side] && p < count; ++p) {
            if (int rc = check_k(given[side][p], side ? b->pairs[p].m : b->pairs[p].n, "a covariance", "covariances", where(p, side), cap)) return rc;
            ks[(size_t)side * count + p] = given[side][p];
        }
    const bool want[2] = {given[0] != nullptr, given[1] != nullptr};   // work items for the sides asked for
    icp::CloudList cl;
    if (!icp::list_clouds(b->pairs, want, cl)) return fail(ICP_ERR_INVALID, "too many work items for one batch");
    icp_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    ScopedPin pin(c);
    // one device buffer and one pinned host buffer of the batch's hold the clouds, the items and the k of the call, so that nothing
    // has to outlive it on the stack: the call returns without a host wait unless an output is wanted.  The allocations come
    // before the batch changes: a call refused for want of memory leaves it as it was
    const icp::ArgsLayout lay = icp::lay_out_args(cl.clouds.size(), cl.items.size(), ks.size());
    HIP_TRY(b->cov_args.wait());   // (the call before has long read the host buffer: no wait in practice)
    HIP_TRY(b->cov_args.ensure(lay.bytes));
    for (int side = 0; side < 2; ++side)
        if (given[side])
            if (int rc = attr_room(b, b->cov, side)) return rc;
    b->begun = false;   // a loop under way is discarded
    for (int side = 0; side < 2; ++side)
        if (given[side]) b->cov.have[side] = false;
    pack_args(b->cov_args.host.p, lay, cl, &ks);
    HIP_TRY(b->cov_args.copy(lay.bytes, st));
    for (int side = 0; side < 2; ++side)   // (the padding between the clouds: never read, never random)
        if (given[side]) HIP_TRY(hipMemsetAsync(b->cov.buf[side].p, 0, attr_bytes(b, b->cov, side), st));
    const char* ds = static_cast<const char*>(b->cov_args.dev.p);
    icp::BatchCovArgs a{};
    a.precision = b->prec;
    a.cap = cap;
    a.regularisation = regularisation;
    a.lambda = regularisation == ICP_COV_FROBENIUS ? lambda : 0.0;
    a.clouds = reinterpret_cast<const icp::VoxelCloud*>(ds);
    a.items = reinterpret_cast<const icp::BatchItem*>(ds + lay.off_items);
    a.n_items = (int)cl.items.size();
    a.k = reinterpret_cast<const int*>(ds + lay.off_ints);
    a.src[0] = b->P0.p;
    a.src[1] = b->Q.p;
    a.src_plane[0] = b->p_plane;
    a.src_plane[1] = b->q_plane;
    a.cov[0] = (double*)b->cov.buf[0].p;
    a.cov[1] = (double*)b->cov.buf[1].p;
    HIP_TRY(icp::launch_batch_covariances(a, st));
    HIP_TRY(b->cov_args.record(st));
    void* const out[2] = {given[0] ? moving_cov_out : nullptr, given[1] ? model_cov_out : nullptr};
    if (out[0] || out[1])
        if (int rc = fetch(b, b->cov, out)) return rc;   // (the one wait of a call that wants an output)
    for (int side = 0; side < 2; ++side)
        if (given[side]) b->cov.have[side] = true;
    return ICP_OK;
}

int icp_batch_get_covariances(icp_batch* b, double* moving_cov_out, double* model_cov_out)
{
    void* const out[2] = {moving_cov_out, model_cov_out};
    return attr_get(b, b->cov, out, "");
}

int icp_batch_set_intensities(icp_batch* b, const double* moving_I, const double* model_I)
{
    if (int rc = ready(b)) return rc;
    const void* const given[2] = {moving_I, model_I};
    if (!given[0] && !given[1]) return fail(ICP_ERR_INVALID, "moving_I == NULL and model_I == NULL");
    if (int rc = attr_reserve(b, b->inten, given, "an intensity")) return rc;
    b->begun = false;   // a loop under way is discarded: its passes so far used other intensities (or none)
    if (given[1]) b->grad.have[1] = false;   // (gradients belong to the model intensities they were made from)
    return attr_commit(b, b->inten, given);
}

int icp_batch_estimate_intensity_gradients(icp_batch* b, const int* k_model, double* grad_out)
{
    if (int rc = ready(b)) return rc;
    if (!k_model) return fail(ICP_ERR_INVALID, "k_model == NULL");
    if (!b->inten.have[1]) return fail(ICP_ERR_STATE, "intensity gradients need the intensities of the models: icp_batch_set_intensities first");
    if (!b->N.have[1]) return fail(ICP_ERR_STATE, "intensity gradients need the model normals: icp_batch_set_model_normals or icp_batch_estimate_normals first");
    static_assert(icp::COV_MAX_K == ICP_COV_MAX_NEIGHBOURS, "the kernel's list holds the largest k");
    int cap = 8;
    for (int p = 0; p < b->count; ++p)
        if (int rc = check_k(k_model[p], b->pairs[p].m, "an intensity gradient", "intensity gradients", where(p, 1), cap)) return rc;
    icp_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    ScopedPin pin(c);
    // every model's k travels through one pinned host buffer of the batch's, so that nothing has to outlive the call on the stack:
    // it returns without a host wait unless the output is wanted.  The allocations come before the batch changes
    if (int rc = ensure_model_items(b)) return rc;   // (waits once, the first time a batch needs its models' work items)
    const size_t k_bytes = (size_t)b->count * sizeof(int);
    HIP_TRY(b->grad_k.wait());   // (the call before has long read the host buffer: no wait in practice)
    HIP_TRY(b->grad_k.ensure(k_bytes));
    if (int rc = attr_room(b, b->grad, 1)) return rc;
    b->begun = false;   // a loop under way is discarded
    b->grad.have[1] = false;
    std::memcpy(b->grad_k.host.p, k_model, k_bytes);
    HIP_TRY(b->grad_k.copy(k_bytes, st));
    HIP_TRY(hipMemsetAsync(b->grad.buf[1].p, 0, attr_bytes(b, b->grad, 1), st));   // (the padding between the models: never read, never random)
    icp::BatchGradArgs a{};
    a.precision = b->prec;
    a.cap = cap;
    a.items = (const icp::BatchItem*)b->q_items.p;
    a.n_items = b->n_q_items;
    a.pairs = (const icp::BatchPair*)b->pairs_d.p;
    a.k = (const int*)b->grad_k.dev.p;
    a.Q_soa = b->Q.p;
    a.N_soa = b->N.buf[1].p;
    a.q_plane = b->q_plane;
    a.int_q = (const double*)b->inten.buf[1].p;
    a.grad = (double*)b->grad.buf[1].p;
    HIP_TRY(icp::launch_batch_intensity_gradients(a, st));
    HIP_TRY(b->grad_k.record(st));
    void* const out[2] = {nullptr, grad_out};
    if (grad_out)
        if (int rc = fetch(b, b->grad, out)) return rc;   // (the one wait of a call that wants the output)
    b->grad.have[1] = true;
    return ICP_OK;
}

int icp_batch_set_intensity_gradients(icp_batch* b, const double* grad)
{
    if (int rc = ready(b)) return rc;
    if (!grad) return fail(ICP_ERR_INVALID, "grad == NULL");
    const void* const given[2] = {nullptr, grad};
    if (int rc = attr_reserve(b, b->grad, given, "an intensity gradient")) return rc;
    b->begun = false;   // a loop under way is discarded
    return attr_commit(b, b->grad, given);
}

int icp_batch_get_intensity_gradients(icp_batch* b, double* grad_out)
{
    void* const out[2] = {nullptr, grad_out};
    return attr_get(b, b->grad, out, "");
}

int icp_batch_set_color_weight(icp_batch* b, const double* lambda)
{
    if (int rc = ready(b)) return rc;
    if (lambda)
        for (int p = 0; p < b->count; ++p)
            if (!(lambda[p] >= 0.0 && lambda[p] <= 1.0))   // (NaN fails both)
                return fail(ICP_ERR_INVALID, "a color weight (lambda) must lie in [0, 1]: pair " + std::to_string(p));
    HIP_TRY(b->color_w.ensure((size_t)b->count * sizeof(double)));
    b->begun = false;   // a loop under way is discarded
    std::vector<double> keep = b->lambda;
    if (lambda) b->lambda.assign(lambda, lambda + b->count);
    else b->lambda.clear();
    b->color_w_set = false;
    if (int rc = upload_color_weights(b)) {
        b->lambda.swap(keep);
        return rc;
    }
    return ICP_OK;
}

int icp_diag_batch_rotation(icp_batch* b, int pair, double* R9)
{
    if (!b || !R9) return fail(ICP_ERR_INVALID, "null argument");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (!b->begun || (b->metric != ICP_GENERALIZED && b->metric != ICP_SYMMETRIC) || !b->tau_seen[pair])
        return fail(ICP_ERR_STATE, "no completed matching pass of this pair in a generalized or a symmetric loop");
    std::memcpy(R9, b->rot.data() + (size_t)pair * 9, 9 * sizeof(double));
    return ICP_OK;
}

namespace {

// create, [normals], begin, run to the end, results, destroy
int run_batch(icp_ctx* c, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos, const int64_t* model_off,
              bool plane, const void* normals_aos, const icp_params* prm, double* T16_out, int* iterations_out, int* passes_out,
              double* err_out, int32_t* idx_out, void* moved_out, int* status_out)
{
    icp_batch* b = nullptr;
    if (int rc = icp_batch_create(c, count, moving_aos, moving_off, model_aos, model_off, prm->precision, &b)) return rc;
    ScopedPin pin(c);
    int rc = ICP_OK;
    if (plane) rc = normals_aos ? icp_batch_set_model_normals(b, normals_aos) : icp_batch_estimate_normals(b, nullptr, nullptr);
    if (rc == ICP_OK) rc = icp_batch_begin(b, prm);
    for (int active = 1; rc == ICP_OK && active > 0;) rc = icp_batch_run(b, 1 << 20, nullptr, &active);
    const int cap = prm->max_iter + 1;
    for (int p = 0; rc == ICP_OK && p < count; ++p)
        rc = icp_batch_state(b, p, status_out ? status_out + p : nullptr, iterations_out ? iterations_out + p : nullptr,
                             passes_out ? passes_out + p : nullptr, err_out ? err_out + (size_t)p * cap : nullptr, cap,
                             T16_out ? T16_out + (size_t)p * 16 : nullptr);
    if (rc == ICP_OK && idx_out) rc = icp_batch_loop_indices(b, idx_out);
    if (rc == ICP_OK && moved_out) rc = icp_batch_get_moving(b, moved_out);
    icp_batch_destroy(b);
    return rc;
}

}  // namespace

int icp_point_to_point_batch(icp_ctx* c, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                             const int64_t* model_off, const icp_params* prm, double* T16_out, int* iterations_out, int* passes_out,
                             double* err_out, int32_t* idx_out, void* moved_out, int* status_out)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (prm->metric != ICP_POINT_TO_POINT) return fail(ICP_ERR_INVALID, "icp_point_to_point_batch runs point-to-point only (icp_point_to_plane_batch)");
    if (prm->max_iter < 1) return fail(ICP_ERR_INVALID, "max_iter must be >= 1");
    return run_batch(c, count, moving_aos, moving_off, model_aos, model_off, false, nullptr, prm, T16_out, iterations_out, passes_out, err_out,
                     idx_out, moved_out, status_out);
}

int icp_point_to_plane_batch(icp_ctx* c, int count, const void* moving_aos, const int64_t* moving_off, const void* model_aos,
                             const int64_t* model_off, const void* normals_aos, const icp_params* prm, double* T16_out,
                             int* iterations_out, int* passes_out, double* err_out, int32_t* idx_out, void* moved_out, int* status_out)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (prm->metric != ICP_POINT_TO_PLANE) return fail(ICP_ERR_INVALID, "icp_point_to_plane_batch: prm->metric must be ICP_POINT_TO_PLANE");
    if (prm->max_iter < 1) return fail(ICP_ERR_INVALID, "max_iter must be >= 1");
    return run_batch(c, count, moving_aos, moving_off, model_aos, model_off, true, normals_aos, prm, T16_out, iterations_out, passes_out,
                     err_out, idx_out, moved_out, status_out);
}

// ---- global registration: descriptors, matching, scoring, RANSAC (the rules: include/icp_mi355x.h; kernels: icp_k_feat.hip) ----
extern "C++" {
namespace {

constexpr int kRansacChunk = 4096;   // hypotheses per pair and scoring launch of icp_batch_ransac

// the candidates of one scoring launch (count x per_pair, 12 values of the batch's precision each; valid: count x per_pair bytes or
// NULL) against the batch's correspondence lists: upload, one launch, download of the counts (one wait)
int score_on_device(icp_batch* b, int per_pair, const std::vector<char>& cand, const uint8_t* valid, const std::vector<char>& thr, int32_t* counts)
{
    icp_ctx* c = b->ctx;
    const size_t total = (size_t)b->count * per_pair;
    HIP_TRY(b->s_cand.ensure(cand.size()));
    HIP_TRY(b->s_valid.ensure(total));
    HIP_TRY(b->s_thr.ensure(thr.size()));
    HIP_TRY(b->s_counts.ensure(total * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(b->s_cand.p, cand.data(), cand.size(), hipMemcpyHostToDevice, c->stream));
    if (valid) HIP_TRY(hipMemcpyAsync(b->s_valid.p, valid, total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b->s_thr.p, thr.data(), thr.size(), hipMemcpyHostToDevice, c->stream));
    icp::BatchScoreArgs a{};
    a.precision = b->prec;
    a.pairs = (const icp::BatchPair*)b->pairs_d.p;
    a.n_pairs = b->count;
    a.cn = (const int*)b->f_cn.p;
    a.ci = (const int32_t*)b->f_ci.p;
    a.cj = (const int32_t*)b->f_cj.p;
    a.P0 = b->P0.p;
    a.p_plane = b->p_plane;
    a.Q = b->Q.p;
    a.q_plane = b->q_plane;
    a.cand = b->s_cand.p;
    a.valid = valid ? (const uint8_t*)b->s_valid.p : nullptr;
    a.thr = b->s_thr.p;
    a.per_pair = per_pair;
    a.counts = (int32_t*)b->s_counts.p;
    HIP_TRY(icp::launch_batch_score(a, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, b->s_counts.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ICP_OK;
}

// R, t of a row-major 4 x 4 -> the 12 values of candidate `at` in the batch's precision
void put_candidate(const icp_batch* b, std::vector<char>& cand, size_t at, const double* T)
{
    double R[9], t[3];
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) R[a * 3 + c] = T[a * 4 + c];
        t[a] = T[a * 4 + 3];
    }
    void* dst = cand.data() + at * 12 * b->esize;
    if (b->prec == ICP_F64) put_rt<double>(dst, R, t);
    else put_rt<float>(dst, R, t);
}

uint64_t ransac_mix(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// batch_score_transforms' decision for one list entry, restated on the host in the batch's precision (this unit is compiled with
// contraction off): the moved point in the front end's arithmetic, the matching's squared distance, d <= thr
template <typename F>
bool host_hit(const double* T, const double* p, const double* q, double thr_d)
{
    const F x = (F)p[0], y = (F)p[1], z = (F)p[2];   // (exact: the points are values of F)
    F o[3];
    for (int a = 0; a < 3; ++a) {
        F c = (F)T[a * 4 + 0] * x;
        c = c + (F)T[a * 4 + 1] * y;
        c = c + (F)T[a * 4 + 2] * z;
        o[a] = c + (F)T[a * 4 + 3];
    }
    if (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2])) return false;
    F dx = (F)q[0] - o[0], dy = (F)q[1] - o[1], dz = (F)q[2] - o[2];
    dx = dx * dx;
    dy = dy * dy;
    dz = dz * dz;
    F d = dx + dy;
    d = d + dz;
    return d <= (F)thr_d;
}

double sqd(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// hypothesis h of a pair whose seed mixed once is s0, over a list of C >= 3 entries: the picks of slots 0, 1, 2 (at most 16 draws, a
// draw equal to an earlier slot is skipped).  false: fewer than three distinct picks (the empty slots keep what they held)
bool draw_triple(uint64_t s0, int h, size_t C, int32_t* slot)
{
    const uint64_t base = ransac_mix(s0 + (uint64_t)h);
    int got = 0;
    for (int r = 0; r < 16 && got < 3; ++r) {
        const int32_t v = (int32_t)(ransac_mix(base + (uint64_t)r) % (uint64_t)C);
        bool seen = false;
        for (int s = 0; s < got; ++s) seen = seen || slot[s] == v;
        if (!seen) slot[got++] = v;
    }
    return got == 3;
}

// the edge check of a triple: LP, LQ hold the list's points, 3 doubles per entry; e == 0 switches it off
bool edges_ok(const double* LP, const double* LQ, const int32_t* slot, double e)
{
    if (!(e > 0.0)) return true;
    static const int ea[3] = {0, 1, 0}, eb[3] = {1, 2, 2};
    for (int k = 0; k < 3; ++k) {
        const double la = std::sqrt(sqd(&LP[3 * slot[ea[k]]], &LP[3 * slot[eb[k]]]));
        const double lb = std::sqrt(sqd(&LQ[3 * slot[ea[k]]], &LQ[3 * slot[eb[k]]]));
        if (!(la >= e * lb && lb >= e * la)) return false;
    }
    return true;
}

// one match into the 32-double moment vector of icp_solve_rigid
void add_match(double* mom, const double* p, const double* q)
{
    mom[ICP_MOM_CNT] += 1.0;
    for (int a = 0; a < 3; ++a) {
        mom[ICP_MOM_SP + a] += p[a];
        mom[ICP_MOM_SQ + a] += q[a];
        for (int c = 0; c < 3; ++c) mom[ICP_MOM_SQP + a * 3 + c] += q[a] * p[c];
    }
}

void identity16(double* T)
{
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

void pose16(const double* R, const double* t, double* T)
{
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) T[a * 4 + c] = R[a * 3 + c];
        T[a * 4 + 3] = t[a];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

bool finite16(const icp_batch* b, const double* T)
{
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(T[k]) || (b->prec == ICP_F32 && !std::isfinite((float)T[k]))) return false;
    return true;
}

}  // namespace
}  // extern "C++" (the templates above)

namespace {

// the one host body of icp_batch_compute_features (stored == false: the caller's normals, checked and uploaded) and of
// icp_batch_compute_features_stored (stored == true: the point normals the batch holds; moving_normals and model_normals are not read)
int compute_features(icp_batch* b, bool stored, const int* k_moving, const int* k_model, const double* moving_normals,
                     const double* model_normals, double* moving_feat_out, double* model_feat_out)
{
    if (int rc = ready(b)) return rc;
    const int* ks_given[2] = {k_moving, k_model};
    const double* nrm_given[2] = {moving_normals, model_normals};
    for (int sd = 0; sd < 2; ++sd) {
        if (!ks_given[sd]) return fail(ICP_ERR_INVALID, std::string("descriptors need a k for both sides: ") + (sd ? "k_model" : "k_moving") + " == NULL");
        const bool asked[2] = {sd == 0, sd == 1};
        if (stored) {
            if (int rc = attr_held(b->pnrm, asked, kPointNormalsFirst)) return rc;
        } else if (!nrm_given[sd])
            return fail(ICP_ERR_INVALID, std::string("descriptors need normals on both sides: ") + (sd ? "model_normals" : "moving_normals") + " == NULL");
    }
    const int count = b->count;
    std::vector<int> ks(2 * (size_t)count, 0);   // every cloud's k, moving clouds first
    int cap = 8;
    for (int sd = 0; sd < 2; ++sd)
        for (int p = 0; p < count; ++p) {
            if (int rc = check_k(ks_given[sd][p], sd ? b->pairs[p].m : b->pairs[p].n, "a descriptor", "descriptors", where(p, sd), cap)) return rc;
            const int64_t* off = sd ? b->qoff.data() : b->moff.data();
            for (int64_t i = 3 * off[p]; !stored && i < 3 * off[p + 1]; ++i)
                if (!std::isfinite(nrm_given[sd][i])) return fail(ICP_ERR_INVALID, "a normal has a NaN or an infinite value" + where(p, sd));
            ks[(size_t)sd * count + p] = ks_given[sd][p];
        }
    const bool both[2] = {true, true};
    icp::CloudList cl;
    if (!icp::list_clouds(b->pairs, both, cl)) return fail(ICP_ERR_INVALID, "too many work items for one batch");
    icp_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    ScopedPin pin(c);
    // the temporaries of the call: the normals, tau and the SPFH of both sides, the clouds, items and k.  The allocations come before
    // the batch changes: a call refused for want of memory leaves it as it was
    enum { NRM, TAU = 2, SPFH = 4, ARGS = 6 };   // (+ sd)
    const icp::ArgsLayout lay = icp::lay_out_args(cl.clouds.size(), cl.items.size(), ks.size());
    std::vector<char> hs(lay.bytes, 0), hn[2];
    Temps tmp(st);
    pack_args(hs.data(), lay, cl, &ks);
    HIP_TRY(tmp.buf[ARGS].ensure(lay.bytes));
    for (int sd = 0; sd < 2; ++sd) {
        const size_t plane = plane_elems(b, sd);
        if (!stored) HIP_TRY(tmp.buf[NRM + sd].ensure(3 * plane * sizeof(double)));
        HIP_TRY(tmp.buf[TAU + sd].ensure(plane * b->esize));
        HIP_TRY(tmp.buf[SPFH + sd].ensure(ICP_FEATURE_BINS * plane * sizeof(double)));
        HIP_TRY(b->feat.buf[sd].ensure(ICP_FEATURE_BINS * plane * sizeof(double)));
        if (!stored) icp::encode(b->pnrm.fmt, side(b, sd != 0), nrm_given[sd], hn[sd]);
    }
    b->feat.have[0] = b->feat.have[1] = false;
    b->have_match = false;   // (matches of other descriptors)
    HIP_TRY(hipMemcpyAsync(tmp.buf[ARGS].p, hs.data(), lay.bytes, hipMemcpyHostToDevice, st));
    for (int sd = 0; sd < 2; ++sd) {
        const size_t plane = plane_elems(b, sd);
        if (!stored) HIP_TRY(hipMemcpyAsync(tmp.buf[NRM + sd].p, hn[sd].data(), hn[sd].size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(tmp.buf[SPFH + sd].p, 0, ICP_FEATURE_BINS * plane * sizeof(double), st));   // (the padding between the clouds: never read, never random)
        HIP_TRY(hipMemsetAsync(b->feat.buf[sd].p, 0, ICP_FEATURE_BINS * plane * sizeof(double), st));
        HIP_TRY(hipMemsetAsync(tmp.buf[TAU + sd].p, 0, plane * b->esize, st));
    }
    const char* ds = static_cast<const char*>(tmp.buf[ARGS].p);
    icp::BatchFeatArgs a{};
    a.precision = b->prec;
    a.cap = cap;
    a.clouds = reinterpret_cast<const icp::VoxelCloud*>(ds);
    a.items = reinterpret_cast<const icp::BatchItem*>(ds + lay.off_items);
    a.n_items = (int)cl.items.size();
    a.k = reinterpret_cast<const int*>(ds + lay.off_ints);
    a.src[0] = b->P0.p;
    a.src[1] = b->Q.p;
    a.src_plane[0] = b->p_plane;
    a.src_plane[1] = b->q_plane;
    for (int sd = 0; sd < 2; ++sd) {
        a.nrm[sd] = (const double*)(stored ? b->pnrm.buf[sd].p : tmp.buf[NRM + sd].p);
        a.tau[sd] = tmp.buf[TAU + sd].p;
        a.spfh[sd] = (double*)tmp.buf[SPFH + sd].p;
        a.feat[sd] = (double*)b->feat.buf[sd].p;
    }
    const hipError_t le = icp::launch_batch_features(a, st);
    const hipError_t se = hipStreamSynchronize(st);   // (the one wait: the temporaries and the host vectors go with the call)
    HIP_TRY(le);
    HIP_TRY(se);
    b->feat.have[0] = b->feat.have[1] = true;
    void* const out[2] = {moving_feat_out, model_feat_out};
    if (out[0] || out[1]) return fetch(b, b->feat, out);
    return ICP_OK;
}

// the 2 * count clouds, moving clouds first, and the work items of all of them on the device (nrm_args), with the pinned buffers
// and the event of icp_batch_estimate_point_normals: made by the first call -- the layout of a batch never changes
int ensure_normals_args(icp_batch* b)
{
    if (b->n_nrm_items != 0) return ICP_OK;
    const bool both[2] = {true, true};
    icp::CloudList cl;
    if (!icp::list_clouds(b->pairs, both, cl)) return fail(ICP_ERR_INVALID, "too many work items for one batch");
    const icp::ArgsLayout lay = icp::lay_out_args(cl.clouds.size(), cl.items.size(), 0);
    const size_t view_bytes = cl.clouds.size() * 3 * sizeof(double);
    HIP_TRY(b->nrm_view.wait());   // (makes the event)
    HIP_TRY(b->nrm_view.host.ensure(view_bytes));
    HIP_TRY(b->nrm_args.ensure(lay.bytes));
    HIP_TRY(b->nrm_view.dev.ensure(view_bytes));
    HIP_TRY(b->nrm_cent.ensure(view_bytes));
    std::memset(b->nrm_args.host.p, 0, lay.bytes);
    pack_args(b->nrm_args.host.p, lay, cl, nullptr);
    HIP_TRY(b->nrm_args.copy(lay.bytes, b->ctx->stream));   // (from a pinned buffer the batch keeps: no wait)
    b->nrm_off_items = lay.off_items;
    b->n_nrm_items = (int)cl.items.size();
    return ICP_OK;
}

}  // namespace

int icp_batch_compute_features(icp_batch* b, const int* k_moving, const int* k_model, const double* moving_normals,
                               const double* model_normals, double* moving_feat_out, double* model_feat_out)
{
    return compute_features(b, false, k_moving, k_model, moving_normals, model_normals, moving_feat_out, model_feat_out);
}

int icp_batch_compute_features_stored(icp_batch* b, const int* k_moving, const int* k_model, double* moving_feat_out, double* model_feat_out)
{
    return compute_features(b, true, k_moving, k_model, nullptr, nullptr, moving_feat_out, model_feat_out);
}

int icp_batch_estimate_point_normals(icp_batch* b, int orient, const double* moving_viewpoints, const double* model_viewpoints,
                                     double* moving_normals_out, double* model_normals_out)
{
    if (int rc = ready(b)) return rc;
    if (orient != ICP_ORIENT_NONE && orient != ICP_ORIENT_VIEWPOINT && orient != ICP_ORIENT_CENTROID)
        return fail(ICP_ERR_INVALID, "unknown orientation of the point normals");
    for (int sd = 0; sd < 2; ++sd)
        if (!b->cov.have[sd])
            return fail(ICP_ERR_STATE, std::string("point normals need the covariances of both sides: the batch holds none of the ") + (sd ? "models" : "moving clouds") +
                                           " (icp_batch_set_covariances or icp_batch_estimate_covariances first)");
    const double* views[2] = {moving_viewpoints, model_viewpoints};
    const int count = b->count, n_clouds = 2 * count;
    if (orient == ICP_ORIENT_VIEWPOINT) {
        for (int sd = 0; sd < 2; ++sd)
            if (!views[sd]) return fail(ICP_ERR_INVALID, std::string("ICP_ORIENT_VIEWPOINT needs a viewpoint for both sides: ") + (sd ? "model_viewpoints" : "moving_viewpoints") + " == NULL");
        for (int sd = 0; sd < 2; ++sd)
            for (int p = 0; p < count; ++p)
                for (int k = 0; k < 3; ++k)
                    if (!std::isfinite(views[sd][3 * p + k]))
                        return fail(ICP_ERR_INVALID, "a viewpoint has a NaN or an infinite value" + where(p, sd));
    }
    icp_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    ScopedPin pin(c);
    // the allocations come before the batch changes: a call refused for want of memory leaves it as it was
    if (int rc = ensure_normals_args(b)) return rc;
    for (int sd = 0; sd < 2; ++sd)
        if (int rc = attr_room(b, b->pnrm, sd)) return rc;
    if (orient == ICP_ORIENT_VIEWPOINT) {
        HIP_TRY(b->nrm_view.wait());   // (the call before has long read the host buffer: no wait in practice; a new event is complete)
        for (int sd = 0; sd < 2; ++sd) std::memcpy(b->nrm_view.host.as<double>() + (size_t)sd * count * 3, views[sd], (size_t)count * 3 * sizeof(double));
        HIP_TRY(b->nrm_view.copy((size_t)n_clouds * 3 * sizeof(double), st));
        HIP_TRY(b->nrm_view.record(st));
    }
    const char* ds = static_cast<const char*>(b->nrm_args.dev.p);
    icp::BatchNormalsArgs a{};
    a.precision = b->prec;
    a.orient = orient;
    a.clouds = reinterpret_cast<const icp::VoxelCloud*>(ds);
    a.n_clouds = n_clouds;
    a.items = reinterpret_cast<const icp::BatchItem*>(ds + b->nrm_off_items);
    a.n_items = b->n_nrm_items;
    a.src[0] = b->P0.p;
    a.src[1] = b->Q.p;
    a.src_plane[0] = b->p_plane;
    a.src_plane[1] = b->q_plane;
    a.cent = (double*)b->nrm_cent.p;
    a.view = orient == ICP_ORIENT_CENTROID ? (const double*)b->nrm_cent.p : orient == ICP_ORIENT_VIEWPOINT ? (const double*)b->nrm_view.dev.p : nullptr;
    for (int sd = 0; sd < 2; ++sd) {
        a.cov[sd] = (const double*)b->cov.buf[sd].p;
        a.nrm[sd] = (double*)b->pnrm.buf[sd].p;
    }
    if (b->metric == ICP_SYMMETRIC) b->begun = false;   // a symmetric loop under way is discarded: its passes so far read other normals
    HIP_TRY(icp::launch_batch_point_normals(a, st));
    b->pnrm.have[0] = b->pnrm.have[1] = true;
    if (orient == ICP_ORIENT_CENTROID) b->have_cent = true;
    void* const out[2] = {moving_normals_out, model_normals_out};
    if (out[0] || out[1]) return fetch(b, b->pnrm, out);   // (the one wait of a call that wants an output)
    return ICP_OK;
}

int icp_batch_set_point_normals(icp_batch* b, const double* moving_normals, const double* model_normals)
{
    if (int rc = ready(b)) return rc;
    const void* const given[2] = {moving_normals, model_normals};
    if (!given[0] && !given[1]) return fail(ICP_ERR_INVALID, "moving_normals == NULL and model_normals == NULL");
    if (int rc = attr_reserve(b, b->pnrm, given, "a normal")) return rc;
    if (b->metric == ICP_SYMMETRIC) b->begun = false;   // a symmetric loop under way is discarded: its passes so far read other normals
    return attr_commit(b, b->pnrm, given);   // (no other loop reads them: one under way goes on)
}

int icp_batch_get_point_normals(icp_batch* b, double* moving_normals_out, double* model_normals_out)
{
    void* const out[2] = {moving_normals_out, model_normals_out};
    return attr_get(b, b->pnrm, out, kPointNormalsFirst);
}

int icp_diag_batch_centroids(icp_batch* b, double* out)
{
    if (int rc = ready(b)) return rc;
    if (!out) return fail(ICP_ERR_INVALID, "output pointer == NULL");
    if (!b->have_cent) return fail(ICP_ERR_STATE, "no icp_batch_estimate_point_normals call with ICP_ORIENT_CENTROID on this batch");
    HIP_TRY(hipMemcpyAsync(out, b->nrm_cent.p, (size_t)b->count * 6 * sizeof(double), hipMemcpyDeviceToHost, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    return ICP_OK;
}

int icp_batch_get_features(icp_batch* b, double* moving_feat_out, double* model_feat_out)
{
    void* const out[2] = {moving_feat_out, model_feat_out};
    return attr_get(b, b->feat, out, " (icp_batch_compute_features first)");
}

int icp_diag_batch_set_features(icp_batch* b, const double* moving_feat, const double* model_feat)
{
    if (int rc = ready(b)) return rc;
    const void* const given[2] = {moving_feat, model_feat};
    if (!given[0] || !given[1]) return fail(ICP_ERR_INVALID, "moving_feat == NULL or model_feat == NULL");
    if (int rc = attr_reserve(b, b->feat, given, nullptr)) return rc;   // (a diagnostic: nothing is scanned)
    b->have_match = false;   // (matches of other descriptors)
    return attr_commit(b, b->feat, given);
}

int icp_batch_match_features(icp_batch* b, int mutual, int32_t* fwd_out, int32_t* rev_out, uint8_t* kept_out)
{
    if (int rc = ready(b)) return rc;
    if (!b->feat.have[0] || !b->feat.have[1]) return fail(ICP_ERR_STATE, "the batch holds no descriptors (icp_batch_compute_features first)");
    icp_ctx* c = b->ctx;
    ScopedPin pin(c);
    if (int rc = ensure_model_items(b)) return rc;
    HIP_TRY(b->f_fwd.ensure((size_t)b->p_plane * sizeof(int32_t)));
    HIP_TRY(b->f_rev.ensure((size_t)b->q_plane * sizeof(int32_t)));
    HIP_TRY(b->f_kept.ensure((size_t)b->p_plane));
    HIP_TRY(b->f_ci.ensure((size_t)b->p_plane * sizeof(int32_t)));
    HIP_TRY(b->f_cj.ensure((size_t)b->p_plane * sizeof(int32_t)));
    HIP_TRY(b->f_cn.ensure((size_t)b->count * sizeof(int)));
    b->have_match = false;
    HIP_TRY(hipMemsetAsync(b->f_fwd.p, 0, (size_t)b->p_plane * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(b->f_rev.p, 0, (size_t)b->q_plane * sizeof(int32_t), c->stream));
    icp::BatchFeatMatchArgs a{};
    a.items[0] = (const icp::BatchItem*)b->items.p;
    a.items[1] = (const icp::BatchItem*)b->q_items.p;
    a.n_items[0] = b->n_items;
    a.n_items[1] = b->n_q_items;
    a.pairs = (const icp::BatchPair*)b->pairs_d.p;
    a.feat[0] = (const double*)b->feat.buf[0].p;
    a.feat[1] = (const double*)b->feat.buf[1].p;
    a.fwd = (int32_t*)b->f_fwd.p;
    a.rev = (int32_t*)b->f_rev.p;
    HIP_TRY(icp::launch_batch_feature_match(a, c->stream));
    std::vector<int32_t> hf((size_t)b->p_plane), hr((size_t)b->q_plane);
    HIP_TRY(hipMemcpyAsync(hf.data(), b->f_fwd.p, hf.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), b->f_rev.p, hr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // kept and the correspondence lists, on the host; the lists go back for batch_score_transforms
    std::vector<uint8_t> kept((size_t)b->p_plane, 0);
    std::vector<int32_t> ci((size_t)b->p_plane, 0), cj((size_t)b->p_plane, 0);
    std::vector<int> cn((size_t)b->count, 0);
    std::vector<std::vector<int32_t>> li((size_t)b->count), lj((size_t)b->count);
    for (int p = 0; p < b->count; ++p) {
        const icp::BatchPair& pr = b->pairs[p];
        for (int i = 0; i < pr.n; ++i) {
            const int32_t j = hf[(size_t)pr.p_off + i];
            const bool k = !mutual || hr[(size_t)pr.q_off + j] == i;
            kept[(size_t)pr.p_off + i] = k ? 1 : 0;
            if (!k) continue;
            ci[(size_t)pr.p_off + cn[p]] = i;
            cj[(size_t)pr.p_off + cn[p]] = j;
            cn[p] += 1;
            li[p].push_back(i);
            lj[p].push_back(j);
        }
    }
    HIP_TRY(hipMemcpyAsync(b->f_kept.p, kept.data(), kept.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b->f_ci.p, ci.data(), ci.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b->f_cj.p, cj.data(), cj.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b->f_cn.p, cn.data(), cn.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (before the host vectors go)
    for (int p = 0; p < b->count; ++p) {
        const icp::BatchPair& pr = b->pairs[p];
        if (fwd_out) std::memcpy(fwd_out + b->moff[p], hf.data() + pr.p_off, (size_t)pr.n * sizeof(int32_t));
        if (kept_out) std::memcpy(kept_out + b->moff[p], kept.data() + pr.p_off, (size_t)pr.n);
        if (rev_out) std::memcpy(rev_out + b->qoff[p], hr.data() + pr.q_off, (size_t)pr.m * sizeof(int32_t));
    }
    b->corr_i.swap(li);
    b->corr_j.swap(lj);
    b->have_match = true;
    return ICP_OK;
}

int icp_batch_score_transforms(icp_batch* b, int per_pair, const double* T16, const double* max_dist, int32_t* count_out)
{
    if (int rc = ready(b)) return rc;
    if (!b->have_match) return fail(ICP_ERR_STATE, "the batch holds no correspondence lists (icp_batch_match_features first)");
    if (per_pair < 1 || per_pair > 65536) return fail(ICP_ERR_INVALID, "per_pair must lie in [1, 65536]");
    if (!T16 || !count_out) return fail(ICP_ERR_INVALID, "T16 == NULL or count_out == NULL");
    for (int p = 0; p < b->count; ++p) {
        for (int k = 0; k < per_pair; ++k) {
            const double* T = T16 + ((size_t)p * per_pair + k) * 16;
            for (int e = 0; e < 16; ++e)
                if (!std::isfinite(T[e]) || (b->prec == ICP_F32 && !std::isfinite((float)T[e])))
                    return fail(ICP_ERR_INVALID, "a candidate transform has a NaN or an infinite value: pair " + std::to_string(p));
            if (!(T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0))
                return fail(ICP_ERR_INVALID, "the bottom row of a candidate transform must be exactly 0 0 0 1: pair " + std::to_string(p));
        }
        if (max_dist && !(max_dist[p] > 0))
            return fail(ICP_ERR_INVALID, "the scoring distance must be > 0 or +INFINITY: pair " + std::to_string(p));
    }
    ScopedPin pin(b->ctx);
    const size_t total = (size_t)b->count * per_pair;
    std::vector<char> cand(total * 12 * b->esize), thr((size_t)b->count * b->esize);
    for (size_t at = 0; at < total; ++at) put_candidate(b, cand, at, T16 + at * 16);
    for (int p = 0; p < b->count; ++p) put_scalar(b, thr.data(), (size_t)p, max_dist ? max_dist[p] * max_dist[p] : INFINITY);
    return score_on_device(b, per_pair, cand, nullptr, thr, count_out);
}

int icp_batch_ransac(icp_batch* b, const icp_ransac_params* prm, const uint64_t* seed, double* T16_out, int32_t* inliers_out,
                     int32_t* correspondences_out, int* status_out)
{
    if (int rc = ready(b)) return rc;
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (!seed) return fail(ICP_ERR_INVALID, "seed == NULL");
    if (prm->hypotheses < 1 || prm->hypotheses > 65536) return fail(ICP_ERR_INVALID, "hypotheses must lie in [1, 65536]");
    if (!(std::isfinite(prm->max_distance) && prm->max_distance > 0.0)) return fail(ICP_ERR_INVALID, "max_distance must be finite and > 0");
    if (!(prm->edge_similarity >= 0.0 && prm->edge_similarity < 1.0)) return fail(ICP_ERR_INVALID, "edge_similarity must lie in [0, 1)");
    if (!b->have_match) return fail(ICP_ERR_STATE, "the batch holds no correspondence lists (icp_batch_match_features first)");
    icp_ctx* c = b->ctx;
    ScopedPin pin(c);
    const int count = b->count, H = prm->hypotheses;
    const double e = prm->edge_similarity;
    // the clouds, widened: P0 and Q as the device holds them
    std::vector<char> ps(3 * (size_t)b->p_plane * b->esize), qs(3 * (size_t)b->q_plane * b->esize);
    HIP_TRY(hipMemcpyAsync(ps.data(), b->P0.p, ps.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(qs.data(), b->Q.p, qs.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    auto point = [b](const std::vector<char>& raw, long long plane, long long at, double* o) {
        for (int k = 0; k < 3; ++k) o[k] = get_scalar(b, raw.data(), (size_t)(k * plane + at));
    };
    const double thr_d = prm->max_distance * prm->max_distance;
    std::vector<char> thr((size_t)count * b->esize);
    for (int p = 0; p < count; ++p) put_scalar(b, thr.data(), (size_t)p, thr_d);
    const double thr_f = get_scalar(b, thr.data(), 0);   // (the threshold as the kernel reads it)

    // the hypotheses of every pair: draws, edge check, solve
    std::vector<int32_t> triples((size_t)count * H * 3, -1), counts((size_t)count * H, -1);
    std::vector<uint8_t> valid((size_t)count * H, 0);
    std::vector<double> Th((size_t)count * H * 16);
    std::vector<std::vector<double>> LP((size_t)count), LQ((size_t)count);   // the list's points, 3 doubles per entry
    for (int p = 0; p < count; ++p) {
        const icp::BatchPair& pr = b->pairs[p];
        const size_t C = b->corr_i[p].size();
        LP[p].resize(3 * C);
        LQ[p].resize(3 * C);
        for (size_t k = 0; k < C; ++k) {
            point(ps, b->p_plane, pr.p_off + b->corr_i[p][k], &LP[p][3 * k]);
            point(qs, b->q_plane, pr.q_off + b->corr_j[p][k], &LQ[p][3 * k]);
        }
        const uint64_t s0 = ransac_mix(seed[p]);
        for (int h = 0; h < H; ++h) {
            const size_t at = (size_t)p * H + h;
            identity16(&Th[at * 16]);
            if (C < 3) continue;
            int32_t* slot = &triples[at * 3];
            if (!draw_triple(s0, h, C, slot)) continue;
            if (!edges_ok(LP[p].data(), LQ[p].data(), slot, e)) continue;
            double mom[ICP_NMOM] = {0}, R[9], t[3];
            for (int s = 0; s < 3; ++s) add_match(mom, &LP[p][3 * slot[s]], &LQ[p][3 * slot[s]]);
            if (icp::solve_rigid(mom, R, t) != ICP_OK) continue;
            double T[16];
            pose16(R, t, T);
            if (!finite16(b, T)) continue;
            std::memcpy(&Th[at * 16], T, sizeof T);
            valid[at] = 1;
        }
    }
    // scoring: every pair's hypotheses [h0, h0 + per) in one launch
    for (int h0 = 0; h0 < H; h0 += kRansacChunk) {
        const int per = std::min(kRansacChunk, H - h0);
        std::vector<char> cand((size_t)count * per * 12 * b->esize);
        std::vector<uint8_t> ok((size_t)count * per);
        std::vector<int32_t> got((size_t)count * per);
        for (int p = 0; p < count; ++p)
            for (int k = 0; k < per; ++k) {
                const size_t at = (size_t)p * H + h0 + k;
                put_candidate(b, cand, (size_t)p * per + k, &Th[at * 16]);
                ok[(size_t)p * per + k] = valid[at];
            }
        if (int rc = score_on_device(b, per, cand, ok.data(), thr, got.data())) return rc;
        for (int p = 0; p < count; ++p)
            for (int k = 0; k < per; ++k) {
                const size_t at = (size_t)p * H + h0 + k;
                if (valid[at]) counts[at] = got[(size_t)p * per + k];
            }
    }
    // winner, refit
    std::vector<double> Tw((size_t)count * 16), Tr((size_t)count * 16);
    std::vector<int32_t> cw((size_t)count, 0), cr((size_t)count, 0);
    std::vector<int> status((size_t)count, ICP_ERR_EMPTY);
    std::vector<uint8_t> refit_ok((size_t)count, 0);
    for (int p = 0; p < count; ++p) {
        identity16(&Tw[(size_t)p * 16]);
        identity16(&Tr[(size_t)p * 16]);
        int best = -1;
        for (int h = 0; h < H; ++h)
            if (valid[(size_t)p * H + h] && (best < 0 || counts[(size_t)p * H + h] > counts[(size_t)p * H + best])) best = h;
        if (best < 0) continue;
        status[p] = ICP_OK;
        const double* T = &Th[((size_t)p * H + best) * 16];
        std::memcpy(&Tw[(size_t)p * 16], T, 16 * sizeof(double));
        cw[p] = counts[(size_t)p * H + best];
        double mom[ICP_NMOM] = {0}, R[9], t[3];
        const size_t C = b->corr_i[p].size();
        for (size_t k = 0; k < C; ++k) {
            const bool hit = b->prec == ICP_F64 ? host_hit<double>(T, &LP[p][3 * k], &LQ[p][3 * k], thr_f) : host_hit<float>(T, &LP[p][3 * k], &LQ[p][3 * k], thr_f);
            if (hit) add_match(mom, &LP[p][3 * k], &LQ[p][3 * k]);
        }
        if (mom[ICP_MOM_CNT] >= 3.0 && icp::solve_rigid(mom, R, t) == ICP_OK) {
            double T2[16];
            pose16(R, t, T2);
            if (finite16(b, T2)) {
                std::memcpy(&Tr[(size_t)p * 16], T2, sizeof T2);
                refit_ok[p] = 1;
            }
        }
    }
    {
        std::vector<char> cand((size_t)count * 12 * b->esize);
        for (int p = 0; p < count; ++p) put_candidate(b, cand, (size_t)p, &Tr[(size_t)p * 16]);
        if (int rc = score_on_device(b, 1, cand, refit_ok.data(), thr, cr.data())) return rc;
    }
    for (int p = 0; p < count; ++p) {
        const bool refit = status[p] == ICP_OK && refit_ok[p] && cr[p] >= cw[p];
        if (T16_out) std::memcpy(T16_out + (size_t)p * 16, refit ? &Tr[(size_t)p * 16] : &Tw[(size_t)p * 16], 16 * sizeof(double));
        if (inliers_out) inliers_out[p] = status[p] == ICP_OK ? (refit ? cr[p] : cw[p]) : 0;
        if (correspondences_out) correspondences_out[p] = (int32_t)b->corr_i[p].size();
        if (status_out) status_out[p] = status[p];
    }
    b->rs_hyp = H;
    b->rs_triples.swap(triples);
    b->rs_valid.swap(valid);
    b->rs_T.swap(Th);
    b->rs_counts.swap(counts);
    return ICP_OK;
}

int icp_diag_batch_ransac(icp_batch* b, int pair, int32_t* triples, uint8_t* valid, double* T16, int32_t* counts)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (b->rs_hyp == 0) return fail(ICP_ERR_STATE, "no icp_batch_ransac run on this batch");
    const size_t H = (size_t)b->rs_hyp, at = (size_t)pair * H;
    if (triples) std::memcpy(triples, b->rs_triples.data() + at * 3, H * 3 * sizeof(int32_t));
    if (valid) std::memcpy(valid, b->rs_valid.data() + at, H);
    if (T16) std::memcpy(T16, b->rs_T.data() + at * 16, H * 16 * sizeof(double));
    if (counts) std::memcpy(counts, b->rs_counts.data() + at, H * sizeof(int32_t));
    return ICP_OK;
}

// ---- plane segmentation (the rule: include/icp_mi355x.h; kernels: icp_k_segment.hip; the host statements: icp_host_math.cpp) ----
extern "C++" {
namespace {

constexpr int kPlaneChunk = 4096;   // hypotheses per cloud and scoring launch of icp_batch_segment_plane: a multiple of PLANE_GROUP
static_assert(kPlaneChunk % icp::PLANE_GROUP == 0, "whole groups per launch");

// what the caller's output pointers of icp_batch_segment_plane are
struct PlaneOut {
    double* planes;
    int32_t* inliers;
    int* status;
    uint8_t* mask[2];
    int32_t* map[2];
};

// icp_batch_segment_plane after its argument checks.  rules: 2 * count, the moving clouds' first.  The sequence is a thinning call's
// (thin_*), with the search in the place of the select launches:  [the clouds come down: the host draws from them]  ->  the
// hypotheses of every searched cloud on the host  ->  per kPlaneChunk hypotheses: planes and valid bytes up, batch_plane_score, counts
// down  ->  winners  ->  batch_plane_refit, moments down  ->  the refits on the host (icp::plane_from_moments)  ->
// batch_plane_decide  ->  thin_counts and onwards as icp_batch_remove_outliers
int segment_plane(icp_batch* src, const std::vector<icp_plane_rule>& rules, const uint64_t* seed, const PlaneOut& o, icp_batch** made)
{
    enum { MASK = T_VALUE, INLIERS = T_OWN, MOMENTS, SLICES, DIST, PLANES, VALID, COUNTS };   // (T_VALUE: this call keeps no double per point)
    const int count = src->count;
    const size_t n_clouds = 2 * (size_t)count;
    hipStream_t st = src->ctx->stream;
    // (host vectors that copies read or write: declared before th, whose temporaries wait for the stream when they go)
    std::vector<char> raw[2];
    std::vector<icp::PlaneJob> jobs0(n_clouds), jobs1, jobs2;
    std::vector<icp::BatchItem> slices;
    std::vector<double> dist(n_clouds, 0.0), hpl, hmom;
    std::vector<uint8_t> hval, hmask;
    std::vector<int32_t> got, hinl;
    std::vector<std::vector<int32_t>> triples(n_clouds), counts(n_clouds);
    std::vector<std::vector<uint8_t>> valid(n_clouds);
    std::vector<std::vector<double>> planes(n_clouds);
    bool any = false;
    int Hmax = 0;
    for (size_t k = 0; k < n_clouds; ++k) {
        const icp_plane_rule& r = rules[k];
        jobs0[k] = icp::PlaneJob{{0, 0, 0, 0}, {0, 0, 0, 0}, r.distance, r.kind, 0, 0, 0};
        dist[k] = r.distance;
        if (r.kind == ICP_PLANE_NONE) continue;
        any = true;
        Hmax = std::max(Hmax, r.hypotheses);
    }
    Thin th(src);
    th.map_out[0] = o.map[0];
    th.map_out[1] = o.map[1];
    if (int rc = thin_begin(th, n_clouds * sizeof(icp::PlaneJob), false, true)) return rc;
    const size_t tmp = (size_t)th.cl.tmp_plane;
    HIP_TRY(th.t.buf[MASK].ensure(tmp));
    HIP_TRY(th.t.buf[INLIERS].ensure(n_clouds * sizeof(int32_t)));
    HIP_TRY(th.t.buf[MOMENTS].ensure(n_clouds * 9 * sizeof(double)));
    if (int rc = thin_upload(th, jobs0.data(), n_clouds * sizeof(icp::PlaneJob))) return rc;
    icp::BatchPlaneArgs a{};
    thin_args(a, th);
    a.jobs = (const icp::PlaneJob*)th.t.buf[T_RULES].p;
    a.moments = (double*)th.t.buf[MOMENTS].p;
    a.mask = (uint8_t*)th.t.buf[MASK].p;
    a.inliers = (int32_t*)th.t.buf[INLIERS].p;
    a.chosen = (int*)th.t.buf[T_FLAG].p;
    jobs1 = jobs0;
    if (any) {
        // the clouds, widened: P0 and Q as the device holds them (the first wait)
        raw[0].resize(3 * (size_t)src->p_plane * src->esize);
        raw[1].resize(3 * (size_t)src->q_plane * src->esize);
        HIP_TRY(hipMemcpyAsync(raw[0].data(), src->P0.p, raw[0].size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(raw[1].data(), src->Q.p, raw[1].size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // the hypotheses of every searched cloud: draws, the plane of the three points, the axis test
        for (size_t k = 0; k < n_clouds; ++k) {
            const icp_plane_rule& r = rules[k];
            if (r.kind == ICP_PLANE_NONE) continue;
            const icp::VoxelCloud& c = th.cl.clouds[k];
            const long long plane = c.side ? src->q_plane : src->p_plane;
            const size_t p = k - (size_t)c.side * count;
            const size_t H = (size_t)r.hypotheses;
            triples[k].assign(3 * H, -1);
            counts[k].assign(H, -1);
            valid[k].assign(H, 0);
            planes[k].assign(4 * H, 0.0);
            const uint64_t s0 = ransac_mix(seed[p] + (uint64_t)c.side);
            for (size_t h = 0; h < H; ++h) {
                int32_t* slot = &triples[k][3 * h];
                if (!draw_triple(s0, (int)h, (size_t)c.n, slot)) continue;
                double abc[9];
                for (int s = 0; s < 3; ++s)
                    for (int d = 0; d < 3; ++d) abc[3 * s + d] = get_scalar(src, raw[c.side].data(), (size_t)(d * plane + c.src_off + slot[s]));
                double* pl = &planes[k][4 * h];
                if (!icp::plane_from_points(abc, abc + 3, abc + 6, pl)) continue;
                if (!icp::plane_axis_ok(pl, r.axis, r.min_cos)) {
                    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
                    continue;
                }
                valid[k][h] = 1;
            }
            for (int first = 0; first < c.n; first += icp::PLANE_SLICE)
                slices.push_back(icp::BatchItem{(int)k, first, std::min(icp::PLANE_SLICE, c.n - first), 0});
        }
        if (slices.size() > (size_t)INT_MAX) return fail(ICP_ERR_INVALID, "too many work items for one batch");
        // scoring: every searched cloud's hypotheses [h0, h0 + per) in one launch; a wait per launch
        const size_t room = (size_t)std::min(kPlaneChunk, (int)icp::round_up(Hmax, icp::PLANE_GROUP));
        HIP_TRY(th.t.buf[SLICES].ensure(slices.size() * sizeof(icp::BatchItem)));
        HIP_TRY(th.t.buf[DIST].ensure(n_clouds * sizeof(double)));
        HIP_TRY(th.t.buf[PLANES].ensure(n_clouds * room * 4 * sizeof(double)));
        HIP_TRY(th.t.buf[VALID].ensure(n_clouds * room));
        HIP_TRY(th.t.buf[COUNTS].ensure(n_clouds * room * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(th.t.buf[SLICES].p, slices.data(), slices.size() * sizeof(icp::BatchItem), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(th.t.buf[DIST].p, dist.data(), n_clouds * sizeof(double), hipMemcpyHostToDevice, st));
        a.slices = (const icp::BatchItem*)th.t.buf[SLICES].p;
        a.n_slices = (int)slices.size();
        a.distance = (const double*)th.t.buf[DIST].p;
        a.planes = (const double*)th.t.buf[PLANES].p;
        a.valid = (const uint8_t*)th.t.buf[VALID].p;
        a.counts = (int32_t*)th.t.buf[COUNTS].p;
        for (int h0 = 0; h0 < Hmax; h0 += kPlaneChunk) {
            const size_t per = (size_t)icp::round_up(std::min(kPlaneChunk, Hmax - h0), icp::PLANE_GROUP);   // <= room
            hpl.assign(n_clouds * per * 4, 0.0);
            hval.assign(n_clouds * per, 0);
            got.assign(n_clouds * per, 0);
            for (size_t k = 0; k < n_clouds; ++k) {
                const size_t H = valid[k].size();
                if (H <= (size_t)h0) continue;
                const size_t len = std::min(per, H - (size_t)h0);
                std::memcpy(&hpl[k * per * 4], &planes[k][4 * (size_t)h0], len * 4 * sizeof(double));
                std::memcpy(&hval[k * per], &valid[k][(size_t)h0], len);
            }
            HIP_TRY(hipMemcpyAsync(th.t.buf[PLANES].p, hpl.data(), hpl.size() * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(th.t.buf[VALID].p, hval.data(), hval.size(), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(th.t.buf[COUNTS].p, 0, got.size() * sizeof(int32_t), st));
            a.per = (int)per;
            HIP_TRY(icp::launch_batch_plane_score(a, st));
            HIP_TRY(hipMemcpyAsync(got.data(), th.t.buf[COUNTS].p, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t k = 0; k < n_clouds; ++k)
                for (size_t h = (size_t)h0; h < std::min(valid[k].size(), (size_t)h0 + per); ++h)
                    if (valid[k][h]) counts[k][h] = got[k * per + (h - (size_t)h0)];
        }
        // winners: the largest count, the lowest h among equals
        for (size_t k = 0; k < n_clouds; ++k) {
            int best = -1;
            for (size_t h = 0; h < valid[k].size(); ++h)
                if (valid[k][h] && (best < 0 || counts[k][h] > counts[k][(size_t)best])) best = (int)h;
            if (best < 0) continue;
            icp::PlaneJob& j = jobs1[k];
            std::memcpy(j.win, &planes[k][4 * (size_t)best], sizeof j.win);
            j.has_plane = 1;
            j.win_count = counts[k][(size_t)best];
        }
        // the refits: the sums on the device, the eigenvector on the host
        hmom.resize(n_clouds * 9);
        HIP_TRY(hipMemcpyAsync(th.t.buf[T_RULES].p, jobs1.data(), n_clouds * sizeof(icp::PlaneJob), hipMemcpyHostToDevice, st));
        HIP_TRY(icp::launch_batch_plane_refit(a, st));
        HIP_TRY(hipMemcpyAsync(hmom.data(), th.t.buf[MOMENTS].p, hmom.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    jobs2 = jobs1;
    for (size_t k = 0; any && k < n_clouds; ++k) {
        icp::PlaneJob& j = jobs2[k];
        if (!j.has_plane || j.win_count < 3) continue;
        if (!icp::plane_from_moments(&hmom[9 * k], &hmom[9 * k + 3], j.fit)) continue;
        j.fit_ok = icp::plane_axis_ok(j.fit, rules[k].axis, rules[k].min_cos) ? 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(th.t.buf[T_RULES].p, jobs2.data(), n_clouds * sizeof(icp::PlaneJob), hipMemcpyHostToDevice, st));
    HIP_TRY(icp::launch_batch_plane_decide(a, st));
    if (int rc = thin_counts(th)) return rc;
    for (int p = 0; p < count; ++p)
        for (int side = 0; side < 2; ++side) {
            const size_t k = (size_t)side * count + p;
            if (th.kept[k] < 1 && rules[k].kind == ICP_PLANE_REMOVE) return fail(ICP_ERR_EMPTY, "every point of the cloud lies on its plane" + where(p, side));
            if (th.kept[k] < 1 && !jobs2[k].has_plane) return fail(ICP_ERR_EMPTY, "the cloud has no plane to keep" + where(p, side));
            if (th.kept[k] < 1) return fail(ICP_ERR_EMPTY, "the cloud's plane keeps no point" + where(p, side));
            if (th.kept[k] > th.cl.clouds[k].n) return fail(ICP_ERR_HIP, "icp_batch_segment_plane: a cloud's kept count is out of range");   // (cannot happen)
        }
    if (int rc = thin_allocate(th, made)) return rc;
    icp::BatchOutlierArgs ca{};   // the compaction is the outlier call's: the same clouds, items, map and planes
    thin_args(ca, th);
    HIP_TRY(icp::launch_batch_outlier_compact(ca, st));
    if (int rc = thin_download(th)) return rc;
    hinl.resize(n_clouds);
    HIP_TRY(hipMemcpyAsync(hinl.data(), th.t.buf[INLIERS].p, n_clouds * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (o.mask[0] || o.mask[1]) {
        hmask.resize(tmp);
        HIP_TRY(hipMemcpyAsync(hmask.data(), th.t.buf[MASK].p, tmp, hipMemcpyDeviceToHost, st));
    }
    if (int rc = thin_finish(th)) return rc;
    for (size_t k = 0; k < n_clouds; ++k) {
        const icp::VoxelCloud& c = th.cl.clouds[k];
        const size_t p = k - (size_t)c.side * count;
        const icp::PlaneJob& j = jobs2[k];
        const bool searched = rules[k].kind != ICP_PLANE_NONE;
        if (o.planes) {
            const double zero[4] = {0, 0, 0, 0};
            std::memcpy(o.planes + 4 * k, !j.has_plane ? zero : th.flag[k] == 1 ? j.fit : j.win, 4 * sizeof(double));
        }
        if (o.inliers) o.inliers[k] = hinl[k];
        if (o.status) o.status[k] = searched && !j.has_plane ? ICP_ERR_EMPTY : ICP_OK;
        if (o.mask[c.side]) std::memcpy(o.mask[c.side] + (c.side ? src->qoff[p] : src->moff[p]), hmask.data() + c.tmp_off, (size_t)c.n);
    }
    src->sg_seen = true;
    src->sg_triples.swap(triples);
    src->sg_valid.swap(valid);
    src->sg_planes.swap(planes);
    src->sg_counts.swap(counts);
    return ICP_OK;
}

}  // namespace
}  // extern "C++"

int icp_batch_segment_plane(icp_batch* src, const icp_plane_rule* moving, const icp_plane_rule* model, const uint64_t* seed, double* planes_out,
                            int32_t* inliers_out, int* status_out, uint8_t* moving_mask_out, uint8_t* model_mask_out, int32_t* moving_map_out,
                            int32_t* model_map_out, icp_batch** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (int rc = ready(src)) return rc;
    static_assert(sizeof(icp_plane_rule) == 48, "the layout of icp_plane_rule");
    std::vector<icp_plane_rule> rules(2 * (size_t)src->count, icp_plane_rule{ICP_PLANE_NONE, 0, 0.0, {0.0, 0.0, 0.0}, 0.0});   // the moving clouds', then the models'
    for (int p = 0; p < src->count; ++p)
        for (int side = 0; side < 2; ++side) {
            const icp_plane_rule* given = side ? model : moving;
            if (!given) continue;
            const icp_plane_rule& r = given[p];
            const int n = side ? src->pairs[p].m : src->pairs[p].n;
            const std::string at = where(p, side);
            if (r.kind == ICP_PLANE_NONE) continue;
            if (r.kind != ICP_PLANE_DETECT && r.kind != ICP_PLANE_REMOVE && r.kind != ICP_PLANE_KEEP) return fail(ICP_ERR_INVALID, "unknown plane rule kind" + at);
            if (!seed) return fail(ICP_ERR_INVALID, "seed == NULL with a rule that searches" + at);
            if (r.hypotheses < 1 || r.hypotheses > 65536) return fail(ICP_ERR_INVALID, "a plane rule's hypotheses must lie in [1, 65536]" + at);
            if (!(std::isfinite(r.distance) && r.distance >= 0.0))   // (NaN fails both)
                return fail(ICP_ERR_INVALID, "a plane rule's distance must be finite and >= 0" + at);
            if (!(std::isfinite(r.axis[0]) && std::isfinite(r.axis[1]) && std::isfinite(r.axis[2])))
                return fail(ICP_ERR_INVALID, "a plane rule's axis must be finite" + at);
            if (!(r.min_cos >= 0.0 && r.min_cos <= 1.0)) return fail(ICP_ERR_INVALID, "a plane rule's min_cos must lie in [0, 1]" + at);
            if (n < 3) return fail(ICP_ERR_INVALID, "a plane needs a cloud of at least 3 points" + at);
            rules[(size_t)side * src->count + p] = r;
        }
    ScopedPin pin(src->ctx);
    icp_batch* made = nullptr;
    const PlaneOut o{planes_out, inliers_out, status_out, {moving_mask_out, model_mask_out}, {moving_map_out, model_map_out}};
    const int rc = segment_plane(src, rules, seed, o, &made);
    return hand_over(src, rc, made, out);
}

int icp_diag_batch_segment(icp_batch* b, int pair, int side, int32_t* triples, uint8_t* valid, double* planes, int32_t* counts)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (side != 0 && side != 1) return fail(ICP_ERR_INVALID, "side must be 0 (the moving cloud) or 1 (the model)");
    if (!b->sg_seen) return fail(ICP_ERR_STATE, "no icp_batch_segment_plane call on this batch");
    const size_t k = (size_t)side * b->count + pair, H = b->sg_valid[k].size();
    if (H == 0) return fail(ICP_ERR_STATE, "the last icp_batch_segment_plane call did not search this cloud");
    if (triples) std::memcpy(triples, b->sg_triples[k].data(), H * 3 * sizeof(int32_t));
    if (valid) std::memcpy(valid, b->sg_valid[k].data(), H);
    if (planes) std::memcpy(planes, b->sg_planes[k].data(), H * 4 * sizeof(double));
    if (counts) std::memcpy(counts, b->sg_counts[k].data(), H * sizeof(int32_t));
    return ICP_OK;
}


int icp_batch_fgr(icp_batch* b, const icp_fgr_params* prm, const uint64_t* seed, double* T16_out, double* weights_out, int32_t* used_out,
                  double* objective_out, int* status_out)
{
    if (int rc = ready(b)) return rc;
    if (!prm) return fail(ICP_ERR_INVALID, "params == NULL");
    if (prm->iterations < 1 || prm->iterations > 1024) return fail(ICP_ERR_INVALID, "iterations must lie in [1, 1024]");
    if (!(std::isfinite(prm->max_distance) && prm->max_distance > 0.0)) return fail(ICP_ERR_INVALID, "max_distance must be finite and > 0");
    if (!(std::isfinite(prm->division_factor) && prm->division_factor > 1.0)) return fail(ICP_ERR_INVALID, "division_factor must be finite and > 1");
    if (prm->decrease_every < 1) return fail(ICP_ERR_INVALID, "decrease_every must be >= 1");
    if (prm->tuples < 0 || prm->tuples > 65536) return fail(ICP_ERR_INVALID, "tuples must lie in [0, 65536]");
    if (prm->tuples > 0 && !(prm->tuple_similarity >= 0.0 && prm->tuple_similarity < 1.0)) return fail(ICP_ERR_INVALID, "tuple_similarity must lie in [0, 1)");
    if (prm->tuples > 0 && !seed) return fail(ICP_ERR_INVALID, "seed == NULL with tuples > 0");
    if (!b->have_match) return fail(ICP_ERR_STATE, "the batch holds no correspondence lists (icp_batch_match_features first)");
    icp_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    ScopedPin pin(c);
    const int count = b->count, I = prm->iterations;
    const double d2 = prm->max_distance * prm->max_distance;
    // the clouds, widened: P0 and Q as the device holds them
    std::vector<char> ps(3 * (size_t)b->p_plane * b->esize), qs(3 * (size_t)b->q_plane * b->esize);
    HIP_TRY(hipMemcpyAsync(ps.data(), b->P0.p, ps.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(qs.data(), b->Q.p, qs.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    auto point = [b](const std::vector<char>& raw, long long plane, long long at, double* o) {
        for (int k = 0; k < 3; ++k) o[k] = get_scalar(b, raw.data(), (size_t)(k * plane + at));
    };
    // the used list of every pair, its scale, its work items
    std::vector<std::vector<int32_t>> used((size_t)count);
    std::vector<int32_t> ui((size_t)b->p_plane, 0), uj((size_t)b->p_plane, 0);
    std::vector<icp::BatchItem> items;
    std::vector<int> item0((size_t)count + 1, 0), status((size_t)count, ICP_ERR_EMPTY);
    std::vector<double> mu((size_t)count, 0.0);
    for (int p = 0; p < count; ++p) {
        const icp::BatchPair& pr = b->pairs[p];
        const std::vector<int32_t>&li = b->corr_i[p], &lj = b->corr_j[p];
        const size_t C = li.size();
        item0[p] = (int)items.size();
        if (prm->tuples == 0) {
            used[p].resize(C);
            for (size_t k = 0; k < C; ++k) used[p][k] = (int32_t)k;
        } else if (C >= 3) {
            std::vector<double> LP(3 * C), LQ(3 * C);
            for (size_t k = 0; k < C; ++k) {
                point(ps, b->p_plane, pr.p_off + li[k], &LP[3 * k]);
                point(qs, b->q_plane, pr.q_off + lj[k], &LQ[3 * k]);
            }
            std::vector<uint8_t> in(C, 0);
            const uint64_t s0 = ransac_mix(seed[p]);
            for (int h = 0; h < prm->tuples; ++h) {
                int32_t slot[3] = {-1, -1, -1};
                if (!draw_triple(s0, h, C, slot) || !edges_ok(LP.data(), LQ.data(), slot, prm->tuple_similarity)) continue;
                in[slot[0]] = in[slot[1]] = in[slot[2]] = 1;
            }
            for (size_t k = 0; k < C; ++k)
                if (in[k]) used[p].push_back((int32_t)k);
        }
        const size_t U = used[p].size();
        if (U < 3) continue;
        // pbar, qbar: sequential sums in list order; D2: the largest squared distance of a used point from its side's mean
        std::vector<double> UP(3 * U), UQ(3 * U);
        double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
        for (size_t k = 0; k < U; ++k) {
            const int32_t i = li[used[p][k]], j = lj[used[p][k]];
            ui[(size_t)pr.p_off + k] = i;
            uj[(size_t)pr.p_off + k] = j;
            point(ps, b->p_plane, pr.p_off + i, &UP[3 * k]);
            point(qs, b->q_plane, pr.q_off + j, &UQ[3 * k]);
            for (int a = 0; a < 3; ++a) {
                sp[a] += UP[3 * k + a];
                sq[a] += UQ[3 * k + a];
            }
        }
        for (int a = 0; a < 3; ++a) {
            sp[a] = sp[a] / (double)U;
            sq[a] = sq[a] / (double)U;
        }
        double D2 = 0.0;
        bool nan = false;
        for (size_t k = 0; k < U; ++k) {
            const double dp = sqd(&UP[3 * k], sp), dq = sqd(&UQ[3 * k], sq);
            nan = nan || std::isnan(dp) || std::isnan(dq);
            D2 = std::max(D2, std::max(dp, dq));
        }
        if (nan || !std::isfinite(D2) || !(D2 > 0.0)) continue;
        status[p] = ICP_OK;
        mu[p] = D2;
        for (size_t first = 0; first < U; first += icp::BATCH_ITEM)
            items.push_back(icp::BatchItem{p, (int)first, (int)std::min((size_t)icp::BATCH_ITEM, U - first), 0});
    }
    item0[count] = (int)items.size();
    const int n_items = (int)items.size();
    // the call's history and results on the host
    std::vector<double> T((size_t)count * 16), objective((size_t)count, 0.0);
    std::vector<double> h_mu((size_t)count * I, 0.0), h_mom((size_t)count * I * ICP_NMOM, 0.0), h_T((size_t)count * I * 16, 0.0);
    for (int p = 0; p < count; ++p) identity16(&T[(size_t)p * 16]);
    std::vector<double> wplane;
    double sec[4] = {0.0, 0.0, 0.0, 0.0};
    if (n_items > 0) {
        const size_t ctl_bytes = (size_t)count * icp::FGR_CTL * sizeof(double), mom_bytes = (size_t)count * ICP_NMOM * sizeof(double);
        HIP_TRY(b->h_fgr.ensure(ctl_bytes + mom_bytes));
        HIP_TRY(b->g_ui.ensure((size_t)b->p_plane * sizeof(int32_t)));
        HIP_TRY(b->g_uj.ensure((size_t)b->p_plane * sizeof(int32_t)));
        HIP_TRY(b->g_items.ensure((size_t)n_items * sizeof(icp::BatchItem)));
        HIP_TRY(b->g_item0.ensure(item0.size() * sizeof(int)));
        HIP_TRY(b->g_ctl.ensure(ctl_bytes));
        HIP_TRY(b->g_partials.ensure((size_t)n_items * ICP_NMOM * sizeof(double)));
        HIP_TRY(b->g_mom.ensure(mom_bytes));
        HIP_TRY(b->g_w.ensure((size_t)b->p_plane * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(b->g_ui.p, ui.data(), ui.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->g_uj.p, uj.data(), uj.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->g_items.p, items.data(), (size_t)n_items * sizeof(icp::BatchItem), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->g_item0.p, item0.data(), item0.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(b->g_w.p, 0, (size_t)b->p_plane * sizeof(double), st));   // (a point that is not used: 0.0)
        HIP_TRY(hipStreamSynchronize(st));   // (before the host vectors could go with a failed call)
        icp::BatchFgrArgs a{};
        a.precision = b->prec;
        a.items = (const icp::BatchItem*)b->g_items.p;
        a.n_items = n_items;
        a.pairs = (const icp::BatchPair*)b->pairs_d.p;
        a.n_pairs = count;
        a.item0 = (const int*)b->g_item0.p;
        a.ui = (const int32_t*)b->g_ui.p;
        a.uj = (const int32_t*)b->g_uj.p;
        a.P0 = b->P0.p;
        a.p_plane = b->p_plane;
        a.Q = b->Q.p;
        a.q_plane = b->q_plane;
        a.ctl = (const double*)b->g_ctl.p;
        a.partials = (double*)b->g_partials.p;
        a.mom = (double*)b->g_mom.p;
        a.weights = (double*)b->g_w.p;
        double* ctl = b->h_fgr.as<double>();
        double* mom = ctl + (size_t)count * icp::FGR_CTL;
        std::vector<char> run((size_t)count, 0);   // the pair is still iterating
        int n_run = 0;
        for (int p = 0; p < count; ++p) n_run += (run[p] = status[p] == ICP_OK ? 1 : 0);
        auto fill_ctl = [&](const std::vector<char>& on) {
            for (int p = 0; p < count; ++p) {
                double* cp = ctl + (size_t)p * icp::FGR_CTL;
                std::memcpy(cp, &T[(size_t)p * 16], 12 * sizeof(double));
                cp[icp::FGR_CTL_MU] = mu[p];
                cp[icp::FGR_CTL_RUN] = on[p] ? 1.0 : 0.0;
            }
        };
        using clk = std::chrono::steady_clock;
        auto secs = [](clk::time_point a, clk::time_point z) { return std::chrono::duration<double>(z - a).count(); };
        for (int it = 0; it < I && n_run > 0; ++it) {
            const clk::time_point t0 = clk::now();
            for (int p = 0; p < count; ++p)
                if (run[p] && it % prm->decrease_every == 0 && mu[p] > d2) mu[p] = std::max(mu[p] / prm->division_factor, d2);
            fill_ctl(run);
            HIP_TRY(hipMemcpyAsync(b->g_ctl.p, ctl, ctl_bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(icp::launch_batch_fgr_terms(a, st));
            HIP_TRY(hipMemcpyAsync(mom, b->g_mom.p, mom_bytes, hipMemcpyDeviceToHost, st));
            const clk::time_point t1 = clk::now();
            HIP_TRY(hipStreamSynchronize(st));
            const clk::time_point t2 = clk::now();
            for (int p = 0; p < count; ++p) {
                if (!run[p]) continue;
                const double* m = mom + (size_t)p * ICP_NMOM;
                double* Tp = &T[(size_t)p * 16];
                const size_t at = (size_t)p * I + it;
                h_mu[at] = mu[p];
                std::memcpy(&h_mom[at * ICP_NMOM], m, ICP_NMOM * sizeof(double));
                std::memcpy(&h_T[at * 16], Tp, 16 * sizeof(double));
                objective[p] = m[ICP_MOM_ERR];
                double R[9], t[3], Tn[16];
                bool ok = icp::solve_point_to_plane(m, R, t, nullptr) == ICP_OK;
                if (ok) {   // T = S T
                    for (int r = 0; r < 3; ++r)
                        for (int cc = 0; cc < 4; ++cc) {
                            const double v = (R[3 * r] * Tp[cc] + R[3 * r + 1] * Tp[4 + cc]) + R[3 * r + 2] * Tp[8 + cc];
                            Tn[4 * r + cc] = cc == 3 ? v + t[r] : v;
                        }
                    Tn[12] = Tn[13] = Tn[14] = 0.0;
                    Tn[15] = 1.0;
                    for (int k = 0; k < 12; ++k) ok = ok && std::isfinite(Tn[k]);
                }
                if (!ok) {
                    status[p] = ICP_ERR_SINGULAR;
                    run[p] = 0;
                    n_run -= 1;
                    continue;
                }
                std::memcpy(Tp, Tn, sizeof Tn);
            }
            sec[0] += secs(t0, t1);
            sec[1] += secs(t1, t2);
            sec[2] += secs(t2, clk::now());
            sec[3] += 1.0;
        }
        // the weights at the final poses, of every pair that iterated
        std::vector<char> on((size_t)count, 0);
        for (int p = 0; p < count; ++p) on[p] = status[p] == ICP_OK || status[p] == ICP_ERR_SINGULAR;
        fill_ctl(on);
        HIP_TRY(hipMemcpyAsync(b->g_ctl.p, ctl, ctl_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(icp::launch_batch_fgr_weights(a, st));
        if (weights_out) {
            wplane.resize((size_t)b->p_plane);
            HIP_TRY(hipMemcpyAsync(wplane.data(), b->g_w.p, wplane.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (int p = 0; p < count; ++p) {
        const icp::BatchPair& pr = b->pairs[p];
        if (T16_out) std::memcpy(T16_out + (size_t)p * 16, &T[(size_t)p * 16], 16 * sizeof(double));
        if (weights_out) {
            if (wplane.empty()) std::memset(weights_out + b->moff[p], 0, (size_t)pr.n * sizeof(double));
            else std::memcpy(weights_out + b->moff[p], wplane.data() + pr.p_off, (size_t)pr.n * sizeof(double));
        }
        if (used_out) used_out[p] = (int32_t)used[p].size();
        if (objective_out) objective_out[p] = objective[p];
        if (status_out) status_out[p] = status[p];
    }
    b->fg_iter = I;
    b->fg_used.swap(used);
    b->fg_mu.swap(h_mu);
    b->fg_mom.swap(h_mom);
    b->fg_T.swap(h_T);
    std::memcpy(b->fg_sec, sec, sizeof sec);
    return ICP_OK;
}

int icp_diag_batch_fgr(icp_batch* b, int pair, int32_t* used_pos, double* mu_hist, double* mom_hist, double* T_hist)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (pair < 0 || pair >= b->count) return fail(ICP_ERR_INVALID, "pair out of range");
    if (b->fg_iter == 0) return fail(ICP_ERR_STATE, "no icp_batch_fgr run on this batch");
    const size_t I = (size_t)b->fg_iter, at = (size_t)pair * I;
    const std::vector<int32_t>& u = b->fg_used[(size_t)pair];
    if (used_pos && !u.empty()) std::memcpy(used_pos, u.data(), u.size() * sizeof(int32_t));
    if (mu_hist) std::memcpy(mu_hist, b->fg_mu.data() + at, I * sizeof(double));
    if (mom_hist) std::memcpy(mom_hist, b->fg_mom.data() + at * ICP_NMOM, I * ICP_NMOM * sizeof(double));
    if (T_hist) std::memcpy(T_hist, b->fg_T.data() + at * 16, I * 16 * sizeof(double));
    return ICP_OK;
}

int icp_diag_batch_fgr_times(icp_batch* b, double* seconds4)
{
    if (!b) return fail(ICP_ERR_INVALID, "null batch");
    if (!seconds4) return fail(ICP_ERR_INVALID, "seconds4 == NULL");
    if (b->fg_iter == 0) return fail(ICP_ERR_STATE, "no icp_batch_fgr run on this batch");
    std::memcpy(seconds4, b->fg_sec, sizeof b->fg_sec);
    return ICP_OK;
}

}  // extern "C"
#pragma GCC visibility pop
