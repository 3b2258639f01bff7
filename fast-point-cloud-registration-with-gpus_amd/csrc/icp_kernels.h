// icp_kernels.h -- host-callable launchers of the gfx950 kernels.  The kernels live in one translation unit per family
// (same flags, gfx950 only; shared device helpers in icp_device.h / icp_device_sparse.h):
//   icp_k_sparse.hip  nn_match_sparse      rows of 128 points: shared rows (Bunny.csv), box hierarchy (configs[4])
//   icp_k_row64.hip   nn_match_row64       rows of 64 points: the hall scan and everything up to 32 768 points
//   icp_k_f64.hip     nn_match_row64_f64   the CPU path's precision on the same structure
//   icp_k_dense.hip   nn_match_kernel / nn_match_f32_v2 (every pair), merge, moments, transform + error, finalize, layout
//   icp_k_batch.hip   nn_match_batch (many pairs per launch), nn_match_batch_rev (reciprocal pairs), trimmed rejection, robust kernels, per-pair finalize, initial transforms
//   icp_k_plane.hip   kNN(4) + normals, OS1 decode + conversion
//   icp_k_setup.hip   duplicates, spatial order, boxes / samples / records, row order + roles, the control block of a pass
//   icp_launch.hip    the dispatch (launch_nn): host code only
//   icp_plan.cpp      the plan a launch follows (icp_plan.h: nn_plan, nn_launch_shape): kernel family, geometry, waves -- no HIP
// Internal to libicp_mi355x.so; the public surface is include/icp_mi355x.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdint.h>

#include "../../include/icp_mi355x.h"
#include "icp_plan.h"

namespace icp {

// the transform of the previous pass, fused into the front of the matching kernel (fp32 kernel only):
// P_out <- R * P_in + t, err_rows[block_x] <- sum |p_new - q[idx_prev]|^2
// Mailbox of an armed / resident launch: ONE 64-byte line, written whole by the host and read whole by ONE load of the
// waiting wave (16 lanes x 4 bytes) -- detecting the message and receiving it are the same memory round trip.
// The line is two 32-byte halves, each carrying the message's tag in its last word next to its share of the payload:
//   w[0..6] = rt[0..6]   w[7] = tag   |   w[8..12] = rt[7..11]   w[13] = cmd   w[14] = tag   w[15] = 0
// (rt = R row-major, then t, rounded to the storage precision).  The host writes each half with one 32-byte vector
// store; whatever the fabric does with the line on its way (a write-combining buffer flushed in two pieces, a read split
// into sectors), a half whose tag is new carries new payload, and the reader accepts the line only when BOTH tags are
// the one it waits for.  tag = low 31 bits of the pass's sequence number, top bit set (a cleared mailbox never
// matches); cmd = ICP_CMD_EXIT under the awaited tag withdraws the kernel.  Where the mailbox lives in host memory,
// block 0 polls it and relays the line to the other blocks through a copy in device memory (`relay`).
#if defined(__HIPCC__)
#define ICP_HOST_DEVICE __host__ __device__
#else
#define ICP_HOST_DEVICE
#endif
struct alignas(64) NNMailbox {
    uint32_t w[16];
};
enum { ICP_MB_TAG0 = 7, ICP_MB_CMD = 13, ICP_MB_TAG1 = 14 };
ICP_HOST_DEVICE inline uint32_t mailbox_tag(double seq) { return (uint32_t)(unsigned long long)seq | 0x80000000u; }
ICP_HOST_DEVICE inline int mailbox_rt_word(int k) { return k < 7 ? k : k + 1; }   // the word rt[k] travels in
enum { ICP_CMD_EXIT = 0, ICP_CMD_MATCH = 1, ICP_CMD_TRANSFORM_MATCH = 2, ICP_CMD_TRANSFORM_ONLY = 3 };
// The same for a registration in double: twelve doubles do not fit one cache line, so the message is TWO lines in four
// 32-byte parts, part h = {rt[3h], rt[3h+1], rt[3h+2] (6 words), cmd, tag}; each part is written by one 32-byte store and
// the reader accepts the message only when all four tags are the awaited one.  A mailbox slot is 128 bytes for both
// precisions (the float message uses its first line).
struct alignas(128) NNMailbox64 {
    uint32_t w[32];
};
enum { ICP_MB64_CMD = 6 };   // (within each part; tags: word 7 of each part)
// How long a block waits for a message before it gives up (which reads as EXIT), in WALL-CLOCK seconds of the device's
// constant 100 MHz counter -- the same budget whatever memory the poll goes to.  Blocks that listen to block 0's relay
// wait twice as long: block 0 decides, and publishes its verdict (message or EXIT) through the relay.  The host side of
// the contract (icp_loop.cpp, kMailLeaseS) never posts a message a block might no longer be waiting for.
#define ICP_MAILBOX_BUDGET_S 4
constexpr long long ICP_MAILBOX_BUDGET_TICKS = (long long)ICP_MAILBOX_BUDGET_S * 100000000ll;
struct NNFusedTransform {
    const double* R9;  // NULL with a mailbox
    const double* t3;
    const int32_t* idx_prev;
    void* P_out;       // SoA, same padding as the input; must not alias it
    double* err_rows;  // >= blocks_x doubles
    const NNMailbox* mailbox = nullptr;  // armed launch (sparse kernel only): R9/t3 are not read
    NNMailbox* relay = nullptr;          // device-memory copy for the blocks other than block 0 (one per context)
    double want = 0.0;                   // sequence number of the (first) message
    bool resident = false;               // the kernel stays for the whole registration: pass p is message want + p
    bool store_first = false;            // resident: the input is not P_out (pristine copy): store the cloud in pass 0 as well
    void* slot_state = nullptr;          // fused launches of the sparse kernels: 9 x n_pad floats -- points (two planes) and matched model points in slot order (or NULL)
    bool slot_valid = false;             // ... the previous pass wrote them
    bool slot_flip = false;              // ... which of the two planes of points this launch reads (it writes the other): 9 x n_pad floats in all
};

// inputs of the early-out ("cull") variant of the packed kernel.  Q_scan is a copy of the model whose
// exact duplicates (same x,y,z as a LOWER index) are voided to +inf: such a point can never be the
// lowest-index minimum, and voiding it keeps one coincident cluster (e.g. the hall scan's 4361
// no-return points) from defeating the early-out for every chunk.  seed_idx: any valid model index
// per moving point (the previous pass's match) or NULL.
struct NNCullInputs {
    const void* Q_scan;
    const int32_t* seed_idx;
    const void* boxes;  // per 8-point chunk of Q_scan: {lo.xyz, hi.xyz, 0, 0} floats (launch_model_boxes), or NULL
    const void* samples = nullptr;  // one point per chunk of Q_scan (launch_model_samples): the sparse kernel's cold start
    int waves64 = 0;                // rows of 64 points: 16 = sixteen waves per block where every row has a CU to itself (icp_set_exclusive)
    const NNTuning* tune = nullptr; // the context's switches (NULL: the defaults)
    // sparse kernel only: when the model's own order has no locality its scan copy is kept in Morton order instead
    // (boxes and samples then describe THAT copy) with q_perm[sorted j] = model index; likewise the moving points are
    // dealt to the blocks in Morton order of their initial positions, p_perm[slot] = point.  NULL = identity.
    const void* Q_scan_sorted = nullptr;
    const int32_t* q_perm = nullptr;
    const int32_t* p_perm = nullptr;
    // diagnostic (sparse kernel): NN_WORK_SLOTS device counters of the work the kernel executes -- the launch then uses
    // the instrumented instantiation.  NULL (the default): the production kernel, nothing is counted.
    unsigned long long* work = nullptr;
    // shared rows (NNPlan::share_blocks): 5 x blocks_x device counters, zero before the first launch (three in rotation from
    // launch to launch, two alternating between the first passes of registrations), and the context's counters of both kinds
    // of launches (host; the launcher advances them).  NULL: every row is one block.
    unsigned int* share_counts = nullptr;
    unsigned long long* share_seq = nullptr;
    unsigned long long* share_cold_seq = nullptr;
    float* seed_pub = nullptr;   // resident launches with shared rows: blocks_x x 384 floats (NNFuse::seed_pub)
    // ordered rows (NNPlan::order): block b of the launch works on row row_order[b]; every block adds the hits of its lists to row_hits[row]
    const int32_t* row_order = nullptr;
    unsigned int* row_hits = nullptr;
    bool order_history = false;      // ... the counters behind row_order were filled by launches of an EARLIER registration too
    const float* records = nullptr;   // hierarchical search: one 160-byte record per chunk of the searched view (launch_model_records) or NULL
};
// What the sparse kernel EXECUTED (it returns the brute-force answer without evaluating most pairs): wave-level tallies.
// One "hit" = one 8-point model chunk processed by one wave = 64 lanes x 2 moving points against that chunk.
enum {
    NN_WORK_FIND_BOXES = 0,       // chunk boxes tested against a block's group box (one lane each, ~12 flop)
    NN_WORK_UPPER_BOXES = 1,      // boxes of the upper hierarchy levels tested the same way
    NN_WORK_HITS_BOX = 2,         // hits that went through the per-point box test (128 points x 12 flop)
    NN_WORK_HITS_XY = 3,          // ... that went on to the xy half of the distances (128 x 8 x 5 flop)
    NN_WORK_HITS_FULL = 4,        // ... whose 128 x 8 distances were evaluated in full (128 x 8 x 3 flop more)
    NN_WORK_SAMPLE_GROUPS = 5,    // cold start: groups of 8 samples scanned by a wave (128 x 8 x 8 flop)
    NN_WORK_BLOCK_PASSES = 6,     // (block, pass) pairs, for normalisation
    NN_WORK_BLOCK_TRANSFORMS = 7, // ... of which applied a transform first (16 waves x 128 points x 15 flop, redundantly)
    NN_WORK_SPEC_LISTS = 8,       // resident launches: (block, pass) pairs that entered a pass with a speculative hit list
    NN_WORK_SPEC_COVERED = 9,     // ... whose list covered the real group box and bound (the pass skipped find + fetch)
    NN_WORK_SPEC_HITS = 10,       // hits on the speculative lists that were used
    NN_WORK_LIST_HITS = 11,       // hits on the lists built by the ordinary find
    NN_WORK_SLOTS = 12
};
// Shared rows: how a launch of `blocks` blocks deals itself to `rows` rows, given the hits every row had in the launch
// before (nn_match_sparse computes this in every block, from the same counters: the pieces below are what it is made of,
// and share_rows_plan is the same computation on the host -- icp_share_rows_plan, tests/test_host.py).
//   parts(row) = clamp(ceil(h / T), 1, cap),  cap = min(64-chunk tiles of the model, 32)
//   T0 = ceil(total / spare) always fits (sum of ceil(h / T0) <= total / T0 + rows = blocks); four tighter targets, 4/8 .. 7/8
//   of T0, are tried and the smallest that fits is taken; never below `min_hits`.  The counts are clamped to 2^20 before
//   anything is added up: 512 rows x 2^20 stays within 32 bits, and with it the guarantee that the parts fit the grid.
constexpr unsigned int SHARE_COUNT_CLAMP = 1u << 20;
constexpr unsigned int SHARE_MAX_PARTS = 32u;
ICP_HOST_DEVICE inline unsigned int share_clamp(unsigned int h) { return h > SHARE_COUNT_CLAMP ? SHARE_COUNT_CLAMP : h; }
ICP_HOST_DEVICE inline unsigned int share_cap(int m_pad)
{
    const unsigned int tiles = (unsigned int)((((m_pad >> 3) + 63) >> 6));
    return tiles < SHARE_MAX_PARTS ? (tiles < 1u ? 1u : tiles) : SHARE_MAX_PARTS;
}
ICP_HOST_DEVICE inline unsigned int share_parts(unsigned int h, unsigned int T, unsigned int cap)
{
    unsigned int S = (h + T - 1u) / T;
    S = S > cap ? cap : S;
    return S < 1u ? 1u : S;
}
ICP_HOST_DEVICE inline unsigned int share_first_target(unsigned int total, unsigned int spare) { return spare ? (total + spare - 1u) / spare : 0xffffffffu; }
ICP_HOST_DEVICE inline unsigned int share_candidate(unsigned int T0, int k) { return (T0 * (unsigned int)(4 + k) + 7u) / 8u; }   // k = 0..3
ICP_HOST_DEVICE inline bool share_tries_candidates(unsigned int T0, unsigned int Tmin, unsigned int spare) { return spare != 0u && T0 > Tmin && T0 < 0x10000000u; }
// sums[k] = blocks the launch would need with candidate k
ICP_HOST_DEVICE inline unsigned int share_pick(unsigned int T0, unsigned int Tmin, const unsigned int (&sums)[4], unsigned int blocks)
{
    unsigned int T = T0;
    for (int k = 3; k >= 0; --k) T = sums[k] <= blocks ? share_candidate(T0, k) : T;   // (the smallest candidate that fits: k = 0 last)
    return T < Tmin ? Tmin : T;
}
// the same on the host: parts_out[rows]; returns the target (hits per block)
unsigned int share_rows_plan(const unsigned int* hits, int rows, int blocks, int m_pad, int min_hits, int* parts_out);

// Ordered rows.  A cloud with many more rows than the machine holds blocks runs them in rounds, in index order, and a pass
// lasts until its last block ends: a heavy row that starts late is the tail of the pass (10 M x 10 M, one GPU, pass 12:
// one row lists 468 000 chunks and takes 8.3 ms; it started at 5.9 ms of a 14.2 ms pass whose blocks add up to 10.0 ms per
// CU).  So the rows are taken heaviest first: every block adds the hits of its lists to its row's counter, and before the
// next launch the counters are sorted (stable, descending; 20 bits) into the order its blocks follow.  Any order is exact.
// SPLIT ROWS.  With the rows in that order and everything else faster, a late pass of the same registration lasts exactly as
// long as its heaviest row (pass 24: 8.2 ms for the row that lists 476 000 chunks, 6.0 ms of work per CU in the whole
// launch).  So the launch gets NN_ORDER_EXTRA blocks beyond its rows, and the rows whose counters exceed a target
// T = max(total / (4 x the blocks the machine holds at once), min) are dealt 2, 4, .. 64 of them: block b finds its role
// -- row, part, parts -- in roles[b]
// (launch_row_order writes them: the split rows first, then the others, heaviest first; -1 = no role).  The parts of a row
// interleave the model's super boxes (part p takes those whose number is p modulo parts), fold their minima into the row's
// 64-bit keys and the last to arrive closes the row -- the protocol of the segment blocks.  Any assignment is exact.
constexpr int NN_ORDER_EXTRA = 4096;   // blocks of an ordered launch beyond its rows
// (round 4) the order is by weight CLASSES -- a count's leading one and NN_ORDER_CLASS_BITS bits behind it; the rows of a class keep the
// curve's order -- and 2^NN_ORDER_XCD_SHIFT consecutive positions of it go to blocks of one XCD (blocks b and b + 8 share one): neighbours
// on the curve list mostly the same chunks, and run side by side behind ONE L2.  10 M x 10 M: 10.6 -> 3.1 GB fetched per pass (raw
// FETCH_SIZE), 4.88 -> 4.77 ms per iteration; classes of 0 / 1 / 2 bits, groups of 8 / 16 / 32: the same within 0.5 %
// (profiles/r4/r4_12_s5_order_classes_xcd_groups.txt)
constexpr int NN_ORDER_CLASS_BITS = 1;
constexpr int NN_ORDER_XCD_SHIFT = 4;
constexpr int NN_ORDER_HEAD = 1024;    // rows (the heaviest) that may be split
// the hierarchical search fetches a hit from one 160-byte record per chunk (icp_kernels.hip, model_records_kernel)
constexpr int NN_REC_WORDS = 40;
size_t model_records_bytes(int m_pad);
hipError_t launch_model_records(const void* Qs_soa, const float* boxes, const int32_t* perm, int m_pad, float* rec, hipStream_t st);

struct RowOrderBuffers {
    unsigned int* keys[2];   // >= rows each
    int32_t* vals[2];        // >= rows each; the order ends up in vals[1]
    void* temp;              // rocPRIM scratch, row_order_temp_bytes(rows)
    size_t temp_bytes;
    int32_t* roles;          // >= rows + NN_ORDER_EXTRA
    unsigned long long* totals;   // 2, zero before the first launch (the sum of the counters, alternating)
    unsigned long long seq;  // launches so far (the caller counts)
    int min_part;            // no part is meant to be smaller than this many hits (0: no row is split)
    int total_div;           // the target: the sum of the counters over this (4 x the blocks the machine holds at once)
    int control = 1;         // up to 16 384 rows: ONE single-workgroup launch (LDS counting sort + roles) instead of keys + rocPRIM sort + roles
    int coarse = NN_ORDER_CLASS_BITS;   // the order's weight classes: bits kept behind a count's leading one (0..3; order_class) -- rows of one class keep the curve's order
};
size_t row_order_temp_bytes(int rows);
// reads AND zeroes hits[rows] (the next launch counts afresh); *roles_out = the roles of rows + NN_ORDER_EXTRA blocks (device pointer)
hipError_t launch_row_order(const RowOrderBuffers& b, unsigned int* hits, int rows, const int32_t** roles_out, hipStream_t st);

// device-side preparation of the sparse kernel's views (icp_set_model / icp_set_moving): scratch owned by the caller
struct PrepBuffers {
    unsigned int* keys[2];   // >= count each
    int32_t* vals[2];        // >= count each
    void* temp;              // rocPRIM radix-sort scratch, prep_sort_temp_bytes(count)
    size_t temp_bytes;
    float* box;              // 4 floats
    double* ext;             // >= ceil(count / smallest group) doubles
};
size_t prep_sort_temp_bytes(int count);
hipError_t launch_duplicates_and_scan_copy(const PrepBuffers& b, const float* X_soa, int n, int n_pad, unsigned char* voided, int* count_dev,
                                           float* scan_out_soa, hipStream_t st);
hipError_t launch_duplicates_and_scan_copy_f64(const PrepBuffers& b, const double* X_soa, int n, int n_pad, unsigned char* voided, int* count_dev,
                                               double* scan_out_soa, hipStream_t st);
// totals_dev: 4 doubles -- summed extents of the groups in the given / the Morton order, for `group` and (if > 0) `group2`
hipError_t launch_morton_order(const PrepBuffers& b, const float* X_soa, int n, int n_pad, int group, int group2, int32_t* perm_out,
                               double* totals_dev, hipStream_t st);
hipError_t launch_gather_sorted(const float* Qs_soa, int m, int m_pad, const int32_t* perm, float* out_soa, int32_t* perm_pad, hipStream_t st);
hipError_t launch_slot_map(const int32_t* perm, int n, int n_pad, int32_t* out, hipStream_t st);
// round 4, the set-up of a cloud in a handful of launches (icp_k_setup.hip): exact duplicates by hashing (table: a power of two of
// >= 2 n 32-bit words, never cleared; gen: the upload's number), the scan copy in the same pass; group extents summed in fixed
// point relative to the bounding cube the layout kernel left in enc[6] (out[2 * which] given order, [2 * which + 1] `order`);
// the curve order of a small cloud; chunk boxes + samples of a flat model in one launch
hipError_t launch_duplicates_hashed(const float* X_soa, int n, int n_pad, unsigned int* table, unsigned int table_entries, unsigned int gen, unsigned char* voided,
                                    int* count_dev, float* scan_out_soa, hipStream_t st);
// (ticket / voided_count / report / seq: the launch's last block leaves the four sums, the duplicate count and `seq` in pinned host
// memory -- the host spins on report->seq; all NULL: nothing is reported)
struct PrepReport { unsigned long long fixed[4]; int voided; unsigned int seq; };
hipError_t launch_extents_fixed(const float* X_soa, int n, int n_pad, const int32_t* order, int group, const unsigned int* enc, unsigned long long* out, int which, hipStream_t st,
                                unsigned int* ticket = nullptr, const int* voided_count = nullptr, PrepReport* report = nullptr, unsigned int seq = 0);
hipError_t launch_curve_order_small(const PrepBuffers& b, const float* X_soa, int n, int n_pad, const unsigned int* enc, int32_t* perm_out, hipStream_t st);
hipError_t launch_model_boxes_samples(const void* Qs_soa, int m_pad, float* boxes, float* samples, hipStream_t st);
size_t model_samples_bytes(int m_pad);
// fp64 form of the sparse search: chunk boxes {lo.xyz, hi.xyz, -, -} and one sample per chunk, in double, of the model itself
size_t model_boxes_f64_bytes(int m_pad);
size_t model_samples_f64_bytes(int m_pad);
hipError_t launch_model_tables_f64(const void* Q_soa, int m_pad, void* boxes, void* samples, hipStream_t st);
hipError_t launch_model_samples(const void* Qs_soa, int m_pad, float* samples, hipStream_t st);
// boxes: model_boxes_bytes(m_pad) -- the chunk boxes, followed by the boxes of every 64 of them and of every 64 of
// those (the upper search levels of a large model)
size_t model_boxes_bytes(int m_pad);
hipError_t launch_model_boxes(const void* Qs_soa, int m_pad, float* boxes, hipStream_t st);

// fused tail of the packed kernel: atomic (d, idx) keys + row tickets, the row's last block produces idx and the
// moment row (see NNTail in icp_kernels.hip).  keys must be all-ones and tickets zero before the first launch;
// the kernel leaves them that way.
struct NNTailArgs {
    int metric;                 // ICP_POINT_TO_POINT / ICP_POINT_TO_PLANE
    unsigned long long* keys;   // [n_pad]
    unsigned int* tickets;      // [blocks_x]
    double* err_tile;           // [blocks_x] device
    int32_t* idx_out;           // [n_pad]
    int32_t* idx_out_odd = nullptr;  // resident launch: odd passes write here (NULL: idx_out)
    const void* Nrm_soa;        // normals (plane)
    double* rows;               // [blocks_x][ICP_NMOM], pinned host or device
    double tag;
    // sparse kernels, point-to-point, rows read by the host: rows of NN_CROW doubles {error share + tag, sum p, sum q,
    // sum q p^T} -- see NNTail in icp_kernels.hip
    int compact = 0;
    int rows_on_device = 0;     // the rows stay in device memory for a later kernel (finalize): no drain, no tag to wait for
    // rows_on_device, nn_match_sparse: the rows are added up inside the launch (NNTail::fin_*, icp_device.h) into fin_out -- pinned
    // host memory (fin_host: the pass's tag lands in its last slot) or a device vector; NULL: a finalize launch follows
    unsigned int* fin_tickets = nullptr;   // [NN_FIN_GROUPS + 1], zero before the first launch
    double* fin_scratch = nullptr;         // [NN_FIN_GROUPS][ICP_NMOM]
    double* fin_out = nullptr;             // [ICP_NMOM]
    int fin_host = 0;
};
constexpr int NN_FIN_GROUPS = 256;     // ranges of rows of an in-launch finalize, at most
constexpr int NN_CROW = 16;            // doubles per compact row
constexpr int NN_CROW_TAG_BITS = 16;   // low mantissa bits of slot 0 that carry the row's tag (mod 2^16)

// matching: per (segment, point) partial minimum + index.  `ft` (optional) = fused transform,
// `opt` (optional) = early-out inputs, `ta` (optional) = fused tail (then no partials are written).
hipError_t launch_nn(const NNPlan& pl, const void* P_soa, const void* Q_soa, void* part_d, int32_t* part_idx,
                     const NNFusedTransform* ft, const NNCullInputs* opt, const NNTailArgs* ta, hipStream_t st);
// stand-alone merge of the segment partials into idx (icp_nn_match_* only; the ICP loop merges
// inside the moments kernel)
hipError_t launch_merge(const NNPlan& pl, const void* part_d, const int32_t* part_idx, int32_t* idx, hipStream_t st);

constexpr int MOM_MAX_BLOCKS = 1024;
// fused: merge segment partials -> idx, gather q[idx], accumulate the metric's moments in fp64.
// partials: [blocks][ICP_NMOM] doubles; returns the number of blocks used in *blocks.
hipError_t launch_moments(const NNPlan& pl, int metric, const void* P_soa, const void* Q_soa, const void* N_soa,
                          const void* part_d, const int32_t* part_idx, int32_t* idx, double* partials, int* blocks,
                          double tag /* stored in slot ICP_NMOM-1 of every row once the row is complete */,
                          const double* err_rows /* device */, int err_count /* folded into slot ICP_MOM_ERR */,
                          hipStream_t st);
// p <- R p + t in place (storage precision, separately rounded mul/add), and
// sum |p_new - q[idx]|^2 in fp64 -> err_partials[block]
hipError_t launch_transform_error(int precision, void* P_soa, int n, int n_pad, const double* R9, const double* t3,
                                  const void* Q_soa, int m_pad, const int32_t* idx, double* err_partials,
                                  int* blocks, hipStream_t st);
// deterministic fixed-order reduction of the per-block partials into the ICP_NMOM-vector
hipError_t launch_finalize(double* mom_out, const double* mom_partials, int mom_blocks, const double* err_partials,
                           int err_blocks, int rows_have_err /* slot 0 of the rows carries error shares */, hipStream_t st, double* scratch = nullptr /* >= 256 x ICP_NMOM doubles: many rows are added in two stages */);

// batched ICP (icp_batch_*, icp_batch.cpp).  Every cloud of a batch starts at a multiple of BATCH_ALIGN elements in
// its SoA plane (x at [off], y at [plane + off], z at [2 * plane + off]); the moving clouds' matches use the same offsets, the
// model normals (point-to-plane) the model's.
// One work item = BATCH_ITEM moving points of one pair, cut from that pair's first point: one block of NN_BLOCK threads,
// the four waves scanning four contiguous quarters of the pair's model for the same points.
constexpr int BATCH_ITEM = 64;
constexpr int BATCH_ALIGN = 64;
constexpr int BATCH_APPLY = 1, BATCH_MATCH = 2;   // per-pair mode bits of one pass (0: the pair is not part of it)
struct BatchItem { int pair, first, count, pad_; };
struct BatchPair { long long p_off, q_off; int n, m, item0, item1; };   // items [item0, item1) belong to the pair, in point order
// a gated pass marks a match it rejected in the top bit of the point's device-side idx entry (indices stay below
// ICP_BATCH_MAX_POINTS); an ungated pass never sets it, so a clear bit reads "kept" whichever pass wrote the entry
constexpr int32_t BATCH_IDX_REJECTED = INT32_MIN, BATCH_IDX_MASK = INT32_MAX;
// pass over every item whose pair's mode is non-zero: [apply rt[pair] + error against idx_prev] -> [match -> idx_cur, moments]
// -> partials[item][0..last slot of the metric]; then mom[pair][ICP_NMOM] = that pair's items added in item order (pairs of
// mode 0 untouched).  F = the batch's precision.
struct BatchPassArgs {
    int precision;             // ICP_F32 / ICP_F64
    int metric;                // ICP_POINT_TO_PLANE: the sums are moments_kernel's plane terms (ICP_MOM_CNT, ICP_MOM_C .. ICP_MOM_B + 5)
    const BatchItem* items;
    int n_items;
    const BatchPair* pairs;
    int n_pairs;
    const int* mode;           // int[n_pairs]: BATCH_APPLY | BATCH_MATCH
    const void* rt;            // RT<F>[n_pairs]: R, t of the pairs that apply
    void* P_soa;               // the moving clouds
    long long p_plane;
    const void* Q_soa;         // the models
    const void* N_soa;         // point-to-plane: the model normals, laid out as Q_soa (else NULL)
    long long q_plane;
    const int32_t* idx_prev;   // the matches the error of this pass is taken against
    int32_t* idx_cur;          // the matches of this pass
    double* partials;          // [n_items][ICP_NMOM]
    double* mom;               // [n_pairs][ICP_NMOM]
    // NULL (the ungated instantiations), or F[n_pairs], every pair's squared maximum correspondence distance (+inf: that pair is
    // not gated): only matches with d <= thr[pair] enter the sums, and the error counts only the points idx_prev marks as kept
    const void* thr;
    // NULL (the fused pass, two launches), or int[n_pairs], every pair's rank K in [1, n] (0: that pair is not trimmed): the pass
    // then runs deferred, in four launches -- nn_match_batch<.., DEFER> leaves every point's winning squared distance in dist,
    // batch_trim_select writes tau[pair] = the K-th smallest of the pair's distances for the pairs that match and are trimmed, and
    // batch_trim_moments keeps the matches with d <= tau[pair] (and d <= thr[pair] where thr is given), marks the others in
    // idx_cur and forms the sums
    const int* trim_rank;
    void* dist;                // F[p_plane], laid out as idx (read and written only with trim_rank)
    void* tau;                 // F[n_pairs], +inf from the host for the pairs that are not trimmed (only with trim_rank)
    // NULL, or uint8[n_pairs], every pair's reciprocity flag, at least one of them set: the pass then runs deferred too --
    // nn_match_batch<.., DEFER>, nn_match_batch_rev (one block per model work item of q_items: rev[q_off + j] = the lowest i that
    // minimises dist2(p_i, q_j) over the pair's moving cloud as the matching launch left it, for the pairs that match and whose flag
    // is set), batch_trim_select only where trim_rank is given, and batch_trim_moments<.., MUTUAL>: kept = (flag == 0 || rev[idx[i]]
    // == i) && d <= tau[pair] (with trim_rank) && d <= thr[pair] (with thr).  Four launches + the reduction, five with trim_rank.
    const uint8_t* recip;
    int32_t* rev;              // [q_plane], laid out as the models (written only with recip; dist is needed too)
    const BatchItem* q_items;  // the model's work items (launch_batch_normals' q_items; read only with recip)
    int n_q_items;
    // NULL, or int[n_pairs], every pair's robust kernel (ICP_ROBUST_*), at least one of them not NONE: the pass then always runs
    // deferred -- nn_match_batch<.., DEFER>, nn_match_batch_rev (with recip), batch_trim_select (with trim_rank) and
    // batch_robust_moments<.., MUTUAL = recip given>: kept as batch_trim_moments decides it, w = the kernel's weight of the match's
    // residual (double), weights[i] = w (0.0 where rejected), ICP_MOM_CNT = the kept count, ICP_MOM_W = sum w, every other slot
    // the term times w; the reduction then runs to ICP_MOM_W.  Three launches with nothing else, up to five.
    const int* robust_kind;
    const double* robust_k;    // double[n_pairs]: every pair's scale k (read only where the kind is not NONE; with robust_kind)
    const double* robust_k2;   // double[n_pairs]: k * k, the host's product
    double* weights;           // double[p_plane], laid out as idx (written only with robust_kind; dist is needed too)
    // metric == ICP_GENERALIZED (never with robust_kind): the pass always runs deferred too, with the point-to-point matching
    // launch -- nn_match_batch<.., DEFER>, nn_match_batch_rev (with recip), batch_trim_select (with trim_rank) and
    // batch_gicp_moments<.., MUTUAL = recip given> (icp_k_gicp.hip): kept as batch_trim_moments decides it and det(S) finite and
    // > 0, the terms of the 6 x 6 system into a plane pass's slots; the reduction runs to ICP_MOM_B + 5.  Three launches, up to five.
    const double* cov_p;       // double[6][p_plane]: xx, xy, xz, yy, yz, zz of every moving point, in the frame of the cloud as uploaded
    const double* cov_q;       // double[6][q_plane]: ... of every model point
    const double* rot;         // double[n_pairs][9]: row-major, the rotation that carries the uploaded cloud's frame into this pass's
    // metric == ICP_COLORED (never with robust_kind): the generalized metric's launches with batch_color_moments<.., MUTUAL = recip
    // given> (icp_k_color.hip) in batch_gicp_moments' place: kept as batch_trim_moments decides it, the geometric and the photometric
    // terms of the 6 x 6 system into a plane pass's slots; the reduction runs to ICP_MOM_B + 5.  N_soa holds the model normals.
    const double* int_p;       // double[p_plane]: every moving point's intensity, laid out as idx
    const double* int_q;       // double[q_plane]: every model point's intensity, laid out as the models
    const double* grad_q;      // double[3][q_plane]: every model point's intensity gradient
    const double* color_w;     // double[n_pairs]: lambda, the weight of the geometric term, in [0, 1]
    // metric == ICP_SYMMETRIC (never with robust_kind): the generalized metric's launches with batch_sym_moments<.., MUTUAL = recip
    // given> (icp_k_sym.hip) in batch_gicp_moments' place: kept as batch_trim_moments decides it, the terms of the symmetric 6 x 6
    // system into a plane pass's slots; the reduction runs to ICP_MOM_B + 5.  rot is the generalized metric's.
    const double* nrm_p;       // double[3][p_plane]: every moving point's unit normal, in the frame of the cloud as uploaded
    const double* nrm_q;       // double[3][q_plane]: every model point's unit normal
};
hipError_t launch_batch_pass(const BatchPassArgs& a, hipStream_t st);
// batch_gicp_moments alone, on the buffers the deferred launches of launch_batch_pass left (called by it; icp_k_gicp.hip)
hipError_t launch_batch_gicp_moments(const BatchPassArgs& a, hipStream_t st);
// batch_color_moments alone, likewise (icp_k_color.hip)
hipError_t launch_batch_color_moments(const BatchPassArgs& a, hipStream_t st);
// batch_sym_moments alone, likewise (icp_k_sym.hip)
hipError_t launch_batch_sym_moments(const BatchPassArgs& a, hipStream_t st);
// evaluation of every pair whose mode is BATCH_MATCH at its present pose (icp_batch_evaluate): the deferred matching launch
// (point-to-point instantiation whatever the metric, P only read) -> idx, dist; batch_eval_moments: kept = d <= thr[pair], rejected
// matches marked in idx, the ICP_EVAL_* terms of the kept ones -> partials; batch_finalize_kernel -> mom[pair][ICP_NMOM] (pairs of
// mode 0 untouched).  Three launches.  Every buffer written here is the evaluation's own: never one of BatchPassArgs.
struct BatchEvalArgs {
    int precision;             // ICP_F32 / ICP_F64
    int metric;                // ICP_POINT_TO_POINT: sum q, sum q q^T; ICP_POINT_TO_PLANE: C (ICP_MOM_C .. + 20)
    const BatchItem* items;
    int n_items;
    const BatchPair* pairs;
    int n_pairs;
    const int* mode;           // int[n_pairs]: BATCH_MATCH for a pair to evaluate, else 0
    const void* P_soa;         // the moving clouds as they stand (read only)
    long long p_plane;
    const void* Q_soa;         // the models
    const void* N_soa;         // point-to-plane: the model normals, laid out as Q_soa (else NULL)
    long long q_plane;
    const void* thr;           // NULL (every match is kept), or F[n_pairs]: the squared distance of the evaluation (+inf: everything)
    int32_t* idx;              // [p_plane]: the matches, BATCH_IDX_REJECTED above the index of a match that was not kept
    void* dist;                // F[p_plane]: every point's winning squared distance
    double* partials;          // [n_items][ICP_NMOM]
    double* mom;               // [n_pairs][ICP_NMOM]
};
hipError_t launch_batch_evaluate(const BatchEvalArgs& a, hipStream_t st);
// the start cloud of a batch that holds initial transforms, in one launch over the same items: P[pair] = apply_rt(rt0[pair],
// P0[pair]), or P0[pair]'s bytes where kind[pair] == BATCH_INIT_COPY; nonfinite[pair] (int[n_pairs], zero before the launch)
// becomes 1 where a transformed point of the pair has a NaN or an infinite coordinate.  The padding of P is not written.
constexpr int BATCH_INIT_APPLY = 0, BATCH_INIT_COPY = 1;
hipError_t launch_batch_init(int precision, const BatchItem* items, int n_items, const BatchPair* pairs, const int* kind,
                             const void* rt0 /* RT<F>[n_pairs] */, const void* P0_soa, void* P_soa, long long p_plane, int* nonfinite,
                             hipStream_t st);
// the neighbours and normals of every pair's model: q_items = work items of BATCH_ITEM MODEL points (BatchItem::first / count
// within the pair's model); one knn4_batch launch (nbr[(q_off + i) * 4 ..]: indices within the pair's model) + one
// normals_batch_kernel launch (Nrm_soa laid out as Q_soa)
hipError_t launch_batch_normals(int precision, const BatchItem* q_items, int n_q_items, const BatchPair* pairs, const void* Q_soa,
                                long long q_plane, int32_t* nbr, void* Nrm_soa, hipStream_t st);
// voxel-grid downsampling of every cloud of a batch (icp_batch_downsample; the rule: include/icp_mi355x.h).  The 2 * n_pairs clouds
// are numbered moving clouds first, then the models; cloud c reads the planes of its side (src[side], src_plane[side]) and owns
// the elements [tmp_off, tmp_off + n) of every per-point temporary.  Work items: BATCH_ITEM points of one cloud (BatchItem::pair =
// the cloud's number), over both sides.
constexpr int VOXEL_TILE = 512;          // keys (and their points) per LDS tile of batch_voxel_group
constexpr int VOXEL_SCAN_BLOCK = 256;    // threads of batch_voxel_keys / batch_voxel_rank: one block per cloud
constexpr long long VOXEL_MAX_CELL = 2097151;   // 21 bits per axis
struct VoxelCloud { long long src_off, tmp_off, dst_off; int n, side; };   // dst_off: where the thinned cloud starts in dst[side] (read by the compaction only)
struct BatchVoxelArgs {
    int precision;             // ICP_F32 / ICP_F64
    const VoxelCloud* clouds;  // [2 * n_pairs]
    int n_clouds;
    const BatchItem* items;    // the work items of all clouds, in cloud order
    int n_items;
    const double* voxel;       // double[n_clouds]: the grid's edge, 0.0 = copy
    const void* src[2];        // P0 and Q of the source batch (read only)
    long long src_plane[2];
    long long tmp_plane;       // elements of every per-point temporary: all clouds of both sides, each at a multiple of BATCH_ALIGN
    unsigned long long* keys;  // [tmp]: the cell of every point, 21 bits per axis
    int* too_fine;             // int[n_clouds]: 1 where an axis has a cell index above VOXEL_MAX_CELL (written for every cloud)
    int32_t* first;            // [tmp]: the lowest index of the point's cell within its cloud (== its own index: it leads the cell)
    void* cent;                // F[3][tmp]: the output point of every leading point
    int32_t* rank;             // [tmp]: leading points before this one in its cloud (the output index of a leading point)
    int32_t* map;              // [tmp]: the output index of the point's cell
    int32_t* count;            // int32[n_clouds]: occupied cells
    void* dst[2];              // P0 and Q of the new batch (the compaction)
    long long dst_plane[2];
};
// batch_voxel_keys (bounds, range check, keys; one block per cloud) -> batch_voxel_group (one wave per work item: first, cent) ->
// batch_voxel_rank (one block per cloud: rank, map, count).  Three launches; dst is not read.
hipError_t launch_batch_voxel_group(const BatchVoxelArgs& a, hipStream_t st);
// batch_voxel_compact: dst[side][k * dst_plane + dst_off + rank[i]] = cent[k][i] for every leading point i.  One launch.
hipError_t launch_batch_voxel_compact(const BatchVoxelArgs& a, hipStream_t st);
// statistical and radius outlier removal of every cloud of a batch (icp_batch_remove_outliers; the rule: include/icp_mi355x.h).
// The clouds, their numbering, their stretches of the per-point temporaries and the work items are the voxel call's (VoxelCloud,
// BatchItem::pair = the cloud's number).  rules[c] is the caller's icp_outlier_rule of cloud c (kind, neighbours, value).
constexpr int OUTLIER_MAX_K = 32;           // == ICP_OUTLIER_MAX_NEIGHBOURS
constexpr int OUTLIER_MAX_GRANULES = 1024;  // ICP_BATCH_MAX_POINTS / BATCH_ITEM: the granule sums of one cloud fit one LDS array
struct OutlierRule { int kind, neighbours; double value; };   // (the layout of icp_outlier_rule)
struct BatchOutlierArgs {
    int precision;             // ICP_F32 / ICP_F64
    int cap;                   // 8, 16 or 32: the register capacity of the scan's list, >= the largest statistical k of the launch
    const VoxelCloud* clouds;  // [2 * n_pairs]
    int n_clouds;
    const BatchItem* items;    // the work items of all clouds, in cloud order
    int n_items;
    const OutlierRule* rules;  // [n_clouds]
    const void* src[2];        // P0 and Q of the source batch (read only)
    long long src_plane[2];
    long long tmp_plane;       // elements of every per-point temporary
    double* score;             // [tmp]: dbar_i (statistical), (double)c_i (radius), 0.0 (copied)
    int32_t* map;              // [tmp]: the index of a kept point in its new cloud, -1 for a removed one
    double* stats;             // double[n_clouds][4]: mean, std, thr, kept
    int32_t* count;            // int32[n_clouds]: kept points (0 where bad)
    int* bad;                  // int[n_clouds]: 1 where mean or std is not finite (written for every cloud)
    void* dst[2];              // P0 and Q of the new batch (the compaction)
    long long dst_plane[2];
};
// batch_outlier_scan (one block of NN_BLOCK threads per work item: score) -> batch_outlier_decide (one block per cloud: the
// ordered sums, stats, bad, map, count).  Two launches; dst is not read.
hipError_t launch_batch_outlier_scan(const BatchOutlierArgs& a, hipStream_t st);
// batch_outlier_compact: dst[side][k * dst_plane + dst_off + map[i]] = src[side][k * src_plane + src_off + i] for every kept i.
hipError_t launch_batch_outlier_compact(const BatchOutlierArgs& a, hipStream_t st);
// per-point covariances of the clouds of a batch (icp_batch_estimate_covariances; the rule: include/icp_mi355x.h).  The clouds and
// their numbering are the voxel call's (moving clouds first; VoxelCloud::src_off is also where the cloud starts in its covariance
// planes, tmp_off and dst_off are not read); the work items cover the clouds of the sides asked for.  One launch, icp_k_gicp.hip.
constexpr int COV_MAX_K = 32;               // == ICP_COV_MAX_NEIGHBOURS
struct BatchCovArgs {
    int precision;             // ICP_F32 / ICP_F64
    int cap;                   // 8, 16 or 32: the register capacity of the list, >= the largest k of the launch
    int regularisation;        // ICP_COV_NONE / ICP_COV_FROBENIUS
    double lambda;             // ICP_COV_FROBENIUS: added to the diagonal
    const VoxelCloud* clouds;  // [2 * n_pairs]
    const BatchItem* items;    // BatchItem::pair = the cloud's number
    int n_items;
    const int* k;              // int[2 * n_pairs]: the neighbours of every cloud that has items
    const void* src[2];        // P0 and Q (read only)
    long long src_plane[2];
    double* cov[2];            // double[6][src_plane[side]]: xx, xy, xz, yy, yz, zz, laid out as the clouds
};
hipError_t launch_batch_covariances(const BatchCovArgs& a, hipStream_t st);
// per-point intensity gradients of the models of a batch (icp_batch_estimate_intensity_gradients; the rule: include/icp_mi355x.h).
// The work items are the models' (launch_batch_normals' q_items: BatchItem::pair = the pair, first within its model).  One launch,
// icp_k_color.hip.
struct BatchGradArgs {
    int precision;             // ICP_F32 / ICP_F64
    int cap;                   // 8, 16 or 32: the register capacity of the list, >= the largest k of the launch
    const BatchItem* items;
    int n_items;
    const BatchPair* pairs;
    const int* k;              // int[n_pairs]: the neighbours of every model
    const void* Q_soa;         // the models (read only)
    const void* N_soa;         // their normals, laid out as Q_soa
    long long q_plane;
    const double* int_q;       // double[q_plane]: the models' intensities
    double* grad;              // double[3][q_plane]: x, y, z of every model point's gradient
};
hipError_t launch_batch_intensity_gradients(const BatchGradArgs& a, hipStream_t st);
// global registration (icp_k_feat.hip; the rules: include/icp_mi355x.h).  Descriptors: the clouds, their numbering, the work items
// and k are the covariance call's, over both sides; two launches, batch_spfh_kernel (-> spfh, tau) and batch_fpfh_kernel (-> feat).
// A descriptor is ICP_FEATURE_BINS doubles; point i of a cloud has its own at [(src_off + i) * ICP_FEATURE_BINS].
struct BatchFeatArgs {
    int precision;             // ICP_F32 / ICP_F64
    int cap;                   // 8, 16 or 32: the register capacity of the list, >= the largest k of the launch
    const VoxelCloud* clouds;  // [2 * n_pairs]
    const BatchItem* items;    // BatchItem::pair = the cloud's number
    int n_items;
    const int* k;              // int[2 * n_pairs]
    const void* src[2];        // P0 and Q (read only)
    long long src_plane[2];
    const double* nrm[2];      // double[3][src_plane[side]]: the caller's normals, laid out as the clouds
    void* tau[2];              // F[src_plane[side]]: the k-th smallest distance of every point (written by the first launch)
    double* spfh[2];           // double[src_plane[side]][ICP_FEATURE_BINS] (written by the first launch, read by the second)
    double* feat[2];           // double[src_plane[side]][ICP_FEATURE_BINS]
};
hipError_t launch_batch_features(const BatchFeatArgs& a, hipStream_t st);
// batch_feature_match, twice: fwd[p_off + i] = the model point of pair p whose descriptor is nearest to moving point i's (the lowest
// index on ties), rev[q_off + j] the same with the sides swapped.  items[0] / items[1]: the work items of the moving clouds / models.
struct BatchFeatMatchArgs {
    const BatchItem* items[2];
    int n_items[2];
    const BatchPair* pairs;
    const double* feat[2];
    int32_t* fwd;              // int32[p_plane]
    int32_t* rev;              // int32[q_plane]
};
hipError_t launch_batch_feature_match(const BatchFeatMatchArgs& a, hipStream_t st);
// batch_score_transforms: counts[pair * per_pair + c] = the entries e < cn[pair] of the pair's correspondence list (ci, cj: int32,
// at p_off + e; indices within the pair's clouds) with dist2(cand . P0[ci[e]], Q[cj[e]]) <= thr[pair] and a finite moved point.
struct BatchScoreArgs {
    int precision;
    const BatchPair* pairs;
    int n_pairs;
    const int* cn;             // int[n_pairs]
    const int32_t* ci;
    const int32_t* cj;
    const void* P0;
    long long p_plane;
    const void* Q;
    long long q_plane;
    const void* cand;          // F[n_pairs][per_pair][12]: R row-major, then t
    const uint8_t* valid;      // uint8[n_pairs][per_pair], or NULL: every candidate is scored
    const void* thr;           // F[n_pairs]
    int per_pair;
    int32_t* counts;           // int32[n_pairs][per_pair]
};
hipError_t launch_batch_score(const BatchScoreArgs& a, hipStream_t st);
// Fast Global Registration (icp_batch_fgr): one iteration's sums, or the weights at the final pose.  Every pair's used list is a
// compacted (ui, uj) index list (int32 at p_off + e, e < U_p; indices within the pair's clouds); the work items cut it into
// BATCH_ITEM entries (BatchItem::first = the first entry).  ctl holds FGR_CTL doubles per pair: the upper three rows of T
// row-major (12), mu, and a flag -- 0.0: the pair takes no part, its blocks return and its row of mom is not written.
//   launch_batch_fgr_terms    batch_fgr_terms<F, false> (one block per item: the terms of the header's rule -> a row of partials,
//                             slots 0 .. ICP_MOM_W) + batch_fgr_finalize (one block per pair: its items' rows in
//                             batch_finalize_kernel's fixed order -> mom[pair][ICP_NMOM], zeros behind ICP_MOM_W).  Two launches.
//   launch_batch_fgr_weights  batch_fgr_terms<F, true>: weights[p_off + ui[e]] = l of entry e (0.0 where the moved point or r2 is
//                             not finite); nothing else is written.  One launch.
constexpr int FGR_CTL = 14, FGR_CTL_MU = 12, FGR_CTL_RUN = 13;
struct BatchFgrArgs {
    int precision;
    const BatchItem* items;
    int n_items;
    const BatchPair* pairs;
    int n_pairs;
    const int* item0;          // int[n_pairs + 1]: items [item0[p], item0[p + 1]) belong to pair p, in list order
    const int32_t* ui;
    const int32_t* uj;
    const void* P0;
    long long p_plane;
    const void* Q;
    long long q_plane;
    const double* ctl;         // double[n_pairs][FGR_CTL]
    double* partials;          // [n_items][ICP_NMOM]
    double* mom;               // [n_pairs][ICP_NMOM]
    double* weights;           // double[p_plane], laid out as idx (written by launch_batch_fgr_weights only)
};
hipError_t launch_batch_fgr_terms(const BatchFgrArgs& a, hipStream_t st);
hipError_t launch_batch_fgr_weights(const BatchFgrArgs& a, hipStream_t st);
// keypoint selection of every cloud of a batch (icp_batch_select_keypoints; the rule: include/icp_mi355x.h; icp_k_keypoint.hip).
// The clouds, their numbering, their stretches of the per-point temporaries and the work items are the outlier call's (VoxelCloud,
// BatchItem::pair = the cloud's number).  rules[c] is the caller's icp_keypoint_rule of cloud c.
struct KeypointRule { int kind, min_neighbours; double salient_radius, non_max_radius, gamma_21, gamma_32; };   // (the layout of icp_keypoint_rule)
struct BatchKeypointArgs {
    int precision;             // ICP_F32 / ICP_F64
    const VoxelCloud* clouds;  // [2 * n_pairs]
    int n_clouds;
    const BatchItem* items;    // the work items of all clouds, in cloud order
    int n_items;
    const KeypointRule* rules; // [n_clouds]
    const void* src[2];        // P0 and Q of the source batch (read only)
    long long src_plane[2];
    long long tmp_plane;       // elements of every per-point temporary
    double* sal;               // [tmp]: sal_i, 0.0 for a copied cloud
    int32_t* map;              // [tmp]: the index of a kept point in its new cloud, -1 for a dropped one (between the launches: the flag)
    int32_t* count;            // int32[n_clouds]: kept points
    void* dst[2];              // P0 and Q of the new batch (the compaction)
    long long dst_plane[2];
    const unsigned long long* src_feat[2];   // the source's descriptors of that side as 64-bit words ([src_plane][ICP_FEATURE_BINS]), or NULL: it holds none
    unsigned long long* dst_feat[2];         // the new batch's, laid out by dst_off (read where src_feat is not NULL)
};
// batch_iss_saliency + batch_iss_select (one block of NN_BLOCK threads per work item: sal, then the flags) -> batch_keypoint_rank
// (one block per cloud: map, count).  Three launches; dst and the descriptors are not read.
hipError_t launch_batch_keypoint_select(const BatchKeypointArgs& a, hipStream_t st);
// batch_keypoint_compact: a kept point's coordinates to dst[side][k * dst_plane + dst_off + map[i]], its descriptor to
// dst_feat[side][(dst_off + map[i]) * ICP_FEATURE_BINS ..].  One launch.
hipError_t launch_batch_keypoint_compact(const BatchKeypointArgs& a, hipStream_t st);
// point normals of every cloud of a batch from its stored covariances (icp_batch_estimate_point_normals; the rule:
// include/icp_mi355x.h; icp_k_normals.hip).  The clouds and their numbering are the covariance call's (moving clouds first;
// VoxelCloud::src_off is where the cloud starts in its coordinate, covariance and normal planes); the work items cover every cloud of
// both sides (BatchItem::pair = the cloud's number).
struct BatchNormalsArgs {
    int precision;             // ICP_F32 / ICP_F64
    int orient;                // ICP_ORIENT_NONE / _VIEWPOINT / _CENTROID
    const VoxelCloud* clouds;  // [2 * n_pairs]
    int n_clouds;
    const BatchItem* items;
    int n_items;
    const void* src[2];        // P0 and Q (read only)
    long long src_plane[2];
    const double* cov[2];      // double[6][src_plane[side]]: xx, xy, xz, yy, yz, zz
    const double* view;        // double[n_clouds][3]: what the normals of each cloud face (ICP_ORIENT_CENTROID: == cent); not read with ICP_ORIENT_NONE
    double* cent;              // double[n_clouds][3]: written by batch_centroid_kernel (ICP_ORIENT_CENTROID only)
    double* nrm[2];            // double[3][src_plane[side]]: x, y, z, laid out as the clouds
};
// [batch_centroid_kernel (one block per cloud: cent), ICP_ORIENT_CENTROID only ->] batch_point_normals_kernel (one wave per work
// item: nrm).  One launch, or two.
hipError_t launch_batch_point_normals(const BatchNormalsArgs& a, hipStream_t st);
// the dominant plane of every cloud of a batch (icp_batch_segment_plane; the rule: include/icp_mi355x.h; icp_k_segment.hip).  The
// clouds, their numbering, their stretches of the per-point temporaries and the work items are the outlier call's.  The host draws
// and solves the hypotheses; the device counts their inliers, sums the winner's moments and decides every point.
constexpr int PLANE_GROUP = 32;            // hypotheses per block of batch_plane_score: one integer counter each, in registers
constexpr int PLANE_SLICE = 4096;          // points per block of batch_plane_score: a large cloud is cut over several blocks
struct PlaneJob {                          // one per cloud
    double win[4];                         // the winning hypothesis: nx, ny, nz, d (zeros: none)
    double fit[4];                         // its refit (read where fit_ok)
    double distance;
    int kind;                              // ICP_PLANE_*
    int has_plane;                         // a valid hypothesis exists
    int win_count;                         // the winner's inliers
    int fit_ok;                            // the refit exists and passed the axis test
};
struct BatchPlaneArgs {
    int precision;             // ICP_F32 / ICP_F64
    const VoxelCloud* clouds;  // [2 * n_pairs]
    int n_clouds;
    const BatchItem* items;    // the work items of all clouds, in cloud order (the compaction's)
    int n_items;
    const void* src[2];        // P0 and Q of the source batch (read only)
    long long src_plane[2];
    long long tmp_plane;       // elements of every per-point temporary
    int32_t* map;              // [tmp]: the index of a kept point in its new cloud, -1 for a removed one
    int32_t* count;            // int32[n_clouds]: kept points
    void* dst[2];              // P0 and Q of the new batch (the compaction)
    long long dst_plane[2];
    // batch_plane_score
    const BatchItem* slices;   // PLANE_SLICE points of one searched cloud each (BatchItem::pair = the cloud's number)
    int n_slices;
    int per;                   // hypotheses per cloud of this launch: a multiple of PLANE_GROUP
    const double* planes;      // double[n_clouds][per][4]
    const uint8_t* valid;      // uint8[n_clouds][per]: 0 = the hypothesis is not counted
    const double* distance;    // double[n_clouds]
    int32_t* counts;           // int32[n_clouds][per], zero before the launch: the blocks of a cloud add their integers
    // batch_plane_refit, batch_plane_decide
    const PlaneJob* jobs;      // [n_clouds]
    double* moments;           // double[n_clouds][9]: the centroid, then xx, xy, xz, yy, yz, zz of the winner's inliers
    uint8_t* mask;             // uint8[tmp]: 1 = the point lies on the returned plane
    int32_t* inliers;          // int32[n_clouds]: the returned plane's count
    int* chosen;               // int[n_clouds]: 1 = the refit is returned, 0 = the winner, -1 = no plane
};
// batch_plane_score<F>: grid (n_slices, per / PLANE_GROUP).  One launch.
hipError_t launch_batch_plane_score(const BatchPlaneArgs& a, hipStream_t st);
// batch_plane_refit<F>: one block per cloud -> moments.  One launch.
hipError_t launch_batch_plane_refit(const BatchPlaneArgs& a, hipStream_t st);
// batch_plane_decide<F>: one block per cloud -> chosen, inliers, mask, map, count.  One launch.  The compaction is the outlier
// call's (launch_batch_outlier_compact: the same clouds, items, map and planes).
hipError_t launch_batch_plane_decide(const BatchPlaneArgs& a, hipStream_t st);

// soa2 (optional): a second copy of the result (the pristine moving cloud); enc (optional, fp32): the cloud's bounding cube as six
// ordered-integer words {~ord(min xyz), ord(max xyz)}, zero before the launch
hipError_t launch_aos_to_soa(int precision, const void* aos, int n, int n_pad, void* soa, hipStream_t st, unsigned int* nonfinite = nullptr, void* soa2 = nullptr,
                             unsigned int* enc = nullptr);
hipError_t launch_soa_to_aos(int precision, const void* soa, int n, int n_pad, void* aos, hipStream_t st);

// model-on-model 4 nearest neighbours (self / rank 0 dropped)
hipError_t launch_knn4(const NNPlan& pl, const void* Q_soa, int32_t* nbr /*[m][4]*/, hipStream_t st);
// fp32: packed, wave-/segment-split top-5 kernel + merge.  part_* hold splits * n_pad * 5 entries.
void knn4_v2_geometry(int m, int num_cus, int* n_pad, int* blocks_x, int* splits, int* seg_len);
int knn4_v2_wave_tiles(int seg_len);   // LDS tiles each of a block's four waves streams its quarter of a segment through
hipError_t launch_knn4_v2(const void* Q_soa, int m, int num_cus, float* part_d, int32_t* part_j, int32_t* nbr,
                          hipStream_t st);
// covariance of the 4 neighbours + fp64 Jacobi eigen-solve per lane -> padded SoA normals on the device
hipError_t launch_normals(int precision, const void* Q_soa, int m, int m_pad, const int32_t* nbr, void* Nrm_soa,
                          hipStream_t st);
hipError_t launch_os1_packets(const uint8_t* packets, int n_packets, const float* alt16, const float* az16,
                              uint32_t* ranges, float* xyz_aos, hipStream_t st);
hipError_t launch_os1_conversion(const uint32_t* ranges, int n, uint32_t encoder0, const float* alt16,
                                 const float* az16, float* xyz_aos, hipStream_t st);

}  // namespace icp
