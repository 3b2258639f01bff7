// icp_plan.h -- the launch plan of a matching pass: which kernel family a pair of clouds runs (NNFamily), its geometry (NNPlan),
// the context's switches (NNTuning), what a family can carry, and the waves and rounds of one launch (nn_launch_shape).
// Pure host logic: nothing here, or in icp_plan.cpp, calls HIP -- tests/plan_check.cpp runs all of it without a device.
// The dispatch that turns a plan into a launch is icp_launch.hip.  Internal to libicp_mi355x.so.
#pragma once
#include <cstddef>

#include "../../include/icp_mi355x.h"

namespace icp {

// Internal HBM layout of a cloud: SoA, x[pad] | y[pad] | z[pad], `pad` >= count.
//   moving cloud: pad = multiple of NN_POINT_ALIGN (whole NN blocks, no bounds checks in the hot loop)
//   model  cloud: pad = multiple of NN_CHUNK; entries [m, m_pad) replicate point m-1, which can
//                 never win a first-minimum search against its lower-index original.
constexpr int NN_BLOCK = 256;        // threads per matching block (4 wave64)
constexpr int NN_POINT_ALIGN = 1024; // moving-point padding granule
constexpr int NN_CHUNK = 16;         // model points per index-tracking chunk

// geometry of the sparse kernels' blocks and hit lists (nn_launch_shape sizes a launch's rounds by these)
constexpr int SP_NW = 16;                       // waves per block (the default; NWS = 8 is the other instantiation)
constexpr int SP_HCAP = 4096;                   // hit-list entries of the hierarchical search = chunks per round (SP_NW * 64 * passes <= this)
constexpr int SP_MAX_PASSES = SP_HCAP / (SP_NW * 64);
// flat search (models below 2^19 points = 65 536 chunks): the list holds 16-bit chunk numbers, twice as many in the same
// 16 KB -- a model of up to 65 536 points is one round of the find (Bunny.csv: 5040 chunks, two rounds with 4096 entries)
constexpr int SP_HCAP_FLAT = 2 * SP_HCAP;
constexpr int R64_NW = 8;                       // rows of 64 points: waves per block (16 with the device to itself)
constexpr int NN_ROLE_ROW_BITS = 21, NN_ROLE_PART_BITS = 6;   // ordered rows: role = row | part << 21 | log2(parts) << 27

// The kernel a plan runs (DESIGN.md section 4 has the table: condition, kernel, waves, what each can carry).
enum class NNFamily {
    Dense,        // nn_match_kernel: one thread per point, every pair (dense fp64; A/B)
    DensePacked,  // nn_match_f32_v2: packed fp32, every pair; its seeded early-out variant where the plan says cull
    Row64,        // nn_match_row64: fp32, rows of 64 points, flat search
    Row128,       // nn_match_sparse: fp32, rows of 128 points, flat or hierarchical search
    Row64F64      // nn_match_row64_f64: fp64 on the structure of Row64
};

struct NNPlan {
    int precision;  // ICP_F32 / ICP_F64
    int n, m;       // real counts
    int n_pad, m_pad;
    NNFamily family;
    int num_cus;        // the CUs the plan was made for (nn_plan's argument, 256 where that is unknown)
    int pts_per_thread; // T
    int blocks_x;       // n_pad / (NN_BLOCK * T); the rows of the Row* families
    int splits;         // S: model segments scanned by different blocks (grid.y); 0: an empty cloud, nothing is launched
    int seg_len;        // model points per segment (multiple of NN_CHUNK)
    int chunk;          // index-tracking chunk of the launched kernel
    int cull;           // the packed kernel may use the seeded-bound / xy early-out variant
    int hier;           // Row128: two-level search (boxes of 64 chunks first) -- large models
    int row;            // Row* families: moving points per block row -- 128 or 64 (0: the dense families)
    int nw;             // Row128: waves per block -- 16, or 8 (two blocks per CU: clouds whose rows outnumber the CUs; launches with a fused tail),
                        // or 4 (four per CU: the hierarchical search of clouds with rows for several rounds of blocks)
    int share_blocks;   // Row128, 8 waves, one launch per pass: blocks of a launch (> blocks_x: the spare ones go to the heavy rows), or 0
    int order;          // Row128, many more rows than the machine holds at once: the blocks of a launch take the rows heaviest first
                        // (by the hits of the launch before) -- see launch_row_order
};

// Every switch the plan and the launchers look at, read ONCE per context (icp_create -> nn_tuning_from_env): nothing on the
// launch path scans the environment (the advisor's finding on round 3), and a test that wants another form creates another
// context.  Defaults = production.  All of these select among forms that give the same bits (INTEGRATION.md lists them).
struct NNTuning {
    int sparse = 1;          // ICP_NN_SPARSE=0: the dense packed kernel (every pair executed; no boxes, no hierarchy)
    int cull = 1;            // ICP_NN_CULL=0: ... without its seeded early-out
    int row = 0;             // ICP_NN_ROW=64 / 128: force the row size of the sparse kernels
    int waves64 = 0;         // ICP_NN_WAVES=16: rows of 64 points as 16-wave blocks (what icp_set_exclusive selects)
    int waves128 = 0;        // ICP_NN_WAVES128=4 / 8 / 16: waves per block of the rows of 128
    int cold8 = 1;           // ICP_NN_COLD8=0: a plan of 4-wave blocks runs its cold launches on 4 waves too
    int hier = -1;           // ICP_NN_HIER=0 / 1: box hierarchy never / always (-1: by the model's size)
    int order = 1;           // ICP_NN_ORDER=0 / 2: rows in index order / heaviest first also where the rows are few
    int share = 1;           // ICP_NN_SHARE=0: no shared rows
    int share_resident = 1;  // ICP_NN_SHARE_RESIDENT=0: a resident launch keeps one block per row
    int speculate = 1;       // ICP_NN_SPECULATE=0: resident launches without their speculative hit list
    int f64_sparse = 1;      // ICP_F64_SPARSE=0: ICP_F64 clouds on the dense thread-per-point kernel
    int sort = -1;           // ICP_SORT=0 / 1: spatially sorted views never / always (-1: by the extent test)
    // ICP_NN_PHASES=file[:pass[:slots[:wipe]]] -- per-wave phase stamps of the matching kernels (tools/phase_report.py); the
    // context owns the log
    long long* phase_log = nullptr;
    long long phase_cap = 0;
    int phase_pass = -1;
    int phase_wipe = 0;
};
NNTuning nn_tuning_from_env();

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
inline int pad_moving(int n) { return n <= 0 ? 0 : round_up(n, NN_POINT_ALIGN); }
inline int pad_model(int m) { return m <= 0 ? 0 : round_up(m, NN_CHUNK); }
size_t elem_size(int precision);

// Choose the family and its geometry.  `num_cus` comes from hipDeviceProp_t::multiProcessorCount.
// force_dense != 0: the geometry of the dense packed kernel (every pair executed) even where the sparse kernel would run
NNPlan nn_plan(int n, int m, int precision, int num_cus, const NNTuning& tune, int force_dense = 0);

// ---- what a plan's family can carry: each written once, here ----
// the geometry is a sparse kernel's: blocks own rows of moving points and search the model through its chunk boxes
inline bool nn_is_sparse(const NNPlan& pl) { return pl.family == NNFamily::Row64 || pl.family == NNFamily::Row128 || pl.family == NNFamily::Row64F64; }
// the transform of the previous pass fused into the kernel's front (NNFusedTransform) / the row tail fused into its end (NNTailArgs)
bool nn_can_fuse_transform(const NNPlan& pl);
bool nn_can_fuse_tail(const NNPlan& pl);
// a fused launch keeps its points and matches in slot order (NNFusedTransform::slot_state): unsplit rows of 128
inline bool nn_keeps_slot_order(const NNPlan& pl) { return pl.family == NNFamily::Row128 && pl.splits == 1; }
// the kernel can add its rows up inside the launch (NNTailArgs::fin_*)
inline bool nn_can_sum_rows_in_launch(const NNPlan& pl) { return pl.family == NNFamily::Row128; }
// moving points a block works on together: what the cloud's spatial order is judged by (decide_moving_order)
inline int nn_moving_group(const NNPlan& pl) { return (pl.family == NNFamily::Row64 || pl.family == NNFamily::Row64F64) ? 64 : 128; }
// Some cloud would search this model through the box hierarchy.  The model is set before the cloud is known, and it gets the
// upper levels and the records whenever this says so (icp_set_model).
bool nn_model_may_be_hier(int m, int precision, const NNTuning& tune);

// ---- the waves and rounds of one launch ----
struct NNLaunchKind {
    bool has_tail;        // the launch carries a fused tail (NNTailArgs)
    bool cold;            // no previous match: neither seeds nor valid slots
    bool order_history;   // ordered rows whose counters hold an EARLIER registration's hits too
    bool exclusive16;     // the context has the device to itself (icp_set_exclusive)
};
struct NNLaunchShape {
    int waves;        // per block: 4, 8 or 16
    int max_passes;   // rounds of 64 x waves hit-list entries a seeded or sampled find may take (0: the dense families list nothing)
};
NNLaunchShape nn_launch_shape(const NNPlan& pl, const NNLaunchKind& kind, const NNTuning& tune);
// threads per block as icp_nn_launch_info reports them: the steady launch with a tail, not exclusive, default switches.
// Row64F64 reports 512 (see the note at icp_nn_launch_info).
int nn_block_threads(const NNPlan& pl);

}  // namespace icp
