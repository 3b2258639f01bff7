// icp_plan.cpp -- the launch plan (icp_plan.h): the switches, the family of a pair of clouds, one function per family for its
// geometry, what a family can carry, the shape of one launch.  Host arithmetic only; the measured reasons for every border are
// next to the line that draws it.
#include "icp_plan.h"

#include <stdlib.h>

namespace icp {

size_t elem_size(int precision) { return precision == ICP_F64 ? sizeof(double) : sizeof(float); }

static int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return atoi(v);
}

// the context's switches, read once (icp_create); ICP_NN_PHASES is parsed by the caller, who owns the log's memory
NNTuning nn_tuning_from_env()
{
    NNTuning t;
    t.sparse = env_int("ICP_NN_SPARSE", 1) ? 1 : 0;
    t.cull = env_int("ICP_NN_CULL", 1) ? 1 : 0;
    t.row = env_int("ICP_NN_ROW", 0);
    t.waves64 = env_int("ICP_NN_WAVES", 0);
    t.waves128 = env_int("ICP_NN_WAVES128", 0);
    t.cold8 = env_int("ICP_NN_COLD8", 1) ? 1 : 0;
    t.hier = env_int("ICP_NN_HIER", -1);
    t.order = env_int("ICP_NN_ORDER", 1);
    t.share = env_int("ICP_NN_SHARE", 1) ? 1 : 0;
    t.share_resident = env_int("ICP_NN_SHARE_RESIDENT", 1) ? 1 : 0;
    t.speculate = env_int("ICP_NN_SPECULATE", 1) ? 1 : 0;
    t.f64_sparse = env_int("ICP_F64_SPARSE", 1) ? 1 : 0;
    t.sort = env_int("ICP_SORT", -1);
    return t;
}

// ------------------------------------------------------------------------------------------------
// the family
// ------------------------------------------------------------------------------------------------
// The flat search lists 16-bit chunk numbers: a model of more than 65 536 chunks of 8 is out of its reach.
static bool beyond_flat_search(int m_pad) { return (m_pad >> 3) > 65536; }

// What the model's size alone says about the hierarchy, before the cloud has a say (ICP_NN_HIER = 0 / 1 overrides): from 2^17
// points up, where the flat pass over the chunk boxes starts to dominate.  A model this says yes to is never given rows of 64.
static bool model_asks_for_hier(int m_pad, const NNTuning& tune) { return tune.hier >= 0 ? tune.hier != 0 : m_pad >= (1 << 17); }

static NNFamily choose_family(const NNPlan& pl, const NNTuning& tune, int force_dense)
{
    const bool empty = pl.n <= 0 || pl.m <= 0;
    if (pl.precision == ICP_F32) {
        if (!tune.sparse || force_dense) return NNFamily::DensePacked;
        if (empty) return NNFamily::Row128;   // (never launched; its buffers are sized as rows of 128)
        // 64-point rows (nn_match_row64: 8 waves per block, one point per lane, one segment) for clouds that cannot
        // fill the machine with 128-point rows and whose model is searched flat; ICP_NN_ROW = 64 / 128 overrides
        // (two 8-wave blocks fit a CU: 512 rows of 64 = 32 768 points can stay on the machine for a whole registration)
        const bool row64 = !model_asks_for_hier(pl.m_pad, tune) && (tune.row == 64 || (tune.row != 128 && pl.n_pad / 64 <= 2 * pl.num_cus));
        return row64 ? NNFamily::Row64 : NNFamily::Row128;
    }
    // fp64 on the sparse structure (nn_match_row64_f64: rows of 64 points, one launch per pass): up to two blocks per CU
    // and a model that is searched flat; ICP_F64_SPARSE=0 keeps the dense thread-per-point kernel
    if (pl.precision == ICP_F64 && !force_dense && !empty && tune.sparse && tune.f64_sparse && pl.n_pad / 64 <= 2 * pl.num_cus && pl.m_pad < (1 << 17))
        return NNFamily::Row64F64;
    return NNFamily::Dense;
}

// (the CU count has no say: whatever the machine holds, some cloud has more rows than that)
bool nn_model_may_be_hier(int m, int precision, const NNTuning& tune)
{
    if (precision != ICP_F32 || m <= 0 || !tune.sparse) return false;   // only Row128 searches through the hierarchy
    const int m_pad = pad_model(m);
    if (model_asks_for_hier(m_pad, tune)) return true;   // every cloud gets rows of 128 and the hierarchy
    if (tune.row == 64) return false;                    // every cloud gets rows of 64, which search flat
    // a cloud with rows of 128 for more than two rounds of blocks: fill_row128's rule at its far end (cloud_asks_for_hier)
    return beyond_flat_search(m_pad) || (tune.hier < 0 && m_pad >= (1 << 16));
}

// ------------------------------------------------------------------------------------------------
// the geometry, family by family
// ------------------------------------------------------------------------------------------------
// Split the model into S segments (grid.y) until the launch has `target_blocks` blocks, no segment shorter than `min_seg`
// points, every segment a multiple of `granule`; S is what is left after the rounding.
static void split_model(NNPlan& pl, int target_blocks, int min_seg, int granule)
{
    int S = (target_blocks + pl.blocks_x - 1) / pl.blocks_x;
    const int max_S = (pl.m_pad + min_seg - 1) / min_seg;
    if (S > max_S) S = max_S;
    if (S < 1) S = 1;
    pl.seg_len = round_up((pl.m_pad + S - 1) / S, granule);
    pl.splits = (pl.m_pad + pl.seg_len - 1) / pl.seg_len;
}

// what the three sparse families share: the seeded early-out over chunks of 8
static void fill_sparse(NNPlan& pl, int row, int pts_per_thread)
{
    pl.cull = 1;
    pl.chunk = 8;
    pl.row = row;
    pl.pts_per_thread = pts_per_thread;
    pl.blocks_x = pl.n_pad / row;
}

// rows of 64 points, fp32 and fp64: one segment, the model searched flat
static void fill_row64(NNPlan& pl)
{
    fill_sparse(pl, 64, pl.family == NNFamily::Row64F64 ? 1 : 2);
    pl.splits = 1;
    pl.seg_len = round_up(pl.m_pad, 8);
}

// rows of 128 points: a block of 16 waves owns 128 moving points
static void fill_row128(NNPlan& pl, const NNTuning& tune)
{
    const int num_cus = pl.num_cus;
    fill_sparse(pl, 128, 2);
    if (pl.n <= 0 || pl.m <= 0) return;
    // large models are searched in two levels (boxes of 64 chunks first): from 2^17 points up (model_asks_for_hier)
    // (round 2: with 16 hits per fetch and the rows taken heaviest first the hierarchy pays from 2^16 model points when
    // the cloud has more rows than shared 8-wave blocks could serve -- 90 000^2: 101.9 -> 87.4 us per iteration,
    // 131 044^2: 152.3 -> 117.9, 65 536^2: 80.6 -> 77.6)
    const bool cloud_asks_for_hier = tune.hier < 0 && pl.m_pad >= (1 << 16) && pl.blocks_x > 2 * num_cus - num_cus / 4;
    pl.hier = (model_asks_for_hier(pl.m_pad, tune) || cloud_asks_for_hier || beyond_flat_search(pl.m_pad)) ? 1 : 0;
    // split the model only while there are fewer blocks than CUs, and never below 1024 model points per block
    // (an unsplit row closes without the key/ticket exchange, worth ~3 us: prefer it from half a machine up)
    split_model(pl, num_cus / 2, 1024, pl.hier ? 512 : 8);   // (a segment starts on a super-box boundary)
    const bool unsplit = pl.splits == 1;
    // Rows of 128 that outnumber the CUs (one 16-wave block each: a second round of blocks) but fit the machine as
    // 8-wave blocks, two to a CU: the 8-wave form, and -- one launch per pass -- the blocks the machine has room for
    // beyond the rows go to the heavy rows (shared rows, see nn_match_sparse).  ICP_NN_WAVES128 = 8 / 16 and
    // ICP_NN_SHARE = 0 override.
    const int w128 = tune.waves128;
    pl.nw = 16;
    // (without spare blocks the 8-wave form loses: 65 536 points = 512 rows, 88 us per iteration against 79 with 16 waves
    // in two rounds; with an eighth of the machine to spare it wins -- 50 176 points: 39.6 against 53.4)
    // The hierarchical search with rows for several rounds of blocks runs them as 8-wave blocks as well, two to a CU: late in
    // a registration a block is a chain of short dependent steps (front end, three levels of boxes, a handful of hits, the
    // row's close: ~19 us for a median of 110 hits) and a second block on the CU fills the waits of the first -- 10 M x 10 M on
    // one GPU: 11.2 -> 8.3 ms per iteration, every pass faster (the first 35.0 -> 33.9 ms, the thirtieth 5.4 -> 3.3)
    // ... and 4-wave blocks, four to a CU: 8.4 -> 7.5 ms (the thirtieth pass 3.2 -> 2.5 ms; the first, cold, stays on 8 waves)
    if (pl.hier && unsplit && w128 != 16 && (w128 == 8 || w128 == 4 || pl.blocks_x >= 2 * num_cus)) pl.nw = w128 == 8 ? 8 : 4;
    if (!pl.hier && unsplit && (w128 == 8 || (w128 != 16 && pl.blocks_x > num_cus && pl.blocks_x <= 2 * num_cus - num_cus / 4))) {
        pl.nw = 8;
        if (tune.share && pl.blocks_x < 2 * num_cus && pl.blocks_x <= 8 * 64) pl.share_blocks = 2 * num_cus;
    }
    // large models (hierarchical search), at least two rounds of blocks: the rows are taken heaviest first (launch_row_order)
    // (ICP_NN_ORDER = 0: index order; 2: also where the rows are few -- the parity tests)
    pl.order = (pl.hier && unsplit && tune.order && (tune.order == 2 || pl.blocks_x >= 2 * num_cus) && pl.blocks_x < (1 << NN_ROLE_ROW_BITS)) ? 1 : 0;   // (a role holds 21 bits of row)
}

// the packed fp32 kernel over every pair: a block (4 waves) owns 64*T moving points, each wave a quarter of the block's segment.
// 8 resident waves per SIMD = 8 blocks per CU saturate the VALU (valu_rate probe).
// (the sweeps that chose these -- points per lane, chunk, blocks per CU, segments: profiles/r1/03_nn_sweep_cull.txt,
// profiles/r3/r3_09_dense_kernel_sweep.txt -- are settled; their switches are gone)
static void fill_dense_packed(NNPlan& pl, const NNTuning& tune)
{
    const int target_blocks = pl.num_cus * 8;
    const int T = (pl.n_pad / 256 >= target_blocks) ? 4 : 2;   // big clouds: 4 points per lane halve the LDS reads
    pl.cull = (T == 2 && tune.cull) ? 1 : 0;
    pl.chunk = pl.cull ? 8 : 16;   // 16 partial sums per chunk would spill under the 64-VGPR cap
    pl.pts_per_thread = T;
    pl.blocks_x = pl.n_pad / (64 * T);
    if (pl.n <= 0 || pl.m <= 0) return;
    split_model(pl, target_blocks, 512, 4 * pl.chunk);   // keep >= 128 model points per wave; four wave quarters of whole chunks
}

// one thread per point (NNCfg of icp_k_dense.hip)
static void fill_dense(NNPlan& pl)
{
    pl.chunk = NN_CHUNK;
    pl.pts_per_thread = pl.precision == ICP_F64 ? 2 : 4;
    pl.blocks_x = pl.n_pad / (NN_BLOCK * pl.pts_per_thread);
    if (pl.n <= 0 || pl.m <= 0) return;
    // small clouds cannot fill 256 CUs along the moving axis alone: split the model range over
    // grid.y until every CU holds 2 blocks of 4 waves; keep >= 256 model points per segment
    split_model(pl, pl.num_cus * 2, 256, NN_CHUNK);
}

NNPlan nn_plan(int n, int m, int precision, int num_cus, const NNTuning& tune, int force_dense)
{
    NNPlan pl{};
    pl.precision = precision;
    pl.n = n;
    pl.m = m;
    pl.n_pad = pad_moving(n);
    pl.m_pad = pad_model(m);
    pl.num_cus = num_cus > 0 ? num_cus : 256;
    pl.family = choose_family(pl, tune, force_dense);
    switch (pl.family) {
        case NNFamily::Dense: fill_dense(pl); break;
        case NNFamily::DensePacked: fill_dense_packed(pl, tune); break;
        case NNFamily::Row64:
        case NNFamily::Row64F64: fill_row64(pl); break;
        case NNFamily::Row128: fill_row128(pl, tune); break;
    }
    return pl;
}

// ------------------------------------------------------------------------------------------------
// what a family can carry
// ------------------------------------------------------------------------------------------------
bool nn_can_fuse_transform(const NNPlan& pl) { return pl.family != NNFamily::Dense && pl.n > 0 && pl.m > 0; }

// (of the packed kernel over every pair only the early-out instantiation -- 2 points per lane, chunks of 8 -- has a tail)
bool nn_can_fuse_tail(const NNPlan& pl)
{
    return (nn_is_sparse(pl) || (pl.family == NNFamily::DensePacked && pl.cull)) && pl.n > 0 && pl.m > 0;
}

// ------------------------------------------------------------------------------------------------
// the shape of one launch
// ------------------------------------------------------------------------------------------------
NNLaunchShape nn_launch_shape(const NNPlan& pl, const NNLaunchKind& kind, const NNTuning& tune)
{
    switch (pl.family) {
        case NNFamily::Row64: {
            // sixteen waves where the context asks for them and every row has a CU to itself
            const int nw = ((tune.waves64 == 16 || kind.exclusive16) && pl.blocks_x <= pl.num_cus) ? 16 : R64_NW;
            return {nw, SP_HCAP / (nw * 64)};
        }
        case NNFamily::Row64F64: {
            const int nw = pl.blocks_x <= pl.num_cus ? 16 : 8;
            return {nw, SP_HCAP / (nw * 64)};
        }
        case NNFamily::Row128: {
            // 8-wave blocks exist with a fused tail only, 4-wave blocks with a fused tail and the hierarchical search only.  A plan
            // of 4-wave blocks runs its COLD launches (no previous match: every block starts from the sample round, and the rows
            // are split by counters that are a registration old) on 8 waves: 10 M x 10 M, first pass 34.9 ms against 44.1
            // (... unless the rows' counters hold a registration's history -- a context's second registration on: the cold pass of a
            // repeat then splits its heavy rows about right and the 4-wave form wins, 5.13 -> 5.04 ms per iteration; without history
            // the share of one rank of eight ran its first registration in 24.1 ms on 8 waves against 26.3 on 4)
            const bool cold8 = kind.cold && tune.cold8 && !kind.order_history;
            const int nw = (pl.nw == 8 && kind.has_tail) ? 8 : (pl.nw == 4 && kind.has_tail && pl.hier) ? (cold8 ? 8 : 4) : SP_NW;
            return {nw, pl.hier ? SP_MAX_PASSES : SP_HCAP_FLAT / (nw * 64)};
        }
        case NNFamily::Dense:
        case NNFamily::DensePacked: break;
    }
    return {NN_BLOCK / 64, 0};
}

int nn_block_threads(const NNPlan& pl)
{
    if (pl.family == NNFamily::Row64F64) return R64_NW * 64;
    return 64 * nn_launch_shape(pl, NNLaunchKind{true, false, false, false}, NNTuning{}).waves;
}

}  // namespace icp
