// plan_check.cpp -- csrc/icp_plan.cpp on the CPU.  Built and run by tests/test_plan.py (with the address and undefined-behaviour
// sanitizers); prints one line per check and exits 0 when all hold.  Three things:
//   * TABLE.  nn_plan over a grid of (n, m, precision, CUs, force_dense, switches) that takes every border of the plan on both
//     sides, one line per plan with every field NNPlan had at the commit named in the first line of tests/golden/plan_table.txt,
//     plus nn_can_fuse_tail, nn_can_fuse_transform and nn_block_threads -- compared with that file.  The file was written by
//     THAT commit's nn_plan, not by the code under test (the recipe, from a checkout of it in $P; nn_plan calls nothing of HIP,
//     so the program runs without a device, and the kernel tables its dispatch refers to are never called):
//         hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -c -o launch.o $P/fast-point-cloud-registration-with-gpus_amd/csrc/icp_launch.hip
//         g++ <the Makefile's HOSTFLAGS> -DPLAN_CHECK_PARENT -I$P/fast-point-cloud-registration-with-gpus_amd/csrc -c -o check.o tests/plan_check.cpp
//         hipcc -o plan_check_parent check.o launch.o -Wl,--unresolved-symbols=ignore-all
//         ./plan_check_parent --print > tests/golden/plan_table.txt
//     The file holds every line of the default switches at 256 CUs; of every other group its name, line count and the 64-bit
//     FNV-1a of its lines.  The fields `version` and `sparse` are gone from NNPlan: field_version / field_sparse derive them
//     from the family.
//   * PREDICATES.  nn_model_may_be_hier against the two probe plans it replaced, and against "some cloud of the grid is
//     searched hierarchically".
//   * SHAPE.  nn_launch_shape for every plan, kind of launch and launch switch: 4, 8 or 16 waves, rounds that fit the family's
//     hit list, and nn_block_threads = the steady launch of the fp32 families.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#ifdef PLAN_CHECK_PARENT
#include "icp_kernels.h"
#else
#include "../fast-point-cloud-registration-with-gpus_amd/csrc/icp_plan.h"
#endif

using namespace icp;

static const char* kParent = "eb3f3e10ea5f0a501d4b2fa23199697acff1cc71";

#ifdef PLAN_CHECK_PARENT
static int field_version(const NNPlan& pl) { return pl.version; }
static int field_sparse(const NNPlan& pl) { return pl.sparse; }
#else
// version -- 1: generic kernel (dense fp64), 2: packed fp32 kernels, 3: fp64 on the sparse structure; sparse -- rows and chunk boxes
static int field_version(const NNPlan& pl)
{
    switch (pl.family) {
        case NNFamily::Dense: return 1;
        case NNFamily::DensePacked:
        case NNFamily::Row64:
        case NNFamily::Row128: return 2;
        case NNFamily::Row64F64: return 3;
    }
    return -1;
}
static int field_sparse(const NNPlan& pl) { return pl.family == NNFamily::Row64 || pl.family == NNFamily::Row128 || pl.family == NNFamily::Row64F64; }
#endif

static int g_failed = 0;

static void check(bool ok, const char* what, ...)
{
    char line[512];
    va_list ap;
    va_start(ap, what);
    std::vsnprintf(line, sizeof line, what, ap);
    va_end(ap);
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", line);
    if (!ok) ++g_failed;
}

// ---- the grid ------------------------------------------------------------------------------------------------
// n, for a machine of C CUs: empty; one block and the padding granule (1 | 1024 | 1025); every border of the plan in n_pad, taken on
// both sides -- rows of 64 filling 2 C and rows of 128 at C (both n_pad = 128 C), rows of 128 at 2 C - C / 4 and at 2 C, the dense
// 4-points-per-lane border n_pad / 256 >= 8 C, blocks_x at 2^21 rows of 128.  (256 CUs: 32 768, 57 344, 65 536, 524 288, 2^28.)
static std::vector<int> n_values(int cus)
{
    const int C = cus > 0 ? cus : 256;
    std::vector<int> v = {-1, 0, 1, 1024, 1025};
    for (int at_most : {128 * C, 128 * (2 * C - C / 4), 128 * 2 * C}) { v.push_back(at_most); v.push_back(at_most + 1); }   // n_pad <= border | the next n_pad
    for (int at_least : {256 * 8 * C, 1 << 28}) { v.push_back(at_least - 1024); v.push_back(at_least - 1023); }            // n_pad < border | n_pad = border
    return v;
}
// m: empty; one chunk of 16 and its neighbours; 1024 and its neighbours (max_S caps every split: the one block row of a 1-point
// cloud asks for 16, 256 and 256 segments); m_pad at 32 768, 2^16, 2^17 and 8 x 65 536, each with the next chunk above it; one
// large model between the borders, where the rounding of a segment shows
static const int kM[] = {-1, 0, 1, 5, 15, 16, 17, 1023, 1024, 1025, 32768, 32769, 65520, 65521, 65537, 131056, 131057, 131073, 524288, 524289, 10000000};
static const int kCus[] = {256, 64, 0};

struct Tuning { const char* name; NNTuning t; };
static std::vector<Tuning> tunings()
{
    std::vector<Tuning> v;
    auto add = [&v](const char* name, void (*set)(NNTuning&)) { Tuning x{name, NNTuning{}}; set(x.t); v.push_back(x); };
    add("default", [](NNTuning&) {});
    add("sparse=0", [](NNTuning& t) { t.sparse = 0; });
    add("cull=0", [](NNTuning& t) { t.cull = 0; });
    add("sparse=0,cull=0", [](NNTuning& t) { t.sparse = 0; t.cull = 0; });
    add("row=64", [](NNTuning& t) { t.row = 64; });
    add("row=128", [](NNTuning& t) { t.row = 128; });
    add("waves128=4", [](NNTuning& t) { t.waves128 = 4; });
    add("waves128=8", [](NNTuning& t) { t.waves128 = 8; });
    add("waves128=16", [](NNTuning& t) { t.waves128 = 16; });
    add("hier=0", [](NNTuning& t) { t.hier = 0; });
    add("hier=1", [](NNTuning& t) { t.hier = 1; });
    add("order=0", [](NNTuning& t) { t.order = 0; });
    add("order=2", [](NNTuning& t) { t.order = 2; });
    add("share=0", [](NNTuning& t) { t.share = 0; });
    add("f64_sparse=0", [](NNTuning& t) { t.f64_sparse = 0; });
    // the pairs the GPU tests use together
    add("row=128,waves128=8", [](NNTuning& t) { t.row = 128; t.waves128 = 8; });
    add("row=128,waves128=4,hier=1", [](NNTuning& t) { t.row = 128; t.waves128 = 4; t.hier = 1; });
    add("order=2,waves128=4", [](NNTuning& t) { t.order = 2; t.waves128 = 4; });
    add("order=2,waves128=8", [](NNTuning& t) { t.order = 2; t.waves128 = 8; });
    return v;
}

// ---- the table -----------------------------------------------------------------------------------------------
static const char* kColumns = "# n m : n_pad m_pad pts_per_thread blocks_x splits seg_len version chunk cull sparse hier row nw share_blocks order : fuse_tail fuse_transform block_threads";

static std::string plan_line(int n, int m, int precision, int cus, const NNTuning& t, int force_dense)
{
    const NNPlan pl = nn_plan(n, m, precision, cus, t, force_dense);
    char b[256];
    std::snprintf(b, sizeof b, "%d %d : %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d : %d %d %d\n", n, m, pl.n_pad, pl.m_pad, pl.pts_per_thread, pl.blocks_x, pl.splits,
                  pl.seg_len, field_version(pl), pl.chunk, pl.cull, field_sparse(pl), pl.hier, pl.row, pl.nw, pl.share_blocks, pl.order, nn_can_fuse_tail(pl) ? 1 : 0,
                  nn_can_fuse_transform(pl) ? 1 : 0, nn_block_threads(pl));
    const bool echoes = pl.precision == precision && pl.n == n && pl.m == m;
    return echoes ? std::string(b) : std::string("plan does not echo its arguments: ") + b;
}

static uint64_t fnv1a(const std::string& s)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) { h ^= c; h *= 0x100000001b3ull; }
    return h;
}

struct Group { std::string name; std::vector<std::string> lines; bool full; };

static std::vector<Group> make_groups()
{
    std::vector<Group> out;
    for (const Tuning& tu : tunings())
        for (int cus : kCus)
            for (int dense = 0; dense < 2; ++dense)
                for (int precision : {ICP_F32, ICP_F64}) {
                    Group g;
                    g.name = std::string("tune=") + tu.name + " cus=" + std::to_string(cus) + " force_dense=" + std::to_string(dense) + (precision == ICP_F32 ? " f32" : " f64");
                    g.full = std::strcmp(tu.name, "default") == 0 && cus == 256;
                    for (int n : n_values(cus))
                        for (int m : kM) g.lines.push_back(plan_line(n, m, precision, cus, tu.t, dense));
                    out.push_back(g);
                }
    return out;
}

static std::string group_header(const Group& g)
{
    std::string all;
    for (const std::string& l : g.lines) all += l;
    char b[64];
    std::snprintf(b, sizeof b, " lines=%zu fnv1a=%016llx\n", g.lines.size(), (unsigned long long)fnv1a(all));
    return "group " + g.name + b;
}

static void print_table(const std::vector<Group>& groups)
{
    std::printf("# nn_plan of commit %s (recipe: tests/plan_check.cpp)\n%s\n", kParent, kColumns);
    for (const Group& g : groups) {
        std::fputs(group_header(g).c_str(), stdout);
        if (g.full)
            for (const std::string& l : g.lines) std::fputs(l.c_str(), stdout);
    }
}

static void check_table(const std::vector<Group>& groups, const char* path)
{
    std::ifstream f(path);
    check(f.good(), "table: %s opens", path);
    if (!f.good()) return;
    std::vector<std::string> file;
    for (std::string l; std::getline(f, l);) file.push_back(l + "\n");
    check(file.size() >= 2 && file[0].find(kParent) != std::string::npos && file[1] == std::string(kColumns) + "\n", "table: written by commit %.7s, the columns this program prints", kParent);
    size_t at = 2, bad = 0, lines = 0;
    for (const Group& g : groups) {
        const std::string head = group_header(g);
        if (at >= file.size() || file[at] != head) {
            ++bad;
            std::printf("FAIL table: %s      was: %s      is:  %s", g.name.c_str(), at < file.size() ? file[at].c_str() : "(end of file)\n", head.c_str());
            if (!g.full) std::printf("     (only this group's hash is kept: print it at both commits to see the lines)\n");
        }
        // (a group whose name is not where it should be: the file is of another grid -- nothing further lines up)
        if (at >= file.size() || file[at].compare(0, 6 + g.name.size() + 1, "group " + g.name + " ") != 0) { check(false, "table: the file's groups are this grid's"); return; }
        ++at;
        lines += g.lines.size();
        if (!g.full) continue;
        for (const std::string& l : g.lines) {
            if (at >= file.size() || file[at] != l) {
                std::printf("FAIL table: %s, first differing line\n     was: %s     is:  %s", g.name.c_str(), at < file.size() ? file[at].c_str() : "(end of file)\n", l.c_str());
                check(false, "table: %s", g.name.c_str());
                return;
            }
            ++at;
        }
    }
    check(at == file.size(), "table: nothing in the file beyond the grid's groups");
    check(bad == 0, "table: %zu plans in %zu groups are what commit %.7s computed", lines, groups.size(), kParent);
}

#ifndef PLAN_CHECK_PARENT
// ---- predicates ----------------------------------------------------------------------------------------------
static void check_predicates()
{
    int cases = 0, differ_probes = 0, differ_grid = 0;
    for (const Tuning& tu : tunings())
        for (int cus : kCus)
            for (int precision : {ICP_F32, ICP_F64})
                for (int m : kM) {
                    // what icp_set_model asked before: the plans of a one-row cloud and of a cloud of 2^22 points
                    const bool probes = precision == ICP_F32 && m > 0 && (nn_plan(128, m, precision, cus, tu.t).hier || nn_plan(1 << 22, m, precision, cus, tu.t).hier);
                    bool some = false;
                    for (int n : n_values(cus)) some = some || nn_plan(n, m, precision, cus, tu.t).hier;
                    const bool rule = nn_model_may_be_hier(m, precision, tu.t);
                    ++cases;
                    if (rule != probes && ++differ_probes == 1) std::printf("     tune=%s cus=%d m=%d: rule %d, probes %d\n", tu.name, cus, m, rule, probes);
                    if (rule != some && ++differ_grid == 1) std::printf("     tune=%s cus=%d m=%d: rule %d, some cloud of the grid %d\n", tu.name, cus, m, rule, some);
                }
    check(differ_probes == 0, "predicates: nn_model_may_be_hier = the two probe plans, %d models x switches x CUs (%d differ)", cases, differ_probes);
    check(differ_grid == 0, "predicates: nn_model_may_be_hier = some cloud of the grid is searched hierarchically (%d differ)", differ_grid);
    // the one-line predicates against the integers they replaced
    int bad = 0;
    for (const Tuning& tu : tunings())
        for (int precision : {ICP_F32, ICP_F64})
            for (int dense = 0; dense < 2; ++dense)
                for (int n : n_values(256))
                    for (int m : kM) {
                        const NNPlan pl = nn_plan(n, m, precision, 256, tu.t, dense);
                        const bool sparse = field_sparse(pl) != 0;
                        bad += nn_is_sparse(pl) != sparse;
                        bad += nn_keeps_slot_order(pl) != (sparse && pl.row != 64 && pl.splits == 1);
                        bad += nn_can_sum_rows_in_launch(pl) != (sparse && field_version(pl) == 2 && pl.row != 64);
                        bad += nn_moving_group(pl) != ((sparse && pl.row == 64) ? 64 : 128);
                    }
    check(bad == 0, "predicates: sparse, slot order, rows summed in the launch, moving group = the expressions they replaced (%d differ)", bad);
}

// ---- the shape of a launch -----------------------------------------------------------------------------------
static void check_shapes()
{
    long long shapes = 0;
    int bad_waves = 0, bad_cap = 0, bad_threads = 0, bad_dense = 0;
    for (const Tuning& tu : tunings())
        for (int cus : kCus)
            for (int precision : {ICP_F32, ICP_F64})
                for (int dense = 0; dense < 2; ++dense)
                    for (int n : n_values(cus))
                        for (int m : kM) {
                            const NNPlan pl = nn_plan(n, m, precision, cus, tu.t, dense);
                            for (int k = 0; k < 16; ++k)
                                for (int waves64 : {0, 16})
                                    for (int cold8 = 0; cold8 < 2; ++cold8) {
                                        NNTuning t = tu.t;
                                        t.waves64 = waves64;
                                        t.cold8 = cold8;
                                        const NNLaunchShape s = nn_launch_shape(pl, NNLaunchKind{(k & 1) != 0, (k & 2) != 0, (k & 4) != 0, (k & 8) != 0}, t);
                                        ++shapes;
                                        bad_waves += !(s.waves == 4 || s.waves == 8 || s.waves == 16);
                                        if (!nn_is_sparse(pl)) { bad_dense += !(s.waves * 64 == NN_BLOCK && s.max_passes == 0); continue; }
                                        const int cap = (pl.family == NNFamily::Row128 && !pl.hier) ? SP_HCAP_FLAT : SP_HCAP;
                                        bad_cap += !(s.max_passes >= 1 && 64 * s.waves * s.max_passes <= cap);
                                    }
                            // (the switches a launch reads beyond the plan's -- waves64, cold8 -- at their defaults, as in every group of the table)
                            if (precision == ICP_F32) bad_threads += nn_block_threads(pl) != 64 * nn_launch_shape(pl, NNLaunchKind{true, false, false, false}, tu.t).waves;
                        }
    check(bad_waves == 0, "shape: 4, 8 or 16 waves in %lld shapes (%d are not)", shapes, bad_waves);
    check(bad_cap == 0, "shape: 64 x waves x rounds fits the family's hit list (%d do not)", bad_cap);
    check(bad_dense == 0, "shape: the dense families run blocks of NN_BLOCK threads and list nothing (%d differ)", bad_dense);
    check(bad_threads == 0, "shape: nn_block_threads = 64 x the waves of the steady launch with a tail, fp32 (%d differ)", bad_threads);
}
#endif

int main(int argc, char** argv)
{
    const std::vector<Group> groups = make_groups();
    if (argc == 2 && std::strcmp(argv[1], "--print") == 0) { print_table(groups); return 0; }
    if (argc != 2) { std::fprintf(stderr, "usage: plan_check --print | plan_check TABLE\n"); return 2; }
    check_table(groups, argv[1]);
#ifndef PLAN_CHECK_PARENT
    check_predicates();
    check_shapes();
#endif
    std::printf(g_failed ? "plan_check FAILED (%d)\n" : "plan_check passed\n", g_failed);
    return g_failed ? 1 : 0;
}
