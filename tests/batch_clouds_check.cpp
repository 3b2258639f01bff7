// batch_clouds_check.cpp -- csrc/icp_batch_clouds.h on the CPU.  Built and run by tests/test_batch_clouds.py (with the address and
// undefined-behaviour sanitizers); prints one line per failed check, a summary, and exits 0 when all hold.  Three things:
//   * CLOUDS.  list_clouds for 1 and 3 pairs, every cloud size drawn from {1, 63, 64, 65, 129} (all combinations) and the three
//     side masks, against a restatement by brute force: which cloud is which, the stretches of the temporaries, and a per-point
//     count of the work items that cover it.
//   * ARGS.  lay_out_args over a grid of cloud, item and int counts: 16-byte boundaries, regions that do not overlap, the exact total.
//   * CODEC.  encode and decode for 1 and 3 pairs, every cloud size of a side drawn from the same five (all combinations), both
//     sides, widths 1, 3 and 6 as planes and 33 as rows, float and double: decode(encode(x)) is x byte for byte, every value sits
//     where a restatement of k * plane + dst[p] + i (planes) and (dst[p] + i) * width + k (rows) puts it, every other byte of the
//     packed buffer is zero, and decode writes nothing outside the caller's array (guard values on both ends).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fast-point-cloud-registration-with-gpus_amd/csrc/icp_batch_clouds.h"

using namespace icp;

static int g_failed = 0, g_checks = 0;

static bool check(bool ok, const char* what, ...)
{
    ++g_checks;
    if (ok) return true;
    char line[512];
    va_list ap;
    va_start(ap, what);
    vsnprintf(line, sizeof line, what, ap);
    va_end(ap);
    if (++g_failed <= 40) printf("FAIL %s\n", line);
    return false;
}

static const int kSizes[5] = {1, 63, 64, 65, 129};
static const bool kMasks[3][2] = {{true, true}, {true, false}, {false, true}};

// pairs as a batch lays them out: every cloud at the next multiple of BATCH_ALIGN of its side's plane (the models' plane starts
// somewhere else than the moving clouds', so that a swapped side shows)
static std::vector<BatchPair> make_pairs(const std::vector<int>& n, const std::vector<int>& m)
{
    std::vector<BatchPair> pairs(n.size());
    long long p_plane = 0, q_plane = 7 * BATCH_ALIGN;
    for (size_t p = 0; p < n.size(); ++p) {
        pairs[p] = BatchPair{p_plane, q_plane, n[p], m[p], 0, 0};
        p_plane += (n[p] + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN;
        q_plane += (m[p] + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN;
    }
    return pairs;
}

static void check_case(const std::vector<int>& n, const std::vector<int>& m, const bool want[2])
{
    const int count = (int)n.size();
    const std::vector<BatchPair> pairs = make_pairs(n, m);
    CloudList cl;
    cl.tmp_plane = -1;
    cl.items.push_back(BatchItem{99, 99, 99, 99});   // (a list that is used twice starts empty)
    const bool ok = list_clouds(pairs, want, cl);
    char tag[128];
    snprintf(tag, sizeof tag, "count %d n0 %d m0 %d mask %d%d", count, n[0], m[0], (int)want[0], (int)want[1]);
    check(ok, "%s: list_clouds refused", tag);
    if (!check(cl.clouds.size() == 2 * (size_t)count, "%s: %zu clouds", tag, cl.clouds.size())) return;
    // which cloud is which, and the stretches of the temporaries
    long long expect_tmp = 0;
    for (int k = 0; k < 2 * count; ++k) {
        const VoxelCloud& c = cl.clouds[k];
        const bool model = k >= count;
        const BatchPair& pr = pairs[model ? k - count : k];
        check(c.side == (model ? 1 : 0), "%s: cloud %d side %d", tag, k, c.side);
        check(c.n == (model ? pr.m : pr.n), "%s: cloud %d n %d", tag, k, c.n);
        check(c.src_off == (model ? pr.q_off : pr.p_off), "%s: cloud %d src_off %lld", tag, k, c.src_off);
        check(c.dst_off == 0, "%s: cloud %d dst_off %lld", tag, k, c.dst_off);
        check(c.tmp_off % BATCH_ALIGN == 0, "%s: cloud %d tmp_off %lld is no multiple of BATCH_ALIGN", tag, k, c.tmp_off);
        check(c.tmp_off >= expect_tmp, "%s: cloud %d tmp_off %lld overlaps the cloud before (ends at %lld)", tag, k, c.tmp_off, expect_tmp);
        int rounded = 0;
        while (rounded < c.n) rounded += BATCH_ALIGN;
        check(c.tmp_off == expect_tmp, "%s: cloud %d tmp_off %lld, the rounded sizes before it sum to %lld", tag, k, c.tmp_off, expect_tmp);
        expect_tmp += rounded;
    }
    check(cl.tmp_plane == expect_tmp, "%s: tmp_plane %lld, the rounded sizes sum to %lld", tag, cl.tmp_plane, expect_tmp);
    // the work items: every point of every wanted cloud in exactly one, none of an unwanted cloud, in cloud order then point order
    std::vector<std::vector<int>> covered(2 * (size_t)count);
    for (int k = 0; k < 2 * count; ++k) covered[k].assign((size_t)cl.clouds[k].n, 0);
    int last_cloud = -1, last_end = 0;
    for (size_t i = 0; i < cl.items.size(); ++i) {
        const BatchItem& it = cl.items[i];
        if (!check(it.pair >= 0 && it.pair < 2 * count, "%s: item %zu names cloud %d", tag, i, it.pair)) return;
        check(want[it.pair >= count ? 1 : 0], "%s: item %zu names the unwanted cloud %d", tag, i, it.pair);
        check(it.count >= 1 && it.count <= BATCH_ITEM, "%s: item %zu count %d", tag, i, it.count);
        check(it.pad_ == 0, "%s: item %zu pad %d", tag, i, it.pad_);
        if (!check(it.first >= 0 && it.count >= 0 && it.first + it.count <= cl.clouds[it.pair].n, "%s: item %zu [%d, +%d) leaves cloud %d", tag, i, it.first, it.count, it.pair)) return;
        if (it.pair == last_cloud) check(it.first == last_end, "%s: item %zu starts at %d, the item before ended at %d", tag, i, it.first, last_end);
        else check(it.pair > last_cloud && it.first == 0, "%s: item %zu (cloud %d, first %d) after cloud %d", tag, i, it.pair, it.first, last_cloud);
        last_cloud = it.pair;
        last_end = it.first + it.count;
        for (int j = 0; j < it.count; ++j) covered[it.pair][(size_t)(it.first + j)] += 1;
    }
    for (int k = 0; k < 2 * count; ++k) {
        const int expect = want[k >= count ? 1 : 0] ? 1 : 0;
        for (int j = 0; j < cl.clouds[k].n; ++j)
            if (covered[k][j] != expect) {
                check(false, "%s: point %d of cloud %d lies in %d items, not %d", tag, j, k, covered[k][j], expect);
                break;
            }
    }
}

static void check_clouds()
{
    for (int mask = 0; mask < 3; ++mask) {
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 5; ++b) check_case({kSizes[a]}, {kSizes[b]}, kMasks[mask]);
        for (int code = 0; code < 5 * 5 * 5 * 5 * 5 * 5; ++code) {
            std::vector<int> n(3), m(3);
            int c = code;
            for (int p = 0; p < 3; ++p) {
                n[p] = kSizes[c % 5];
                c /= 5;
                m[p] = kSizes[c % 5];
                c /= 5;
            }
            check_case(n, m, kMasks[mask]);
        }
    }
}

static size_t next16(size_t v)
{
    while (v % 16 != 0) ++v;
    return v;
}

static void check_args()
{
    static const size_t clouds[] = {2, 6, 7, 200}, items[] = {0, 1, 2, 3, 1000}, ints[] = {0, 1, 2, 6, 7, 200};
    for (size_t c : clouds)
        for (size_t i : items)
            for (size_t k : ints) {
                const ArgsLayout l = lay_out_args(c, i, k);
                const size_t end_clouds = c * sizeof(VoxelCloud), end_items = l.off_items + i * sizeof(BatchItem);
                check(l.off_items % 16 == 0 && l.off_ints % 16 == 0, "args %zu %zu %zu: offsets %zu %zu are not 16-byte aligned", c, i, k, l.off_items, l.off_ints);
                check(l.off_items >= end_clouds && l.off_ints >= end_items, "args %zu %zu %zu: regions overlap", c, i, k);
                check(l.off_items == next16(end_clouds) && l.off_ints == next16(end_items), "args %zu %zu %zu: offsets %zu %zu leave a gap", c, i, k, l.off_items, l.off_ints);
                check(l.bytes == l.off_ints + k * sizeof(int), "args %zu %zu %zu: %zu bytes", c, i, k, l.bytes);
            }
}

template <typename E>
static void check_codec_case(const std::vector<int>& n, const std::vector<int>& m, bool model, int width, Layout layout)
{
    const std::vector<BatchPair> pairs = make_pairs(n, m);
    const std::vector<int>& len = model ? m : n;
    std::vector<int64_t> off(len.size() + 1, 0);
    for (size_t p = 0; p < len.size(); ++p) off[p + 1] = off[p] + len[p];
    const BatchPair& last = pairs.back();
    const long long plane = (model ? last.q_off : last.p_off) + (len.back() + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN;
    const Side s = make_side(pairs, off.data(), plane, model);
    const Format f{width, layout, sizeof(E)};
    char tag[160];
    snprintf(tag, sizeof tag, "codec %s width %d %s side %d sizes %d/%d/%d", sizeof(E) == 8 ? "f64" : "f32", width, layout == ROWS ? "rows" : "planes",
             (int)model, len[0], len.size() > 1 ? len[1] : 0, len.size() > 2 ? len[2] : 0);
    for (size_t p = 0; p < len.size(); ++p) check(s.dst[p] == (model ? pairs[p].q_off : pairs[p].p_off), "%s: dst[%zu] %lld", tag, p, s.dst[p]);
    const size_t total = (size_t)off.back() * width, guard = 16;
    const E sentinel = (E)-12345;
    std::vector<E> own(guard + total + guard, sentinel), back(guard + total + guard, sentinel);
    for (size_t i = 0; i < total; ++i) own[guard + i] = (E)(1 + i);   // (never 0, never the sentinel; exact in a float up to 2^24)
    std::vector<char> raw(3, 'x');   // (a vector that is used twice starts over)
    encode(f, s, own.data() + guard, raw);
    if (!check(raw.size() == (size_t)width * (size_t)plane * sizeof(E) && raw.size() == f.bytes(plane), "%s: %zu packed bytes", tag, raw.size())) return;
    std::vector<char> expect(raw.size(), 0);
    E* e = reinterpret_cast<E*>(expect.data());
    for (size_t p = 0; p < len.size(); ++p)
        for (int i = 0; i < len[p]; ++i)
            for (int k = 0; k < width; ++k) {
                const size_t at = layout == ROWS ? (size_t)(s.dst[p] + i) * width + k : (size_t)(k * plane + s.dst[p] + i);
                if (!check(at < (size_t)width * (size_t)plane, "%s: the restatement leaves the buffer", tag)) return;
                e[at] = own[guard + (size_t)(off[p] + i) * width + k];
            }
    check(std::memcmp(raw.data(), expect.data(), raw.size()) == 0, "%s: a value is misplaced or a padding byte is not zero", tag);
    decode(f, s, raw.data(), back.data() + guard);
    check(std::memcmp(back.data(), own.data(), own.size() * sizeof(E)) == 0, "%s: decode(encode(x)) != x, or a guard value was written", tag);
}

static void check_codec()
{
    static const int widths[4] = {1, 3, 6, 33};
    for (int w = 0; w < 4; ++w)
        for (int model = 0; model < 2; ++model) {
            const Layout layout = widths[w] == 33 ? ROWS : PLANES;
            for (int a = 0; a < 5; ++a) {
                check_codec_case<float>({kSizes[a]}, {kSizes[a]}, model != 0, widths[w], layout);
                check_codec_case<double>({kSizes[a]}, {kSizes[a]}, model != 0, widths[w], layout);
            }
            for (int code = 0; code < 5 * 5 * 5; ++code) {   // the side's three sizes: all combinations; the other side's: rotated
                const std::vector<int> own{kSizes[code % 5], kSizes[code / 5 % 5], kSizes[code / 25]}, other{own[1], own[2], own[0]};
                check_codec_case<float>(model ? other : own, model ? own : other, model != 0, widths[w], layout);
                check_codec_case<double>(model ? other : own, model ? own : other, model != 0, widths[w], layout);
            }
        }
}

int main()
{
    check_clouds();
    check_args();
    check_codec();
    printf("%d checks, %d failed\n", g_checks, g_failed);
    if (g_failed == 0) printf("batch_clouds_check passed\n");
    return g_failed == 0 ? 0 : 1;
}
