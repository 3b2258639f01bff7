// icp_wire.cpp -- mailbox lines, row formats, the row sweep, the adders and the tag allocator (see icp_wire.h)
#include "icp_wire.h"

#include <atomic>
#include <cassert>
#include <cstring>

namespace icp {

bool cpu_has_avx()
{
#if defined(__x86_64__)
    static const bool have = __builtin_cpu_supports("avx");
    return have;
#else
    return false;
#endif
}

namespace {

// the sweep and the adders exist once for each of the two formats, with the format a constant: no other RowFormat may reach them
bool is_compact(const RowFormat& fmt)
{
    assert(&fmt == &kCompactRows || &fmt == &kFullRows);
    return &fmt == &kCompactRows;
}

#if defined(__x86_64__)
__attribute__((target("avx"))) void store_line_avx(uint32_t* dst, const uint32_t* line)
{
    _mm256_store_si256(reinterpret_cast<__m256i*>(dst), _mm256_load_si256(reinterpret_cast<const __m256i*>(line)));
    _mm256_store_si256(reinterpret_cast<__m256i*>(dst + 8), _mm256_load_si256(reinterpret_cast<const __m256i*>(line + 8)));
}

// Rows of format F added up in block order: one 4-double accumulator per 32 bytes of a row takes all its slots at
// once.  Every slot is still the sum of its values in block order, starting from zero -- the bits of the scalar loop -- but
// the chains advance together instead of one after the other (hall: 256 rows, once per pass, on the path between the last
// row's arrival and the next message).  The tag bits are masked off as a row is loaded; a sector without a tag is not masked
// at all (F is a constant, the loops over v unroll).
template <const RowFormat& F>
__attribute__((target("avx"))) void add_rows_avx(const double* rows, int count, double* out)
{
    constexpr int V = (int)F.stride / 4;
    __m256d keep[V], a[V];
    for (int v = 0; v < V; ++v) {
        keep[v] = _mm256_castsi256_pd(_mm256_set_epi64x((long long)F.keep(4 * v + 3), (long long)F.keep(4 * v + 2), (long long)F.keep(4 * v + 1), (long long)F.keep(4 * v)));
        a[v] = _mm256_setzero_pd();
    }
    for (int b = 0; b < count; ++b) {
        const double* r = rows + (size_t)b * F.stride;
        for (int v = 0; v < V; ++v) {
            const bool plain = (F.keep(4 * v) & F.keep(4 * v + 1) & F.keep(4 * v + 2) & F.keep(4 * v + 3)) == ~0ull;
            const __m256d x = _mm256_loadu_pd(r + 4 * v);
            a[v] = _mm256_add_pd(a[v], plain ? x : _mm256_and_pd(x, keep[v]));
        }
    }
    for (int v = 0; v < V; ++v) _mm256_storeu_pd(out + 4 * v, a[v]);
}
#endif

void add_rows_scalar(const double* rows, int count, const RowFormat& fmt, double* out)
{
    for (size_t k = 0; k < fmt.stride; ++k) out[k] = 0.0;
    for (int b = 0; b < count; ++b) {
        const double* row = rows + (size_t)b * fmt.stride;
        for (size_t k = 0; k < fmt.stride; ++k) {
            unsigned long long bits;
            std::memcpy(&bits, &row[k], sizeof bits);
            bits &= fmt.keep(k);
            double v;
            std::memcpy(&v, &bits, sizeof v);
            out[k] += v;
        }
    }
}

}  // namespace

void post_message(NNMailbox* mb, const double* R9, const double* t3, int cmd, double seq, bool wide)
{
    alignas(32) uint32_t line[16];
    std::memset(line, 0, sizeof line);
    const uint32_t tag = seq == 0.0 ? 0u : mailbox_tag(seq);
    if (R9 && t3) {
        for (int k = 0; k < 12; ++k) {
            const float f = (float)(k < 9 ? R9[k] : t3[k - 9]);
            std::memcpy(&line[mailbox_rt_word(k)], &f, sizeof f);
        }
    }
    line[ICP_MB_CMD] = (uint32_t)cmd;
    line[ICP_MB_TAG0] = tag;
    line[ICP_MB_TAG1] = tag;
#if defined(__x86_64__)
    if (wide && cpu_has_avx()) {
        store_line_avx(mb->w, line);
        bar_fence();
        return;
    }
#endif
    // no 32-byte stores: the payload first, then (fenced) the two tags -- the reader still accepts only a line whose
    // tags both match, so the order of the words within a half does not matter
    volatile uint32_t* dst = mb->w;
    for (int k = 0; k < 16; ++k)
        if (k != ICP_MB_TAG0 && k != ICP_MB_TAG1) dst[k] = line[k];
    bar_fence();
    dst[ICP_MB_TAG0] = tag;
    dst[ICP_MB_TAG1] = tag;
    bar_fence();
}

void post_message64(NNMailbox* mb, const double* R9, const double* t3, int cmd, double seq, bool wide)
{
    alignas(32) uint32_t line[32];
    std::memset(line, 0, sizeof line);
    const uint32_t tag = seq == 0.0 ? 0u : mailbox_tag(seq);
    for (int h = 0; h < 4; ++h) {
        if (R9 && t3)
            for (int k = 0; k < 3; ++k) {
                const int i = 3 * h + k;
                const double v = i < 9 ? R9[i] : t3[i - 9];
                std::memcpy(&line[h * 8 + 2 * k], &v, sizeof v);
            }
        line[h * 8 + ICP_MB64_CMD] = (uint32_t)cmd;
        line[h * 8 + 7] = tag;
    }
    uint32_t* dstw = reinterpret_cast<uint32_t*>(mb);
#if defined(__x86_64__)
    if (wide && cpu_has_avx()) {
        store_line_avx(dstw, line);
        store_line_avx(dstw + 16, line + 16);
        bar_fence();
        return;
    }
#endif
    volatile uint32_t* dst = dstw;
    for (int k = 0; k < 32; ++k)
        if ((k & 7) != 7) dst[k] = line[k];
    bar_fence();
    for (int h = 0; h < 4; ++h) dst[h * 8 + 7] = tag;
    bar_fence();
}

double row_tag(const double* rows, int b, const RowFormat& fmt)
{
    const volatile unsigned long long* q = reinterpret_cast<const volatile unsigned long long*>(rows + (size_t)b * fmt.stride);
    const unsigned long long t = q[fmt.tag_slot] & fmt.tag_mask;
    for (size_t k = fmt.tag_slot + fmt.tag_step; k < fmt.stride; k += fmt.tag_step)
        if ((q[k] & fmt.tag_mask) != t) return -1.0;
    if (fmt.tag_mask != ~0ull) return (double)t;
    double v;
    std::memcpy(&v, &t, sizeof v);
    return v;
}

// The kernels wrote their rows into mapped pinned memory, each row released to system scope before (or with) its tag.
// The poll is a SWEEP over the rows whose tag is still missing -- the cache misses of different rows overlap, where polling
// row b to completion before looking at row b + 1 takes them one after the other -- and fetches a row's other lines as soon
// as its tag is seen (tools/rows_probe.hip: 256 rows 6.6 -> 5.8 us).
// (round 3 tried a LIST of the rows still missing instead of the flags -- a sweep then costs what is missing, not the row count:
// no difference on the hall loop, 8.99-9.07 against 8.92-9.04 us per iteration on one box; the tags are compared as the
// integers they are -- a full row's double by its bits.)
// F is a constant: the rows of a pass arrive within a microsecond of each other, and what is done per arriving row is on the
// path to the next message -- with the format read at run time the hall iteration took 9.24 us instead of 8.94 and the
// point-to-plane one 14.86 instead of 14.21 (profiles/loop/01_ab_format_read_at_run_time.txt).
namespace {
template <const RowFormat& F>
int sweep_rows_of(const double* rows, int count, double tag, unsigned char* seen, std::chrono::steady_clock::time_point t0, double limit_s, double* first_row_s)
{
    constexpr size_t lines = F.stride * sizeof(double) / 64, tag_line = F.tag_slot * sizeof(double) / 64;
    const double want = F.shows(tag);
    unsigned long long want_bits = (unsigned long long)want;
    if (F.tag_mask == ~0ull) std::memcpy(&want_bits, &want, sizeof want_bits);
    const volatile unsigned long long* tags = reinterpret_cast<const volatile unsigned long long*>(rows);
    std::memset(seen, 0, (size_t)count);
    int left = count;
    unsigned spins = 0;
    while (left > 0) {
        for (int r = 0; r < count; ++r) {
            const volatile unsigned long long* t = tags + (size_t)r * F.stride;
            if (seen[r] || (t[F.tag_slot] & F.tag_mask) != want_bits) continue;
            bool whole = true;   // (the row is there when every tagged slot shows the tag)
            for (size_t k = F.tag_slot + F.tag_step; k < F.stride; k += F.tag_step) whole = whole && (t[k] & F.tag_mask) == want_bits;
            if (!whole) continue;
            seen[r] = 1;
            --left;
            const char* row = reinterpret_cast<const char*>(rows + (size_t)r * F.stride);
            for (size_t l = 0; l < lines; ++l)
                if (l != tag_line) __builtin_prefetch(row + 64 * l);
            if (left == count - 1 && first_row_s) *first_row_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        if (left > 0 && (++spins & 0x3f) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
            break;  // something is wrong (fault, hang): the caller lets the runtime report it
    }
    if (left == 0) std::atomic_thread_fence(std::memory_order_acquire);
    return left;
}
}  // namespace

int sweep_rows(const double* rows, int count, const RowFormat& fmt, double tag, unsigned char* seen,
               std::chrono::steady_clock::time_point t0, double limit_s, double* first_row_s)
{
    return is_compact(fmt) ? sweep_rows_of<kCompactRows>(rows, count, tag, seen, t0, limit_s, first_row_s)
                           : sweep_rows_of<kFullRows>(rows, count, tag, seen, t0, limit_s, first_row_s);
}

namespace {
template <const RowFormat& F>
bool sum_rows_of(const double* rows, int count, bool wide, double* mom)
{
    double sum[F.stride];
    bool avx = false;
#if defined(__x86_64__)
    avx = wide && cpu_has_avx();
    if (avx) add_rows_avx<F>(rows, count, sum);
#endif
    if (!avx) add_rows_scalar(rows, count, F, sum);
    for (size_t k = 0; k < F.stride; ++k)
        if (F.keep(k)) mom[F.moment(k)] += sum[k];
    return avx;
}
}  // namespace

bool sum_rows(const double* rows, int count, const RowFormat& fmt, bool wide, double mom[ICP_NMOM])
{
    return is_compact(fmt) ? sum_rows_of<kCompactRows>(rows, count, wide, mom) : sum_rows_of<kFullRows>(rows, count, wide, mom);
}

uint64_t take_tags(uint64_t& seq, uint64_t count)
{
    constexpr uint64_t kMod = kCompactRows.tag_mask + 1;   // (the format that shows the fewest bits of a tag)
    uint64_t first = seq + 1;
    if (first % kMod == 0 || first / kMod != (first + count - 1) / kMod) first = (first / kMod + 1) * kMod + 1;   // (count << kMod)
    seq = first + count - 1;
    return first;
}

}  // namespace icp
