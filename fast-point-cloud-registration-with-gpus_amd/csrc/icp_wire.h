// icp_wire.h -- the byte-level protocol between the host and a running kernel, free of any device call and of icp_ctx:
// the mailbox lines the host posts, the two formats of the rows a pass sends back through pinned memory, the sweep that
// polls their tags, the adders, and the allocator of the tags.  icp_loop.cpp decides what is posted and what is waited for;
// tests/wire_check.cpp runs this unit on the CPU.
#pragma once
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif

#include <chrono>
#include <cstddef>
#include <cstdint>

#include "icp_kernels.h"

#pragma GCC visibility push(hidden)

namespace icp {

// orders the stores of a mailbox message before its sequence number (and pushes them out, should the mailbox ever
// live in write-combining memory: the `lock or` compilers emit for a seq_cst fence does not do that)
inline void bar_fence()
{
#if defined(__x86_64__) || defined(__i386__)
    _mm_sfence();
#else
    __sync_synchronize();
#endif
}

bool cpu_has_avx();   // (false: every `wide` below is ignored)

// ---- mailbox lines (layout: icp_kernels.h, NNMailbox / NNMailbox64) ----------------------------------------------
// One message = one 64-byte line: each 32-byte half is written by ONE vector store and carries the tag in its last word,
// then one fence pushes the line out.  R9 / t3 may be NULL (commands that carry no transform); seq = 0 clears the mailbox
// (no tag ever equals 0).  !wide (ICP_MAILBOX=plain, a CPU without AVX): word by word -- the payload, a fence, the tags.
void post_message(NNMailbox* mb, const double* R9, const double* t3, int cmd, double seq, bool wide);
// the message of a registration in double (NNMailbox64): four 32-byte parts {3 doubles, cmd, tag}, one vector store each
void post_message64(NNMailbox* mb, const double* R9, const double* t3, int cmd, double seq, bool wide);

// ---- rows ------------------------------------------------------------------------------------------------------
// A pass's rows in pinned memory, one per block, in one of two formats.  A row is `stride` doubles; the slots tag_slot,
// tag_slot + tag_step, ... carry its completion tag in the bits of tag_mask (the rest of such a slot still belongs to the
// sum), and the row is there when all of them show the tag waited for.  Slot 0 is the row's share of moment mom_slot0, slot
// k > 0 its share of moment k + mom_shift.  There are exactly the two formats below, and the functions take one of these two
// objects (checked): the sweep and the adders are compiled once for each, with the format a constant.
struct RowFormat {
    size_t stride, tag_slot, tag_step;
    unsigned long long tag_mask;
    size_t mom_slot0, mom_shift;
    constexpr size_t moment(size_t k) const { return k == 0 ? mom_slot0 : k + mom_shift; }
    // the bits of slot k that belong to the sum (tag_step is a power of two: no division on the path of a pass)
    constexpr unsigned long long keep(size_t k) const { return k >= tag_slot && ((k - tag_slot) & (tag_step - 1)) == 0 ? ~tag_mask : ~0ull; }
    // what a complete row of the pass with completion tag `tag` shows (row_tag)
    double shows(double tag) const { return tag_mask == ~0ull ? tag : (double)((unsigned long long)tag & tag_mask); }
};
// compact (sparse kernels, fp32 point-to-point): {error share, sum p, sum q, sum q p^T} -- no point count -- written by ONE
// store per row; the first slot of every 32-byte sector (0, 4, 8, 12) carries the low NN_CROW_TAG_BITS bits of the tag in
// its low mantissa bits (2^-36 of a sum: nothing in fp32, which is why fp64 registrations never use this format)
inline constexpr RowFormat kCompactRows{NN_CROW, 0, 4, (1ull << NN_CROW_TAG_BITS) - 1ull, ICP_MOM_ERR, ICP_MOM_SP - 1};
// full: the ICP_NMOM slots of the moment vector, slot k moment k, the last one the tag as a double of its own (not a moment)
inline constexpr RowFormat kFullRows{ICP_NMOM, ICP_NMOM - 1, ICP_NMOM, ~0ull, 0, 0};
static_assert(NN_CROW == 16 && ICP_NMOM == 32, "the AVX adders take rows of sixteen and of 32 doubles");   // (whole 32-byte sectors)

// the tag row b carries now; a row whose tagged slots disagree (half written) carries none: -1
double row_tag(const double* rows, int b, const RowFormat& fmt);

// Polls the tags of rows [0, count) until every row shows `tag` or limit_s seconds have passed since t0; seen[r] = 1 for
// the rows that arrived.  Returns how many are still missing.  first_row_s (optional): when the first row was seen, from t0.
int sweep_rows(const double* rows, int count, const RowFormat& fmt, double tag, unsigned char* seen,
               std::chrono::steady_clock::time_point t0, double limit_s, double* first_row_s = nullptr);

// The rows added up, in block order, every slot from zero with its tag bits cleared -- the same bits whichever adder runs --
// and added to the moment vector: a full row slot for slot, a compact row's error share to ICP_MOM_ERR and the rest to
// ICP_MOM_SP .. ICP_MOM_SQP + 8 (it carries no point count).  Returns whether a wide (AVX) adder ran.
bool sum_rows(const double* rows, int count, const RowFormat& fmt, bool wide, double mom[ICP_NMOM]);

// Completion tags are consecutive integers.  A compact row shows only the low NN_CROW_TAG_BITS bits of its tag, and a
// wiped row shows zero: no tag that is ever waited for may have those bits all zero.  Returns the first of `count`
// consecutive tags that are safe in that sense and reserves them (seq: the last tag handed out).
uint64_t take_tags(uint64_t& seq, uint64_t count);

}  // namespace icp

#pragma GCC visibility pop
