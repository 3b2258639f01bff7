// icp_ctx.h -- the host-side state shared by icp_api.cpp, icp_clouds.cpp and icp_loop.cpp (internal: nothing here is exported)
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <sched.h>
#include <string>

#include "../../include/icp_mi355x.h"
#include "icp_host_loop.h"
#include "icp_kernels.h"
#include "icp_lcomm.h"
#include "icp_wire.h"

#pragma GCC visibility push(hidden)

extern thread_local std::string g_last_error;

inline int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return fail(ICP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

constexpr int kMailSlots = 4;  // armed launches: ring of mailboxes (one is live at a time)
constexpr size_t kMailSlotBytes = sizeof(icp::NNMailbox64);   // a slot holds a float message (one line) or a double one (two)
inline icp::NNMailbox* mail_slot(icp::NNMailbox* base, int slot) { return reinterpret_cast<icp::NNMailbox*>(reinterpret_cast<char*>(base) + (size_t)slot * kMailSlotBytes); }

// device memory, pinned host memory and an event that go with whatever holds them: none can be copied, all free in their destructor
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }   // (moved, not copied: the loop swaps its ping-pong clouds)
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes < 256 ? 256 : bytes;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t bytes)   // (what it held is not kept)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    // what was recorded last has ended; the first use makes the event (a new one is complete)
    hipError_t wait() { return ev ? hipEventSynchronize(ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    hipError_t record(hipStream_t st) { return hipEventRecord(ev, st); }
};

// arguments of a launch that travel through a pinned buffer their owner keeps, so that nothing has to outlive the call on the
// stack and the call waits for nothing: wait (the copy before has read the pinned side), ensure, fill host, copy, record
struct Staged {
    DevBuf dev;
    PinnedBuf host;
    Event ev;
    hipError_t wait() { return ev.wait(); }
    hipError_t ensure(size_t bytes)
    {
        hipError_t e = host.ensure(bytes);
        return e == hipSuccess ? dev.ensure(bytes) : e;
    }
    hipError_t copy(size_t bytes, hipStream_t st) { return hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, st); }
    hipError_t record(hipStream_t st) { return ev.record(st); }
};

struct LoopState {
    bool active = false;
    bool pending = false;   // an enqueue awaits its complete
    icp::HostLoop H;        // error series, stop rule, minimisation, transform composition (host only)
    int applied_idx = 0;    // idx buffer used by the last applied transform
    int mom_blocks = 0, err_blocks = 0;
    double seconds_nn = 0.0;
    double seconds_host = 0.0;  // host half of the passes (error, stop rule, solve), summed while profiling is on
    bool timed_nn = false;
    bool numeric_failure = false;  // the minimisation refused the last pass's moments: the loop is over, its state stays readable
    bool host_reduce = false;  // how the pending enqueue's partial rows are being reduced
    bool final_poll = false;   // ... inside the launch itself, which leaves the vector and the pass's tag in c->h_final (the host polls ONE tag)
    bool matched = false;      // a matching pass of THIS loop has filled idx[cur]
    bool rows_compact = false;  // the pending rows are compact (NN_CROW doubles; slot 0 = error share with the tag in its low mantissa bits)
    double wait_tag = 0.0;      // completion tag of the pending enqueue's rows
    // armed launch: the matching pass AFTER the pending one is already enqueued and waits for its (R, t)
    bool armed = false;
    bool slot_written = false;   // the pending (or last completed) pass was an armed launch that left points and matches in slot order
    bool slot_flip = false;      // ... in this plane of the slot-order points (the next such launch reads it and writes the other)
    double armed_tag = 0.0;
    int armed_slot = 0;
    int armed_prev_cur = 0;
    bool armed_compact = false;
    std::chrono::steady_clock::time_point armed_at{};   // when the armed pass was launched (mailbox lease)
    icp::NNMailbox* live_mailbox = nullptr;             // a resident kernel is running and listens here
    bool from_pristine = false;  // the loop started from the cloud icp_set_moving uploaded: it can be run again from the copy
    long long steps = 0;         // completed (enqueue + complete) steps of this loop
    int route = 0;               // ICP_ROUTE_* bits of the pending (then: last completed) pass -- icp_diag_loop_moments
    bool mom_valid = false;      // c->h_mom holds the vector HostLoop::advance last received in this loop
};

// the calling thread's affinity, narrowed to the device's NUMA node for the duration of one entry point (see icp_create)
struct ScopedPin {
    bool restore = false;
    cpu_set_t saved;
    explicit ScopedPin(const icp_ctx* c);
    ~ScopedPin() { if (restore) (void)sched_setaffinity(0, sizeof saved, &saved); }
    ScopedPin(const ScopedPin&) = delete;
    ScopedPin& operator=(const ScopedPin&) = delete;
};

struct __attribute__((visibility("hidden"))) icp_ctx {   // (the public header only names it; the units export their C entry points explicitly)
    int device = 0;
    int num_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool profiling = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    int prec = -1;  // precision of the resident clouds (model and moving must agree)
    int n = 0, m = 0;
    bool have_model = false, have_moving = false, have_normals = false;
    DevBuf P0;  // pristine copy of the moving cloud as uploaded (icp_reset_moving)
    DevBuf Qbox;  // chunk bounding boxes of Qs
    DevBuf Qrec;  // large models (hierarchical search): one 160-byte record per chunk -- box, coordinates, indices (launch_model_records)
    bool have_records = false;
    DevBuf Qsamp; // one point per chunk of Qs
    DevBuf Qss;   // Morton-ordered scan copy (sparse kernel), when the model's own order has no locality
    DevBuf Qperm; // ... and its permutation: sorted position -> model index
    DevBuf Pperm; // slot -> moving point (Morton order of the initial positions), when the cloud's own order has no locality
    DevBuf slot_state; // fused launches of the sparse kernels: moving points (two planes) + matched model points in slot order (9 x n_pad floats)
    DevBuf share_counts;                        // shared rows (NNPlan::share_blocks): 5 x blocks_x hit counters (3 in rotation from launch to launch, 2 for first passes)
    mutable unsigned long long share_seq = 0;   // ... the launches so far (advanced by the launcher)
    mutable unsigned long long share_cold_seq = 0;   // ... and those that were the first pass of a registration
    DevBuf order_roles, order_totals;  // ... the roles of the launch's blocks (split rows: icp_kernels.h, NN_ORDER_*), the sum of the counters
    unsigned long long order_seq = 0;
    int order_regs = 0;                // registrations (loops) that have run ordered launches with these counters
    int order_launches = 0;            // ... ordered launches of the loop that is running
    int split_min = -1;                // the smallest part of a split row, in hits of the launch before (ICP_NN_SPLIT_MIN; 0: no row is split; -1: 512 per wave of a block)
    DevBuf row_hits, order_keys[2], order_vals[2], order_tmp;   // ordered rows (NNPlan::order): hits per row, and the sort that turns them into the next launch's order
    const int32_t* row_order = nullptr;          // ... the order the next launch follows (device; NULL: index order)
    DevBuf seed_pub;                            // ... resident launches: blocks_x x 384 floats, the matches of split rows for their other blocks
    bool exclusive = false;                     // icp_set_exclusive: the caller owns the device -- rows of 64 points run as 16-wave blocks, one to a CU
    bool share_auto = true;                     // ... ICP_SHARE_AUTO=0: never resident of its own accord (see share_wants_resident)
    int share_resident_after = -1;              // ... ICP_SHARE_RESIDENT_AFTER=n: a registration runs armed launches for n passes, then one resident kernel (< 0, the default: armed throughout)
    bool model_sorted = false, moving_sorted = false;
    // scratch of the device-side preparation (duplicate flags, Morton order, extent test)
    DevBuf prep_keys[2], prep_vals[2], prep_tmp, prep_small, prep_ext, prep_voided, prep_perm;
    struct PrepSmall { float box[4]; double totals[4]; int voided; int pad_; unsigned int enc[6]; unsigned int ticket; unsigned int pad2_; unsigned long long fixed[4]; };
    icp::PrepReport* h_prep = nullptr;   // pinned, coherent: where the short set-up's last launch leaves its sums (the host spins on its seq word)
    unsigned int prep_seq = 0;
    void* h_stage = nullptr;             // pinned, mapped: small clouds are laid out straight from here (no separate copy command)
    size_t h_stage_cap = 0;
    // round 4, the short set-up of clouds of up to kPrepSmallMax points: exact duplicates by hashing (a table that is never cleared:
    // entries carry the upload's generation), and the spatial-order decision remembered per (cloud kind, size, group) -- a sensor's next
    // scan has the order of the one before: while the given order's summed group extent stays within a quarter of the remembered one
    // and the remembered decision was "own order", the curve sort that only served to confirm it is not run (ICP_SORT overrides)
    static constexpr int kPrepSmallMax = 65536;
    DevBuf dup_table;
    unsigned int dup_gen = 0;
    struct OrderMemo { bool valid = false; int count = 0, group = 0; bool sorted = false; double given_rel = 0.0; };
    OrderMemo memo_model, memo_moving;
    DevBuf fin_scratch;      // finalize in two stages (many rows): 256 x ICP_NMOM doubles
    DevBuf fin_tickets;      // rows added up inside the matching launch (NNTail::fin_*): NN_FIN_GROUPS + 1 tickets, zero between launches
    double* h_final = nullptr;   // ... and where the launch leaves its ICP_NMOM vector for the host: pinned, coherent; the pass's tag in the last slot
    DevBuf work;             // icp_set_work_counting: NN_WORK_SLOTS counters of the work the sparse kernel executes
    bool count_work = false;
    DevBuf phase_log;        // ICP_NN_PHASES diagnostic
    size_t phase_slots = 0;
    std::string phase_path;
    DevBuf P, P2, Q, Qs, Nrm, stage;  // Qs: duplicate-voided scan copy of the model (fp32 early-out kernel)
    bool have_scan_copy = false;
    int voided = 0;  // P2: ping-pong target of the transform fused into the matching kernel
    DevBuf part_d, part_idx, idx[2];
    int cur = 0;  // idx buffer written by the most recent matching pass
    bool idx_valid = false;  // idx[cur] holds matches of the resident clouds
    DevBuf mom_partials, err_partials, mom_own, nbr;
    DevBuf keys, tickets;              // fused tail of the matching kernel: (d, idx) keys per moving point, row tickets
    size_t rows_cap = 0;               // rows available in mom_partials / h_mom_partials, err_partials / h_err_partials
    unsigned char* rows_seen = nullptr;   // [rows_cap] the host's poll: rows of the pending pass already arrived
    int rows_format = -1;              // format of the rows last written to h_mom_partials: 1 compact, 0 full, -1 none yet
    bool fused_tail = true;            // ICP_FUSED_TAIL=0 keeps matching and moments as two kernels
    bool use_boxes = true;             // (false with ICP_NN_SPARSE=0: the dense kernels, no boxes)
    bool mail_wide = true;             // ICP_MAILBOX=plain: write the mailbox line word by word (payload, fence, tags) -- the path of a CPU without AVX
    icp::NNTuning tune{};              // every switch the plan and the launchers look at, read once in icp_create
    double* mom_dev = nullptr;
    double* h_mom = nullptr;  // pinned: the reduced ICP_NMOM vector as the host solve reads it
    unsigned int* h_nonfinite = nullptr;  // pinned, coherent: points with a NaN / infinite coordinate seen by the last upload
    // single-GPU fast path: the moments / transform kernels store their per-block partial rows straight
    // into mapped pinned host memory and the host adds them in block order -- no finalize launch, no
    // D2H blit.  (With an external moments buffer, i.e. the multi-GPU driver, the device finalize runs.)
    double* h_mom_partials = nullptr;  // [MOM_MAX_BLOCKS][ICP_NMOM]
    double* h_err_partials = nullptr;  // [rows_cap]
    uint64_t tag_seq = 0;              // completion tag of the most recent moments launch (exact in a double)
    int profile_stride = 0;            // time every n-th matching launch (0 = never)
    uint64_t nn_launch_count = 0;
    double prof_seconds_nn = 0.0;      // cumulative over loops since icp_set_profiling
    int prof_nn_launches = 0;
    long long prof_nn_passes = 0;      // matching passes inside those launches (resident kernels run many)
    uint64_t resident_launch_count = 0;
    // ICP_TRACE=1: host-side time split of the loop, printed by icp_destroy
    bool trace = false;
    double tr_first_row = 0.0, tr_last_row = 0.0;
    std::chrono::steady_clock::time_point tr_rows_done{};
    bool trace_passes = false;         // ICP_TRACE=2: one line per pass of a resident registration
    double tr_enqueue = 0, tr_wait = 0, tr_reduce = 0, tr_solve = 0;
    uint64_t tr_n = 0;
    void* comm = nullptr;              // RCCL communicator (icp_comm_init): the loop all-reduces its vector itself
    icp::LocalComm* lcomm = nullptr;   // host-memory communicator (icp_comm_init_local): the vector is summed over the node's ranks on the host
    // test hook (ICP_DEBUG="stall=pass:seconds", read by icp_create): the host sleeps once, right before it would publish
    // the message of that pass of a registration -- a descheduled host thread, as the mailbox lease has to survive it
    int debug_stall_pass = -1;
    double debug_stall_s = 0.0;
    int debug_lose_pass = -1;          // test hook (ICP_DEBUG=lose=pass): the message of that pass is never posted, once
    bool debug_shared_resident = false; // test hook (ICP_DEBUG=shared_resident): ranks that share a device may keep resident kernels
    int moving_group = 0;              // group size the moving cloud's order was judged on (0: not judged)
    std::chrono::steady_clock::time_point posted_at{};   // resident loop: when the pending pass's message went out (the row poll's time-out counts from here)
    bool moving_untouched = false;     // c->P (or the pristine copy standing in for it) still holds what icp_set_moving uploaded
    bool rows_timed_out = false;       // the last failure of icp_loop_complete was a pass that never delivered its rows
    int recoveries = 0;                // registrations finished step-wise after such a time-out (icp_recoveries)
    int pin_mode = 1;                  // ICP_PIN: 0 never, 1 scoped (default), 2 narrowed once and kept
    bool have_local_cpus = false;
    cpu_set_t local_cpus;              // CPUs of the device's NUMA node (sysfs local_cpulist)
    std::chrono::steady_clock::time_point rows_done_at{};   // when the host last saw a pass's rows complete (mailbox lease)
    bool arm = true;                   // ICP_ARMED=0: icp_loop_run never enqueues a pass ahead of its (R, t)
    bool shares_device = false;        // a rank of the attached node communicator runs on the same device: nothing is armed ahead (see icp_comm_init_local)
    int resident = 1;                  // ICP_RESIDENT=0: icp_loop_run never keeps one kernel for a whole registration; 2: also where shared rows are preferred
    bool resident_refused = false;     // the resident kernel does not fit the machine with this plan: do not try again
    // ring of mailboxes for armed / resident launches, in pinned mapped host memory, and the device-memory relay.
    // (Fine-grained device memory written through the PCIe BAR is ~0.5 us faster per message and needs no relay --
    // tools/mailbox_probe.hip -- but with the HIP runtime that PyTorch bundles the waiting kernel never sees a
    // store made after it started; host memory polled by ONE block works with every runtime.)
    icp::NNMailbox* h_mail = nullptr;
    bool mail_in_bar = false;
    bool moving_is_pristine = false;   // icp_reset_moving: P is stale, the cloud to use is P0 (copied on first need)
    // fine-grained device memory: ordinary (coarse-grained) device memory is cached per XCD L2, and a block polling
    // it from another XCD keeps reading its stale line (seen as 24 of 128 blocks never receiving the message)
    icp::NNMailbox* relay = nullptr;
    uint64_t mail_seq = 0;
    // Who adds up the moment rows: the host, as their tags arrive in pinned memory (no synchronisation, and what armed and
    // resident launches need) -- or, for clouds of more than kHostRowsMax rows, the device (two-stage finalize, 256 bytes come
    // back): 78 125 rows of the 10 M-point cloud are 20 MB over PCIe and a pass through them on one core per iteration,
    // 0.7 ms of 13 (profiles/r3: the library-issued RCCL route, which reduces on the device, was FASTER than the default).
    // Round 4: from 1 025 rows up (beyond what the host's sweep takes) the sparse kernels add their rows up INSIDE the launch (two
    // levels of tickets, NNTail::fin_*) and leave the vector with the pass's tag in pinned memory: no finalize launches, no copy, no
    // synchronisation, and such a pass can be armed ahead like any other.
    static constexpr int kHostRowsMax = 1024;
    bool host_reduce() const { return !comm && mom_dev == (double*)mom_own.p && h_mom_partials != nullptr && (plan.blocks_x <= host_rows_max || plan.n == 0); }
    int host_rows_max = kHostRowsMax;   // (ICP_HOST_ROWS_MAX: A/B runs)
    // the plan half of "this plan's rows are added up inside the launch" (the buffers: ensure_work_buffers; the rest: fin_in_launch)
    bool sums_in_launch(const icp::NNPlan& pl) const { return icp::nn_can_sum_rows_in_launch(pl) && pl.blocks_x > host_rows_max && icp::nn_can_fuse_tail(pl); }
    icp::NNPlan plan{};
    LoopState loop;
};

// shared between the units (icp_api.cpp: use, ScopedPin; icp_clouds.cpp: the clouds and the work buffers; icp_loop.cpp: make_cull)
int use(icp_ctx* c);
int require_clouds(icp_ctx* c);
int ensure_work_buffers(icp_ctx* c);
int materialize_moving(icp_ctx* c);
int download_idx(icp_ctx* c, int which, int32_t* out);
icp::NNCullInputs make_cull(const icp_ctx* c, const int32_t* seed);

#pragma GCC visibility pop
