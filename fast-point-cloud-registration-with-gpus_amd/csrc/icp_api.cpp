// icp_api.cpp -- the C ABI of libicp_mi355x.so (include/icp_mi355x.h): device query, context, communicators, setters,
// the matching-only and normals entry points, the diagnostic and bench entry points, the OS1 conversions.
// The resident clouds are set up in icp_clouds.cpp, the ICP driver loop runs in icp_loop.cpp; their shared state is icp_ctx.h.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <unistd.h>
#include <vector>

#include "../../include/icp_mi355x_diag.h"
#include "icp_comm.h"
#include "icp_ctx.h"

thread_local std::string g_last_error;

static constexpr size_t kPhaseSlots = 512 * 1024;  // ICP_NN_PHASES: 10 stamps per wave

ScopedPin::ScopedPin(const icp_ctx* c)
{
    if (!c || c->pin_mode != 1 || !c->have_local_cpus) return;
    const int cpu = sched_getcpu();
    if (cpu >= 0 && cpu < CPU_SETSIZE && CPU_ISSET(cpu, &c->local_cpus)) return;   // already next to the device: nothing to do
    cpu_set_t both;
    if (sched_getaffinity(0, sizeof saved, &saved) != 0) return;
    CPU_AND(&both, &saved, &c->local_cpus);
    if (CPU_COUNT(&both) == 0) return;                                              // the caller may not run there at all
    if (sched_setaffinity(0, sizeof both, &both) == 0) restore = true;
}

int use(icp_ctx* c)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return ICP_OK;
}

#pragma GCC visibility push(default)   // (the C ABI: exported although its icp_ctx is a hidden type)
extern "C" {

int icp_abi_version(void) { return ICP_ABI_VERSION; }

const char* icp_strerror(int code)
{
    switch (code) {
        case ICP_OK: return "ok";
        case ICP_ERR_INVALID: return "invalid argument";
        case ICP_ERR_NO_DEVICE: return "no usable gfx950 HIP device (there is no CPU fallback)";
        case ICP_ERR_HIP: return "HIP runtime error";
        case ICP_ERR_EMPTY: return "no model point, or no correspondence within the maximum distance";
        case ICP_ERR_SINGULAR: return "point-to-plane system is not positive definite";
        case ICP_ERR_IO: return "dataset file missing or malformed";
        case ICP_ERR_STATE: return "call sequence error";
        case ICP_ERR_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}

const char* icp_last_error(void) { return g_last_error.c_str(); }

int icp_device_count(void)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ICP_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    return n;
}

// The loop is a conversation between one host thread and the GPU (mailbox through the PCIe BAR, moment rows through pinned
// host memory): on a two-socket machine every message of a thread running on the other socket crosses the socket link
// too -- measured on the hall loop 13.05 us per iteration from the GPU's own NUMA node, 14.4-14.6 us from the other one,
// and a coin toss when the scheduler chooses (tools/numa_probe.py).  The library therefore wants the calling thread on a
// CPU that sysfs lists as local to the device -- but a drop-in library must not leave its caller's affinity changed.
// So the narrowing is SCOPED: an entry point that talks to the GPU in a loop (icp_create while it allocates and first
// touches the pinned buffers, icp_loop_run, icp_loop_complete, icp_point_to_*) narrows the mask only if the thread is
// currently running on a remote CPU, and puts the caller's mask back before it returns.
//   ICP_PIN=0  never touch the affinity;  ICP_PIN=1 (default) scoped as above;
//   ICP_PIN=2  narrow once in icp_create and leave it narrowed (the behaviour of round 1; a dedicated worker thread).
static bool parse_local_cpus(int device, cpu_set_t* local)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return false; }
    for (char* p = bus; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    std::FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return false;
    char line[4096] = {0};
    const bool got = std::fgets(line, sizeof line, f) != nullptr;
    std::fclose(f);
    if (!got) return false;
    CPU_ZERO(local);
    for (const char* p = line; *p;) {                      // "0-63,128-191"
        char* end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') { b = std::strtol(p + 1, &end, 10); p = end; }
        for (long k = a; k <= b && k < CPU_SETSIZE; ++k) if (k >= 0) CPU_SET((int)k, local);
        if (*p == ',') ++p; else break;
    }
    return CPU_COUNT(local) > 0;
}

int icp_create(int device, icp_ctx** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    const int nd = icp_device_count();
    if (nd <= 0) return fail(ICP_ERR_NO_DEVICE, "no HIP device visible: " + g_last_error);
    if (device < 0 || device >= nd) return fail(ICP_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ICP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    icp_ctx* c = new (std::nothrow) icp_ctx();
    if (!c) return fail(ICP_ERR_NOMEM, "context allocation failed");
    c->device = device;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char* v = std::getenv("ICP_PIN")) c->pin_mode = (v[0] == '0') ? 0 : (v[0] == '2') ? 2 : 1;
    c->have_local_cpus = c->pin_mode != 0 && parse_local_cpus(device, &c->local_cpus);
    if (c->pin_mode == 2 && c->have_local_cpus) {   // narrowed once and kept (a thread dedicated to this context)
        cpu_set_t cur, both;
        if (sched_getaffinity(0, sizeof cur, &cur) == 0) {
            CPU_AND(&both, &cur, &c->local_cpus);
            if (CPU_COUNT(&both) != 0 && CPU_COUNT(&both) != CPU_COUNT(&cur)) (void)sched_setaffinity(0, sizeof both, &both);
        }
    }
    ScopedPin pin(c);   // (the pinned host buffers below are allocated and first touched next to the device)
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_mom, ICP_NMOM * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_nonfinite, 64, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_final, ICP_NMOM * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) std::memset(c->h_final, 0, ICP_NMOM * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_prep, sizeof(icp::PrepReport), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) std::memset(c->h_prep, 0, sizeof(icp::PrepReport));
    if (e == hipSuccess) {
        // mailbox: fine-grained device memory written through the PCIe BAR when the machine allows it (every block
        // polls its own memory), else pinned host memory polled by block 0 and relayed (ICP_MAILBOX=host forces that)
        // (ICP_MAILBOX: a comma list of `host` -- pinned memory + relay -- and `plain` -- the line written word by word)
        const char* mv = std::getenv("ICP_MAILBOX");
        if (mv && std::strstr(mv, "plain")) c->mail_wide = false;
        int large_bar = 0;
        if (!(mv && std::strstr(mv, "host")) && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) == hipSuccess && large_bar &&
            hipExtMallocWithFlags((void**)&c->h_mail, kMailSlots * kMailSlotBytes, hipDeviceMallocFinegrained) == hipSuccess) {
            c->mail_in_bar = true;
        } else {
            (void)hipGetLastError();
            e = hipHostMalloc((void**)&c->h_mail, kMailSlots * kMailSlotBytes, hipHostMallocMapped | hipHostMallocCoherent);
        }
        if (e == hipSuccess) { std::memset(c->h_mail, 0, kMailSlots * kMailSlotBytes); icp::bar_fence(); }
    }
    if (e == hipSuccess) {
        if (hipExtMallocWithFlags((void**)&c->relay, kMailSlotBytes, hipDeviceMallocFinegrained) == hipSuccess) {
            e = hipMemset(c->relay, 0, kMailSlotBytes);
        } else {
            (void)hipGetLastError();
            c->relay = nullptr;  // no armed / resident launches on this device: every pass is launched after its solve
        }
    }

    if (e != hipSuccess) {
        const std::string msg = std::string("context setup: ") + hipGetErrorString(e);
        icp_destroy(c);
        return fail(ICP_ERR_HIP, msg);
    }
    c->stream = c->own_stream;
    // test hooks, one variable: ICP_DEBUG="stall=pass:seconds,lose=pass,shared_resident" (tests/test_gpu_runtime.py, tests/test_gpu_parity.py)
    if (const char* v = std::getenv("ICP_DEBUG")) {
        if (const char* q = std::strstr(v, "lose=")) c->debug_lose_pass = std::atoi(q + 5);
        if (const char* q = std::strstr(v, "stall=")) {
            int pass = -1;
            double sec = 0.0;
            if (std::sscanf(q + 6, "%d:%lf", &pass, &sec) == 2 && pass >= 0 && sec > 0.0 && sec < 30.0) { c->debug_stall_pass = pass; c->debug_stall_s = sec; }
        }
        c->debug_shared_resident = std::strstr(v, "shared_resident") != nullptr;
    }
    c->tune = icp::nn_tuning_from_env();
    c->use_boxes = c->tune.sparse != 0;
    if (const char* v = std::getenv("ICP_ARMED")) c->arm = !(v[0] == '0');
    if (const char* v = std::getenv("ICP_RESIDENT")) c->resident = v[0] == '0' ? 0 : (v[0] == '2' ? 2 : 1);
    if (const char* v = std::getenv("ICP_SHARE_RESIDENT_AFTER")) c->share_resident_after = std::atoi(v);
    if (const char* v = std::getenv("ICP_SHARE_AUTO")) c->share_auto = !(v[0] == '0');
    if (const char* v = std::getenv("ICP_NN_SPLIT_MIN")) c->split_min = std::max(0, std::atoi(v));   // (A/B runs and tests)
    if (const char* v = std::getenv("ICP_HOST_ROWS_MAX")) c->host_rows_max = std::max(1, std::atoi(v));
    if (const char* v = std::getenv("ICP_TRACE")) { c->trace = v[0] == '1' || v[0] == '2'; c->trace_passes = v[0] == '2'; }
    if (const char* v = std::getenv("ICP_FUSED_TAIL")) c->fused_tail = !(v[0] == '0');
    if (const char* v = std::getenv("ICP_NN_PHASES")) {
        // diagnostic, ICP_NN_PHASES=file[:pass[:slots[:wipe]]] -- the matching kernel stamps its phases per wave; the last launch's
        // stamps are written to the named file (raw int64) when the context is destroyed -- tools/phase_report.py reads it.
        // pass: stamp this pass of a resident launch only (-1 / empty: every pass, the last one survives); slots: room for more than
        // the default 3277 sixteen-wave blocks (160 stamps a block); wipe = 1: the log is cleared ahead of every launch
        std::string spec = v;
        std::vector<std::string> part;
        for (size_t at = 0;;) { const size_t q = spec.find(':', at); part.push_back(spec.substr(at, q == std::string::npos ? q : q - at)); if (q == std::string::npos) break; at = q + 1; }
        size_t slots = kPhaseSlots;
        if (part.size() > 1 && !part[1].empty()) c->tune.phase_pass = std::atoi(part[1].c_str());
        if (part.size() > 2 && !part[2].empty()) { const long long w = std::atoll(part[2].c_str()); if (w > 0 && w <= (1ll << 28)) slots = (size_t)w; }
        if (part.size() > 3 && !part[3].empty()) c->tune.phase_wipe = std::atoi(part[3].c_str()) != 0;
        if (!part[0].empty() && c->phase_log.ensure(slots * sizeof(long long)) == hipSuccess &&
            hipMemset(c->phase_log.p, 0, slots * sizeof(long long)) == hipSuccess) {
            c->phase_path = part[0];
            c->phase_slots = slots;
            c->tune.phase_log = (long long*)c->phase_log.p;
            c->tune.phase_cap = (long long)slots;
        }
    }
    *out = c;
    return ICP_OK;
}

void icp_destroy(icp_ctx* c)
{
    if (!c) return;
    if (c->trace && c->tr_n)
        std::fprintf(stderr, "[icp trace] %llu iterations: enqueue %.2f us, wait %.2f us, reduce %.2f us, solve %.2f us (host, per iteration)\n",
                     (unsigned long long)c->tr_n, 1e6 * c->tr_enqueue / c->tr_n, 1e6 * c->tr_wait / c->tr_n,
                     1e6 * c->tr_reduce / c->tr_n, 1e6 * c->tr_solve / c->tr_n);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) { icp::comm_destroy(c->comm); c->comm = nullptr; }
    if (c->lcomm) { icp::lcomm_destroy(c->lcomm); c->lcomm = nullptr; }
    if (c->phase_log.p && !c->phase_path.empty()) {
        std::vector<long long> h(c->phase_slots);
        if (hipMemcpy(h.data(), c->phase_log.p, c->phase_slots * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = std::fopen(c->phase_path.c_str(), "wb")) { std::fwrite(h.data(), sizeof(long long), h.size(), f); std::fclose(f); }
        }
        c->phase_log.release();
    }
    DevBuf* bufs[] = {&c->work, &c->fin_scratch, &c->fin_tickets, &c->dup_table, &c->slot_state, &c->share_counts, &c->seed_pub, &c->row_hits, &c->order_keys[0], &c->order_keys[1], &c->order_vals[0], &c->order_vals[1], &c->order_tmp, &c->order_roles, &c->order_totals, &c->P0, &c->P, &c->P2, &c->Q, &c->Qs, &c->Qbox, &c->Qrec, &c->Qsamp, &c->Qss, &c->Qperm, &c->Pperm, &c->prep_keys[0], &c->prep_keys[1], &c->prep_vals[0], &c->prep_vals[1], &c->prep_tmp, &c->prep_small, &c->prep_ext, &c->prep_voided, &c->prep_perm, &c->Nrm, &c->stage, &c->part_d, &c->part_idx, &c->idx[0], &c->idx[1],
                      &c->mom_partials, &c->err_partials, &c->mom_own, &c->nbr, &c->keys, &c->tickets};
    for (DevBuf* b : bufs) b->release();
    if (c->h_mom) (void)hipHostFree(c->h_mom);
    if (c->h_nonfinite) (void)hipHostFree(c->h_nonfinite);
    if (c->h_final) (void)hipHostFree(c->h_final);
    if (c->h_prep) (void)hipHostFree(c->h_prep);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_mail) { if (c->mail_in_bar) (void)hipFree(c->h_mail); else (void)hipHostFree(c->h_mail); }
    if (c->relay) (void)hipFree(c->relay);
    if (c->h_mom_partials) (void)hipHostFree(c->h_mom_partials);
    delete[] c->rows_seen;
    if (c->h_err_partials) (void)hipHostFree(c->h_err_partials);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int icp_comm_unique_id(void* out_bytes)
{
    if (!out_bytes) return fail(ICP_ERR_INVALID, "out == NULL");
    std::string err;
    const int rc = icp::comm_unique_id(out_bytes, err);
    return rc == ICP_OK ? ICP_OK : fail(rc, err);
}

int icp_comm_init(icp_ctx* c, const void* id_bytes, int rank, int world)
{
    if (int rc = use(c)) return rc;
    if (!id_bytes || world < 1 || rank < 0 || rank >= world) return fail(ICP_ERR_INVALID, "bad communicator arguments");
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    if (c->comm) { icp::comm_destroy(c->comm); c->comm = nullptr; }
    HIP_TRY(c->mom_own.ensure(ICP_NMOM * sizeof(double)));
    if (!c->mom_dev) c->mom_dev = (double*)c->mom_own.p;
    std::string err;
    const int rc = icp::comm_init(id_bytes, rank, world, &c->comm, err);
    return rc == ICP_OK ? ICP_OK : fail(rc, err);
}

int icp_comm_destroy(icp_ctx* c)
{
    if (int rc = use(c)) return rc;
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->comm) { icp::comm_destroy(c->comm); c->comm = nullptr; }
    if (c->lcomm) { icp::lcomm_destroy(c->lcomm); c->lcomm = nullptr; c->shares_device = false; }
    return ICP_OK;
}

int icp_comm_random_id(void* out_bytes)
{
    if (!out_bytes) return fail(ICP_ERR_INVALID, "out == NULL");
    std::memset(out_bytes, 0, ICP_COMM_ID_BYTES);
    FILE* f = std::fopen("/dev/urandom", "rb");
    size_t got = f ? std::fread(out_bytes, 1, 16, f) : 0;
    if (f) std::fclose(f);
    if (got != 16) {  // fall back to clock + pid: unique enough for a segment name on one node
        const uint64_t a = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count(), b = (uint64_t)getpid();
        std::memcpy(out_bytes, &a, 8);
        std::memcpy((char*)out_bytes + 8, &b, 8);
    }
    return ICP_OK;
}

int icp_comm_init_local(icp_ctx* c, const void* id_bytes, int rank, int world)
{
    if (int rc = use(c)) return rc;
    if (!id_bytes || world < 1 || rank < 0 || rank >= world) return fail(ICP_ERR_INVALID, "bad communicator arguments");
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    if (c->comm) return fail(ICP_ERR_STATE, "a device communicator is attached: destroy it first");
    // (a caller that installed its own moments buffer sums it across ranks itself, between enqueue and complete: with the node
    // communicator on top the vector would be summed twice -- the advisor's finding on round 3)
    if (c->mom_dev != nullptr && c->mom_dev != (double*)c->mom_own.p)
        return fail(ICP_ERR_STATE, "an external moments buffer is installed (icp_loop_set_moments_dev): its owner reduces it; remove it first");
    if (c->lcomm) { icp::lcomm_destroy(c->lcomm); c->lcomm = nullptr; }
    std::string err;
    const int rc = icp::lcomm_create(id_bytes, rank, world, &c->lcomm, err);
    if (rc != ICP_OK) return fail(rc, err);
    // Do two ranks of this communicator sit on ONE device (a rehearsal; the deployment is one process per GPU)?  Then no pass is
    // armed ahead of its (R, t): the waiting blocks of one rank can keep the running pass of the other off the CUs, and with an
    // exchange between the ranks that is a circular wait (seen with two ranks of the 10 M-point configuration on one GPU: a
    // pass missing its last rows after the 2 s poll budget).  Every rank leaves its device's PCI address in its slot of one
    // sum; plain launches wait on nothing that is not running.
    c->shares_device = false;
    if (world > 1 && world <= ICP_NMOM) {
        hipDeviceProp_t prop{};
        double ids[ICP_NMOM] = {0};
        // (an address of all zeros is "unknown": such ranks are not taken to share anything)
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && (prop.pciDomainID | prop.pciBusID | prop.pciDeviceID) != 0)
            ids[rank] = (double)(((long long)prop.pciDomainID << 16) | ((long long)prop.pciBusID << 8) | (long long)prop.pciDeviceID);
        if (int rc2 = icp::lcomm_allreduce_sum_f64(c->lcomm, ids, world, err)) return fail(rc2, err);
        for (int r = 0; r < world; ++r)
            if (r != rank && ids[r] != 0.0 && ids[r] == ids[rank]) c->shares_device = true;
    }
    return ICP_OK;
}

struct icp_lcomm { icp::LocalComm* p; };

int icp_lcomm_create(const void* id_bytes, int rank, int world, icp_lcomm** out)
{
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    *out = nullptr;
    std::string err;
    icp::LocalComm* p = nullptr;
    if (int rc = icp::lcomm_create(id_bytes, rank, world, &p, err)) return fail(rc, err);
    *out = new icp_lcomm{p};
    return ICP_OK;
}

int icp_lcomm_allreduce(icp_lcomm* h, double* v, int count)
{
    if (!h) return fail(ICP_ERR_INVALID, "null communicator");
    std::string err;
    const int rc = icp::lcomm_allreduce_sum_f64(h->p, v, count, err);
    return rc == ICP_OK ? ICP_OK : fail(rc, err);
}

void icp_lcomm_destroy(icp_lcomm* h)
{
    if (!h) return;
    icp::lcomm_destroy(h->p);
    delete h;
}

int icp_set_stream(icp_ctx* c, void* hip_stream)
{
    if (int rc = use(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return ICP_OK;
}

int icp_set_profiling(icp_ctx* c, int enable)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    c->profiling = enable != 0;
    c->profile_stride = enable > 0 ? enable : 0;
    c->prof_seconds_nn = 0.0;
    c->prof_nn_launches = 0;
    c->prof_nn_passes = 0;
    // the stride counts from here: the first launch after this call is a timed one
    c->nn_launch_count = 0;
    c->resident_launch_count = 0;
    return ICP_OK;
}

int icp_set_exclusive(icp_ctx* c, int on)
{
    if (int rc = use(c)) return rc;
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    if (c->exclusive != (on != 0)) c->resident_refused = false;   // (another kernel variant: the occupancy question is asked again)
    c->exclusive = on != 0;
    return ICP_OK;
}

int icp_set_work_counting(icp_ctx* c, int enable)
{
    if (int rc = use(c)) return rc;
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (enable) {
        HIP_TRY(c->work.ensure(icp::NN_WORK_SLOTS * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(c->work.p, 0, icp::NN_WORK_SLOTS * sizeof(unsigned long long)));
    }
    c->count_work = enable != 0;
    return ICP_OK;
}

int icp_get_work_counters(icp_ctx* c, uint64_t* out, int reset)
{
    if (int rc = use(c)) return rc;
    if (!out) return fail(ICP_ERR_INVALID, "out == NULL");
    if (!c->work.p) return fail(ICP_ERR_STATE, "work counting was never enabled");
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->work.p, icp::NN_WORK_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(c->work.p, 0, icp::NN_WORK_SLOTS * sizeof(unsigned long long)));
    return ICP_OK;
}

int icp_nn_match_resident(icp_ctx* c, float* kernel_ms)
{
    if (int rc = use(c)) return rc;
    if (int rc = require_clouds(c)) return rc;
    if (int rc = ensure_work_buffers(c)) return rc;
    if (int rc = materialize_moving(c)) return rc;
    if (kernel_ms) HIP_TRY(hipEventRecord(c->ev0, c->stream));
    const icp::NNCullInputs cull = make_cull(c, nullptr);
    HIP_TRY(icp::launch_nn(c->plan, c->P.p, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, nullptr, &cull, nullptr, c->stream));
    if (kernel_ms) HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(icp::launch_merge(c->plan, c->part_d.p, (const int32_t*)c->part_idx.p, (int32_t*)c->idx[c->cur].p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->idx_valid = true;
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, c->ev0, c->ev1));
    return ICP_OK;
}

int icp_nn_match_bench(icp_ctx* c, int reps, float* total_ms) { return icp_nn_match_bench_ex(c, reps, 1, total_ms); }

int icp_nn_match_bench_ex(icp_ctx* c, int reps, int seeded, float* total_ms)
{
    if (int rc = use(c)) return rc;
    if (int rc = require_clouds(c)) return rc;
    if (reps <= 0 || !total_ms) return fail(ICP_ERR_INVALID, "reps/total_ms");
    if (int rc = ensure_work_buffers(c)) return rc;
    if (int rc = materialize_moving(c)) return rc;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    // seeded with the most recent correspondences when there are any: this is how the loop launches it
    const icp::NNCullInputs cull = make_cull(c, (seeded && c->idx_valid) ? (const int32_t*)c->idx[c->cur].p : nullptr);
    for (int r = 0; r < reps; ++r)
        HIP_TRY(icp::launch_nn(c->plan, c->P.p, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, nullptr, &cull, nullptr, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    // (behind the timed span) the last launch's partial results become the context's correspondences, as icp_nn_match_resident's
    // do: icp_get_indices after a seeded launch answers for THAT launch, not for the pass that seeded it
    HIP_TRY(icp::launch_merge(c->plan, c->part_d.p, (const int32_t*)c->part_idx.p, (int32_t*)c->idx[c->cur].p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->idx_valid = true;
    HIP_TRY(hipEventElapsedTime(total_ms, c->ev0, c->ev1));
    return ICP_OK;
}

// the reference's methodology (src/CUDA/Matching_opt.cu:213-226): events around EVERY launch, warm-ups first, the caller
// takes the minimum (and the mean) of the `reps` durations
int icp_nn_match_bench_launches(icp_ctx* c, int reps, int warmups, int mode, float* each_ms)
{
    if (int rc = use(c)) return rc;
    if (int rc = require_clouds(c)) return rc;
    if (reps <= 0 || warmups < 0 || !each_ms || mode < 0 || mode > 2) return fail(ICP_ERR_INVALID, "reps/warmups/mode/each_ms");
    if (c->loop.pending) return fail(ICP_ERR_STATE, "an enqueue is in flight");
    if (int rc = ensure_work_buffers(c)) return rc;
    if (int rc = materialize_moving(c)) return rc;
    icp::NNPlan pl = c->plan;
    const bool dense = mode == 2;
    if (dense) {
        if (c->prec != ICP_F32) return fail(ICP_ERR_INVALID, "the dense packed kernel is fp32");
        pl = icp::nn_plan(c->n, c->m, c->prec, c->num_cus, c->tune, 1);
        const size_t S = pl.splits > 0 ? (size_t)pl.splits : 1;
        HIP_TRY(c->part_d.ensure(S * (size_t)pl.n_pad * sizeof(float)));
        HIP_TRY(c->part_idx.ensure(S * (size_t)pl.n_pad * sizeof(int32_t)));
    }
    const icp::NNCullInputs cull = make_cull(c, (mode == 0 && c->idx_valid) ? (const int32_t*)c->idx[c->cur].p : nullptr);
    for (int r = -warmups; r < reps; ++r) {
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        HIP_TRY(icp::launch_nn(pl, c->P.p, c->Q.p, c->part_d.p, (int32_t*)c->part_idx.p, nullptr, dense ? nullptr : &cull, nullptr, c->stream));
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(hipEventSynchronize(c->ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        if (r >= 0) each_ms[r] = ms;
    }
    if (dense) {   // the partial buffers may have grown: nothing else depends on the dense plan
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ICP_OK;
}

int icp_share_rows_plan(const uint32_t* hits, int rows, int blocks, int model_points, int min_hits, int32_t* parts, uint32_t* target)
{
    if (!hits || !parts || rows < 1 || blocks < rows || model_points < 1 || min_hits < 1) return fail(ICP_ERR_INVALID, "icp_share_rows_plan: bad arguments");
    const unsigned int T = icp::share_rows_plan(hits, rows, blocks, icp::pad_model(model_points), min_hits, parts);
    if (target) *target = T;
    return ICP_OK;
}

int icp_diag_row_roles(icp_ctx* c, uint32_t* hits_io, int rows, int min_part, int total_div, int control, int32_t* roles_out)
{
    if (int rc = use(c)) return rc;
    if (!hits_io || !roles_out || rows < 1 || rows >= (1 << icp::NN_ROLE_ROW_BITS)) return fail(ICP_ERR_INVALID, "icp_diag_row_roles: bad arguments");
    static_assert(ICP_ROLES_EXTRA == icp::NN_ORDER_EXTRA, "the header's constant is the kernels'");
    DevBuf hits, keys[2], vals[2], tmp, roles, totals;
    const size_t rb = (size_t)rows * sizeof(unsigned int);
    auto body = [&]() -> int {
        HIP_TRY(hits.ensure(rb));
        for (int k = 0; k < 2; ++k) { HIP_TRY(keys[k].ensure(rb)); HIP_TRY(vals[k].ensure(rb)); }
        HIP_TRY(tmp.ensure(icp::row_order_temp_bytes(rows)));
        HIP_TRY(roles.ensure(((size_t)rows + icp::NN_ORDER_EXTRA) * sizeof(int32_t)));
        HIP_TRY(totals.ensure(2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(totals.p, 0, totals.cap, c->stream));
        HIP_TRY(hipMemcpyAsync(hits.p, hits_io, rb, hipMemcpyHostToDevice, c->stream));
        icp::RowOrderBuffers b{};
        for (int k = 0; k < 2; ++k) { b.keys[k] = (unsigned int*)keys[k].p; b.vals[k] = (int32_t*)vals[k].p; }
        b.temp = tmp.p; b.temp_bytes = tmp.cap; b.roles = (int32_t*)roles.p; b.totals = (unsigned long long*)totals.p;
        b.seq = 0; b.min_part = min_part; b.total_div = total_div; b.control = control;
        const int32_t* out = nullptr;
        HIP_TRY(icp::launch_row_order(b, (unsigned int*)hits.p, rows, &out, c->stream));
        HIP_TRY(hipMemcpyAsync(roles_out, out, ((size_t)rows + icp::NN_ORDER_EXTRA) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hits_io, hits.p, rb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return ICP_OK;
    };
    const int rc = body();
    DevBuf* all[] = {&hits, &keys[0], &keys[1], &vals[0], &vals[1], &tmp, &roles, &totals};
    for (DevBuf* d : all) d->release();
    return rc;
}

static void report_launch(const icp::NNPlan& pl, int* splits, int* blocks, int* threads, int* n_pad, int* m_pad)
{
    if (splits) *splits = pl.splits;
    if (blocks) *blocks = pl.blocks_x * pl.splits;
    if (threads) *threads = icp::nn_block_threads(pl);
    if (n_pad) *n_pad = pl.n_pad;
    if (m_pad) *m_pad = pl.m_pad;
}

int icp_nn_launch_info_ex(icp_ctx* c, int dense, int* splits, int* blocks, int* threads, int* n_pad, int* m_pad)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    report_launch(icp::nn_plan(c->n, c->m, c->prec, c->num_cus, c->tune, dense ? 1 : 0), splits, blocks, threads, n_pad, m_pad);
    return ICP_OK;
}

int icp_nn_launch_info(icp_ctx* c, int* splits, int* blocks, int* threads, int* n_pad, int* m_pad)
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    // (the geometry of the resident clouds, also before their first launch has fixed the plan)
    const bool fixed = c->plan.n == c->n && c->plan.m == c->m && c->plan.precision == c->prec;
    report_launch(fixed ? c->plan : icp::nn_plan(c->n, c->m, c->prec, c->num_cus, c->tune), splits, blocks, threads, n_pad, m_pad);
    return ICP_OK;
}

static int nn_match_host(icp_ctx* c, const void* P, int n, const void* Q, int m, int precision, int32_t* idx)
{
    if (int rc = use(c)) return rc;
    if (n < 0 || m < 0) return fail(ICP_ERR_INVALID, "negative size");
    if (n == 0) return ICP_OK;
    if (m == 0) return fail(ICP_ERR_EMPTY, "empty model cloud");
    if (!P || !Q || !idx) return fail(ICP_ERR_INVALID, "null pointer");
    if (int rc = icp_set_model(c, Q, m, precision)) return rc;
    if (int rc = icp_set_moving(c, P, n, precision)) return rc;
    if (int rc = icp_nn_match_resident(c, nullptr)) return rc;
    return download_idx(c, c->cur, idx);
}

int icp_nn_match_f32(icp_ctx* c, const float* P, int n, const float* Q, int m, int32_t* idx)
{
    return nn_match_host(c, P, n, Q, m, ICP_F32, idx);
}

int icp_nn_match_f64(icp_ctx* c, const double* P, int n, const double* Q, int m, int32_t* idx)
{
    return nn_match_host(c, P, n, Q, m, ICP_F64, idx);
}

// ---- normals -----------------------------------------------------------------------------------
int icp_diag_knn4_geometry(icp_ctx* c, int m, int out[5])
{
    if (!c) return fail(ICP_ERR_INVALID, "null context");
    if (!out || m < 5) return fail(ICP_ERR_INVALID, "icp_diag_knn4_geometry: bad arguments");
    icp::knn4_v2_geometry(m, c->num_cus, &out[0], &out[1], &out[2], &out[3]);
    out[4] = icp::knn4_v2_wave_tiles(out[3]);
    return ICP_OK;
}

int icp_estimate_normals(icp_ctx* c, void* nxyz_out, int32_t* nbr_out)
{
    if (int rc = use(c)) return rc;
    if (!c->have_model) return fail(ICP_ERR_STATE, "no model resident");
    const int m = c->m;
    if (m == 0) return fail(ICP_ERR_EMPTY, "empty model cloud");
    if (m < 5) return fail(ICP_ERR_INVALID, "normals need at least 5 model points (k = 4 neighbours + self)");
    icp::NNPlan pl = icp::nn_plan(m, m, c->prec, c->num_cus, c->tune);
    HIP_TRY(c->nbr.ensure((size_t)m * 4 * sizeof(int32_t)));
    const size_t es = icp::elem_size(c->prec);
    HIP_TRY(c->Nrm.ensure(3 * (size_t)pl.m_pad * es));
    if (c->prec == ICP_F32) {
        int n_pad, bx, S, seg;
        icp::knn4_v2_geometry(m, c->num_cus, &n_pad, &bx, &S, &seg);
        // the per-segment top-5 lists reuse the matching partial buffers
        HIP_TRY(c->part_d.ensure((size_t)S * n_pad * 5 * sizeof(float)));
        HIP_TRY(c->part_idx.ensure((size_t)S * n_pad * 5 * sizeof(int32_t)));
        HIP_TRY(icp::launch_knn4_v2(c->Q.p, m, c->num_cus, (float*)c->part_d.p, (int32_t*)c->part_idx.p, (int32_t*)c->nbr.p,
                                    c->stream));
    } else {
        HIP_TRY(icp::launch_knn4(pl, c->Q.p, (int32_t*)c->nbr.p, c->stream));
    }
    // covariance + eigen-solve on the device, straight into the resident (padded SoA) normal cloud
    HIP_TRY(icp::launch_normals(c->prec, c->Q.p, m, pl.m_pad, (const int32_t*)c->nbr.p, c->Nrm.p, c->stream));
    if (nxyz_out) {
        HIP_TRY(c->stage.ensure(3 * (size_t)m * es));
        HIP_TRY(icp::launch_soa_to_aos(c->prec, c->Nrm.p, m, pl.m_pad, c->stage.p, c->stream));
        HIP_TRY(hipMemcpyAsync(nxyz_out, c->stage.p, 3 * (size_t)m * es, hipMemcpyDeviceToHost, c->stream));
    }
    if (nbr_out)
        HIP_TRY(hipMemcpyAsync(nbr_out, c->nbr.p, (size_t)m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_normals = true;
    return ICP_OK;
}

int icp_os1_packets_to_cartesian(icp_ctx* c, const uint8_t* packets, int n_packets, const float alt16[16],
                                 const float az16[16], float* xyz_out, uint32_t* ranges_out)
{
    if (int rc = use(c)) return rc;
    if (n_packets < 0 || (n_packets > 0 && (!packets || !xyz_out)) || !alt16 || !az16) return fail(ICP_ERR_INVALID, "bad arguments");
    if (n_packets == 0) return ICP_OK;
    const size_t n = (size_t)n_packets * 256, bytes = (size_t)n_packets * 12608;
    DevBuf d_pk, d_ang, d_r, d_xyz;
    auto body = [&]() -> int {
        HIP_TRY(d_pk.ensure(bytes));
        HIP_TRY(d_ang.ensure(32 * sizeof(float)));
        HIP_TRY(d_r.ensure(n * sizeof(uint32_t)));
        HIP_TRY(d_xyz.ensure(3 * n * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_pk.p, packets, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_ang.p, alt16, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync((float*)d_ang.p + 16, az16, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(icp::launch_os1_packets((const uint8_t*)d_pk.p, n_packets, (const float*)d_ang.p, (const float*)d_ang.p + 16,
                                        (uint32_t*)d_r.p, (float*)d_xyz.p, c->stream));
        HIP_TRY(hipMemcpyAsync(xyz_out, d_xyz.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (ranges_out) HIP_TRY(hipMemcpyAsync(ranges_out, d_r.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return ICP_OK;
    };
    const int rc = body();
    d_pk.release(); d_ang.release(); d_r.release(); d_xyz.release();
    return rc;
}

int icp_os1_to_cartesian(icp_ctx* c, const uint32_t* ranges, int n, uint32_t encoder0, const float alt16[16],
                         const float az16[16], float* xyz_out)
{
    if (int rc = use(c)) return rc;
    if (n < 0 || (n > 0 && (!ranges || !xyz_out)) || !alt16 || !az16) return fail(ICP_ERR_INVALID, "bad arguments");
    if (n == 0) return ICP_OK;
    DevBuf d_r, d_ang, d_xyz;
    auto body = [&]() -> int {
        HIP_TRY(d_r.ensure((size_t)n * sizeof(uint32_t)));
        HIP_TRY(d_ang.ensure(32 * sizeof(float)));
        HIP_TRY(d_xyz.ensure(3 * (size_t)n * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_r.p, ranges, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_ang.p, alt16, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync((float*)d_ang.p + 16, az16, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(icp::launch_os1_conversion((const uint32_t*)d_r.p, n, encoder0, (const float*)d_ang.p,
                                           (const float*)d_ang.p + 16, (float*)d_xyz.p, c->stream));
        HIP_TRY(hipMemcpyAsync(xyz_out, d_xyz.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return ICP_OK;
    };
    const int rc = body();
    d_r.release(); d_ang.release(); d_xyz.release();
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop
