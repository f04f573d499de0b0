// libstormck: C-ABI of the MI355X block-checksum engine (declarations and the
// reference interface each entry point replaces: include/stormck.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <functional>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <dlfcn.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/uio.h>
#include <unistd.h>

#include <cerrno>

#include <rccl/rccl.h>  // types and declarations only: RCCL is loaded at run time (multi_root.h)

#include "../../include/stormck.h"
#include "commit_plan.h"
#include "dispatch.h"
#include "kernels.h"
#include "blob_probe.h"
#include "space_probe.h"
#include "objlist_probe.h"
#include "route_plan.h"
#include "update_plan.h"
#include "objlist_insert.h"
#include "blob_insert.h"
#include "xxh64_host.h"

using namespace stormck;

namespace {

thread_local std::string g_last_error;

// Fork-join pool for the host-side passes (commit planning, copies into pinned
// staging). Spawning threads per call cost about 30 us each, which at 16 threads was
// most of a 1M-record planning pass. Workers spin briefly after a job (the commit
// issues its passes back to back), then park on a condition variable.
class ForkJoin {
  public:
    static ForkJoin& get() {
        // never destroyed: workers may be parked at exit. A fork()ed child has none of
        // the parent's workers, so it drops the instance and builds its own.
        static std::once_flag once;
        std::call_once(once, [] { pthread_atfork(nullptr, nullptr, [] { instance_ = nullptr; }); });
        std::lock_guard<std::mutex> g(make_mu_);
        if (!instance_) instance_ = new ForkJoin();
        return *instance_;
    }
    unsigned size() const { return nw_ + 1; }
    // How long another caller's job is predicted to hold the pool, in microseconds (0: the
    // pool is free; advisory). A routed call that finds the pool held either waits for it or
    // runs on its own thread, which run() never queues, whichever it predicts is faster.
    double busy_for_us() {
        if (run_mu_.try_lock()) {
            run_mu_.unlock();
            return 0.0;
        }
        return std::max(1.0, busy_until_.load(std::memory_order_relaxed) - clock_us());
    }
    // fn(t) for t in [0, parts); parts is clamped to size(); the caller runs t = 0.
    // expected_us: how long the job is predicted to take (what busy_for_us reports).
    template <class F>
    void run(unsigned parts, F&& fn, double expected_us = 0) {
        parts = std::min(parts, size());
        if (parts <= 1) {
            fn(0u);
            return;
        }
        std::lock_guard<std::mutex> serial(run_mu_);
        busy_until_.store(clock_us() + expected_us, std::memory_order_relaxed);
        std::function<void(unsigned)> job = [&](unsigned t) {
            if (t < parts) fn(t);
        };
        job_ = &job;
        remaining_.store(nw_, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> g(mu_);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        job(0);
        while (remaining_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }

    // CPUs the process may use at once: its affinity mask, capped by the smallest CPU quota
    // on its cgroup's path (a GPU box grants each GPU's process 16 CPUs of a 256-CPU host by
    // quota). cgroup v2: cpu.max from the process's own cgroup (/proc/self/cgroup "0::/path",
    // e.g. a systemd slice on a bare host) up to the root of the mount, as a container sees
    // it; cgroup v1: cpu.cfs_quota_us / cpu.cfs_period_us of the cpu controller's mount.
    static unsigned usable_cpus() {
        cpu_set_t set;
        unsigned cpus = std::max(1u, std::thread::hardware_concurrency());
        if (sched_getaffinity(0, sizeof set, &set) == 0) cpus = std::max(1, CPU_COUNT(&set));
        double quota = 0;  // smallest quota found, in CPUs (0: none)
        auto take = [&](double q) {
            if (q > 0 && (quota == 0 || q < quota)) quota = q;
        };
        std::string rel;  // the process's cgroup v2 path
        if (FILE* f = std::fopen("/proc/self/cgroup", "r")) {
            char line[4096];
            while (std::fgets(line, sizeof line, f))
                if (std::strncmp(line, "0::", 3) == 0) {
                    rel = line + 3;
                    while (!rel.empty() && (rel.back() == '\n' || rel.back() == '/')) rel.pop_back();
                }
            std::fclose(f);
        }
        for (std::string dir = rel;; dir = dir.substr(0, dir.rfind('/'))) {
            if (FILE* f = std::fopen(("/sys/fs/cgroup" + dir + "/cpu.max").c_str(), "r")) {
                char q[32] = {};
                unsigned long long period = 0;
                if (std::fscanf(f, "%31s %llu", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0)
                    take(std::strtod(q, nullptr) / static_cast<double>(period));
                std::fclose(f);
            }
            if (dir.empty() || dir.find('/') == std::string::npos) break;
        }
        for (const char* d : {"/sys/fs/cgroup/cpu,cpuacct", "/sys/fs/cgroup/cpu"}) {
            long long q = -1, period = 0;
            if (FILE* f = std::fopen((std::string(d) + "/cpu.cfs_quota_us").c_str(), "r")) {
                if (std::fscanf(f, "%lld", &q) != 1) q = -1;
                std::fclose(f);
            }
            if (FILE* f = std::fopen((std::string(d) + "/cpu.cfs_period_us").c_str(), "r")) {
                if (std::fscanf(f, "%lld", &period) != 1) period = 0;
                std::fclose(f);
            }
            if (q > 0 && period > 0) {
                take(static_cast<double>(q) / static_cast<double>(period));
                break;
            }
        }
        if (quota > 0) cpus = std::min(cpus, std::max(1u, static_cast<unsigned>(quota + 0.5)));
        return cpus;
    }
    unsigned cpus() const { return cpus_; }

  private:
    ForkJoin() {
        cpus_ = usable_cpus();
        nw_ = std::min(16u, cpus_) - 1;
        for (unsigned i = 0; i < nw_; ++i) std::thread([this, i] { loop(i + 1); }).detach();
    }
    void loop(unsigned id) {
        uint64_t seen = 0;
        for (;;) {
            uint64_t g = gen_.load(std::memory_order_acquire);
            // a short spin catches the next pass of the same call (the commit issues its
            // passes back to back); longer ones would burn the CPU quota a GPU box gives the
            // process (16 CPUs there, with 256 in the affinity mask) while nothing runs
            for (const double t0 = clock_us(); g == seen && clock_us() - t0 < kSpinUs;) {
                std::this_thread::yield();
                g = gen_.load(std::memory_order_acquire);
            }
            if (g == seen) {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
                g = gen_.load(std::memory_order_acquire);
            }
            seen = g;
            (*job_)(id);
            remaining_.fetch_sub(1, std::memory_order_release);
        }
    }
    static constexpr double kSpinUs = 50.0;
    static double clock_us() {
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    static inline ForkJoin* instance_ = nullptr;
    static inline std::mutex make_mu_;
    std::atomic<double> busy_until_{0.0};
    unsigned nw_ = 0, cpus_ = 1;
    std::mutex run_mu_, mu_;
    std::condition_variable cv_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<unsigned> remaining_{0};
    const std::function<void(unsigned)>* job_ = nullptr;
};

// The pool as a call allowed host_threads threads (0 = the pool) finds it. routed: a call that
// may use the pool asks how long another call's job holds it (route_plan.h route_on); the
// plan entry points price a free pool.
Pool pool_facts(uint32_t host_threads, bool routed) {
    ForkJoin& fj = ForkJoin::get();
    Pool p;
    p.size = fj.size();
    p.cpus = fj.cpus();
    p.threads = host_threads ? std::min<unsigned>(host_threads, p.size) : p.size;
    p.busy_us = routed && p.threads > 1 ? fj.busy_for_us() : 0.0;
    return p;
}

// Host threads a call may use: `threads` of the pool (0 = the pool).
unsigned pool_threads(uint32_t threads) { return pool_facts(threads, false).threads; }

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? STORMCK_ENOMEM : STORMCK_EHIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

static_assert(kPlanRingSlots == kRingSlots && kPlanPipePieces == uint64_t{kPipeMaxChunks} * kChunkPieces &&
                  kPlanMultiPieces == kMultiPieces && kPlanOrderBuckets == kOrderBuckets && kPlanNodeLds == kNodeLds,
              "dispatch.h plans with the limits of kernels.h");

// Cached answer to "is there a usable gfx950 device?" per process.
int device_check() {
    static std::once_flag once;
    static int status = STORMCK_OK;
    static std::string why;
    std::call_once(once, [] {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count == 0) {
            status = STORMCK_ENODEV;
            why = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count == 0");
            return;
        }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, 0) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            status = STORMCK_ENODEV;
            why = std::string("device 0 is not gfx950: ") + prop.gcnArchName;
        }
    });
    if (status != STORMCK_OK) g_last_error = why;
    return status;
}

// Compute units of the calling thread's current device (0 if unknown), cached per device.
uint64_t cu_count() {
    static std::atomic<int> cache[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            return 0;
        }
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return static_cast<uint64_t>(v);
}

// Fault slots of the ring kernels (kernels.h PipeCtl), one per (device, stream). A ring
// kernel whose bounded wait expired stores its fault code into the slot of the stream it
// was launched on and writes no checksum for the blocks of the stalled workgroup (a verify
// counts them as mismatches). A caller reads only its own stream's slot: the
// host-synchronous entry points after their sync (take_fault on the library's staging
// streams, or on the commit's stream), stormck_device_status(stream) for the asynchronous
// ones, so a fault never reaches a caller on another stream (include/stormck.h). The slots
// are pinned, device-mapped, coherent words, allocated with the device's table by
// stormck_init or the first call that sets up the device (never inside a stream capture).
// A table holds kFaultSlots streams; past that, the slot of the least recently launched
// stream whose word is clear is reused. That stream's last ring launch is then older than
// the last launches of 1,023 other streams, while a ring kernel runs for tens of
// microseconds, so in practice it has ended; a graph captured on it would still write the
// old slot on a later replay, which is why captured launches need a stream of their own
// among at most kFaultSlots live ones (include/stormck.h).
constexpr uint32_t kFaultSlots = 1024;

struct FaultTable {
    std::mutex mu;
    uint32_t* words = nullptr;                   // kFaultSlots words
    std::vector<hipStream_t> owner;              // slot -> stream
    std::vector<uint64_t> last_launch;           // slot -> sequence number of its last ring launch (0: free)
    std::vector<std::pair<hipStream_t, uint32_t>> index;  // stream -> slot, for the streams that have one
    uint64_t clock = 0;

    int find(hipStream_t st) const {
        for (const auto& e : index)
            if (e.first == st) return static_cast<int>(e.second);
        return -1;
    }
};
FaultTable g_faults[64];

// Allocate a device's fault slots (caller holds t.mu).
int fault_table_alloc(FaultTable& t) {
    if (t.words) return STORMCK_OK;
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, kFaultSlots * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent));
    std::memset(p, 0, kFaultSlots * sizeof(uint32_t));
    t.words = static_cast<uint32_t*>(p);
    t.owner.assign(kFaultSlots, nullptr);
    t.last_launch.assign(kFaultSlots, 0);
    return STORMCK_OK;
}

int fault_table_ready(int dev) {
    if (dev < 0 || dev >= 64) return fail(STORMCK_EINVAL, "device index beyond 64");
    FaultTable& t = g_faults[dev];
    std::lock_guard<std::mutex> g(t.mu);
    return fault_table_alloc(t);
}

// The fault slot a ring kernel launched on stream `st` of the current device writes.
int fault_slot(hipStream_t st, uint32_t** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(STORMCK_EINVAL, "device index beyond 64");
    FaultTable& t = g_faults[dev];
    std::lock_guard<std::mutex> g(t.mu);
    if (!t.words) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone)
            return fail(STORMCK_EINVAL, "first ring-kernel launch on device " + std::to_string(dev) +
                                            " inside a stream capture: call stormck_init(" + std::to_string(dev) +
                                            ") before capturing");
        const int rc = fault_table_alloc(t);
        if (rc) return rc;
    }
    int s = t.find(st);
    if (s < 0) {
        // a free slot, else the least recently launched one whose word is clear
        int pick = -1;
        for (uint32_t i = 0; i < kFaultSlots && pick < 0; ++i)
            if (t.last_launch[i] == 0) pick = static_cast<int>(i);
        if (pick < 0) {
            uint64_t oldest = UINT64_MAX;
            for (uint32_t i = 0; i < kFaultSlots; ++i)
                if (__atomic_load_n(t.words + i, __ATOMIC_ACQUIRE) == 0 && t.last_launch[i] < oldest) {
                    oldest = t.last_launch[i];
                    pick = static_cast<int>(i);
                }
            if (pick < 0) return fail(STORMCK_EHIP, "every ring-kernel fault slot holds an unreported fault");
            for (size_t k = 0; k < t.index.size(); ++k)
                if (t.index[k].second == static_cast<uint32_t>(pick)) {
                    t.index[k] = t.index.back();
                    t.index.pop_back();
                    break;
                }
        }
        s = pick;
        t.owner[s] = st;
        t.index.emplace_back(st, static_cast<uint32_t>(s));
    }
    t.last_launch[s] = ++t.clock;
    *out = t.words + s;
    return STORMCK_OK;
}

std::string fault_text(uint32_t code) {
    const uint32_t k = code & 0xff;
    const char* kernel = k == kFaultWideMulti ? "k_xxh64_wide_multi" : (k == kFaultCommitMulti ? "k_commit_level_multi" : "ring kernel");
    const char* side = (code & kFaultStager) ? "a stager wave's wait for the chain" : "the chain wave's wait for a staged chunk";
    return std::string(kernel) + ": ring staging stalled (" + side +
           " expired); no checksum was written for the blocks of the stalled workgroup";
}

// After a sync of stream `st` on device `dev`: STORMCK_EHIP with the fault's text if a
// ring kernel launched on `st` reported one since the last check (the slot is then
// cleared), else STORMCK_OK. Other streams' slots are not read.
int take_fault(int dev, hipStream_t st) {
    if (dev < 0 || dev >= 64) return STORMCK_OK;
    FaultTable& t = g_faults[dev];
    uint32_t code = 0;
    {
        std::lock_guard<std::mutex> g(t.mu);
        if (!t.words) return STORMCK_OK;
        const int s = t.find(st);
        if (s < 0) return STORMCK_OK;
        code = __atomic_exchange_n(t.words + s, 0u, __ATOMIC_ACQ_REL);
    }
    if (code == 0) return STORMCK_OK;
    return fail(STORMCK_EHIP, "device " + std::to_string(dev) + ": " + fault_text(code));
}

// STORMCK_DEBUG_STALL_CHUNK=c: stager wave 1 of workgroup 0 of every ring kernel never
// reports chunk c (c >= 1), so the chain's wait expires (tests of the fault path only);
// with STORMCK_DEBUG_STALL_STREAM=<stream handle>, only the launches on that stream.
uint32_t debug_stall(hipStream_t st) {
    static const uint32_t c = [] {
        const char* e = std::getenv("STORMCK_DEBUG_STALL_CHUNK");
        return e ? static_cast<uint32_t>(std::strtoul(e, nullptr, 10)) : 0u;
    }();
    static const uintptr_t only = [] {
        const char* e = std::getenv("STORMCK_DEBUG_STALL_STREAM");
        return e ? static_cast<uintptr_t>(std::strtoull(e, nullptr, 0)) : uintptr_t{0};
    }();
    return (only == 0 || reinterpret_cast<uintptr_t>(st) == only) ? c : 0u;
}

// Runtime choices as compile-time constants, so that each kernel family's launch is written
// once, in a generic lambda: with_consts(f, a, b) calls f(std::bool_constant<a>{},
// std::bool_constant<b>{}); with_int<1, 3, 8>(w, f) calls f(std::integral_constant<int, w>{})
// for a listed w. A lambda excludes with `if constexpr` the combinations no plan asks for
// (dispatch.h), so they are not instantiated: the variants of the probe build among them.
#define STORMCK_V(C) decltype(C)::value
template <class F>
void with_consts(F&& f) { f(); }
template <class F, class... Rest>
void with_consts(F&& f, bool b, Rest... rest) {
    if (b) with_consts([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_consts([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <int... Vs, class F>
void with_int(int v, F&& f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// The wide-multi launch of a checksum batch and of a commit level: the fault slot of the
// launch's stream, the debug stall, and the workgroup shape as constants.
// launch(BPW, RING, CHUNK, DBL, fault, stall) launches the caller's kernel.
template <class F>
int launch_wide_multi(const MultiShape& s, hipStream_t st, F&& launch) {
    uint32_t* fault = nullptr;  // the fault slot of this launch's stream
    if (s.ring) {
        const int frc = fault_slot(st, &fault);
        if (frc) return frc;
    }
    const uint32_t stall = debug_stall(st);
    auto shape = [&](auto BPW, auto RING) {
        constexpr bool wide = STORMCK_V(BPW) == kMultiBpwWide;
        launch(BPW, RING, std::integral_constant<uint32_t, wide ? kChunkPiecesWide : kChunkPieces>{},
               std::bool_constant<wide>{}, fault, stall);
    };
    using Ring = std::integral_constant<uint32_t, kRingSlots>;
    if constexpr (kProbes) {  // the rejected 16-block / whole-block-staging variants
        if (s.ring && s.bpw == kMultiBpwWide) {
            shape(std::integral_constant<int, kMultiBpwWide>{}, Ring{});
            return STORMCK_OK;
        }
        if (!s.ring) {
            shape(std::integral_constant<int, kMultiBpw>{}, std::integral_constant<uint32_t, 0>{});
            return STORMCK_OK;
        }
    }
    if (s.bpw == kMultiBpw) shape(std::integral_constant<int, kMultiBpw>{}, Ring{});
    else shape(std::integral_constant<int, kMultiBpwRing>{}, Ring{});
    return STORMCK_OK;
}

// Stream-ordered workspaces (the gather order) come from a private pool per device that
// keeps what it has reserved across calls; the device's default pool, which other
// libraries of the process (torch's hipMallocAsync backend) may use, is left as it is.
int workspace_pool(hipMemPool_t* out) {
    static std::mutex mu;
    static hipMemPool_t pools[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(STORMCK_EINVAL, "device index beyond 64");
    std::lock_guard<std::mutex> g(mu);
    if (!pools[dev]) {
        hipMemPoolProps props;
        std::memset(&props, 0, sizeof props);
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t p = nullptr;
        HIP_TRY(hipMemPoolCreate(&p, &props));
        uint64_t thr = UINT64_MAX;
        HIP_TRY(hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &thr));
        pools[dev] = p;
    }
    *out = pools[dev];
    return STORMCK_OK;
}

// One batch on stream `st`: the plan is plan_checksum's (dispatch.h, with the measurements
// behind every threshold). remote: the blocks are host memory read in place over PCIe.
int launch_checksum(const uint8_t* base, uint64_t stride, const uint32_t* lens, uint32_t len, const uint64_t* offs,
                    uint64_t n, uint64_t* out, const uint64_t* expected, unsigned long long* first_bad,
                    unsigned long long* n_bad, hipStream_t st, bool remote = false) {
    const Query q{n, len, lens != nullptr, offs != nullptr, expected != nullptr, remote,
                  static_cast<unsigned>(reinterpret_cast<uintptr_t>(base) & 15), stride};
    const Plan p = plan_checksum(q, cu_count(), knobs());
    const dim3 grid(p.grid), block(p.block);
    switch (p.kernel) {
        case Kernel::TooLarge:
            return fail(STORMCK_EINVAL, "batch too large for one launch");
        case Kernel::Wide:
            with_consts([&](auto LENS, auto OFFS, auto VER) {
                hipLaunchKernelGGL((k_xxh64_wide<STORMCK_V(LENS), STORMCK_V(OFFS), STORMCK_V(VER)>), grid, block, 0, st,
                                   base, stride, lens, len, offs, n, out, expected, first_bad, n_bad);
            }, q.lens, q.offs, q.verify);
            break;
        case Kernel::WideMulti: {
            const int rc = launch_wide_multi(p.multi, st, [&](auto BPW, auto RING, auto CHUNK, auto DBL, uint32_t* fault,
                                                              uint32_t stall) {
                with_consts([&](auto LENS, auto OFFS, auto VER) {
                    hipLaunchKernelGGL((k_xxh64_wide_multi<STORMCK_V(LENS), STORMCK_V(OFFS), STORMCK_V(VER), STORMCK_V(BPW),
                                                           STORMCK_V(RING), STORMCK_V(CHUNK), STORMCK_V(DBL)>),
                                       grid, block, 0, st, base, stride, lens, len, offs, n, out, expected, first_bad, n_bad,
                                       fault, stall);
                }, q.lens, q.offs, q.verify);
            });
            if (rc) return rc;
            break;
        }
        case Kernel::GldsVar:  // 2-wave workgroups: the probe build's kernels before round 3
            with_int<1, 2, 3, kGldsWaves>(p.waves, [&](auto W) {
                with_consts([&](auto VER, auto SKEW, auto LENS, auto OFFS) {
                    constexpr int w = STORMCK_V(W);
                    if constexpr ((STORMCK_V(LENS) || STORMCK_V(OFFS)) && (kProbes || w != 2) &&
                                  (!STORMCK_V(SKEW) || w == kGldsWaves))
                        hipLaunchKernelGGL((k_xxh64_glds_var<kTileStripes, kAuxNT, STORMCK_V(VER), w,
                                                             STORMCK_V(SKEW) ? kSkewTiles : 0, STORMCK_V(LENS), STORMCK_V(OFFS)>),
                                           grid, block, 0, st, base, stride, lens, len, offs, n, out, expected, first_bad,
                                           n_bad, nullptr);
                }, q.verify, p.persistent, q.lens, q.offs);
            });
            break;
        case Kernel::GldsVarOrdered: {
            hipMemPool_t pool = nullptr;
            const int prc = workspace_pool(&pool);
            if (prc) return prc;
            const uint64_t words = (uint64_t{kOrderBuckets} * 3 + n + 1) & ~uint64_t{1};
            void* ws = nullptr;
            HIP_TRY(hipMallocFromPoolAsync(&ws, p.ws_bytes, pool, st));
            uint32_t* bounds = static_cast<uint32_t*>(ws);  // [first, end) per bucket (end: totals first)
            uint32_t* cursor = bounds + 2 * kOrderBuckets;
            uint32_t* order = cursor + kOrderBuckets;
            uint64_t* s_offs = reinterpret_cast<uint64_t*>(bounds + words);
            uint32_t* s_lens = lens ? reinterpret_cast<uint32_t*>(s_offs + n) : nullptr;
            uint64_t* s_out = p.defer ? reinterpret_cast<uint64_t*>(  // 8-byte aligned after the lengths
                                            (reinterpret_cast<uintptr_t>(s_offs + n) + (lens ? n * 4 : 0) + 7) & ~uintptr_t{7})
                                      : nullptr;
            hipError_t orc = hipSuccess;
            with_consts([&](auto IDX) {
                if constexpr (kProbes || !STORMCK_V(IDX))
                    orc = order_pass<STORMCK_V(IDX)>(offs, lens, n, bounds, cursor, order, s_offs, s_lens, st);
            }, p.idx);
            HIP_TRY(orc);
#ifdef STORMCK_PROBES
            if (p.rank)
                hipLaunchKernelGGL(k_order_rank, dim3(static_cast<unsigned>(n / kGldsBlocks)), dim3(kGldsBlocks), 0, st,
                                   order, s_offs, s_lens, static_cast<uint64_t>(grid.x));
#endif
            lens = s_lens;
            offs = s_offs;
            const bool scatter = p.defer && !p.contig;  // hashed into the sorted positions, scattered after
            with_consts([&](auto SKEW, auto LENS, auto CONTIG, auto DEFER) {
                constexpr int skew = STORMCK_V(SKEW) ? kSkewTiles : 0;
                if constexpr (STORMCK_V(CONTIG)) {
                    if constexpr (kProbes && STORMCK_V(SKEW))
                        hipLaunchKernelGGL((k_xxh64_glds_var<kTileStripes, kAuxNT, false, kGldsWaves, kSkewTiles,
                                                             STORMCK_V(LENS), true, true, true>),
                                           grid, block, 0, st, base, stride, lens, len, offs, n, out, expected, first_bad,
                                           n_bad, order);
                } else if constexpr (STORMCK_V(DEFER)) {
                    hipLaunchKernelGGL((k_xxh64_glds_var<kTileStripes, kAuxNT, false, kGldsWaves, skew, STORMCK_V(LENS), true>),
                                       grid, block, 0, st, base, stride, lens, len, offs, n, s_out, expected, first_bad, n_bad,
                                       nullptr);
                } else {
                    hipLaunchKernelGGL((k_xxh64_glds_var<kTileStripes, kAuxNT, false, kGldsWaves, skew, STORMCK_V(LENS), true,
                                                         true>),
                                       grid, block, 0, st, base, stride, lens, len, offs, n, out, expected, first_bad, n_bad,
                                       order);
                }
            }, p.persistent, q.lens, p.contig, scatter);
            if (scatter) hipLaunchKernelGGL(k_order_scatter, dim3(2048), dim3(256), 0, st, order, s_out, out, n);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipFreeAsync(ws, st));
            return STORMCK_OK;
        }
        case Kernel::Glds:  // the 8-wave workgroups synchronise their ring; 4 waves: probe build
            with_int<1, 2, 3, 4, kGldsWaves>(p.waves, [&](auto W) {
                with_consts([&](auto VER) {
                    constexpr int w = STORMCK_V(W);
                    if constexpr (kProbes || w != 4)
                        hipLaunchKernelGGL((k_xxh64_glds<kTileStripes, kRing, kAuxNT, true, STORMCK_V(VER), w, w == kGldsWaves>),
                                           grid, block, 0, st, base, stride, len, n, out, expected, first_bad, n_bad);
                }, q.verify);
            });
            break;
        case Kernel::GldsSkew:
            with_consts([&](auto VER) {
                hipLaunchKernelGGL((k_xxh64_glds_skew<kTileStripes, kAuxNT, STORMCK_V(VER), kGldsWaves, kSkewTiles>), grid,
                                   block, 0, st, base, stride, len, n, out, expected, first_bad, n_bad);
            }, q.verify);
            break;
        case Kernel::QuadSpread:
            with_consts([&](auto LENS, auto OFFS, auto VER) {
                hipLaunchKernelGGL((k_xxh64_quad<kU, STORMCK_V(LENS), STORMCK_V(OFFS), STORMCK_V(VER), false, kQuadSpreadDepth, 64>),
                                   grid, block, 0, st, base, stride, lens, len, offs, n, out, expected, first_bad, n_bad);
            }, q.lens, q.offs, q.verify);
            break;
        default:  // Kernel::Quad
            with_consts([&](auto LENS, auto OFFS, auto VER) {
                hipLaunchKernelGGL((k_xxh64_quad<kU, STORMCK_V(LENS), STORMCK_V(OFFS), STORMCK_V(VER)>), grid, block, 0, st,
                                   base, stride, lens, len, offs, n, out, expected, first_bad, n_bad);
            }, q.lens, q.offs, q.verify);
    }
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

// Optional phase timing of host-orchestrated calls (STORMCK_TRACE=1 -> stderr).
struct PhaseTimer {
    bool on;
    const char* what;
    std::chrono::steady_clock::time_point t0, last;
    std::string log;
    explicit PhaseTimer(const char* w) : on(std::getenv("STORMCK_TRACE") != nullptr), what(w) {
        t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char* phase) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        std::snprintf(buf, sizeof buf, " %s=%.3fms", phase, std::chrono::duration<double, std::milli>(now - last).count());
        log += buf;
        last = now;
    }
    ~PhaseTimer() {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[stormck] %s total=%.3fms%s\n", what,
                     std::chrono::duration<double, std::milli>(now - t0).count(), log.c_str());
    }
};

__global__ void k_init_result(uint64_t* r, uint64_t n) {
    if (threadIdx.x == 0) {
        r[0] = n;
        r[1] = 0;
    }
}

// ---- per-device context for the host-memory path ---------------------------------
constexpr uint64_t kChunkBytes = 256ULL << 20;  // bytes of block data per pipeline stage
static_assert(kStageChunkBytes == kChunkBytes, "route_plan.h prices the staging chunk of the stages");
constexpr int kStages = 2;

struct Stage {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t ready = nullptr;     // split leg: the same, waited for without spinning (blocking sync)
    uint8_t* pinned = nullptr;      // staging for pageable sources
    uint8_t* d_data = nullptr;
    uint32_t* d_lens = nullptr;
    uint64_t* d_offs = nullptr;     // split leg: block offsets of an in-place gather
    uint64_t* d_out = nullptr;
    uint64_t* h_out = nullptr;      // pinned
    uint64_t* d_expected = nullptr;
    uint64_t* d_result = nullptr;   // verify: first_bad, n_bad
    uint64_t* h_result = nullptr;   // pinned
    // what the stage holds (to drain its outputs)
    uint64_t first = 0, count = 0;
    bool busy = false;
};

struct DeviceCtx {
    std::mutex mu;
    int device = -1;
    bool ready = false;
    Stage st[kStages];
    // f1: the dirty records (commit order) and their checksums in coherent pinned host
    // memory, which the level kernels read and write in place over PCIe (zero-copy)
    stormck_dirty_block* commit_rec = nullptr;
    uint64_t* commit_cs = nullptr;
    uint64_t commit_n = 0;
};

std::mutex g_ctx_mu;
std::vector<std::unique_ptr<DeviceCtx>> g_ctx;

int get_ctx(DeviceCtx** out) {
    int rc = device_check();
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    rc = fault_table_ready(dev);  // the ring kernels' fault slots come with the device's context
    if (rc) return rc;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (g_ctx.size() <= static_cast<size_t>(dev)) g_ctx.resize(dev + 1);
    if (!g_ctx[dev]) {
        g_ctx[dev].reset(new DeviceCtx());
        g_ctx[dev]->device = dev;  // fixed for the context's life (read under its own mutex only)
    }
    *out = g_ctx[dev].get();
    return STORMCK_OK;
}

int ensure_ready(DeviceCtx* c) {
    if (c->ready) return STORMCK_OK;
    for (Stage& s : c->st) {
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.ready, hipEventDisableTiming | hipEventBlockingSync));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.pinned), kChunkBytes, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&s.d_data, kChunkBytes));
        const uint64_t maxb = kChunkBytes / 8;  // smallest admissible stride is 8 bytes per block
        HIP_TRY(hipMalloc(&s.d_lens, maxb * 4));
        HIP_TRY(hipMalloc(&s.d_offs, maxb * 8));
        HIP_TRY(hipMalloc(&s.d_out, maxb * 8));
        HIP_TRY(hipMalloc(&s.d_expected, maxb * 8));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.h_out), maxb * 8, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&s.d_result, 16));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.h_result), 16, hipHostMallocDefault));
    }
    c->ready = true;
    return STORMCK_OK;
}

void release_ctx(DeviceCtx* c) {
    if (!c || (!c->ready && !c->commit_rec)) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(c->device);
    for (Stage& s : c->st) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        (void)hipFree(s.d_data);
        (void)hipFree(s.d_lens);
        (void)hipFree(s.d_offs);
        (void)hipFree(s.d_out);
        (void)hipFree(s.d_expected);
        (void)hipFree(s.d_result);
        (void)hipHostFree(s.pinned);
        (void)hipHostFree(s.h_out);
        (void)hipHostFree(s.h_result);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.ready) (void)hipEventDestroy(s.ready);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        s = Stage();
    }
    c->ready = false;
    if (c->commit_rec) (void)hipHostFree(c->commit_rec);
    if (c->commit_cs) (void)hipHostFree(c->commit_cs);
    c->commit_rec = nullptr;
    c->commit_cs = nullptr;
    c->commit_n = 0;
    (void)hipSetDevice(prev);
}

// Whether this process can read the first and the last byte of [p, p + bytes) (e.g. not a
// device address the CPU mapping leaves inaccessible), without faulting. Only the two
// endpoints are checked: a range with an unmapped page in its middle passes, and the host
// threads then fault on it as a plain memcpy would (include/stormck.h asks for readable
// ranges; this check only turns device memory passed by mistake into EINVAL). One
// process_vm_readv of the two bytes from this process itself (EFAULT when either is not
// readable), or, where that syscall is not permitted, a write of each byte into a pipe.
bool host_readable(const void* p, uint64_t bytes) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    uint8_t got[2];
    iovec local = {got, 2};
    iovec remote[2] = {{const_cast<uint8_t*>(b), 1}, {const_cast<uint8_t*>(b + (bytes ? bytes - 1 : 0)), 1}};
    const ssize_t r = process_vm_readv(getpid(), &local, 1, remote, 2, 0);
    if (r == 2) return true;
    if (r >= 0 || errno == EFAULT) return false;
    static std::mutex mu;  // the syscall is filtered here (seccomp): the pipe
    static int fds[2] = {-1, -1};
    std::lock_guard<std::mutex> g(mu);
    if (fds[0] < 0 && pipe2(fds, O_NONBLOCK | O_CLOEXEC) != 0) return true;  // cannot tell: as before
    for (const uint8_t* q : {b, b + (bytes ? bytes - 1 : 0)}) {
        if (write(fds[1], q, 1) != 1) return errno != EFAULT;
        uint8_t sink = 0;
        (void)!read(fds[0], &sink, 1);
    }
    return true;
}

// Where a host-path argument lives. hipPointerGetAttributes names HIP's own allocations and
// registrations; plain host memory is unknown to it (an error, or hipMemoryTypeUnregistered),
// and so is device memory HIP did not map itself. An address it does not name is taken as
// host memory only when the process can read it, so such device memory is an argument
// error rather than a fault on a host thread.
enum class Mem {
    kPageable,    // ordinary host memory: host threads read it; the devices through staging
    kPinned,      // page-locked host memory: DMA-able
    kMapped,      // page-locked and mapped (stormck_host_register, hipHostMalloc): also read in place
    kDevice,      // HBM: the _device entry points
    kUnreadable,  // unknown to HIP and not readable by the host
};
// Host ranges registered through stormck_host_register (storm registers cache.data once, at
// start-up): classify() answers kMapped for them from this list rather than asking the HIP
// runtime, which takes its memory-object lock (storm's smallest commits pay every fixed cost of
// the routed call; verdict r05 item 4). Ranges leave the list in stormck_host_unregister.
// The list is kRegSlots atomic [lo, hi) slots, read without a lock (writers hold g_reg_mu);
// ranges past them are left to the runtime query.
constexpr int kRegSlots = 16;
std::mutex g_reg_mu;
std::atomic<uintptr_t> g_reg_lo[kRegSlots], g_reg_hi[kRegSlots];
std::atomic<int> g_reg_n{0};  // slots in use (a bound on the scan)

bool in_registered(const void* p, uint64_t bytes) {
    const int n = g_reg_n.load(std::memory_order_acquire);
    const uintptr_t x = reinterpret_cast<uintptr_t>(p);
    for (int k = 0; k < n; ++k) {
        const uintptr_t lo = g_reg_lo[k].load(std::memory_order_acquire);
        const uintptr_t hi = g_reg_hi[k].load(std::memory_order_acquire);
        if (lo && x >= lo && x < hi && bytes <= hi - x) return true;
    }
    return false;
}

void reg_add(void* p, uint64_t bytes) {
    std::lock_guard<std::mutex> g(g_reg_mu);
    for (int k = 0; k < kRegSlots; ++k)
        if (g_reg_lo[k].load(std::memory_order_relaxed) == 0) {
            g_reg_hi[k].store(reinterpret_cast<uintptr_t>(p) + bytes, std::memory_order_release);
            g_reg_lo[k].store(reinterpret_cast<uintptr_t>(p), std::memory_order_release);
            if (k >= g_reg_n.load(std::memory_order_relaxed)) g_reg_n.store(k + 1, std::memory_order_release);
            return;
        }
}

void reg_remove(void* p) {
    std::lock_guard<std::mutex> g(g_reg_mu);
    for (int k = 0; k < kRegSlots; ++k)
        if (g_reg_lo[k].load(std::memory_order_relaxed) == reinterpret_cast<uintptr_t>(p)) {
            g_reg_lo[k].store(0, std::memory_order_release);
            g_reg_hi[k].store(0, std::memory_order_release);
        }
}

Mem classify(const void* p, uint64_t bytes) {
    if (in_registered(p, std::max<uint64_t>(bytes, 1))) return Mem::kMapped;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) == hipSuccess) {
        if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return Mem::kDevice;
        // managed memory is DMA-able but has no hipHostGetDevicePointer mapping, which the
        // in-place (kMapped) kernels need: it takes the copy engine
        if (a.type == hipMemoryTypeManaged) return Mem::kPinned;
        if (a.type == hipMemoryTypeHost) return a.devicePointer ? Mem::kMapped : Mem::kPinned;
    } else {
        (void)hipGetLastError();
    }
    return host_readable(p, bytes) ? Mem::kPageable : Mem::kUnreadable;
}

// The error of a host-path argument that host threads must not read.
int not_host_memory(Mem m) {
    return m == Mem::kDevice ? fail(STORMCK_EINVAL, "base is device memory: use the _device entry points")
                             : fail(STORMCK_EINVAL, "base is not readable host memory");
}

// Parallel memcpy into pinned staging (pageable sources): a single thread cannot
// feed PCIe Gen5; a few threads can.
void par_copy(uint8_t* dst, const uint8_t* src, uint64_t bytes, uint64_t min_per_thread = 8ULL << 20) {
    ForkJoin& fj = ForkJoin::get();
    // 8 copy threads saturate host memory bandwidth; more only contend with the HIP
    // runtime's own threads for the box's cores
    const unsigned nt = static_cast<unsigned>(std::min<uint64_t>({8, fj.size(), std::max<uint64_t>(1, bytes / min_per_thread)}));
    fj.run(nt, [&](unsigned t) {
        const uint64_t lo = bytes * t / nt, hi = bytes * (t + 1) / nt;
        std::memcpy(dst + lo, src + lo, hi - lo);
    });
}

// n host blocks: block i at base + (offs ? offs[i] : i * stride), (lens ? lens[i] : len) bytes.
struct Blocks {
    const uint8_t* base = nullptr;
    uint64_t stride = 0;
    const uint64_t* offs = nullptr;
    const uint32_t* lens = nullptr;
    uint32_t len = 0;
    uint64_t n = 0;
    const uint8_t* at(uint64_t i) const { return base + (offs ? offs[i] : i * stride); }
    uint64_t len_of(uint64_t i) const { return lens ? lens[i] : len; }
    uint64_t bytes(uint64_t a, uint64_t b) const {
        if (!lens) return (b - a) * len;
        uint64_t s = 0;
        for (uint64_t i = a; i < b; ++i) s += lens[i];
        return s;
    }
    uint64_t longest() const {
        if (!lens) return len;
        uint64_t m = 0;
        for (uint64_t i = 0; i < n; ++i) m = std::max<uint64_t>(m, lens[i]);
        return m;
    }
};

// Where a call's checksums go: called from host threads and device workers at once, on
// disjoint blocks.
struct Sink {
    virtual ~Sink() = default;
    virtual void one(uint64_t i, uint64_t h) = 0;
    virtual void range(uint64_t i0, uint64_t cnt, const uint64_t* cs) {
        for (uint64_t k = 0; k < cnt; ++k) one(i0 + k, cs[k]);
    }
};

struct OutSink final : Sink {
    uint64_t* out;
    explicit OutSink(uint64_t* o) : out(o) {}
    void one(uint64_t i, uint64_t h) override { out[i] = h; }
    void range(uint64_t i0, uint64_t cnt, const uint64_t* cs) override { std::memcpy(out + i0, cs, cnt * 8); }
};

// ---- the stage engine: one chunk of host blocks through one stage ------------------------
// The host pipeline (fixed chunks, front to back) and a split's device part (chunks claimed
// from the back of its queue) both run their chunks through the device context's stages
// with these three functions: issue() enqueues a chunk on the stage's stream, drain() waits
// for it and hands its results on, abandon() clears the stages after a failure.

// Where a chunk's rows are when its kernel runs.
enum class Rows {
    kDma,      // copied into the stage's HBM from where they are (page-locked memory)
    kStaged,   // copied there through the stage's pinned buffer (pageable memory)
    kStrided,  // read in place over the link, stride apart (mapped memory)
    kGather,   // read in place at the blocks' offsets (mapped memory: a commit's height)
};

struct Chunk {
    const Blocks* B = nullptr;
    uint64_t first = 0, count = 0;       // blocks [first, first + count) of B
    uint32_t plan_len = 0;               // the length the kernels plan with (HostBatch::plan_len)
    const uint64_t* expected = nullptr;  // verify: compare instead of returning checksums
    Rows rows = Rows::kDma;
    const uint8_t* d_base = nullptr;     // in place: the device's address of B->base
};

// How drain() waits for a stage. The pipeline's caller spins on `done`. A split's device
// worker waits for `ready` in the kernel (a blocking-sync event: an interrupt wakes it),
// holding no CPU: the host threads it runs beside use all the CPU the process gets (a GPU
// box caps it by quota, so a spinning waiter would throttle them).
enum class Wait { kSpin, kBlock };

struct StageEngine {
    DeviceCtx* c;
    Wait wait;

    hipEvent_t event(const Stage& s) const { return wait == Wait::kSpin ? s.done : s.ready; }

    // Upload the chunk's rows (or, in place, its offsets) and lengths, launch, copy the
    // checksums (verify: the {first_bad, n_bad} pair) back into the stage's pinned buffers.
    int issue(Stage& s, const Chunk& ch) const {
        const Blocks& B = *ch.B;
        const uint64_t a = ch.first, cnt = ch.count;
        const bool in_place = ch.rows == Rows::kStrided || ch.rows == Rows::kGather;
        const uint8_t* base = s.d_data;
        uint64_t stride = B.stride;
        const uint64_t* offs = nullptr;
        if (!in_place) {
            // bytes to move: up to the end of the last block in the chunk
            const uint64_t bytes = (cnt - 1) * B.stride + B.len_of(a + cnt - 1);
            const uint8_t* src = B.at(a);
            if (ch.rows == Rows::kStaged) {
                // the pinned buffer may be refilled only after its H2D finished: the drain of
                // this stage before the issue guarantees that
                par_copy(s.pinned, src, bytes);
                src = s.pinned;
            }
            HIP_TRY(hipMemcpyAsync(s.d_data, src, bytes, hipMemcpyHostToDevice, s.stream));
            if (B.lens) HIP_TRY(hipMemcpyAsync(s.d_lens, B.lens + a, cnt * 4, hipMemcpyHostToDevice, s.stream));
        } else {
            uint8_t* pin = s.pinned;
            if (ch.rows == Rows::kGather) {  // the chunk's offsets
                std::memcpy(pin, B.offs + a, cnt * 8);
                HIP_TRY(hipMemcpyAsync(s.d_offs, pin, cnt * 8, hipMemcpyHostToDevice, s.stream));
                pin += cnt * 8;
                base = ch.d_base;
                stride = 0;
                offs = s.d_offs;
            } else {  // strided rows, read where they are
                base = ch.d_base + a * B.stride;
            }
            if (B.lens) {
                std::memcpy(pin, B.lens + a, cnt * 4);
                HIP_TRY(hipMemcpyAsync(s.d_lens, pin, cnt * 4, hipMemcpyHostToDevice, s.stream));
            }
        }
        using ull = unsigned long long;
        uint64_t* out = s.d_out;
        ull *first_bad = nullptr, *n_bad = nullptr;
        if (ch.expected) {
            HIP_TRY(hipMemcpyAsync(s.d_expected, ch.expected + a, cnt * 8, hipMemcpyHostToDevice, s.stream));
            s.h_result[0] = cnt;  // "no mismatch" until a block lowers it
            s.h_result[1] = 0;
            HIP_TRY(hipMemcpyAsync(s.d_result, s.h_result, 16, hipMemcpyHostToDevice, s.stream));
            out = nullptr;
            first_bad = reinterpret_cast<ull*>(s.d_result);
            n_bad = reinterpret_cast<ull*>(s.d_result + 1);
        }
        const int rc = launch_checksum(base, stride, B.lens ? s.d_lens : nullptr, ch.plan_len, offs, cnt, out,
                                       ch.expected ? s.d_expected : nullptr, first_bad, n_bad, s.stream, in_place);
        if (rc) return rc;
        if (ch.expected) HIP_TRY(hipMemcpyAsync(s.h_result, s.d_result, 16, hipMemcpyDeviceToHost, s.stream));
        else HIP_TRY(hipMemcpyAsync(s.h_out, s.d_out, cnt * 8, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipEventRecord(event(s), s.stream));
        s.first = a;
        s.count = cnt;
        s.busy = true;
        return STORMCK_OK;
    }

    // Wait for what the stage holds, if anything: its checksums go to `sink`, a verify's
    // mismatches into *first_bad (the lowest index, of the call's blocks) and *n_bad.
    int drain(Stage& s, bool verify, Sink* sink, uint64_t* first_bad, uint64_t* n_bad) const {
        if (!s.busy) return STORMCK_OK;
        const hipError_t e = hipEventSynchronize(event(s));
        s.busy = false;
        if (e != hipSuccess) return fail(STORMCK_EHIP, std::string("host stage: ") + hipGetErrorString(e));
        // a stalled ring kernel wrote no checksum (or no mismatch) for some blocks: nothing
        // of this stage reaches the caller
        const int frc = take_fault(c->device, s.stream);
        if (frc) return frc;
        if (!verify) {
            sink->range(s.first, s.count, s.h_out);
        } else if (s.h_result[1] > 0) {
            *n_bad += s.h_result[1];
            *first_bad = std::min<uint64_t>(*first_bad, s.first + s.h_result[0]);
        }
        return STORMCK_OK;
    }

    // A call that fails part-way must leave nothing in flight and no stage marked busy: the
    // stages are reused, and the next call's drain would hand that call the stale results.
    void abandon() const {
        for (Stage& s : c->st) {
            (void)hipStreamSynchronize(s.stream);
            s.busy = false;
        }
    }
};

// ---- one validated description of a host-memory batch --------------------------------------
struct HostBatch {
    Blocks B;
    uint64_t bytes = 0;     // hashed in all
    uint64_t longest = 0;   // the longest block
    uint64_t extent = 0;    // from base to the end of the last block
    uint64_t step = 8;      // a block's share of a staging chunk: the stride (one block: its length), at least 8
    uint32_t plan_len = 0;  // what the kernels plan with: len, or the longest of per-block lengths (at least 1)
};

constexpr const char* kBlocksOverlap = "stride smaller than a block length (blocks overlap)";

// The one pass over `lens`: sizes, the overlap rule, and what the legs derive from them.
int measure_batch(uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, HostBatch* hb) {
    *hb = HostBatch();
    Blocks& B = hb->B;
    B.stride = stride;
    B.lens = lens;
    B.len = len;
    B.n = n;
    hb->bytes = uint64_t{len} * n;
    hb->longest = len;
    if (lens) {
        hb->bytes = hb->longest = 0;
        for (uint64_t i = 0; i < n; ++i) {
            hb->bytes += lens[i];
            hb->longest = std::max<uint64_t>(hb->longest, lens[i]);
        }
    }
    if (n > 1 && stride < hb->longest) return fail(STORMCK_EINVAL, kBlocksOverlap);
    if (n == 0) return STORMCK_OK;
    hb->extent = (n - 1) * stride + B.len_of(n - 1);
    hb->step = n == 1 ? std::max<uint64_t>(hb->longest, 8) : std::max<uint64_t>(stride, 8);
    hb->plan_len = lens ? static_cast<uint32_t>(std::max<uint64_t>(hb->longest, 1)) : len;
    return STORMCK_OK;
}

// A batch entry point's arguments, checked in one order for every leg: base, the result
// array (out or expected; result_null is the entry point's message for it), overlap, and for
// the legs that stage whole blocks through 256 MiB chunks (staged) the block step. An empty
// batch has nothing to check: hb->B.n == 0, and the caller zeroes its outputs.
int host_batch(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, const void* result,
               const char* result_null, bool staged, HostBatch* hb) {
    if (n == 0) {
        *hb = HostBatch();
        return STORMCK_OK;
    }
    if (!base) return fail(STORMCK_EINVAL, "base is null");
    if (!result) return fail(STORMCK_EINVAL, result_null);
    const int rc = measure_batch(stride, lens, len, n, hb);
    if (rc) return rc;
    hb->B.base = static_cast<const uint8_t*>(base);
    if (staged && hb->step > kChunkBytes) return fail(STORMCK_EINVAL, "block stride exceeds the staging chunk (256 MiB)");
    return STORMCK_OK;
}

// An empty batch verifies: nothing mismatches.
int empty_batch(uint64_t* first_bad, uint64_t* n_bad) {
    if (first_bad) *first_bad = 0;
    if (n_bad) *n_bad = 0;
    return STORMCK_OK;
}

// The status of a verify entry point whose leg ran: mismatches are its own status.
int verify_status(int rc, const uint64_t* n_bad) {
    if (rc) return rc;
    return *n_bad > 0 ? fail(STORMCK_EMISMATCH, "checksum mismatch") : STORMCK_OK;
}

// The host pipeline of checksum_host / verify_host on the current device. Blocks are
// processed in chunks of whole blocks (<= kChunkBytes of stride); stage k's H2D+kernel+D2H
// run on its own stream while the host fills the other stage. known: what the caller's
// classify() said of the blocks' memory (null: not asked yet).
int host_pipeline(const HostBatch& hb, const Mem* known, uint64_t* out, const uint64_t* expected, uint64_t* first_bad,
                  uint64_t* n_bad) {
    const Blocks& B = hb.B;
    if (B.n == 0) return empty_batch(first_bad, n_bad);
    DeviceCtx* c = nullptr;
    int rc = get_ctx(&c);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    rc = ensure_ready(c);
    if (rc) return rc;
    const Mem mem = known ? *known : classify(B.base, hb.extent);
    if (mem == Mem::kDevice || mem == Mem::kUnreadable) return not_host_memory(mem);

    const StageEngine eng{c, Wait::kSpin};
    OutSink sink(out);
    Chunk ch;
    ch.B = &B;
    ch.plan_len = hb.plan_len;
    ch.expected = expected;
    ch.rows = mem == Mem::kPageable ? Rows::kStaged : Rows::kDma;
    const uint64_t per_chunk = std::max<uint64_t>(1, kChunkBytes / hb.step);
    uint64_t fb = B.n, nb = 0;
    for (uint64_t k = 0; ch.first < B.n && rc == STORMCK_OK; ch.first += per_chunk, ++k) {
        Stage& s = c->st[k % kStages];
        rc = eng.drain(s, expected != nullptr, &sink, &fb, &nb);
        ch.count = std::min<uint64_t>(per_chunk, B.n - ch.first);
        if (rc == STORMCK_OK) rc = eng.issue(s, ch);
    }
    for (Stage& s : c->st)
        if (rc == STORMCK_OK) rc = eng.drain(s, expected != nullptr, &sink, &fb, &nb);
    if (rc) {
        eng.abandon();
        return rc;
    }
    if (first_bad) *first_bad = fb;
    if (n_bad) *n_bad = nb;
    return STORMCK_OK;
}

// The same from raw arguments (out or expected is set): validate, then run.
int host_pipeline(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint64_t* out,
                  const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad) {
    HostBatch hb;
    const int rc = host_batch(base, stride, lens, len, n, expected ? static_cast<const void*>(expected) : out,
                              "out is null", true, &hb);
    return rc ? rc : host_pipeline(hb, nullptr, out, expected, first_bad, n_bad);
}

// A caller's device list: 1..64 entries.
int check_device_list(const int* devices, int n_devices) {
    if (!devices || n_devices <= 0 || n_devices > 64) return fail(STORMCK_EINVAL, "devices: 1..64 entries");
    return STORMCK_OK;
}

// Visible gfx950 devices, in the order given; unique: each once.
int check_devices(const int* devices, int n_devices, bool unique, std::vector<int>* out) {
    int rc = check_device_list(devices, n_devices);
    if (rc) return rc;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    out->clear();
    for (int k = 0; k < n_devices; ++k) {
        if (devices[k] < 0 || devices[k] >= count)
            return fail(STORMCK_EINVAL, "devices[" + std::to_string(k) + "] = " + std::to_string(devices[k]) +
                                            " is not a visible device");
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, devices[k]));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(STORMCK_ENODEV, "devices[" + std::to_string(k) + "] is not gfx950: " + prop.gcnArchName);
        if (!unique || std::find(out->begin(), out->end(), devices[k]) == out->end()) out->push_back(devices[k]);
    }
    return STORMCK_OK;
}

// One host batch over several devices from one process (storm is one Go process): the
// blocks split into contiguous ranges whose sizes differ by at most one (as the ranks of
// storm_amd/dist.py shard_range), and range k runs host_pipeline on devices[k] in its
// own host thread, so each device's PCIe link carries its own range. A device may be
// listed more than once; its ranges then share its staging (per-device mutex) and run
// one after another. Returns the failing status of the lowest-numbered range, with its
// message, or STORMCK_OK.
int host_pipeline_multi(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                        uint64_t* out, const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad,
                        const int* devices, int n_devices) {
    int rc = check_device_list(devices, n_devices);
    if (rc) return rc;
    if (n == 0) return empty_batch(first_bad, n_bad);
    rc = device_check();
    if (rc) return rc;
    std::vector<int> listed;  // duplicates kept: a device listed twice gets two ranges
    rc = check_devices(devices, n_devices, false, &listed);
    if (rc) return rc;
    const uint64_t parts = std::min<uint64_t>(static_cast<uint64_t>(n_devices), std::max<uint64_t>(n, 1));
    if (parts == 1 || n <= 1) {
        int prev = 0;
        HIP_TRY(hipGetDevice(&prev));
        HIP_TRY(hipSetDevice(devices[0]));
        rc = host_pipeline(base, stride, lens, len, n, out, expected, first_bad, n_bad);
        const std::string msg = g_last_error;
        (void)hipSetDevice(prev);
        g_last_error = msg;
        return rc;
    }
    if (!base) return fail(STORMCK_EINVAL, "base is null");
    struct Part {
        uint64_t lo = 0, hi = 0, fb = 0, nb = 0;
        int rc = STORMCK_OK;
        std::string err;
    };
    std::vector<Part> part(parts);
    const uint64_t q = n / parts, r = n % parts;
    for (uint64_t k = 0; k < parts; ++k) {
        part[k].lo = k * q + std::min(k, r);
        part[k].hi = part[k].lo + q + (k < r ? 1 : 0);
    }
    const uint8_t* b8 = static_cast<const uint8_t*>(base);
    auto work = [&](uint64_t k) {
        Part& P = part[k];
        if (hipSetDevice(devices[k]) != hipSuccess) {
            P.rc = STORMCK_EHIP;
            P.err = "hipSetDevice failed";
            return;
        }
        const uint64_t cnt = P.hi - P.lo;
        P.rc = host_pipeline(b8 + P.lo * stride, stride, lens ? lens + P.lo : nullptr, len, cnt,
                             out ? out + P.lo : nullptr, expected ? expected + P.lo : nullptr, &P.fb, &P.nb);
        if (P.rc) P.err = g_last_error;  // this worker thread's message
    };
    int prev = 0;  // the calling thread runs range 0 and then gets its own device back
    HIP_TRY(hipGetDevice(&prev));
    std::vector<std::thread> threads;
    threads.reserve(parts - 1);
    uint64_t spawned = 1;
    try {
        for (; spawned < parts; ++spawned) threads.emplace_back(work, spawned);
    } catch (const std::system_error&) {
        // no more threads: the calling thread runs the ranges that have none
    }
    for (uint64_t k = 0; k < parts; ++k)
        if (k == 0 || k >= spawned) work(k);
    (void)hipSetDevice(prev);
    for (std::thread& t : threads) t.join();
    uint64_t fb = n, nb = 0;
    for (uint64_t k = 0; k < parts; ++k) {
        const Part& P = part[k];
        if (P.rc) return fail(P.rc, "device " + std::to_string(devices[k]) + " (blocks " + std::to_string(P.lo) +
                                        ".." + std::to_string(P.hi) + "): " + P.err);
        if (expected && P.nb) {
            nb += P.nb;
            fb = std::min(fb, P.lo + P.fb);
        }
    }
    if (first_bad) *first_bad = fb;
    if (n_bad) *n_bad = nb;
    return STORMCK_OK;
}

#include "multi_root.h"
#include "scrub.h"
#include "trace.h"

}  // namespace

// ============================================================================
extern "C" {

int stormck_abi_version(void) { return STORMCK_ABI_VERSION; }

#ifndef STORMCK_SRC_SHA
#define STORMCK_SRC_SHA "unknown"
#endif
const char* stormck_build_id(void) { return "sha256:" STORMCK_SRC_SHA; }

const char* stormck_last_error(void) { return g_last_error.c_str(); }

int stormck_device_count(int* count) {
    if (!count) return fail(STORMCK_EINVAL, "count is null");
    *count = 0;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        (void)hipGetLastError();
        return STORMCK_OK;
    }
    int n = 0;
    for (int d = 0; d < c; ++d) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++n;
    }
    *count = n;
    return STORMCK_OK;
}

int stormck_init(int device) {
    int rc = device_check();
    if (rc) return rc;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(STORMCK_EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    DeviceCtx* c = nullptr;
    rc = get_ctx(&c);  // host-path staging is allocated on first host call
    if (rc) return rc;
    return fault_table_ready(device);  // the ring kernels' fault slots, before any capture can start
}

int stormck_device_status(void* stream) {
    int rc = device_check();
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "stream is being captured: check its status after launching the graph");
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return take_fault(dev, static_cast<hipStream_t>(stream));
}

int stormck_device_alloc(uint64_t bytes, void** d_ptr) {
    if (!d_ptr) return fail(STORMCK_EINVAL, "d_ptr is null");
    *d_ptr = nullptr;
    if (bytes == 0) return fail(STORMCK_EINVAL, "bytes is 0");
    int rc = device_check();
    if (rc) return rc;
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return STORMCK_OK;
}

#ifdef STORMCK_PROBES
// Probe build only (not in include/stormck.h): the arena placement modes measured and
// rejected in round 4 (mode 0 hipMalloc, 2 hipDeviceMallocContiguous). Mode 1, a VMM
// reservation backed by hipMemCreate chunks, was deleted in round 6: no better placement,
// and twice it read wrong blocks.
int stormck_device_alloc_placed(uint64_t bytes, uint32_t mode, uint64_t chunk_bytes, void** d_ptr,
                                uint64_t* mapped_chunk) {
    (void)chunk_bytes;
    if (!d_ptr) return fail(STORMCK_EINVAL, "d_ptr is null");
    *d_ptr = nullptr;
    if (mapped_chunk) *mapped_chunk = 0;
    if (bytes == 0) return fail(STORMCK_EINVAL, "bytes is 0");
    if (mode != 0 && mode != 2) return fail(STORMCK_EINVAL, "unknown allocation mode (0 hipMalloc, 2 contiguous)");
    int rc = device_check();
    if (rc) return rc;
    if (mode == 0) HIP_TRY(hipMalloc(d_ptr, bytes));
    else HIP_TRY(hipExtMallocWithFlags(d_ptr, bytes, hipDeviceMallocContiguous));
    return STORMCK_OK;
}
#endif

int stormck_device_free(void* d_ptr) {
    if (!d_ptr) return STORMCK_OK;
    int rc = device_check();
    if (rc) return rc;
    HIP_TRY(hipFree(d_ptr));
    return STORMCK_OK;
}

int stormck_stream_forget(void* stream) {
    int rc = device_check();
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(STORMCK_EINVAL, "device index beyond 64");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(st));  // no ring kernel of this stream may write the slot later
    FaultTable& t = g_faults[dev];
    uint32_t code = 0;
    {
        std::lock_guard<std::mutex> g(t.mu);
        const int s = t.find(st);
        if (s < 0 || !t.words) return STORMCK_OK;
        code = __atomic_exchange_n(t.words + s, 0u, __ATOMIC_ACQ_REL);
        t.owner[s] = nullptr;
        t.last_launch[s] = 0;  // free for the next stream
        for (size_t k = 0; k < t.index.size(); ++k)
            if (t.index[k].second == static_cast<uint32_t>(s)) {
                t.index[k] = t.index.back();
                t.index.pop_back();
                break;
            }
    }
    if (code == 0) return STORMCK_OK;
    return fail(STORMCK_EHIP, "device " + std::to_string(dev) + ": " + fault_text(code));
}

void stormck_shutdown(void) {
    multi_release();
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (auto& c : g_ctx) {
        if (c) {
            std::lock_guard<std::mutex> g2(c->mu);
            release_ctx(c.get());
        }
    }
}

int stormck_checksum_device(const void* d_base, uint64_t stride, const uint32_t* d_lens, uint32_t len, uint64_t n,
                            uint64_t* d_out, void* stream) {
    if (n == 0) return STORMCK_OK;
    if (!d_base || !d_out) return fail(STORMCK_EINVAL, "null device pointer");
    if (!d_lens && n > 1 && stride < len) return fail(STORMCK_EINVAL, "stride smaller than len (blocks overlap)");
    int rc = device_check();
    if (rc) return rc;
    return launch_checksum(static_cast<const uint8_t*>(d_base), stride, d_lens, len, nullptr, n, d_out, nullptr,
                           nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int stormck_checksum_gather_device(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                                   uint32_t len, uint64_t n, uint64_t* d_out, void* stream) {
    if (n == 0) return STORMCK_OK;
    if (!d_base || !d_offsets || !d_out) return fail(STORMCK_EINVAL, "null device pointer");
    int rc = device_check();
    if (rc) return rc;
    return launch_checksum(static_cast<const uint8_t*>(d_base), 0, d_lens, len, d_offsets, n, d_out, nullptr,
                           nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int stormck_verify_device(const void* d_base, uint64_t stride, const uint32_t* d_lens, uint32_t len, uint64_t n,
                          const uint64_t* d_expected, uint64_t* d_result, void* stream) {
    if (!d_result) return fail(STORMCK_EINVAL, "d_result is null");
    if (n > 0 && (!d_base || !d_expected)) return fail(STORMCK_EINVAL, "null device pointer");
    if (!d_lens && n > 1 && stride < len) return fail(STORMCK_EINVAL, "stride smaller than len (blocks overlap)");
    int rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // d_result = {n, 0}: "no mismatch" until a block lowers it.
    hipLaunchKernelGGL(k_init_result, dim3(1), dim3(64), 0, st, d_result, n);
    HIP_TRY(hipGetLastError());
    if (n == 0) return STORMCK_OK;
    return launch_checksum(static_cast<const uint8_t*>(d_base), stride, d_lens, len, nullptr, n, nullptr, d_expected,
                           reinterpret_cast<unsigned long long*>(d_result),
                           reinterpret_cast<unsigned long long*>(d_result + 1), st);
}

int stormck_checksum_host(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                          uint64_t* out) {
    return host_pipeline(base, stride, lens, len, n, out, nullptr, nullptr, nullptr);
}

int stormck_verify_host(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                        const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad) {
    if (!expected || !first_bad || !n_bad) return fail(STORMCK_EINVAL, "null argument");
    return verify_status(host_pipeline(base, stride, lens, len, n, nullptr, expected, first_bad, n_bad), n_bad);
}

int stormck_checksum_host_multi(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                                uint64_t* out, const int* devices, int n_devices) {
    if (n > 0 && !out) return fail(STORMCK_EINVAL, "out is null");
    return host_pipeline_multi(base, stride, lens, len, n, out, nullptr, nullptr, nullptr, devices, n_devices);
}

int stormck_verify_host_multi(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                              const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, const int* devices,
                              int n_devices) {
    if (!expected || !first_bad || !n_bad) return fail(STORMCK_EINVAL, "null argument");
    return verify_status(
        host_pipeline_multi(base, stride, lens, len, n, nullptr, expected, first_bad, n_bad, devices, n_devices), n_bad);
}

uint64_t stormck_xxh64(const void* p, uint64_t n_bytes) {
    static const uint8_t empty = 0;
    return host::xxh64(n_bytes ? p : &empty, n_bytes);
}

int stormck_checksum(const void* p, uint64_t n_bytes, uint64_t* out) {
    if (!out) return fail(STORMCK_EINVAL, "out is null");
    if (n_bytes > 0 && !p) return fail(STORMCK_EINVAL, "p is null");
    // Latency dispatch of a single call. One buffer is four serial chains, so the GPU
    // brings no parallelism to it: measured on MI355X, the device single call
    // (stormck_checksum_gpu) is slower than one host core at every length, 72 B to
    // 256 MiB (DESIGN_LOG.md §5, "Single calls"). The crossover is therefore "never";
    // STORMCK_SINGLE_GPU_MIN=<bytes> sends single calls of at least that many bytes to
    // the device (A/B measurement only).
    if (n_bytes >= knobs().single_gpu_min) return stormck_checksum_gpu(p, n_bytes, out);
    *out = stormck_xxh64(p, n_bytes);
    return STORMCK_OK;
}

int stormck_checksum_gpu(const void* p, uint64_t n_bytes, uint64_t* out) {
    if (!out) return fail(STORMCK_EINVAL, "out is null");
    static const uint8_t empty = 0;
    if (n_bytes == 0) p = &empty;  // XXH64 of an empty slice: nothing is read
    if (!p) return fail(STORMCK_EINVAL, "p is null");
    if (n_bytes > kChunkBytes)
        return fail(STORMCK_EINVAL, "single device call longer than the 256 MiB staging chunk "
                                    "(stormck_checksum hashes any length)");
    if (n_bytes > kSingleMax)
        return host_pipeline(p, 0, nullptr, static_cast<uint32_t>(n_bytes), 1, out, nullptr, nullptr, nullptr);
    // latency path: memcpy into pinned staging, one kernel that reads it over PCIe and
    // writes the checksum into pinned memory, one sync
    DeviceCtx* c = nullptr;
    int rc = get_ctx(&c);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    rc = ensure_ready(c);
    if (rc) return rc;
    Stage& s = c->st[0];
    std::memcpy(s.pinned, p, n_bytes);
    hipLaunchKernelGGL(k_xxh64_single, dim3(1), dim3(256), 0, s.stream, s.pinned, static_cast<uint32_t>(n_bytes),
                       s.h_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s.stream));
    *out = s.h_out[0];
    return STORMCK_OK;
}

int stormck_host_register(void* p, uint64_t bytes) {
    if (!p || bytes == 0) return fail(STORMCK_EINVAL, "empty range");
    int rc = device_check();
    if (rc) return rc;
    // portable: pinned for every device of the process (stormck_checksum_host_multi DMAs
    // ranges of one registered buffer to several devices)
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    reg_add(p, bytes);
    // registered memory is what the device and split legs read: set up the current device's
    // stages now (pinned and device buffers, ~0.3 s once per process) rather than inside the
    // first routed call that splits (storm registers cache.data once, at start-up). Best
    // effort: a failure here is the first device call's to report.
    const std::string before = g_last_error;  // a best-effort failure is not this call's error
    DeviceCtx* c = nullptr;
    if (get_ctx(&c) == STORMCK_OK) {
        std::lock_guard<std::mutex> g(c->mu);
        (void)ensure_ready(c);
    }
    g_last_error = before;
    return STORMCK_OK;
}

int stormck_host_device_pointer(void* p, void** d_p) {
    if (!p || !d_p) return fail(STORMCK_EINVAL, "null pointer");
    int rc = device_check();
    if (rc) return rc;
    HIP_TRY(hipHostGetDevicePointer(d_p, p, 0));
    return STORMCK_OK;
}

int stormck_host_unregister(void* p) {
    int rc = device_check();
    if (rc) return rc;
    reg_remove(p);
    HIP_TRY(hipHostUnregister(p));
    return STORMCK_OK;
}

int stormck_pointer_level_device(const uint64_t* d_child_cs, uint64_t m, uint64_t child_addr_base, uint64_t rev,
                                 uint8_t child_type, uint32_t fanout, uint64_t* d_parent_cs, void* stream) {
    if (m == 0) return STORMCK_OK;
    if (!d_child_cs || !d_parent_cs) return fail(STORMCK_EINVAL, "null device pointer");
    if (fanout == 0 || fanout > kMaxFanout) return fail(STORMCK_EINVAL, "fanout out of range");
    int rc = device_check();
    if (rc) return rc;
    const Plan p = plan_pointer_level((m + fanout - 1) / fanout, fanout, cu_count(), knobs());
    const dim3 grid(p.grid), block(p.block);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (p.kernel) {
        case Kernel::TooLarge:
            return fail(STORMCK_EINVAL, "level too large");
        case Kernel::Wide:
            hipLaunchKernelGGL(k_pointer_level_wide, grid, block, 0, st, d_child_cs, m, child_addr_base, rev, child_type,
                               fanout, d_parent_cs);
            break;
        case Kernel::PointerPc:  // 2 or 4 chain waves per workgroup: probe build (rejected)
            with_int<1, 2, 4>(p.waves, [&](auto C) {
                with_consts([&](auto SR) {
                    if constexpr (STORMCK_V(C) == 1 ? !STORMCK_V(SR) : kProbes)
                        hipLaunchKernelGGL((k_pointer_level_pc<STORMCK_POINTERS_PER_BLOCK, kRingTile, kRingPrefetch, STORMCK_V(C),
                                                               STORMCK_V(SR)>),
                                           grid, block, 0, st, d_child_cs, m, child_addr_base, rev, child_type, d_parent_cs);
                }, p.simd_roles);
            });
            break;
        default:  // Kernel::Quad
            hipLaunchKernelGGL(k_pointer_level, grid, block, 0, st, d_child_cs, m, child_addr_base, rev, child_type, fanout,
                               d_parent_cs);
    }
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}


int stormck_pointer_node_device(const stormck_pointer* d_entries, const uint8_t* d_types, uint32_t count,
                                uint32_t fanout, uint64_t* d_out_cs, void* stream) {
    if (!d_out_cs || (count > 0 && (!d_entries || !d_types))) return fail(STORMCK_EINVAL, "null device pointer");
    if (fanout == 0 || fanout > kMaxFanout || count > fanout) return fail(STORMCK_EINVAL, "count/fanout out of range");
    int rc = device_check();
    if (rc) return rc;
    static_assert(sizeof(stormck_pointer) == 24, "Pointer is 24 bytes");
    hipLaunchKernelGGL(k_pointer_node, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint64_t*>(d_entries), d_types, count, fanout, d_out_cs);
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

int stormck_pack_pointer_blocks_device(const uint64_t* d_child_cs, uint64_t m, uint64_t child_addr_base, uint64_t rev,
                                       uint8_t child_type, uint32_t fanout, void* d_blocks, uint64_t dst_stride,
                                       void* stream) {
    if (m == 0) return STORMCK_OK;
    if (!d_child_cs || !d_blocks) return fail(STORMCK_EINVAL, "null device pointer");
    if (fanout == 0 || fanout > kMaxFanout) return fail(STORMCK_EINVAL, "fanout out of range");
    if (dst_stride < pointer_block_size(fanout) || (dst_stride & 7) || (reinterpret_cast<uintptr_t>(d_blocks) & 7))
        return fail(STORMCK_EINVAL, "dst_stride/d_blocks must be 8-byte aligned and hold a pointer block");
    int rc = device_check();
    if (rc) return rc;
    hipLaunchKernelGGL(k_pack_pointer_blocks, dim3(2048), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       d_child_cs, m, child_addr_base, rev, child_type, fanout, static_cast<uint8_t*>(d_blocks),
                       dst_stride);
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

uint64_t stormck_merkle_workspace_bytes(uint64_t n, uint32_t fanout) {
    if (fanout < 2) return 0;
    uint64_t total = 0;
    for (uint64_t m = n; m > 1;) {
        m = (m + fanout - 1) / fanout;
        total += m;
    }
    return total * 8;
}

int stormck_merkle_root_device(const uint64_t* d_leaf_cs, uint64_t n, uint64_t leaf_addr_base,
                               uint64_t node_addr_base, uint64_t rev, uint32_t fanout, void* d_workspace,
                               uint64_t workspace_bytes, stormck_pointer* d_root, uint8_t* d_root_type,
                               void* stream) {
    if (!d_root || !d_root_type) return fail(STORMCK_EINVAL, "null root pointer");
    if (fanout < 2 || fanout > kMaxFanout) return fail(STORMCK_EINVAL, "fanout out of range");
    if (n > 0 && !d_leaf_cs) return fail(STORMCK_EINVAL, "d_leaf_cs is null");
    if (n > 0 && (workspace_bytes < stormck_merkle_workspace_bytes(n, fanout) || (n > 1 && !d_workspace)))
        return fail(STORMCK_EINVAL, "workspace too small (stormck_merkle_workspace_bytes)");
    int rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* root = reinterpret_cast<uint64_t*>(d_root);
    if (n == 0) {
        hipLaunchKernelGGL(k_set_root, dim3(1), dim3(64), 0, st, nullptr, 0ULL, 0ULL, static_cast<uint8_t>(STORMCK_FREE_BLOCK),
                           root, d_root_type);
        HIP_TRY(hipGetLastError());
        return STORMCK_OK;
    }
    const uint64_t* cur = d_leaf_cs;
    uint64_t m = n, addr_base = leaf_addr_base, next_addr = node_addr_base;
    uint8_t type = STORMCK_LEAF_BLOCK;
    uint64_t* ws = static_cast<uint64_t*>(d_workspace);
    while (m > 1) {
        const uint64_t pm = (m + fanout - 1) / fanout;
        rc = stormck_pointer_level_device(cur, m, addr_base, rev, type, fanout, ws, st);
        if (rc) return rc;
        cur = ws;
        ws += pm;
        addr_base = next_addr;
        next_addr += pm;
        m = pm;
        type = STORMCK_POINTER_BLOCK;
    }
    hipLaunchKernelGGL(k_set_root, dim3(1), dim3(64), 0, st, cur, addr_base, rev, type, root, d_root_type);
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

int stormck_shard_plan(uint64_t n_total, uint32_t n_shards, const int* devices, int n_devices, stormck_shard* shards,
                       uint64_t* root_addr) {
    return shard_plan(n_total, n_shards, devices, n_devices, shards, root_addr);
}

int stormck_merkle_root_multi(const stormck_shard* shards, uint32_t n_shards, uint64_t rev, uint64_t root_addr,
                              uint32_t fanout, stormck_pointer* root, uint8_t* root_type, stormck_pointer* shard_roots,
                              uint8_t* shard_types) {
    return merkle_root_multi(shards, n_shards, rev, root_addr, fanout, root, root_type, shard_roots, shard_types);
}

int stormck_multi_layout(const stormck_shard* shards, uint32_t n_shards, int32_t* devices, uint32_t* n_devices,
                         uint32_t* rows, uint32_t* table_row) {
    if (!shards || n_shards == 0) return fail(STORMCK_EINVAL, "shards: at least one");
    if (!devices || !n_devices || !rows || !table_row) return fail(STORMCK_EINVAL, "null argument");
    MultiLayout lay;
    const int rc = multi_layout(shards, n_shards, &lay);
    if (rc) return rc;
    for (size_t d = 0; d < lay.devs.size(); ++d) devices[d] = lay.devs[d];
    *n_devices = static_cast<uint32_t>(lay.devs.size());
    *rows = static_cast<uint32_t>(lay.R);
    for (uint32_t s = 0; s < n_shards; ++s) table_row[s] = lay.map[s];
    return STORMCK_OK;
}

int stormck_read_verify_fd(int fd, const uint64_t* addresses, const uint32_t* lens, uint64_t n, uint64_t block_size,
                           void* dst, uint64_t dst_stride, const uint64_t* expected, uint32_t flags,
                           uint64_t* first_bad, uint64_t* n_bad) {
    if (!first_bad || !n_bad) return fail(STORMCK_EINVAL, "null result pointer");
    *first_bad = n;
    *n_bad = 0;
    if (n == 0) return STORMCK_OK;
    if (fd < 0 || !addresses || !lens || !dst || !expected) return fail(STORMCK_EINVAL, "null argument");
    if (block_size == 0) return fail(STORMCK_EINVAL, "block_size is 0");
    // An O_DIRECT descriptor (pkg/filedev's device file opened to bypass the page cache,
    // the reference's TODO at persistence/init.go:54 / cache/cache.go:82) only takes
    // whole, aligned blocks: reads cover block_size bytes into 512-byte aligned slots.
    const int fl = fcntl(fd, F_GETFL);
    if (fl < 0) return fail(STORMCK_EINVAL, std::string("fcntl(F_GETFL): ") + std::strerror(errno));
    const bool direct = (fl & O_DIRECT) != 0;
    const bool full = direct || (flags & STORMCK_READ_FULL_BLOCK) != 0;
    if (direct && ((reinterpret_cast<uintptr_t>(dst) | dst_stride | block_size) & 511))
        return fail(STORMCK_EINVAL, "O_DIRECT descriptor: dst, dst_stride and block_size must be 512-byte aligned");
    const uint64_t max_addr = (static_cast<uint64_t>(INT64_MAX) - block_size) / block_size;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t want = full ? block_size : lens[i];
        if (lens[i] > block_size || want > dst_stride) return fail(STORMCK_EINVAL, "block does not fit its slot");
        if (addresses[i] > max_addr)
            return fail(STORMCK_EINVAL, "address " + std::to_string(addresses[i]) + " of block index " +
                                            std::to_string(i) + " is beyond any file offset");
    }
    int rc = device_check();
    if (rc) return rc;
    // Reads (Store.ReadBlock: Seek(address*BlockSize) + Read) run on a pool of reader
    // threads that take pieces of the batch in index order from one shared counter, so
    // the pool streams across super-chunk boundaries without joining; the GPU verifies
    // each 1 GiB super-chunk as soon as its last piece has landed. Runs of consecutive
    // addresses whose slots are contiguous (full blocks, dst_stride == block_size) are
    // read with one pread of up to kRunBytes. An O_DIRECT descriptor reaches the device,
    // whose rate needs queue depth: 32 reader threads instead of 16 (STORMCK_READ_THREADS
    // overrides; on the test boxes' overlay filesystem, counts from 8 to 64 measured the
    // same within its run-to-run noise, DESIGN_LOG.md §11 f2/f3).
    constexpr uint64_t kRunBytes = 1ULL << 20;
    const uint64_t max_run = full && dst_stride == block_size ? std::max<uint64_t>(1, kRunBytes / block_size) : 1;
    unsigned nt = direct ? 32u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = std::getenv("STORMCK_READ_THREADS")) nt = std::max(1, std::atoi(e));
    uint64_t super_bytes = 1ULL << 30;  // STORMCK_READ_SUPER_BYTES: smaller super-chunks, for tests
    if (const char* e = std::getenv("STORMCK_READ_SUPER_BYTES")) super_bytes = std::max(1LL, std::atoll(e));
    const uint64_t per_super = std::max<uint64_t>(1, super_bytes / std::max<uint64_t>(dst_stride, 1));
    const uint64_t nsuper = (n + per_super - 1) / per_super;
    const uint64_t piece = std::max<uint64_t>(max_run, 16);  // blocks per work item
    const uint64_t pps = (per_super + piece - 1) / piece;     // pieces per full super-chunk
    auto pieces_in = [&](uint64_t sc) {
        const uint64_t lo = sc * per_super, hi = std::min(n, lo + per_super);
        return (hi - lo + piece - 1) / piece;
    };
    const uint64_t npieces = (nsuper - 1) * pps + pieces_in(nsuper - 1);
    std::unique_ptr<std::atomic<uint64_t>[]> landed(new std::atomic<uint64_t>[nsuper]);
    for (uint64_t sc = 0; sc < nsuper; ++sc) landed[sc].store(0);
    std::atomic<uint64_t> next{0};
    std::atomic<int> err{0}, err_no{0};
    std::atomic<uint64_t> bad_index{n};
    std::atomic<bool> stop{false};
    std::mutex mu;
    std::condition_variable cv;
    auto note_bad = [&](uint64_t idx) {  // the lowest failing index wins
        uint64_t cur = bad_index.load();
        while (idx < cur && !bad_index.compare_exchange_weak(cur, idx)) {
        }
    };
    auto read_range = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi;) {
            uint64_t k = i + 1;
            while (k < hi && k - i < max_run && addresses[k] == addresses[k - 1] + 1) ++k;
            uint8_t* d = static_cast<uint8_t*>(dst) + i * dst_stride;
            const uint64_t want = full ? (k - i) * block_size : lens[i];
            const uint64_t off = addresses[i] * block_size;
            uint64_t got = 0;
            while (got < want) {
                const ssize_t r = pread(fd, d + got, want - got, static_cast<off_t>(off + got));
                if (r <= 0) {
                    if (r < 0) err_no.store(errno);
                    err.store(r < 0 ? 1 : 2);
                    note_bad(i + (full ? got / block_size : 0));
                    return false;
                }
                got += static_cast<uint64_t>(r);
            }
            i = k;
        }
        return true;
    };
    auto reader = [&] {
        while (!stop.load(std::memory_order_relaxed) && !err.load(std::memory_order_relaxed)) {
            const uint64_t p = next.fetch_add(1);
            if (p >= npieces) return;
            const uint64_t sc = p / pps, lo = sc * per_super + (p % pps) * piece;
            const uint64_t hi = std::min({n, (sc + 1) * per_super, lo + piece});
            const bool ok = read_range(lo, hi);
            if (!ok || landed[sc].fetch_add(1) + 1 == pieces_in(sc)) {
                std::lock_guard<std::mutex> g(mu);  // pairs with the verifier's predicate check
                cv.notify_all();
            }
            if (!ok) return;
        }
    };
    // STORMCK_DEBUG_READER_LIMIT=k: thread creation "fails" after k readers (tests)
    static const long reader_limit = [] {
        const char* e = std::getenv("STORMCK_DEBUG_READER_LIMIT");
        return e ? std::atol(e) : -1L;
    }();
    std::vector<std::thread> pool;
    try {
        pool.reserve(static_cast<size_t>(std::min<uint64_t>(nt, npieces)));
        for (unsigned t = 0; t < std::min<uint64_t>(nt, npieces); ++t) {
            if (reader_limit >= 0 && static_cast<long>(t) >= reader_limit)
                throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            pool.emplace_back(reader);
        }
    } catch (const std::exception&) {
        // no more threads (std::system_error) or no memory for the vector: carry on with
        // the readers already started; with none, this thread reads everything first
        if (pool.empty()) reader();
    }
    rc = STORMCK_OK;
    for (uint64_t sc = 0; sc < nsuper; ++sc) {
        {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return landed[sc].load() == pieces_in(sc) || err.load(); });
        }
        if (err.load()) break;
        const uint64_t lo = sc * per_super, hi = std::min(n, lo + per_super);
        uint64_t fb = 0, nb = 0;
        rc = host_pipeline(static_cast<uint8_t*>(dst) + lo * dst_stride, dst_stride, lens + lo, 0, hi - lo, nullptr,
                           expected + lo, &fb, &nb);
        if (rc) break;
        if (nb) {
            *n_bad += nb;
            *first_bad = std::min<uint64_t>(*first_bad, lo + fb);
        }
    }
    stop.store(true);
    for (auto& t : pool) t.join();
    if (err.load()) {
        const std::string what = err.load() == 1 ? std::string("pread failed (") + std::strerror(err_no.load()) + ")"
                                                 : std::string("short read (block beyond end of device)");
        return fail(STORMCK_EINVAL, what + " at block index " + std::to_string(bad_index.load()));
    }
    return verify_status(rc, n_bad);
}

int stormck_key_tags_device(const void* d_keys, uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens,
                            uint32_t len, uint64_t n, uint64_t* d_out, void* stream) {
    if (n == 0) return STORMCK_OK;
    if (!d_keys || !d_out) return fail(STORMCK_EINVAL, "null device pointer");
    int rc = device_check();
    if (rc) return rc;
    const uint8_t* k = static_cast<const uint8_t*>(d_keys);
    const KeyTagsPlan p = plan_key_tags(stride, len, n, d_offsets != nullptr, d_lens != nullptr,
                                        static_cast<unsigned>(reinterpret_cast<uintptr_t>(k) & 15));
    if (p.too_large) return fail(STORMCK_EINVAL, "batch too large for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.batches > 0) {
        // tags leave by non-temporal stores: the 8 B-per-key write stream costs the
        // read stream about a quarter of the rate, nt stores recover ~3 %
        // (tools/probe_keys.hip, profiles/r02_keys/)
        constexpr int kKeyStore = 1;
        if (p.pieces <= 4)
            with_int<1, 2, 3, 4>(p.pieces, [&](auto P) {
                with_consts([&](auto FIXED) {
                    hipLaunchKernelGGL((k_key_tags_ring<kAuxNT, STORMCK_V(P), kKeyRing, kKeysPerWave,
                                                        STORMCK_V(FIXED) ? 16 * STORMCK_V(P) : 0, kKeyStore>),
                                       dim3(p.grid), dim3(kThreads), p.lds, st, k, len, p.batches, d_out);
                }, p.fixed_len);
            });
        else
            hipLaunchKernelGGL(k_key_tags_lds<kAuxNT>, dim3(p.grid), dim3(kThreads), p.lds, st, k,
                               static_cast<uint32_t>(stride), len, p.batches, kKeysPerWave, d_out);
        HIP_TRY(hipGetLastError());
        if (p.tail == 0) return STORMCK_OK;
        k += p.batches * 64 * stride;
        d_out += p.batches * 64;
    }
    with_consts([&](auto OFFS, auto LENS) {
        hipLaunchKernelGGL((k_key_tags<STORMCK_V(OFFS), STORMCK_V(LENS)>), dim3(p.tail_grid), dim3(kThreads), 0, st, k, stride,
                           d_offsets, d_lens, len, p.tail, d_out);
    }, d_offsets != nullptr, d_lens != nullptr);
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}


}  // extern "C" (the commit's legs and the routing engine below are internal C++)

namespace {

// commit_plan.h's executor on the pool: fn(t, lo, hi) over contiguous ranges of [0, count)
// on min(cap, pool, count / grain + 1) threads.
struct PoolPar {
    unsigned cap;
    uint64_t grain;
    template <class F>
    unsigned operator()(uint64_t count, F&& fn) const {
        if (cap <= 1 || count < grain) {  // storm's small commits: no pool, not even its lock
            fn(0u, uint64_t{0}, count);
            return 1;
        }
        ForkJoin& fj = ForkJoin::get();
        const unsigned nt = static_cast<unsigned>(std::min<uint64_t>({cap, kMaxParts, fj.size(), count / grain + 1}));
        fj.run(nt, [&](unsigned t) { fn(t, count * t / nt, count * (t + 1) / nt); });
        return nt;
    }
};
// The planning passes (heights, the order) and the record staging, on at most `threads`
// pool threads (0 = the pool).
PoolPar plan_par(uint32_t threads = 0) { return {threads ? threads : kMaxParts, 16384}; }  // the pool has at most 16
PoolPar stage_par(uint32_t threads = 0) { return {threads ? std::min(threads, 8u) : 8u, 8192}; }

// Validation and heights of a commit, the same for every leg; nothing is changed.
int commit_forest(const stormck_dirty_block* blocks, uint64_t n, uint64_t revision, uint32_t threads, Heights* H) {
    const CommitError e = commit_heights(blocks, n, revision, plan_par(threads), H);
    if (e == CommitError::Ok) return STORMCK_OK;
    return fail(e == CommitError::NoMem ? STORMCK_ENOMEM : STORMCK_EINVAL, commit_error_message(e));
}

// The device leg of a planned commit: the level kernels read and write d_arena in place.
int commit_device_run(void* d_arena, stormck_dirty_block* blocks, const Heights& H, uint64_t revision,
                      uint64_t* last_allocated_block, uint64_t* out_checksums, void* stream, PhaseTimer& pt) {
    ForkJoin& fj = ForkJoin::get();
    const uint64_t n = H.n, nu = H.n_upper, n0 = H.n0();
    // the LDS-DMA level kernels need 16-byte aligned rows, and pay only when blocks are
    // longer than a few of their 512-byte rows (as launch_checksum's kVarMinLen)
    const bool glds_levels =
        (reinterpret_cast<uintptr_t>(d_arena) & 15) == 0 && !H.data_off16 && H.longest > knobs().var_min_len;

    // device resources before the records are touched: a failure here leaves them as given
    DeviceCtx* c = nullptr;
    int rc = get_ctx(&c);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    rc = ensure_ready(c);
    if (rc) return rc;
    if (c->commit_n < n) {
        if (c->commit_rec) (void)hipHostFree(c->commit_rec);
        if (c->commit_cs) (void)hipHostFree(c->commit_cs);
        c->commit_rec = nullptr;
        c->commit_cs = nullptr;
        c->commit_n = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->commit_rec), n * sizeof(stormck_dirty_block),
                              hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->commit_cs), n * 8, hipHostMallocCoherent));
        c->commit_n = n;
    }
    stormck_dirty_block* d_blocks = nullptr;
    uint64_t* d_cs = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_blocks), c->commit_rec, 0));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_cs), c->commit_cs, 0));
    pt.mark("ctx");

    // Commit order: level 0 in index order, then the upper levels by height (index order
    // within a height). `order` (commit position -> caller's index) is materialised only
    // when it is not the identity. Level 0's part is all the first launch needs; the
    // upper part is built while level 0 hashes.
    CommitOrder O;
    if (!H.prefix0()) {
        order_level0(H, plan_par(), &O);
        pt.mark("order0");
    }
    const std::vector<uint32_t>& order = O.order;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const Knobs kn = commit_knobs();
    const uint64_t ncu = cu_count();
    uint8_t* arena = static_cast<uint8_t*>(d_arena);
    auto launch_level = [&](uint64_t lo, uint64_t cnt) -> int {
        const Plan p = plan_commit_level(cnt, ncu, glds_levels, kn);
        const dim3 grid(p.grid), block(p.block);
        switch (p.kernel) {
            case Kernel::TooLarge:
                return fail(STORMCK_EINVAL, "level too large");
            case Kernel::Glds:
                with_int<1, 3, kGldsWaves>(p.waves, [&](auto W) {
                    hipLaunchKernelGGL((k_commit_level_glds<kTileStripes, kAuxNT, STORMCK_V(W)>), grid, block, 0, st, arena,
                                       d_blocks, lo, cnt, d_cs);
                });
                break;
            case Kernel::Wide:
                hipLaunchKernelGGL(k_commit_level_wide, grid, block, 0, st, arena, d_blocks, lo, d_cs);
                break;
            case Kernel::WideMulti: {
                const int mrc = launch_wide_multi(p.multi, st, [&](auto BPW, auto RING, auto CHUNK, auto DBL, uint32_t* fault,
                                                                   uint32_t stall) {
                    hipLaunchKernelGGL((k_commit_level_multi<STORMCK_V(BPW), STORMCK_V(RING), STORMCK_V(CHUNK), STORMCK_V(DBL)>),
                                       grid, block, 0, st, arena, d_blocks, lo, cnt, d_cs, fault, stall);
                });
                if (mrc) return mrc;
                break;
            }
            default:  // Kernel::Quad
                hipLaunchKernelGGL(k_commit_level<kU>, grid, block, 0, st, arena, d_blocks, lo, cnt, d_cs);
        }
        HIP_TRY(hipGetLastError());
        return STORMCK_OK;
    };
    // Records are copied in commit order into the context's coherent pinned buffer,
    // which the level kernels read over PCIe (56 B per block beside its ~32 KiB of HBM
    // reads; no DMA command, so nothing queues behind or between the hashing launches).
    // Relocation (cache/cache.go:114-118: the k-th relocating block in commit order gets
    // address last + k) is applied to the caller's record as it is copied. Each launch
    // writes its checksums into pinned memory too; `back` lists the launches, so the
    // host moves a launch's checksums to the caller's order while later ones run.
    uint64_t last = *last_allocated_block;
    auto stage_records = [&](uint64_t a, uint64_t b) {
        stormck_dirty_block* rec = c->commit_rec;
        if (!H.relocating && order.empty()) {
            par_copy(reinterpret_cast<uint8_t*>(rec + a), reinterpret_cast<const uint8_t*>(blocks + a),
                     (b - a) * sizeof(stormck_dirty_block), 1ULL << 20);
            return;
        }
        relocate_range(blocks, O, a, b, revision, H.relocating != 0, &last, stage_par(),
                       [rec](uint64_t k, const stormck_dirty_block& r) { rec[k] = r; });
    };
    struct Back {
        uint64_t lo, cnt;
        hipEvent_t hashed;
    };
    std::vector<Back> back;
    auto send_back = [&](uint64_t lo, uint64_t cnt) -> int {
        back.push_back({lo, cnt, nullptr});
        HIP_TRY(hipEventCreateWithFlags(&back.back().hashed, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(back.back().hashed, st));
        return STORMCK_OK;
    };
    auto run = [&]() -> int {
        // Level 0 in growing chunks: a first chunk of 2 x kStreamBatch blocks (one LDS-DMA
        // workgroup per CU) starts the device after a small upload; each next chunk is 3x
        // the previous, small enough that its records (56 B per block over PCIe) arrive
        // before the previous chunk's blocks (~32 KiB each at HBM rate) are hashed.
        // A small commit (storm's per-revision commit: ~1,200 leaves under one pointer
        // block) returns its checksums in one piece after the last level: an event
        // recorded between two launches holds the second one back by about 4 us
        // (profiles/r02_c5_multi/), more than copying a few thousand checksums costs.
        const bool one_piece = commit_one_piece(nu, n0);
        uint64_t unsent = 0;  // first commit position not yet covered by `back`
        for (uint64_t lo = 0, cnt, next = kn.commit_first; lo < n0; lo += cnt, next = cnt * kn.commit_growth) {
            cnt = level0_chunk(n0 - lo, next);
            stage_records(lo, lo + cnt);
            int e = launch_level(lo, cnt);
            if (e) return e;
            if (!one_piece) {
                e = send_back(lo, cnt);
                if (e) return e;
                unsent = lo + cnt;
            }
        }
        pt.mark("level0_issue");
        if (nu == 0) return STORMCK_OK;
        // Upper levels, planned while level 0 hashes.
        order_upper(H, plan_par(), &O);
        pt.mark("order_upper");
        stage_records(n0, n);
        int e = STORMCK_OK;
        for (uint32_t l = 1; l <= H.max_h; ++l) {
            const uint64_t lo = O.level_start[l], cnt = O.level_start[l + 1] - lo;
            if (cnt == 0) continue;
            e = launch_level(lo, cnt);
            if (e) return e;
        }
        return send_back(unsent, n - unsent);
    };
    rc = run();
    *last_allocated_block = last;  // the relocations applied to the caller's records so far
    if (rc == STORMCK_OK) {
        // checksums to the caller's order, each launch's slice as soon as it is back
        for (const Back& x : back) {
            if (hipEventSynchronize(x.hashed) != hipSuccess) {
                rc = fail(STORMCK_EHIP, "commit: checksum copy-back failed");
                break;
            }
            rc = take_fault(c->device, st);  // a stalled ring level wrote no checksum for some blocks
            if (rc) break;
            const unsigned tn = static_cast<unsigned>(std::min<uint64_t>({8, fj.size(), x.cnt / 65536 + 1}));
            fj.run(tn, [&](unsigned t) {
                const uint64_t lo = x.lo + x.cnt * t / tn, hi = x.lo + x.cnt * (t + 1) / tn;
                if (order.empty()) {
                    std::memcpy(out_checksums + lo, c->commit_cs + lo, (hi - lo) * 8);
                } else {
                    for (uint64_t k = lo; k < hi; ++k) out_checksums[order[k]] = c->commit_cs[k];
                }
            });
        }
    }
    // nothing of this call may still be in flight when it returns (pinned buffers are reused)
    const hipError_t s1 = hipStreamSynchronize(st);
    for (Back& x : back) (void)hipEventDestroy(x.hashed);
    if (rc == STORMCK_OK && s1 != hipSuccess) rc = fail(STORMCK_EHIP, std::string("commit: ") + hipGetErrorString(s1));
    if (rc == STORMCK_OK) rc = take_fault(c->device, st);
    pt.mark("device");
    return rc;
}

}  // namespace

// ---- routing of host-memory work: host, device and split legs ------------------------
// The cost model, the rates, the split queue and the decision of a routed call are
// route_plan.h; here are the facts it decides on and the legs it chooses among. One engine
// runs the host and split legs (split_run; the host leg is a split without devices).
namespace {

// The one model of the process.
RouteModel& route_model() {
    static RouteModel m(host::has_x4());
    return m;
}

double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The devices routed calls may use (stormck_route_devices); empty: the caller's current one.
std::mutex g_route_mu;
std::vector<int> g_route_devs;

int route_devices(std::vector<int>* out) {
    {
        std::lock_guard<std::mutex> g(g_route_mu);
        *out = g_route_devs;
    }
    if (out->empty()) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        out->push_back(dev);
    }
    return STORMCK_OK;
}

// The devices a split may use: the caller's list, each device once, or the route devices.
int split_devices(const int* devices, int n_devices, std::vector<int>* out) {
    return (devices || n_devices) ? check_devices(devices, n_devices, true, out) : route_devices(out);
}

// One persistent host thread per device drives that device's part of a split (a thread per
// call would cost ~30 us to start). A call owns a worker from acquire() to wait(); a balanced
// split whose worker another call owns runs without that device. Calls acquire the workers
// they wait for in ascending device order (split_run), so two fixed-mode calls over the same
// devices listed in different orders cannot each hold one and wait for the other.
class DevWorker {
  public:
    static DevWorker* of(int dev) {
        if (dev < 0 || dev >= 64) return nullptr;
        static std::once_flag once;
        std::call_once(once, [] {
            pthread_atfork(nullptr, nullptr, [] {  // a fork()ed child has none of the threads
                for (auto& w : table_) w = nullptr;
            });
        });
        std::lock_guard<std::mutex> g(make_mu_);
        if (!table_[dev]) table_[dev] = new DevWorker(dev);  // never destroyed: its thread may be parked at exit
        return table_[dev];
    }
    // Take the worker for one call: wait for it, or give up at once if another call owns it.
    bool acquire(bool wait_if_busy) {
        if (wait_if_busy) {
            own_.lock();
            return true;
        }
        return own_.try_lock();
    }
    // Run fn on the acquired worker; wait() joins it and releases the worker.
    void start(std::function<void()> fn) {
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = std::move(fn);
            pending_ = true;
        }
        cv_.notify_all();
    }
    void wait() {
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return !pending_; });
            job_ = nullptr;
        }
        own_.unlock();
    }

  private:
    explicit DevWorker(int dev) : dev_(dev) { std::thread([this] { loop(); }).detach(); }
    void loop() {
        (void)hipSetDevice(dev_);
        (void)hipGetLastError();
        for (;;) {
            std::function<void()> fn;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return pending_ && job_ != nullptr; });
                fn = job_;
            }
            fn();
            {
                std::lock_guard<std::mutex> g(mu_);
                pending_ = false;
            }
            cv_.notify_all();
        }
    }
    static inline DevWorker* table_[64] = {};
    static inline std::mutex make_mu_;
    int dev_;
    std::mutex own_, mu_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool pending_ = false;
};

// XXH64 of blocks [a, b), four chains at once where the CPU has AVX-512: take(i, hash).
template <class Take>
void hash_blocks(const Blocks& B, uint64_t a, uint64_t b, Take&& take) {
    uint64_t i = a;
    for (; host::has_x4() && i + 4 <= b; i += 4) {
        const unsigned char* p4[4];
        size_t n4[4];
        uint64_t h4[4];
        for (int q = 0; q < 4; ++q) {
            p4[q] = B.at(i + q);
            n4[q] = B.len_of(i + q);
        }
        host::xxh64_x4(p4, n4, h4);
        for (int q = 0; q < 4; ++q) take(i + q, h4[q]);
    }
    for (; i < b; ++i) take(i, host::xxh64(B.at(i), B.len_of(i)));
}

struct SplitArgs {
    Blocks B;
    uint32_t plan_len = 0;               // the longest block, which the kernels plan with
    const uint64_t* expected = nullptr;  // verify: compare instead of returning checksums
    Sink* sink = nullptr;                // checksums
    bool in_place = false;               // devices read B.base in place (mapped memory), not by DMA copies
    double bytes_per_block = 1.0;        // set by split_run
};

struct DevRun {
    int rc = STORMCK_OK;
    std::string err;
    uint64_t blocks = 0, bytes = 0, first_bad = UINT64_MAX, n_bad = 0;
    double busy_us = 0;
    double started = 0, first_issue = 0;  // when the worker began, issued its first chunk (now_us clock)
    double first_done = 0;                // when its first chunk came back (0: none)
    bool cold = false;                    // the device's staging was set up in this call
    double finished = 0;
    uint64_t first_bytes = 0;             // that chunk's bytes
};

// One device's part of a split, on its worker thread (the current device is its own):
// chunks claimed from the back of the queue through the device context's two stages (the
// stage engine, waiting without spinning: Wait::kBlock), and the timing the route model learns from.
// In-place mode (mapped memory: registered, as the Go binding's cache.data) lets the kernels
// read the chunk's blocks over the link where they are, strided or at the offsets of a
// commit's scattered blocks, and needs no copy engine: a chunk is one launch and one small
// copy back, so the first one returns soonest. DMA mode (page-locked memory the device cannot
// map) copies the chunk's rows into HBM first, as the host pipeline's stages do.
void device_part(const SplitArgs& A, SplitQueue& q, double lat_us, DevRun* r) {
    auto failed = [&](int rc) {
        r->rc = rc;
        r->err = g_last_error;
    };
    DeviceCtx* c = nullptr;
    int rc = get_ctx(&c);
    if (rc) return failed(rc);
    std::lock_guard<std::mutex> g(c->mu);
    r->cold = !c->ready;
    rc = ensure_ready(c);
    if (rc) return failed(rc);
    const Blocks& B = A.B;
    const uint8_t* d_base = nullptr;
    if (A.in_place) {
        void* d = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&d, const_cast<uint8_t*>(B.base), 0);
        if (e != hipSuccess)
            return failed(fail(STORMCK_EHIP, std::string("split: hipHostGetDevicePointer: ") + hipGetErrorString(e)));
        d_base = static_cast<const uint8_t*>(d);
    }
    const double bpb = A.bytes_per_block;
    // blocks per chunk: what the staging chunk holds (DMA), or the offsets and lengths its
    // pinned buffer holds, about a chunk's worth of bytes (in place)
    const uint64_t step = B.n == 1 ? std::max<uint64_t>(B.len_of(0), 8) : std::max<uint64_t>(B.stride, 8);
    uint64_t max_blocks = A.in_place
        ? std::max<uint64_t>(1, std::min<uint64_t>(kChunkBytes / 12, static_cast<uint64_t>(kChunkBytes / bpb)))
        : std::max<uint64_t>(1, kChunkBytes / step);
    // a strided chunk may take the copy engine (issue below): its rows, stride apart, must
    // fit the staging buffer whatever the blocks' lengths
    if (!B.offs) max_blocks = std::min<uint64_t>(max_blocks, std::max<uint64_t>(1, kChunkBytes / step));
    // chunks of at most 1/16 of the call (and at least kSplitDmaBytes): each claim is sized
    // from what the host threads have actually left, so a host faster or slower than its
    // rate moves the devices' later claims instead of leaving one large chunk in flight
    // at the end
    max_blocks = std::min<uint64_t>(
        max_blocks, std::max<uint64_t>(1, static_cast<uint64_t>(
                                              std::max(kSplitDmaBytes, bpb * static_cast<double>(B.n) / 16.0) / bpb)));
    double inflight = 0, t0 = 0, t_end = 0;
    double stage_bytes[kStages] = {};
    const StageEngine eng{c, Wait::kBlock};
    Chunk ch;
    ch.B = &B;
    ch.plan_len = B.lens ? A.plan_len : B.len;
    ch.expected = A.expected;
    ch.d_base = d_base;

    auto drain = [&](int k) -> int {
        Stage& s = c->st[k];
        if (!s.busy) return STORMCK_OK;
        const uint64_t cnt = s.count;
        const int drc = eng.drain(s, A.expected != nullptr, A.sink, &r->first_bad, &r->n_bad);
        inflight -= stage_bytes[k];
        if (drc) return drc;
        r->blocks += cnt;
        r->bytes += static_cast<uint64_t>(stage_bytes[k]);
        t_end = now_us();
        if (r->first_done == 0) {
            r->first_done = t_end;
            r->first_bytes = static_cast<uint64_t>(stage_bytes[k]);
        }
        return STORMCK_OK;
    };

    r->started = now_us();
    for (uint64_t k = 0;; ++k) {
        const int st = static_cast<int>(k % kStages);
        rc = drain(st);
        if (rc) break;
        uint64_t a = 0, b = 0;
        if (!q.device(inflight, inflight > 0 ? kSplitChunkUs : lat_us, max_blocks, &a, &b)) break;
        if (t0 == 0) r->first_issue = t0 = now_us();
        stage_bytes[st] = static_cast<double>(B.bytes(a, b));
        inflight += stage_bytes[st];
        ch.first = a;
        ch.count = b - a;
        // strided rows go through the copy engine when the chunk is large (55.7 GB/s against
        // ~43 for kernels reading in place, profiles/r05_second/), in place when it is small
        // (no copy to wait for: the first chunk returns sooner)
        ch.rows = B.offs ? Rows::kGather
                         : (!A.in_place || stage_bytes[st] >= kSplitDmaBytes ? Rows::kDma : Rows::kStrided);
        rc = eng.issue(c->st[st], ch);
        if (rc) break;
    }
    for (int k = 0; k < kStages && rc == STORMCK_OK; ++k) rc = drain(k);
    if (rc) {
        eng.abandon();
        return failed(rc);
    }
    r->busy_us = t_end > t0 ? t_end - t0 : 0;
    r->finished = now_us();
}

struct SplitResult {
    uint64_t first_bad = 0, n_bad = 0, device_blocks = 0;
};

constexpr uint64_t kLatencyProbeBytes = 32ULL << 20;

bool trace_on() {
    static const bool on = std::getenv("STORMCK_TRACE") != nullptr;
    return on;
}

// One call's blocks on `pl` host threads and the devices `devs` at once (the host leg when
// devs is empty). fixed: STORMCK_SPLIT_BALANCED, or the number of blocks (the last ones)
// the devices hash. Verify (A.expected): *R gets the lowest mismatching index (n if none)
// and the count over both sides.
int split_run(SplitArgs& A, const std::vector<int>& devs, unsigned pl, uint64_t fixed, SplitResult* R) {
    const Blocks& B = A.B;
    const uint64_t n = B.n;
    R->first_bad = n;
    R->n_bad = 0;
    R->device_blocks = 0;
    if (n == 0) return STORMCK_OK;
    const uint64_t bytes = B.bytes(0, n);
    const double bpb = std::max(1.0, static_cast<double>(bytes) / static_cast<double>(n));
    A.bytes_per_block = bpb;
    const stormck_route_rates rt = route_model().now();
    ForkJoin& fj = ForkJoin::get();
    const unsigned nd = static_cast<unsigned>(devs.size());
    pl = std::max(1u, std::min(pl, split_threads(fj.size(), fj.cpus(), nd)));
    const double r_dev = A.in_place ? rt.link_inplace : rt.link_pinned;
    const double r_host = host_rate(rt, pl, bytes);
    const double lat = rt.device_latency;
    const double t_post = now_us();

    // the workers this call gets, taken in ascending device order whatever the caller's order
    // (fixed mode waits for each, so one global order rules out a deadlock between two calls);
    // balanced: a worker that another call owns is left out (the host takes its share)
    std::vector<DevRun> runs(nd);
    std::vector<unsigned> order(nd);
    for (unsigned k = 0; k < nd; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return devs[a] < devs[b]; });
    std::vector<std::pair<unsigned, DevWorker*>> got;
    for (unsigned k : order) {
        DevWorker* w = DevWorker::of(devs[k]);
        if (!w) {
            runs[k].rc = STORMCK_EINVAL;
            runs[k].err = "device index beyond 64";
            continue;
        }
        if (w->acquire(fixed != STORMCK_SPLIT_BALANCED)) got.emplace_back(k, w);
    }
    // the queue's balance counts the devices that take part, not the ones listed
    const unsigned nposted = static_cast<unsigned>(got.size());
    SplitQueue q(n, nposted ? fixed : 0, bpb, r_host, r_dev, nposted);
    std::vector<DevWorker*> posted;
    for (auto& [k, w] : got) {
        DevRun* out = &runs[k];
        w->start([&A, &q, lat, out] { device_part(A, q, lat, out); });
        posted.push_back(w);
    }

    // the host part: pieces from the front, small enough near the meeting point to balance
    const uint64_t want = nposted ? static_cast<uint64_t>(static_cast<double>(bytes) / (64.0 * pl) / bpb)
                                  : n / (uint64_t{pl} * 8);
    const uint64_t piece =
        (std::max<uint64_t>(nposted ? 8 : 4, nposted ? std::min<uint64_t>(want, 1024) : want) + 3) / 4 * 4;
    std::atomic<uint64_t> host_blocks{0}, host_bytes{0}, bad_n{0}, bad_first{n};
    auto work = [&](unsigned) {
        uint64_t my_n = 0, my_first = n, my_blocks = 0, my_bytes = 0, a = 0, b = 0;
        while (q.host(piece, &a, &b)) {
            hash_blocks(B, a, b, [&](uint64_t i, uint64_t h) {
                if (!A.expected) {
                    A.sink->one(i, h);
                } else if (h != A.expected[i]) {
                    ++my_n;
                    my_first = std::min(my_first, i);
                }
            });
            my_blocks += b - a;
            my_bytes += B.bytes(a, b);
        }
        host_blocks.fetch_add(my_blocks, std::memory_order_relaxed);
        host_bytes.fetch_add(my_bytes, std::memory_order_relaxed);
        if (my_n) {
            bad_n.fetch_add(my_n, std::memory_order_relaxed);
            uint64_t cur = bad_first.load(std::memory_order_relaxed);
            while (my_first < cur && !bad_first.compare_exchange_weak(cur, my_first, std::memory_order_relaxed)) {
            }
        }
    };
    const unsigned parts = static_cast<unsigned>(std::min<uint64_t>(pl, (n + piece - 1) / piece));
    const double h0 = now_us();
    fj.run(parts, work, static_cast<double>(bytes) / (r_host + nposted * r_dev));
    const double h_us = now_us() - h0;
    for (DevWorker* w : posted) w->wait();
    const double t_back = now_us();  // the caller has every device's results

    uint64_t fb = bad_first.load(), nb = bad_n.load();
    for (unsigned k = 0; k < nd; ++k) {
        const DevRun& r = runs[k];
        if (r.rc) return fail(r.rc, "device " + std::to_string(devs[k]) + ": " + r.err);
        R->device_blocks += r.blocks;
        if (r.n_bad) {
            nb += r.n_bad;
            fb = std::min(fb, r.first_bad);
        }
    }
    if (host_blocks.load() + R->device_blocks != n)
        return fail(STORMCK_EHIP, "split: " + std::to_string(n - host_blocks.load() - R->device_blocks) +
                                      " blocks left unhashed");
    R->first_bad = fb;
    R->n_bad = nb;
    RouteModel& m = route_model();
    // host rates from host legs only: in a split the host threads share host memory with
    // the devices' reads (and leave them a CPU), so their rate there is not the host leg's
    // the plans compare against (c5's learned cap fell 25 % under the measured host leg
    // and the c5 batch split where the host alone was faster, profiles/r05_eighth/)
    if (posted.empty()) m.learn_host(host_bytes.load(), parts, h_us);
    const double fixed_us = kDevBatchCallUs + static_cast<double>(A.plan_len) / kDevChainBytesPerUs;
    for (const DevRun& r : runs) {
        m.learn_link(A.in_place ? Link::kInplace : Link::kPinned, r.bytes, r.busy_us - fixed_us);
        // the start latency as the call sees it: from posting the device's part until the
        // caller holds its results (the caller's own wake-up included when the device
        // finished last), less its bytes over the link; from parts small enough that the
        // link time is a minor, well-estimated share of that
        if (r.first_done > 0 && r.bytes <= kLatencyProbeBytes && !r.cold) {
            const double back = r.finished > h0 + h_us ? t_back : r.finished;
            m.learn_latency(r.bytes, r_dev, back - t_post);
        }
    }
    if (trace_on()) {
        const double t_end = now_us();
        std::string d;
        char buf[256];
        for (size_t k = 0; k < runs.size(); ++k) {
            const DevRun& r = runs[k];
            std::snprintf(buf, sizeof buf,
                          " dev%d{blocks=%llu start=%.1f issue=%.1f first_back=%.1f(%.2fMB) end=%.1f}", devs[k],
                          static_cast<unsigned long long>(r.blocks), r.started - t_post, r.first_issue - t_post,
                          r.first_done - t_post, r.first_bytes / 1e6, r.finished - t_post);
            d += buf;
        }
        std::fprintf(stderr, "[stormck] split n=%llu pl=%u host{blocks=%llu end=%.1f} total=%.1f us%s\n",
                     static_cast<unsigned long long>(n), parts, static_cast<unsigned long long>(host_blocks.load()),
                     h0 + h_us - t_post, t_end - t_post, d.c_str());
    }
    return STORMCK_OK;
}

// ---- f1 on the host threads: the plan and the heights ---------------------------------
struct CommitPlan {
    CommitOrder O;              // the commit order and where each height starts in it
    std::vector<uint64_t> off;  // commit position -> data_offset
    std::vector<uint32_t> len;  // commit position -> length
};

// The commit order of a validated forest and the relocation in that order, on at most
// `threads` pool threads. Everything is allocated before the first record changes.
void commit_plan(stormck_dirty_block* blocks, const Heights& H, uint64_t revision, uint64_t* last_allocated_block,
                 uint32_t threads, CommitPlan* P) {
    commit_order(H, plan_par(threads), &P->O);
    P->off.resize(H.n);
    P->len.resize(H.n);
    uint64_t* off = P->off.data();
    uint32_t* len = P->len.data();
    relocate_range(blocks, P->O, 0, H.n, revision, H.relocating != 0, last_allocated_block, stage_par(threads),
                   [off, len](uint64_t k, const stormck_dirty_block& r) {
                       off[k] = r.data_offset;
                       len[k] = r.length;
                   });
}

// A height's checksums: the caller's out_checksums and, through the block's origin, the
// Pointer and type its parent keeps (PostCommitFunc, cache/trace.go:274-320).
struct CommitSink final : Sink {
    uint8_t* arena;
    const stormck_dirty_block* blocks;
    const CommitOrder& O;
    uint64_t lo;  // this height's first commit position
    uint64_t* out;
    CommitSink(uint8_t* a, const stormck_dirty_block* b, const CommitOrder& o, uint64_t l, uint64_t* c)
        : arena(a), blocks(b), O(o), lo(l), out(c) {}
    void one(uint64_t k, uint64_t h) override {
        const uint64_t i = O.at(lo + k);
        const stormck_dirty_block& b = blocks[i];
        out[i] = h;
        if (b.origin_pointer != STORMCK_NO_ORIGIN) {
            const uint64_t ptr[3] = {h, b.address, b.birth_revision};
            std::memcpy(arena + b.origin_pointer, ptr, sizeof ptr);
            arena[b.origin_type] = b.type;
        }
    }
};

// The host and split legs of a validated commit: plan, then the heights, children first:
// height 0 (the leaves) on the host threads and `devs` at once (devices read the registered
// arena in place), every other height on the host threads (they hold a few pointer blocks).
int commit_host_run(uint8_t* arena, stormck_dirty_block* blocks, const Heights& H, uint64_t revision,
                    uint64_t* last_allocated_block, uint64_t* out, uint32_t threads, const std::vector<int>& devs,
                    uint64_t device_leaves, uint64_t* device_done) {
    CommitPlan P;
    commit_plan(blocks, H, revision, last_allocated_block, threads, &P);
    ForkJoin& fj = ForkJoin::get();
    const unsigned nt = threads ? std::min<unsigned>(threads, fj.size()) : fj.size();
    const std::vector<int> none;
    for (size_t l = 0; l + 1 < P.O.level_start.size(); ++l) {
        const uint64_t lo = P.O.level_start[l], cnt = P.O.level_start[l + 1] - lo;
        if (cnt == 0) continue;
        SplitArgs A;
        A.B.base = arena;
        A.B.offs = P.off.data() + lo;
        A.B.lens = P.len.data() + lo;
        A.B.n = cnt;
        A.plan_len = static_cast<uint32_t>(std::max<uint64_t>(A.B.longest(), 1));
        A.in_place = true;
        CommitSink sink(arena, blocks, P.O, lo, out);
        A.sink = &sink;
        const bool split = l == 0 && !devs.empty();
        SplitResult R;
        const int rc = split_run(A, split ? devs : none, host_threads_for(A.B.bytes(0, cnt), nt),
                                 split ? device_leaves : STORMCK_SPLIT_BALANCED, &R);
        if (rc) return rc;
        if (split && device_done) *device_done = R.device_blocks;
    }
    return STORMCK_OK;
}

// Work queued on `st` has finished (a query when it is idle, else a synchronise): what host
// threads read next is what it wrote. NULL: nothing to wait for (include/stormck.h,
// stormck_commit: storm writes cache.data on the host; the query cost 0.07 us of a 3.8 us
// three-block commit, tools/route_overhead.cpp).
int stream_drained(hipStream_t st) {
    if (!st) return STORMCK_OK;
    if (hipStreamQuery(st) == hipSuccess) return STORMCK_OK;
    (void)hipGetLastError();
    HIP_TRY(hipStreamSynchronize(st));
    return STORMCK_OK;
}

// A validated batch on `pl` host threads and the devices `devs` at once (split_run): the
// host leg when devs is empty, else the split leg (stormck_checksum_split / the routed
// batch's split), whose devices read the blocks in place or by DMA.
int batch_legs(const HostBatch& hb, uint64_t* out, const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad,
               const std::vector<int>& devs, unsigned pl, uint64_t device_blocks, uint64_t* device_done, bool in_place) {
    SplitArgs A;
    A.B = hb.B;
    A.in_place = in_place;
    A.plan_len = hb.plan_len;
    A.expected = expected;
    OutSink sink(out);
    A.sink = &sink;
    SplitResult R;
    const int rc = split_run(A, devs, pl, device_blocks, &R);
    if (rc) return rc;
    if (first_bad) *first_bad = R.first_bad;
    if (n_bad) *n_bad = R.n_bad;
    if (device_done) *device_done = R.device_blocks;
    return STORMCK_OK;
}

// The host leg of a batch on at most `nt` pool threads: no device involved.
int batch_host_leg(const HostBatch& hb, uint64_t* out, const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad,
                   unsigned nt) {
    return batch_legs(hb, out, expected, first_bad, n_bad, {}, host_threads_for(hb.bytes, nt), STORMCK_SPLIT_BALANCED,
                      nullptr, false);
}

// The explicit host-leg entry points: any readable host memory, `threads` pool threads (0 = the
// pool). The host leg stages nothing, so it has no limit on the block step.
int host_leg_entry(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint64_t* out,
                   const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t threads) {
    HostBatch hb;
    const int rc = host_batch(base, stride, lens, len, n, expected ? static_cast<const void*>(expected) : out,
                              "null argument", false, &hb);
    if (rc || n == 0) return rc;
    if (!host_readable(base, hb.extent)) return fail(STORMCK_EINVAL, "base is not readable host memory");
    return batch_host_leg(hb, out, expected, first_bad, n_bad, pool_threads(threads));
}

// The routed batch: the leg the cost model predicts is fastest (*leg_used).
int batch_routed(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint64_t* out,
                 const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t host_threads,
                 uint32_t* leg_used) {
    if (leg_used) *leg_used = STORMCK_LEG_NONE;
    HostBatch hb;
    int rc = host_batch(base, stride, lens, len, n, expected ? static_cast<const void*>(expected) : out, "null argument",
                        false, &hb);
    if (rc) return rc;
    rc = device_check();  // a batch entry point of the GPU engine: no device, no batch
    if (rc) return rc;
    if (n == 0) return empty_batch(first_bad, n_bad);
    // a batch that one host thread hashes faster than any device can start returning takes
    // the host leg without planning (host_only), before any fact the decision below needs is
    // gathered; it only needs the range to be readable host memory (registered, or readable:
    // what the host leg alone checks), not its kind
    if (host_only(route_model().host_thread(), hb.bytes)) {
        if (!in_registered(base, hb.extent) && !host_readable(base, hb.extent))
            return not_host_memory(classify(base, hb.extent));
        if (leg_used) *leg_used = STORMCK_LEG_HOST;
        return batch_host_leg(hb, out, expected, first_bad, n_bad, 1);
    }
    const Mem mem = classify(base, hb.extent);
    if (mem == Mem::kDevice || mem == Mem::kUnreadable) return not_host_memory(mem);
    const stormck_route_rates rt = route_model().now();
    std::vector<int> devs;
    rc = route_devices(&devs);
    if (rc) return rc;
    const bool pinned = mem != Mem::kPageable;
    // the device pipeline stages whole blocks through 256 MiB chunks
    const Route route = route_batch(rt, n, hb.bytes, hb.longest, pinned, hb.step <= kChunkBytes,
                                    static_cast<unsigned>(devs.size()), pool_facts(host_threads, true));
    if (leg_used) *leg_used = route.plan.leg;
    if (route.plan.leg == STORMCK_LEG_DEVICE) {
        const double t0 = now_us();
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur));
        rc = devs.size() == 1 && devs[0] == cur
                 ? host_pipeline(hb, &mem, out, expected, first_bad, n_bad)
                 : host_pipeline_multi(base, stride, lens, len, n, out, expected, first_bad, n_bad, devs.data(),
                                       static_cast<int>(devs.size()));
        if (rc == STORMCK_OK)
            route_model().learn_link(pinned ? Link::kPinned : Link::kPageable, hb.bytes / devs.size(),
                                     now_us() - t0 - kDevBatchCallUs -
                                         static_cast<double>(hb.longest) / kDevChainBytesPerUs);
        return rc;
    }
    const unsigned pl = host_threads_for(hb.bytes, route.threads);
    if (route.plan.leg == STORMCK_LEG_SPLIT)
        return batch_legs(hb, out, expected, first_bad, n_bad, devs, pl, STORMCK_SPLIT_BALANCED, nullptr,
                          mem == Mem::kMapped);
    return batch_host_leg(hb, out, expected, first_bad, n_bad, pl);
}

// The explicit split entry points: pinned or registered memory, the listed devices (or the
// route devices), the host part on host_threads threads (0 = the pool).
int split_entry(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint64_t* out,
                const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, const int* devices, int n_devices,
                uint32_t host_threads, uint64_t device_blocks, uint64_t* device_done) {
    if (device_done) *device_done = 0;
    HostBatch hb;
    int rc = host_batch(base, stride, lens, len, n, expected ? static_cast<const void*>(expected) : out, "null argument",
                        true, &hb);
    if (rc) return rc;
    rc = device_check();
    if (rc) return rc;
    std::vector<int> devs;
    rc = split_devices(devices, n_devices, &devs);
    if (rc) return rc;
    if (n == 0) return empty_batch(first_bad, n_bad);
    const Mem mem = classify(base, hb.extent);
    if (mem == Mem::kDevice || mem == Mem::kUnreadable) return not_host_memory(mem);
    if (mem == Mem::kPageable)
        return fail(STORMCK_EINVAL, "the split leg needs pinned or registered host memory (stormck_host_register)");
    return batch_legs(hb, out, expected, first_bad, n_bad, devs, host_threads_for(hb.bytes, pool_threads(host_threads)),
                      device_blocks, device_done, mem == Mem::kMapped);
}

}  // namespace

extern "C" {

// ---- f1: the device, host and split legs (plan, then run) and the routed commit ----------
// Every leg validates first and with one rule set (commit_plan.h commit_heights): an error
// changes nothing.
int stormck_commit_device(void* d_arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                          uint64_t* last_allocated_block, uint64_t* out_checksums, void* stream) {
    static_assert(sizeof(stormck_dirty_block) == 56, "stormck_dirty_block ABI");
    if (n == 0) return STORMCK_OK;
    if (!d_arena || !blocks || !last_allocated_block || !out_checksums) return fail(STORMCK_EINVAL, "null argument");
    PhaseTimer pt("commit");
    Heights H;
    const int rc = commit_forest(blocks, n, revision, 0, &H);  // before the device check
    if (rc) return rc;
    pt.mark("heights");
    return commit_device_run(d_arena, blocks, H, revision, last_allocated_block, out_checksums, stream, pt);
}

int stormck_commit_host(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                        uint64_t* last_allocated_block, uint64_t* out_checksums, uint32_t threads) {
    if (n == 0) return STORMCK_OK;
    if (!arena || !blocks || !last_allocated_block || !out_checksums) return fail(STORMCK_EINVAL, "null argument");
    Heights H;
    const int rc = commit_forest(blocks, n, revision, threads, &H);
    if (rc) return rc;
    return commit_host_run(static_cast<uint8_t*>(arena), blocks, H, revision, last_allocated_block, out_checksums, threads,
                           {}, 0, nullptr);
}

int stormck_commit_split(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                         uint64_t* last_allocated_block, uint64_t* out_checksums, const int* devices, int n_devices,
                         uint32_t host_threads, uint64_t device_leaves, uint64_t* device_done) {
    if (device_done) *device_done = 0;
    if (n == 0) return STORMCK_OK;
    if (!arena || !blocks || !last_allocated_block || !out_checksums) return fail(STORMCK_EINVAL, "null argument");
    int rc = device_check();
    if (rc) return rc;
    std::vector<int> devs;
    rc = split_devices(devices, n_devices, &devs);
    if (rc) return rc;
    const Mem mem = classify(arena, 1);
    if (mem != Mem::kMapped)
        return fail(STORMCK_EINVAL, "the split commit needs the arena registered (stormck_host_register)");
    Heights H;
    rc = commit_forest(blocks, n, revision, host_threads, &H);
    if (rc) return rc;
    return commit_host_run(static_cast<uint8_t*>(arena), blocks, H, revision, last_allocated_block, out_checksums,
                           host_threads, devs, device_leaves, device_done);
}

int stormck_commit(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                   uint64_t* last_allocated_block, uint64_t* out_checksums, void* stream, uint32_t host_threads,
                   uint32_t* leg_used) {
    if (leg_used) *leg_used = STORMCK_LEG_NONE;
    if (n == 0) return STORMCK_OK;
    if (!arena || !blocks || !last_allocated_block || !out_checksums) return fail(STORMCK_EINVAL, "null argument");
    int rc = device_check();  // the routed commit is the GPU engine's: no device, no commit
    if (rc) return rc;
    const Mem mem = classify(arena, 1);
    if (mem == Mem::kDevice) {  // an HBM arena: only the device reaches it
        if (leg_used) *leg_used = STORMCK_LEG_DEVICE;
        return stormck_commit_device(arena, blocks, n, revision, last_allocated_block, out_checksums, stream);
    }
    if (mem == Mem::kUnreadable) return not_host_memory(mem);
    const bool registered = mem == Mem::kMapped;
    // a forest one host thread hashes faster than any device can start returning (storm's
    // smallest commits: a few blocks) takes the host leg without planning (host_only), before
    // the forest is walked
    if (host_only(route_model().host_thread(), blocks, n)) {
        if (leg_used) *leg_used = STORMCK_LEG_HOST;
        rc = registered ? stream_drained(static_cast<hipStream_t>(stream)) : STORMCK_OK;
        if (rc) return rc;
        return stormck_commit_host(arena, blocks, n, revision, last_allocated_block, out_checksums, 1);
    }
    const stormck_route_rates rt = route_model().now();
    std::vector<int> devs;
    rc = route_devices(&devs);
    if (rc) return rc;
    // one walk of the forest serves the router and the chosen leg; on the pool, as the
    // device leg's always was (host_threads bounds the hashing, which comes after the choice)
    Heights H;
    rc = commit_forest(blocks, n, revision, 0, &H);
    if (rc) return rc;
    CommitShape shape;
    commit_shape(H, blocks, n, &shape);
    const Route route =
        route_commit(rt, shape, registered, static_cast<unsigned>(devs.size()), pool_facts(host_threads, true));
    if (leg_used) *leg_used = route.plan.leg;
    if (route.plan.leg == STORMCK_LEG_DEVICE) {
        void* d_arena = nullptr;  // the kernels read and write the registered arena in place
        HIP_TRY(hipHostGetDevicePointer(&d_arena, arena, 0));
        PhaseTimer pt("commit");  // the heights are walked already
        return commit_device_run(d_arena, blocks, H, revision, last_allocated_block, out_checksums, stream, pt);
    }
    // host threads read the arena now: device work the caller queued on `stream` (e.g. a
    // kernel writing blocks into the registered arena) must have landed first
    rc = registered ? stream_drained(static_cast<hipStream_t>(stream)) : STORMCK_OK;
    if (rc) return rc;
    if (route.plan.leg != STORMCK_LEG_SPLIT) devs.clear();
    return commit_host_run(static_cast<uint8_t*>(arena), blocks, H, revision, last_allocated_block, out_checksums,
                           route.threads, devs, STORMCK_SPLIT_BALANCED, nullptr);
}

// ---- host-memory batches ---------------------------------------------------------------
int stormck_checksum_host_leg(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                              uint64_t* out, uint32_t threads) {
    return host_leg_entry(base, stride, lens, len, n, out, nullptr, nullptr, nullptr, threads);
}

int stormck_verify_host_leg(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                            const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t threads) {
    if (!first_bad || !n_bad) return fail(STORMCK_EINVAL, "null argument");
    *first_bad = n;
    *n_bad = 0;
    return verify_status(host_leg_entry(base, stride, lens, len, n, nullptr, expected, first_bad, n_bad, threads), n_bad);
}

int stormck_checksum_batch(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                           uint64_t* out, uint32_t host_threads, uint32_t* leg_used) {
    return batch_routed(base, stride, lens, len, n, out, nullptr, nullptr, nullptr, host_threads, leg_used);
}

int stormck_verify_batch(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                         const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t host_threads,
                         uint32_t* leg_used) {
    if (leg_used) *leg_used = STORMCK_LEG_NONE;
    if (!first_bad || !n_bad) return fail(STORMCK_EINVAL, "null argument");
    return verify_status(
        batch_routed(base, stride, lens, len, n, nullptr, expected, first_bad, n_bad, host_threads, leg_used), n_bad);
}

int stormck_checksum_split(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                           uint64_t* out, const int* devices, int n_devices, uint32_t host_threads,
                           uint64_t device_blocks, uint64_t* device_done) {
    return split_entry(base, stride, lens, len, n, out, nullptr, nullptr, nullptr, devices, n_devices, host_threads,
                       device_blocks, device_done);
}

int stormck_verify_split(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                         const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, const int* devices,
                         int n_devices, uint32_t host_threads, uint64_t device_blocks, uint64_t* device_done) {
    if (!first_bad || !n_bad) return fail(STORMCK_EINVAL, "null argument");
    return verify_status(split_entry(base, stride, lens, len, n, nullptr, expected, first_bad, n_bad, devices, n_devices,
                                     host_threads, device_blocks, device_done),
                         n_bad);
}

// ---- the route model, for callers and tests --------------------------------------------
int stormck_route_get_rates(stormck_route_rates* rates) {
    if (!rates) return fail(STORMCK_EINVAL, "rates is null");
    *rates = route_model().now();
    return STORMCK_OK;
}

int stormck_route_set_rates(const stormck_route_rates* rates, uint32_t flags) {
    if (flags & ~STORMCK_RATES_FREEZE) return fail(STORMCK_EINVAL, "unknown flags");
    if (rates && !(rates->host_thread > 0 && rates->host_memory > 0 && rates->host_cached > 0 && rates->link_pinned > 0 &&
                   rates->link_pageable > 0 && rates->link_inplace > 0 && rates->device_latency >= 0))
        return fail(STORMCK_EINVAL, "every rate must be positive (and the latency not negative)");
    route_model().set(rates, (flags & STORMCK_RATES_FREEZE) != 0);
    return STORMCK_OK;
}

int stormck_route_devices(const int* devices, int n_devices) {
    std::vector<int> devs;
    if (n_devices != 0) {
        int rc = check_device_list(devices, n_devices);
        if (rc) return rc;
        rc = device_check();
        if (rc) return rc;
        rc = check_devices(devices, n_devices, true, &devs);
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> g(g_route_mu);
    g_route_devs = devs;
    return STORMCK_OK;
}

int stormck_route_plan_batch(uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint32_t memory,
                             uint32_t host_threads, uint32_t n_devices, uint32_t* leg, double* predicted_us) {
    if (!leg) return fail(STORMCK_EINVAL, "leg is null");
    if (memory > STORMCK_MEM_PINNED) return fail(STORMCK_EINVAL, "unknown memory kind");
    HostBatch s;
    const int rc = measure_batch(stride, lens, len, n, &s);
    if (rc) return rc;
    const LegPlan p = route_batch(route_model().now(), n, s.bytes, s.longest, memory == STORMCK_MEM_PINNED,
                                  s.step <= kChunkBytes, n_devices, pool_facts(host_threads, false)).plan;
    *leg = n ? p.leg : STORMCK_LEG_NONE;
    if (predicted_us) std::memcpy(predicted_us, p.us, sizeof p.us);
    return STORMCK_OK;
}

int stormck_route_plan_commit(const stormck_dirty_block* blocks, uint64_t n, uint32_t memory, uint32_t host_threads,
                              uint32_t n_devices, uint32_t* leg, double* predicted_us) {
    if (!leg) return fail(STORMCK_EINVAL, "leg is null");
    if (memory > STORMCK_MEM_PINNED) return fail(STORMCK_EINVAL, "unknown memory kind");
    if (n > 0 && !blocks) return fail(STORMCK_EINVAL, "blocks is null");
    Heights H;
    if (commit_heights(blocks, n, 0, plan_par(host_threads), &H) != CommitError::Ok)
        return fail(STORMCK_EINVAL, "malformed forest (parent range or cycle)");
    CommitShape shape;
    commit_shape(H, blocks, n, &shape);
    const LegPlan p = route_commit(route_model().now(), shape, memory == STORMCK_MEM_PINNED, n_devices,
                                   pool_facts(host_threads, false)).plan;
    *leg = n ? p.leg : STORMCK_LEG_NONE;
    if (predicted_us) std::memcpy(predicted_us, p.us, sizeof p.us);
    return STORMCK_OK;
}

uint64_t stormck_scrub_workspace_bytes(uint64_t n_blocks) { return scrub_workspace_bytes(n_blocks); }

int stormck_scrub_device(const void* d_store, const stormck_scrub_layout* layout, void* d_workspace,
                         uint64_t workspace_bytes, uint32_t* d_reachable, stormck_scrub_report* report, void* stream) {
    return scrub_device(d_store, layout, d_workspace, workspace_bytes, d_reachable, report, stream);
}

int stormck_scrub_tree_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                              uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, void* d_workspace,
                              uint64_t workspace_bytes, uint32_t* d_reachable, stormck_scrub_report* report, void* stream) {
    return scrub_tree_device(d_store, layout, root, root_type, leaf_kind, leaf_len, d_workspace, workspace_bytes,
                             d_reachable, report, stream);
}

int stormck_scrub_host(const void* store, const stormck_scrub_layout* layout, uint32_t* reachable,
                       stormck_scrub_report* report, uint32_t host_threads) {
    return scrub_host(store, layout, reachable, report, host_threads);
}

int stormck_scrub_tree_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                            uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, uint32_t* reachable,
                            stormck_scrub_report* report, uint32_t host_threads) {
    return scrub_tree_host(store, layout, root, root_type, leaf_kind, leaf_len, reachable, report, host_threads);
}

uint64_t stormck_trace_workspace_bytes(uint64_t n_tags) { return trace_workspace_bytes(n_tags); }

int stormck_trace_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                         uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* d_tags, uint64_t n,
                         uint32_t flags, stormck_trace_result* d_results, uint64_t* d_leaf_checksums, void* d_workspace,
                         uint64_t workspace_bytes, stormck_trace_report* report, void* stream) {
    return trace_device(d_store, layout, root, root_type, leaf_kind, leaf_len, d_tags, n, flags, d_results,
                        d_leaf_checksums, d_workspace, workspace_bytes, report, stream);
}

int stormck_trace_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                       uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* tags, uint64_t n,
                       uint32_t flags, stormck_trace_result* results, uint64_t* leaf_checksums,
                       stormck_trace_report* report, uint32_t host_threads) {
    return trace_host(store, layout, root, root_type, leaf_kind, leaf_len, tags, n, flags, results, leaf_checksums,
                      report, host_threads);
}

int stormck_fill_synthetic_device(void* d_dst, uint64_t stride, uint64_t n, uint64_t first, uint64_t seed,
                                  void* stream) {
    if (n == 0) return STORMCK_OK;
    if (!d_dst || (stride & 15) || stride == 0 || (reinterpret_cast<uintptr_t>(d_dst) & 15))
        return fail(STORMCK_EINVAL, "fill_synthetic needs a 16-byte aligned destination and stride");
    int rc = device_check();
    if (rc) return rc;
    hipLaunchKernelGGL(k_fill_synthetic, dim3(8192), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint8_t*>(d_dst), stride, n, first, seed);
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

#ifdef STORMCK_DEBUG_QUAD
// Debug build only (not in include/stormck.h): the partial-quad merge counter
// (kernels.h quad_bcast), and a self-test kernel that merges with lanes 1-3 of every
// quad inactive, so a test can see the counter move.
__global__ void k_debug_partial_quad(uint64_t* out) {
    const uint32_t lane = threadIdx.x & 63;
    if ((lane & 3) == 0) out[lane / 4] = quad_bcast<1>(0x1234 + lane);
}

int stormck_debug_partial_quads(uint64_t* count, int reset) {
    if (!count) return fail(STORMCK_EINVAL, "count is null");
    int rc = device_check();
    if (rc) return rc;
    unsigned long long v = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_partial_quads), sizeof v));
    if (reset) {
        const unsigned long long z = 0;
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_partial_quads), &z, sizeof z));
    }
    *count = v;
    return STORMCK_OK;
}

int stormck_debug_partial_quad_selftest(void) {
    int rc = device_check();
    if (rc) return rc;
    uint64_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, 16 * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_debug_partial_quad, dim3(1), dim3(64), 0, nullptr, d);
    const hipError_t e = hipDeviceSynchronize();
    (void)hipFree(d);
    if (e != hipSuccess) return fail(STORMCK_EHIP, hipGetErrorString(e));
    return STORMCK_OK;
}
#endif

}  // extern "C" (the lookup below calls stormck_key_tags_device and the trace's engine)

namespace {

#include "lookup.h"
#include "objects.h"
#include "spaces.h"
#include "get.h"
#include "update.h"
#include "insert.h"

}  // namespace

extern "C" {

uint64_t stormck_lookup_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block) {
    return lookup_workspace_bytes(n_keys, chunks_per_block);
}

int stormck_lookup_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                          uint8_t root_type, const stormck_objectlist_params* params, const void* d_keys,
                          uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t len, uint64_t n,
                          uint32_t flags, stormck_lookup_result* d_results, stormck_trace_result* d_trace_results,
                          uint64_t* d_tags, void* d_workspace, uint64_t workspace_bytes, stormck_lookup_report* report,
                          void* stream) {
    return lookup_device(d_store, layout, root, root_type, params, d_keys, stride, d_offsets, d_lens, len, n, flags,
                         d_results, d_trace_results, d_tags, d_workspace, workspace_bytes, report, stream);
}

int stormck_lookup_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                        uint8_t root_type, const stormck_objectlist_params* params, const void* keys, uint64_t stride,
                        const uint64_t* offsets, const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags,
                        stormck_lookup_result* results, stormck_trace_result* trace_results, uint64_t* tags,
                        stormck_lookup_report* report, uint32_t host_threads) {
    return lookup_host(store, layout, root, root_type, params, keys, stride, offsets, lens, len, n, flags, results,
                       trace_results, tags, report, host_threads);
}

uint64_t stormck_objects_workspace_bytes(uint64_t n_ids) { return objects_workspace_bytes(n_ids); }

int stormck_objects_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                           uint8_t root_type, const stormck_blob_params* params, const void* d_ids, uint64_t id_stride,
                           uint64_t n, uint32_t flags, stormck_object_result* d_results, void* d_objects,
                           uint64_t out_stride, void* d_workspace, uint64_t workspace_bytes,
                           stormck_objects_report* report, void* stream) {
    return objects_device(d_store, layout, root, root_type, params, d_ids, id_stride, n, flags, d_results, d_objects,
                          out_stride, d_workspace, workspace_bytes, report, stream);
}

int stormck_objects_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                         uint8_t root_type, const stormck_blob_params* params, const void* ids, uint64_t id_stride,
                         uint64_t n, uint32_t flags, stormck_object_result* results, void* objects, uint64_t out_stride,
                         stormck_objects_report* report, uint32_t host_threads) {
    return objects_host(store, layout, root, root_type, params, ids, id_stride, n, flags, results, objects, out_stride,
                        report, host_threads);
}

uint64_t stormck_spaces_workspace_bytes(uint64_t n_ids, uint32_t spaces_per_block) {
    return spaces_workspace_bytes(n_ids, spaces_per_block);
}

int stormck_spaces_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                          uint8_t root_type, const uint16_t* addressing_offsets, const uint64_t* d_ids, uint64_t n,
                          uint32_t flags, stormck_space_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_spaces_report* report, void* stream) {
    return spaces_device(d_store, layout, root, root_type, addressing_offsets, d_ids, n, flags, d_results, d_workspace,
                         workspace_bytes, report, stream);
}

int stormck_spaces_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                        uint8_t root_type, const uint16_t* addressing_offsets, const uint64_t* ids, uint64_t n,
                        uint32_t flags, stormck_space_result* results, stormck_spaces_report* report,
                        uint32_t host_threads) {
    return spaces_host(store, layout, root, root_type, addressing_offsets, ids, n, flags, results, report, host_threads);
}

uint64_t stormck_get_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block) {
    return get_workspace_bytes(n_keys, chunks_per_block);
}

int stormck_get_device(const void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                       const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                       const uint32_t* d_lens, uint32_t len, uint64_t n, uint32_t flags, stormck_get_result* d_results,
                       void* d_objects, uint64_t out_stride, void* d_workspace, uint64_t workspace_bytes,
                       stormck_get_report* report, void* stream) {
    return get_device(d_store, layout, space_id, params, d_keys, stride, d_offsets, d_lens, len, n, flags, d_results,
                      d_objects, out_stride, d_workspace, workspace_bytes, report, stream);
}

int stormck_get_host(const void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                     const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                     const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags, stormck_get_result* results,
                     void* objects, uint64_t out_stride, stormck_get_report* report, uint32_t host_threads) {
    return get_host(store, layout, space_id, params, keys, stride, offsets, lens, len, n, flags, results, objects,
                    out_stride, report, host_threads);
}

uint64_t stormck_update_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block) {
    return update_workspace_bytes(n_keys, chunks_per_block);
}

int stormck_update_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                          const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                          const uint32_t* d_lens, uint32_t len, uint64_t n, const void* d_objects, uint64_t in_stride,
                          uint32_t flags, stormck_update_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_update_report* report, void* stream) {
    return update_device(d_store, layout, space_id, params, d_keys, stride, d_offsets, d_lens, len, n, d_objects, in_stride,
                         flags, d_results, d_workspace, workspace_bytes, report, stream);
}

int stormck_update_host(void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                        const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                        const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride,
                        uint32_t flags, stormck_update_result* results, stormck_update_report* report,
                        uint32_t host_threads) {
    return update_host(store, layout, space_id, params, keys, stride, offsets, lens, len, n, objects, in_stride, flags,
                       results, report, host_threads);
}

uint64_t stormck_insert_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block) {
    return insert_workspace_bytes(n_keys, chunks_per_block);
}

int stormck_insert_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                          const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                          const uint32_t* d_lens, uint32_t len, uint64_t n, const void* d_objects, uint64_t in_stride,
                          uint32_t flags, stormck_insert_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_insert_report* report, void* stream) {
    return insert_device(d_store, layout, space_id, params, d_keys, stride, d_offsets, d_lens, len, n, d_objects, in_stride,
                         flags, d_results, d_workspace, workspace_bytes, report, stream);
}

int stormck_insert_host(void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                        const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                        const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride,
                        uint32_t flags, stormck_insert_result* results, stormck_insert_report* report,
                        uint32_t host_threads) {
    return insert_host(store, layout, space_id, params, keys, stride, offsets, lens, len, n, objects, in_stride, flags,
                       results, report, host_threads);
}

}  // extern "C"
