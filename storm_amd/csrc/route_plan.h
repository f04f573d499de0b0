// The routing of host-memory work, as arithmetic: the cost model, the rates it learns, the
// queue a split's host threads and devices share, and the decision of a routed call.
// Work that lives in host memory (storm's cache.data: the Go shim's ChecksumBatch,
// VerifyChecksumBatch and CommitBatch) runs on one of three legs:
//   host    the library's pool threads hash the blocks, four at a time with AVX-512;
//   device  the device(s) hash them over PCIe (the host pipeline; kernels reading the
//           registered arena in place for a commit);
//   split   both at once, on disjoint blocks of the one call: the host threads take pieces
//           from the front, each device takes chunks from the back, each chunk sized so
//           that the device finishes when everyone else does (SplitQueue), until they meet.
// The routed entry points take the leg with the smallest predicted time, from rates that
// start at priors measured on MI355X and that every call large enough to
// time measures again (RouteModel). route_batch and route_commit are the whole decision of a
// routed call; the call and its stormck_route_plan_* entry point both ask them.
// Pure host code (no HIP, no thread pool, no error state; tests/cpp/route_plan_test.cpp
// compiles it with a plain C++17 compiler). stormck.hip gathers the facts (memory kind,
// devices, pool), asks for the decision and runs the leg (split_run, device_part).
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <numeric>

#include "../../include/stormck.h"
#include "commit_plan.h"  // CommitShape

namespace stormck {

// A host pass is split over threads only in pieces of at least this many bytes (~10 us of
// hashing on one core, about what the pool's fork/join costs).
constexpr uint64_t kHostMinBytesPerThread = 256 * 1024;
constexpr double kHostLevelUs = 10.0;             // fork/join of a parallel pass
constexpr double kDevCallUs = 10.0;               // device commit: a call
constexpr double kDevLevelUs = 6.0;               // device commit: a launch per height
constexpr double kDevChainBytesPerUs = 1600.0;    // one 4-lane XXH64 chain on gfx950 (32 KiB in ~20 us)
constexpr double kDevBatchCallUs = 16.0;          // stage, launch, copy back and sync one small batch
constexpr double kStageCopyBytesPerUs = 55000.0;  // pageable -> pinned staging copy (8 threads)
constexpr uint64_t kStageChunkBytes = 256ULL << 20;  // the device pipeline's staging chunk (stormck.hip kChunkBytes)
constexpr double kSplitChunkUs = 8.0;             // a chunk issued behind one in flight: launch, copy back
constexpr double kSplitMinClaimBytes = 1 << 20;   // a smaller device claim costs about what it saves
constexpr double kSplitDmaBytes = 32 << 20;       // strided claims from this size take the copy engine
constexpr double kSplitGain = 0.95;               // the split is taken only when predicted 5% faster
constexpr double kSplitGainCached = 0.8;          // ... 20% for a call of at most kHostCacheBytes
constexpr double kHostOnlyUs = 10.0;              // calls one host thread finishes this fast are not planned
constexpr double kSplitMinSaveUs = 30.0;          // ... and only when it saves at least this much

// Priors, bytes/us: the rates measured on an MI355X box with its EPYC 9575F host
// (profiles/r04_batch_e2e/, r04_commit_e2e/).
constexpr double kPriorHostThreadX4 = 48000.0;  // one thread hashing four blocks at once (AVX-512)
constexpr double kPriorHostThread = 24000.0;    // one thread, scalar XXH64 (no AVX-512)
constexpr double kPriorHostMemory = 180000.0;   // the pool: host memory bound (the slower box, 179 GB/s)
constexpr double kPriorLinkPinned = 55000.0;    // the device pipeline from pinned / registered memory
constexpr double kPriorLinkPageable = 55000.0;  // the same through pinned staging, copy overlapped
constexpr double kPriorLinkInplace = 50000.0;   // kernels reading registered memory in place (49-55 GB/s)
constexpr double kPriorDeviceLatencyUs = 150.0; // a split's device part until its first chunk is back
                                                // (profiles/r05_first/: c5-size splits ~150 us over the host)
constexpr double kLearnWeight = 0.25;           // EWMA weight of one call's observed rate
constexpr uint64_t kLearnMinHostBytes = 8ULL << 20;   // below: fork/join noise
constexpr uint64_t kLearnMinLinkBytes = 64ULL << 20;  // below: launch and sync noise
// A host pass of at most this many bytes can run from the host's caches (a storm commit,
// ~38 MB, written by the caller just before): the pool's cap on it is learned apart from
// the cap on passes that stream from DRAM (c5 on the pool: ~100 us = 380 GB/s, against
// 180-330 GB/s for an 8 GiB batch, profiles/r05_third/).
constexpr uint64_t kHostCacheBytes = 64ULL << 20;

enum class Link { kPinned, kPageable, kInplace };

// The rates, shared by every call of the process (stormck.hip keeps the one instance).
// x4: the host hashes four blocks at once (AVX-512), which sets the per-thread prior.
class RouteModel {
  public:
    explicit RouteModel(bool x4)
        : prior_thread_(x4 ? kPriorHostThreadX4 : kPriorHostThread), r_(priors()), ht_(r_.host_thread) {}
    stormck_route_rates now() {
        std::lock_guard<std::mutex> g(mu_);
        return r_;
    }
    // host_thread alone, without the lock: what a routed call's host-only test reads
    double host_thread() const { return ht_.load(std::memory_order_relaxed); }
    void set(const stormck_route_rates* r, bool freeze) {
        std::lock_guard<std::mutex> g(mu_);
        r_ = r ? *r : priors();
        r_.observations = 0;
        frozen_ = freeze;
        ht_.store(r_.host_thread, std::memory_order_relaxed);
    }
    // A host pass: `bytes` hashed on `threads` threads in `us`. One thread measures the
    // per-thread rate; a pool pass either the threads (it ran at their rate) or the cap
    // that host memory and shared cores put on them (it ran below it).
    void learn_host(uint64_t bytes, unsigned threads, double us) {
        if (bytes < kLearnMinHostBytes || us <= 0) return;
        // the plans add the fork/join of a spread pass on top of bytes / rate: learn the
        // rate without it
        const double rate = static_cast<double>(bytes) / std::max(1.0, us - (threads > 1 ? kHostLevelUs : 0.0));
        std::lock_guard<std::mutex> g(mu_);
        if (frozen_) return;
        double& cap = bytes <= kHostCacheBytes ? r_.host_cached : r_.host_memory;
        if (threads <= 1) {
            r_.host_thread = ewma(r_.host_thread, rate);
        } else if (rate >= 0.8 * threads * r_.host_thread) {
            r_.host_thread = ewma(r_.host_thread, rate / threads);
            cap = std::max(cap, rate);
        } else {
            cap = ewma(cap, rate);
        }
        ht_.store(r_.host_thread, std::memory_order_relaxed);
        ++r_.observations;
    }
    // One device's transfer: `bytes` in `us` beyond the call's fixed latency.
    void learn_link(Link k, uint64_t bytes, double us) {
        if (bytes < kLearnMinLinkBytes || us <= 0) return;
        const double rate = static_cast<double>(bytes) / us;
        std::lock_guard<std::mutex> g(mu_);
        if (frozen_) return;
        double& r = k == Link::kPinned ? r_.link_pinned : (k == Link::kPageable ? r_.link_pageable : r_.link_inplace);
        r = ewma(r, rate);
        ++r_.observations;
    }
    // A split's device part: its first chunk came back `us` after the call posted it, of
    // which `bytes` over the link at the current rate account for `bytes / rate`.
    // One observation moves the latency up by at most a quarter of itself (plus 25 us): a
    // spike (the device's first kernel launches in a process loading their code, tens of
    // ms) would otherwise price the devices out of every later split, and a device that
    // never gets a chunk is never measured again to correct it.
    void learn_latency(uint64_t bytes, double rate, double us) {
        if (us <= 0 || rate <= 0) return;
        std::lock_guard<std::mutex> g(mu_);
        if (frozen_) return;
        const double lat = std::min(std::max(1.0, us - static_cast<double>(bytes) / rate),
                                    2.0 * r_.device_latency + 100.0);
        r_.device_latency = ewma(r_.device_latency, lat);
        ++r_.observations;
    }

  private:
    stormck_route_rates priors() const {
        stormck_route_rates r;
        std::memset(&r, 0, sizeof r);
        r.host_thread = prior_thread_;
        r.host_memory = kPriorHostMemory;
        r.host_cached = kPriorHostMemory;
        r.link_pinned = kPriorLinkPinned;
        r.link_pageable = kPriorLinkPageable;
        r.link_inplace = kPriorLinkInplace;
        r.device_latency = kPriorDeviceLatencyUs;
        return r;
    }
    static double ewma(double old, double obs) { return old + kLearnWeight * (obs - old); }
    const double prior_thread_;
    std::mutex mu_;
    stormck_route_rates r_;
    std::atomic<double> ht_;
    bool frozen_ = false;
};

// Aggregate rate of `threads` host threads.
inline double host_rate(const stormck_route_rates& r, unsigned threads, uint64_t bytes) {
    const double cap = bytes <= kHostCacheBytes ? r.host_cached : r.host_memory;
    return threads <= 1 ? r.host_thread : std::min(threads * r.host_thread, cap);
}

// Host threads a split may use beside `nd` device workers: the pool (`pool` threads), less one
// CPU per device where the pool alone would take every CPU the process may use (`cpus`). A
// device's worker and the HIP runtime threads serving it need a CPU now and then; on a GPU
// box, whose process gets 16 CPUs by quota, 16 hashing threads beside them starved them, and
// c5-size splits lost 20-30 % (profiles/r05_seventh/).
inline unsigned split_threads(unsigned pool, unsigned cpus, unsigned nd) {
    if (nd == 0) return pool;
    return pool + nd > cpus ? std::max(1u, cpus > nd ? cpus - nd : 1u) : pool;
}

// Threads a host pass of `bytes` uses out of `nt` allowed.
inline unsigned host_threads_for(uint64_t bytes, unsigned nt) {
    return static_cast<unsigned>(std::min<uint64_t>(std::max(1u, nt), std::max<uint64_t>(1, bytes / kHostMinBytesPerThread)));
}

// The blocks of one call, shared by its host threads (from the front) and its devices
// (from the back). Balanced: a device claims b bytes so that, with I bytes in flight and
// rate r_d, it finishes no later than the host threads and the other devices (rate r_o)
// finish the R bytes nobody has claimed:
//     L + (I + b) / r_d = (R - b) / r_o   ->   b = (R / r_o - L - I / r_d) / (1 / r_d + 1 / r_o)
// (L: the chunk's latency); a claim below kSplitMinClaimBytes ends the device's part.
// Fixed: the devices own exactly the last `fixed` blocks, the host threads the others.
class SplitQueue {
  public:
    SplitQueue(uint64_t n, uint64_t fixed, double bytes_per_block, double r_host, double r_dev, unsigned ndev)
        : lo_(0), hi_(n), split_(fixed == STORMCK_SPLIT_BALANCED ? UINT64_MAX : n - std::min(fixed, n)),
          bpb_(bytes_per_block), r_host_(r_host), r_dev_(r_dev), ndev_(ndev) {}
    bool host(uint64_t piece, uint64_t* a, uint64_t* b) {
        std::lock_guard<std::mutex> g(mu_);
        const uint64_t end = split_ != UINT64_MAX ? split_ : hi_;
        if (lo_ >= end) return false;
        *a = lo_;
        *b = std::min(end, lo_ + piece);
        lo_ = *b;
        return true;
    }
    bool device(double inflight, double lat_us, uint64_t max_blocks, uint64_t* a, uint64_t* b) {
        std::lock_guard<std::mutex> g(mu_);
        uint64_t cnt = 0;
        if (split_ != UINT64_MAX) {
            if (hi_ <= split_) return false;
            cnt = std::min(max_blocks, hi_ - split_);
        } else {
            if (hi_ <= lo_) return false;
            const uint64_t avail = hi_ - lo_;
            const double R = static_cast<double>(avail) * bpb_;
            const double r_o = r_host_ + (std::max(ndev_, 1u) - 1) * r_dev_;
            const double want = r_o <= 0 ? R : (R / r_o - lat_us - inflight / r_dev_) / (1.0 / r_dev_ + 1.0 / r_o);
            if (want < kSplitMinClaimBytes) return false;
            cnt = std::min<uint64_t>({static_cast<uint64_t>(want / bpb_), max_blocks, avail});
            if (cnt == 0) return false;
        }
        *a = hi_ - cnt;
        *b = hi_;
        hi_ -= cnt;
        return true;
    }

  private:
    std::mutex mu_;
    uint64_t lo_, hi_, split_;
    double bpb_, r_host_, r_dev_;
    unsigned ndev_;
};

// ---- the cost model -------------------------------------------------------------------
struct LegPlan {
    uint32_t leg = STORMCK_LEG_HOST;
    double us[3] = {0, INFINITY, INFINITY};  // host, device, split
    double best() const { return us[leg == STORMCK_LEG_DEVICE ? 1 : (leg == STORMCK_LEG_SPLIT ? 2 : 0)]; }
};

// The split is taken only when it is predicted to save both kSplitGain of the best single
// leg and kSplitMinSaveUs: on small calls the devices' part is a few chunks whose start and
// finish vary by tens of microseconds (profiles/r05_fourth/), more than it could save. A
// call of at most kHostCacheBytes needs kSplitGainCached: its host leg runs twice as fast
// from warm host caches as from cold ones (c5 on the pool: 77 us called back to back,
// 135-170 us between other work, profiles/r05_learn/), so its learned rate is a blend and
// the prediction loose, and the device's part gains nothing from the caches. Measured on six
// boxes, the split never beat the pool by more than 6% at c5 size, and beat one host
// thread by 1.6-2x.
inline void pick_leg(LegPlan* p, double bytes) {
    double best = p->us[0];
    p->leg = STORMCK_LEG_HOST;
    if (p->us[1] < best) {
        best = p->us[1];
        p->leg = STORMCK_LEG_DEVICE;
    }
    const double gain = bytes <= static_cast<double>(kHostCacheBytes) ? kSplitGainCached : kSplitGain;
    if (p->us[2] < gain * best && p->us[2] < best - kSplitMinSaveUs) p->leg = STORMCK_LEG_SPLIT;
}

// Time of a split that hashes `bytes` on host threads at r_h and devices at r_d together,
// or INFINITY if it beats the host alone (host_us) by nothing.
inline double split_us(double bytes, double r_h, double r_d, double lat, double overhead, double host_us) {
    const double t = (bytes + r_d * lat) / (r_h + r_d) + overhead;
    return t < host_us ? t : INFINITY;
}

// A call one host thread finishes faster than any device can start returning (kHostOnlyUs: a
// device's start latency is tens of microseconds) is not planned: the routed call takes the
// host leg on its own thread at once, paying no planning, no device list and no pool
// (storm's smallest commits, every revision: the singularity, cache/cache.go:64-85).
// bytes / host_thread < kHostOnlyUs, as a bound on the bytes.
inline bool host_only(double host_thread, uint64_t bytes) {
    return static_cast<double>(bytes) < kHostOnlyUs * host_thread;
}

// The same of a forest's records before anything has walked them: the sum stops at the
// bound, without a division per block (a 111-block `-tags test` forest paid 0.1 us for them).
inline bool host_only(double host_thread, const stormck_dirty_block* blocks, uint64_t n) {
    const double bound = kHostOnlyUs * host_thread;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n && static_cast<double>(total) < bound; ++i) total += blocks[i].length;
    return host_only(host_thread, total);
}

// The pool as a routed call finds it: the threads the call may use (its host_threads, capped
// by the pool), the pool's size, the CPUs the process may use, and for how long another
// call's job is predicted to hold the pool (0: it is free).
struct Pool {
    unsigned threads = 1, size = 1, cpus = 1;
    double busy_us = 0;
};

// The three legs of a host-memory batch of n blocks (`bytes` in all, the longest `longest`):
// the host threads; the device pipeline (a call, one chain over the longest block, the bytes
// over ndev links, and for pageable memory the first chunk's staging copy, which nothing
// overlaps; staged_ok: a block fits the staging chunk); the split (pinned memory only: from
// pageable memory the devices need host threads to copy, which hash faster than they copy),
// the devices reading in place after their start latency.
inline LegPlan plan_batch(const stormck_route_rates& r, uint64_t n, uint64_t nbytes, uint64_t longest, bool pinned,
                          bool staged_ok, unsigned nt, unsigned ndev, unsigned pool, unsigned cpus) {
    LegPlan p;
    const unsigned pl = host_threads_for(nbytes, nt);
    const double bytes = static_cast<double>(nbytes), chain = static_cast<double>(longest) / kDevChainBytesPerUs;
    const double level = pl > 1 ? kHostLevelUs : 0.0;
    const double r_h = host_rate(r, pl, nbytes);
    p.us[0] = bytes / r_h + level;
    if (ndev && staged_ok) {
        const double link = pinned ? r.link_pinned : r.link_pageable;
        const double fill = pinned ? 0.0 : static_cast<double>(std::min<uint64_t>(nbytes, kStageChunkBytes)) / kStageCopyBytesPerUs;
        p.us[1] = kDevBatchCallUs + chain + bytes / (ndev * link) + fill;
        if (pinned && n >= 2) {
            const unsigned ps = std::min(pl, split_threads(pool, cpus, ndev));
            p.us[2] = split_us(bytes, host_rate(r, ps, nbytes), ndev * r.link_inplace, r.device_latency,
                               ps > 1 ? kHostLevelUs : 0.0, p.us[0]);
        }
    }
    pick_leg(&p, bytes);
    return p;
}

// One height of a commit on the host threads: its bytes at the threads' rate, at least one
// block's chain, and a fork/join when it is spread.
inline double host_height_us(const stormck_route_rates& r, const CommitShape& s, size_t l, unsigned nt) {
    const unsigned pl = host_threads_for(s.bytes[l], nt);
    const double t = std::max(static_cast<double>(s.bytes[l]) / host_rate(r, pl, s.bytes[l]),
                              static_cast<double>(s.longest[l]) / r.host_thread);
    return t + (pl > 1 ? kHostLevelUs : 0.0);
}

// The three legs of a commit: the host threads, height by height; the device in place over
// the link (a call, then per height a launch and the longer of one chain over its longest
// block and its bytes over the link); the split (height 0, the leaves, on both; the upper
// heights on the host). The device legs need a registered arena.
inline LegPlan plan_commit(const stormck_route_rates& r, const CommitShape& s, bool registered, unsigned nt,
                           unsigned ndev, unsigned pool, unsigned cpus) {
    LegPlan p;
    p.us[0] = 0;
    for (size_t l = 0; l < s.cnt.size(); ++l) p.us[0] += host_height_us(r, s, l, nt);
    if (registered && ndev && !s.cnt.empty()) {
        p.us[1] = kDevCallUs;
        for (size_t l = 0; l < s.cnt.size(); ++l)
            p.us[1] += kDevLevelUs + std::max(static_cast<double>(s.longest[l]) / kDevChainBytesPerUs,
                                              static_cast<double>(s.bytes[l]) / r.link_inplace);
        if (s.cnt[0] >= 2) {
            const double h0 = host_height_us(r, s, 0, nt);
            const unsigned pl = std::min(host_threads_for(s.bytes[0], nt), split_threads(pool, cpus, ndev));
            const double t0 = split_us(static_cast<double>(s.bytes[0]), host_rate(r, pl, s.bytes[0]), ndev * r.link_inplace,
                                       r.device_latency, pl > 1 ? kHostLevelUs : 0.0, h0);
            p.us[2] = p.us[0] - h0 + t0;
        }
    }
    pick_leg(&p, static_cast<double>(std::accumulate(s.bytes.begin(), s.bytes.end(), uint64_t{0})));
    return p;
}

// ---- the decision of a routed call -------------------------------------------------------
// The leg a routed call takes and the host threads it takes it with.
struct Route {
    LegPlan plan;
    unsigned threads = 1;
};

// The decision of a call of `bytes` in all, whose plan with t host threads is plan(t). The
// host-only shortcut: one thread, the host's time alone. Else the plan with the threads the
// call may use, unless another call holds the pool: waiting for it pays only when the
// predicted wait plus this call's time on the pool beats this call on its own thread (a small
// call behind a large one runs at once on its caller's thread; a large one queues behind it).
template <class PlanWith>
Route route_on(const stormck_route_rates& r, uint64_t bytes, const Pool& pool, PlanWith&& plan) {
    Route rt;
    if (host_only(r.host_thread, bytes)) {
        rt.plan.us[0] = static_cast<double>(bytes) / r.host_thread;
        return rt;
    }
    rt.threads = std::max(1u, pool.threads);
    if (rt.threads > 1 && pool.busy_us > 0 && !(pool.busy_us + plan(rt.threads).best() < plan(1u).best()))
        rt.threads = 1;
    rt.plan = plan(rt.threads);
    return rt;
}

// The routed batch (stormck_checksum_batch, stormck_verify_batch, stormck_route_plan_batch).
inline Route route_batch(const stormck_route_rates& r, uint64_t n, uint64_t bytes, uint64_t longest, bool pinned,
                         bool staged_ok, unsigned ndev, const Pool& pool) {
    return route_on(r, bytes, pool, [&](unsigned t) {
        return plan_batch(r, n, bytes, longest, pinned, staged_ok, t, ndev, pool.size, pool.cpus);
    });
}

// The routed commit of a validated forest (stormck_commit, stormck_route_plan_commit).
inline Route route_commit(const stormck_route_rates& r, const CommitShape& s, bool registered, unsigned ndev,
                          const Pool& pool) {
    return route_on(r, std::accumulate(s.bytes.begin(), s.bytes.end(), uint64_t{0}), pool,
                    [&](unsigned t) { return plan_commit(r, s, registered, t, ndev, pool.size, pool.cpus); });
}

}  // namespace stormck
