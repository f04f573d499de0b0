// The routing of host-memory work (storm_amd/csrc/route_plan.h) against a model written out
// here from the header's constants, not its functions: the predicted times and the leg of a
// batch and of a commit, the margins of pick_leg, the host-only bound, the busy-pool rule, the
// split queue (balanced and fixed claims, alone and from 8 host and 3 device threads at once)
// and what the rate model learns. Doubles are compared to 1e-9 relative: each is a handful of
// IEEE operations. No GPU and no library.
#include "../../storm_amd/csrc/route_plan.h"

#include <cstdio>
#include <string>
#include <thread>
#include <vector>

using namespace stormck;

static int failures = 0;
static void expect_true(const std::string& what, bool ok) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
}
static bool near(double a, double b) {
    if (std::isinf(a) || std::isinf(b)) return a == b;
    return std::fabs(a - b) <= 1e-9 * std::max(std::fabs(a), std::fabs(b));
}
static void expect_near(const std::string& what, double got, double want) {
    if (near(got, want)) return;
    ++failures;
    std::printf("FAIL %s: got %.17g, want %.17g\n", what.c_str(), got, want);
}

static stormck_route_rates rates(double thread, double memory, double cached, double pinned, double pageable,
                                 double inplace, double latency) {
    stormck_route_rates r;
    std::memset(&r, 0, sizeof r);
    r.host_thread = thread;
    r.host_memory = memory;
    r.host_cached = cached;
    r.link_pinned = pinned;
    r.link_pageable = pageable;
    r.link_inplace = inplace;
    r.device_latency = latency;
    return r;
}
static const stormck_route_rates kBase = rates(40000, 180000, 180000, 55000, 50000, 52000, 120);
static const stormck_route_rates kRateSets[] = {
    kBase,
    rates(40000, 180000, 90000, 55000, 50000, 52000, 120),     // the cached cap apart from the memory cap
    rates(40000, 180000, 180000, 500, 500, 500, 120),          // a slow link
    rates(2000, 8000, 8000, 55000, 50000, 50000, 150),         // a slow host
    rates(400000, 4000000, 4000000, 55000, 50000, 52000, 1),   // a fast host
};
struct PoolCpus {
    unsigned pool, cpus;
};
static const PoolCpus kPools[] = {{16, 16}, {16, 256}, {4, 4}};

// ---- the model --------------------------------------------------------------------------
static double m_rate(const stormck_route_rates& r, unsigned t, uint64_t bytes) {
    if (t <= 1) return r.host_thread;
    const double cap = bytes <= kHostCacheBytes ? r.host_cached : r.host_memory;
    return t * r.host_thread < cap ? t * r.host_thread : cap;
}
static unsigned m_threads(uint64_t bytes, unsigned nt) {
    const uint64_t pieces = bytes / kHostMinBytesPerThread;
    const unsigned t = nt < 1 ? 1 : nt;
    return pieces < 1 ? 1 : (pieces < t ? static_cast<unsigned>(pieces) : t);
}
static unsigned m_beside(unsigned pool, unsigned cpus, unsigned nd) {
    if (nd == 0 || pool + nd <= cpus) return pool;
    return cpus > nd ? cpus - nd : 1;
}
struct Model {
    double us[3];
    uint32_t leg;
    double best() const { return leg == STORMCK_LEG_SPLIT ? us[2] : (leg == STORMCK_LEG_DEVICE ? us[1] : us[0]); }
};
static void m_choose(Model* m, double bytes) {
    const double single = m->us[1] < m->us[0] ? m->us[1] : m->us[0];
    m->leg = m->us[1] < m->us[0] ? STORMCK_LEG_DEVICE : STORMCK_LEG_HOST;
    const double gain = bytes <= static_cast<double>(kHostCacheBytes) ? kSplitGainCached : kSplitGain;
    if (m->us[2] < gain * single && m->us[2] < single - kSplitMinSaveUs) m->leg = STORMCK_LEG_SPLIT;
}
static double m_split(double bytes, double r_h, double r_d, double lat, bool spread, double host_us) {
    const double t = (bytes + r_d * lat) / (r_h + r_d) + (spread ? kHostLevelUs : 0.0);
    return t < host_us ? t : INFINITY;
}
static Model m_batch(const stormck_route_rates& r, uint64_t n, uint64_t bytes, uint64_t longest, bool pinned,
                     bool staged_ok, unsigned nt, unsigned ndev, PoolCpus pc) {
    Model m{{0, INFINITY, INFINITY}, STORMCK_LEG_HOST};
    const double B = static_cast<double>(bytes);
    const unsigned pl = m_threads(bytes, nt);
    m.us[0] = B / m_rate(r, pl, bytes) + (pl > 1 ? kHostLevelUs : 0.0);
    if (ndev > 0 && staged_ok) {
        m.us[1] = kDevBatchCallUs + static_cast<double>(longest) / kDevChainBytesPerUs +
                  B / (ndev * (pinned ? r.link_pinned : r.link_pageable));
        if (!pinned) m.us[1] += static_cast<double>(bytes < kStageChunkBytes ? bytes : kStageChunkBytes) / kStageCopyBytesPerUs;
        if (pinned && n >= 2) {
            const unsigned ps = std::min(pl, m_beside(pc.pool, pc.cpus, ndev));
            m.us[2] = m_split(B, m_rate(r, ps, bytes), ndev * r.link_inplace, r.device_latency, ps > 1, m.us[0]);
        }
    }
    m_choose(&m, B);
    return m;
}
static double m_height(const stormck_route_rates& r, uint64_t bytes, uint64_t longest, unsigned nt) {
    const unsigned pl = m_threads(bytes, nt);
    const double spread = static_cast<double>(bytes) / m_rate(r, pl, bytes);
    const double chain = static_cast<double>(longest) / r.host_thread;
    return (spread > chain ? spread : chain) + (pl > 1 ? kHostLevelUs : 0.0);
}
static Model m_commit(const stormck_route_rates& r, const CommitShape& s, bool registered, unsigned nt, unsigned ndev,
                      PoolCpus pc) {
    Model m{{0, INFINITY, INFINITY}, STORMCK_LEG_HOST};
    double total = 0;
    for (size_t l = 0; l < s.cnt.size(); ++l) {
        m.us[0] += m_height(r, s.bytes[l], s.longest[l], nt);
        total += static_cast<double>(s.bytes[l]);
    }
    if (registered && ndev > 0 && !s.cnt.empty()) {
        m.us[1] = kDevCallUs;
        for (size_t l = 0; l < s.cnt.size(); ++l) {
            const double chain = static_cast<double>(s.longest[l]) / kDevChainBytesPerUs;
            const double link = static_cast<double>(s.bytes[l]) / r.link_inplace;
            m.us[1] += kDevLevelUs + (chain > link ? chain : link);
        }
        if (s.cnt[0] >= 2) {
            const double h0 = m_height(r, s.bytes[0], s.longest[0], nt);
            const unsigned pl = std::min(m_threads(s.bytes[0], nt), m_beside(pc.pool, pc.cpus, ndev));
            m.us[2] = m.us[0] - h0 + m_split(static_cast<double>(s.bytes[0]), m_rate(r, pl, s.bytes[0]),
                                             ndev * r.link_inplace, r.device_latency, pl > 1, h0);
        }
    }
    m_choose(&m, total);
    return m;
}
static void expect_plan(const std::string& what, const LegPlan& p, const Model& m) {
    for (int k = 0; k < 3; ++k) expect_near(what + " us[" + std::to_string(k) + "]", p.us[k], m.us[k]);
    expect_true(what + " leg", p.leg == m.leg);
}

// ---- batch and commit times ---------------------------------------------------------------
static void test_batch_times() {
    const uint64_t L = 32768;
    // 64 MiB is 2,048 blocks: host_cached on and below it, host_memory above
    const uint64_t counts[] = {1, 2, 13, 100, 2047, 2048, 2049, 16384, 262144};
    int splits = 0, devices = 0, hosts = 0, reduced = 0;
    for (size_t ri = 0; ri < sizeof kRateSets / sizeof kRateSets[0]; ++ri)
        for (uint64_t n : counts)
            for (int pinned = 0; pinned < 2; ++pinned)
                for (int staged_ok = 0; staged_ok < 2; ++staged_ok)
                    for (unsigned nt : {1u, 4u, 16u})
                        for (unsigned ndev : {0u, 1u, 2u, 8u})
                            for (PoolCpus pc : kPools) {
                                const stormck_route_rates& r = kRateSets[ri];
                                const std::string what = "batch rates" + std::to_string(ri) + " n=" + std::to_string(n) +
                                                         " pinned=" + std::to_string(pinned) + " ok=" + std::to_string(staged_ok) +
                                                         " nt=" + std::to_string(nt) + " nd=" + std::to_string(ndev) +
                                                         " pool=" + std::to_string(pc.pool) + "/" + std::to_string(pc.cpus);
                                const LegPlan p = plan_batch(r, n, n * L, L, pinned != 0, staged_ok != 0, nt, ndev, pc.pool, pc.cpus);
                                const Model m = m_batch(r, n, n * L, L, pinned != 0, staged_ok != 0, nt, ndev, pc);
                                expect_plan(what, p, m);
                                if (!ndev || !staged_ok) expect_true(what + " no device leg", std::isinf(p.us[1]) && std::isinf(p.us[2]));
                                if (!pinned || n == 1) expect_true(what + " no split", std::isinf(p.us[2]));
                                splits += p.leg == STORMCK_LEG_SPLIT;
                                devices += p.leg == STORMCK_LEG_DEVICE;
                                hosts += p.leg == STORMCK_LEG_HOST;
                                reduced += ndev && split_threads(pc.pool, pc.cpus, ndev) < pc.pool;
                            }
    expect_true("the batch cases take every leg", splits > 0 && devices > 0 && hosts > 0);
    expect_true("the batch cases take both branches of split_threads", reduced > 0);
    // values worked out by hand: 512 MiB on 4 threads, pageable, one device
    const uint64_t B = 16384 * L;
    const LegPlan p = plan_batch(kBase, 16384, B, L, false, true, 4, 1, 16, 16);
    expect_near("batch host by hand", p.us[0], B / 160000.0 + 10.0);
    expect_near("batch device by hand", p.us[1], 16.0 + L / 1600.0 + B / 50000.0 + (256 << 20) / 55000.0);
    expect_true("split_threads (16, 16, 1) == 15", split_threads(16, 16, 1) == 15);
    expect_true("split_threads (16, 256, 8) == 16", split_threads(16, 256, 8) == 16);
    expect_true("split_threads (4, 4, 8) == 1", split_threads(4, 4, 8) == 1);
    expect_true("split_threads (4, 4, 0) == 4", split_threads(4, 4, 0) == 4);
    expect_true("host_threads_for", host_threads_for(0, 16) == 1 && host_threads_for(3 * 262144 + 5, 16) == 3 &&
                                        host_threads_for(1 << 30, 16) == 16 && host_threads_for(1 << 30, 0) == 1);
}

static CommitShape shape(std::initializer_list<uint64_t> cnt, uint64_t leaf_len, uint64_t upper_len) {
    CommitShape s;
    size_t l = 0;
    for (uint64_t c : cnt) {
        const uint64_t len = l++ == 0 ? leaf_len : upper_len;
        s.cnt.push_back(c);
        s.bytes.push_back(c * len);
        s.longest.push_back(len);
    }
    return s;
}

static void test_commit_times() {
    const CommitShape shapes[] = {
        shape({2, 1}, 31808, 19248),            // storm's smallest commit
        shape({1}, 32768, 0),                   // one block: no split
        shape({100, 10, 1}, 632, 320),          // `-tags test`
        shape({70, 1}, 32768, 19248),
        shape({2047, 2, 1}, 32768, 19248),      // leaves either side of 64 MiB
        shape({2048, 2, 1}, 32768, 19248),
        shape({2049, 2, 1}, 32768, 19248),
        shape({131072, 110, 1}, 32768, 19248),  // 4 GiB of leaves
        CommitShape(),
    };
    int splits = 0, devices = 0, hosts = 0;
    for (size_t ri = 0; ri < sizeof kRateSets / sizeof kRateSets[0]; ++ri)
        for (size_t si = 0; si < sizeof shapes / sizeof shapes[0]; ++si)
            for (int registered = 0; registered < 2; ++registered)
                for (unsigned nt : {1u, 4u, 16u})
                    for (unsigned ndev : {0u, 1u, 2u, 8u})
                        for (PoolCpus pc : kPools) {
                            const stormck_route_rates& r = kRateSets[ri];
                            const CommitShape& s = shapes[si];
                            const std::string what = "commit rates" + std::to_string(ri) + " shape" + std::to_string(si) +
                                                     " reg=" + std::to_string(registered) + " nt=" + std::to_string(nt) +
                                                     " nd=" + std::to_string(ndev) + " pool=" + std::to_string(pc.pool) + "/" +
                                                     std::to_string(pc.cpus);
                            const LegPlan p = plan_commit(r, s, registered != 0, nt, ndev, pc.pool, pc.cpus);
                            expect_plan(what, p, m_commit(r, s, registered != 0, nt, ndev, pc));
                            if (!registered || !ndev) expect_true(what + " no device leg", std::isinf(p.us[1]) && std::isinf(p.us[2]));
                            if (s.cnt.empty() || s.cnt[0] < 2) expect_true(what + " no split", std::isinf(p.us[2]));
                            splits += p.leg == STORMCK_LEG_SPLIT;
                            devices += p.leg == STORMCK_LEG_DEVICE;
                            hosts += p.leg == STORMCK_LEG_HOST;
                        }
    expect_true("the commit cases take every leg", splits > 0 && devices > 0 && hosts > 0);
    // by hand: two leaves and their pointer block on one thread, the device in place
    const LegPlan p = plan_commit(kBase, shapes[0], true, 1, 1, 16, 16);
    expect_near("commit host by hand", p.us[0], 63616 / 40000.0 + 19248 / 40000.0);
    expect_near("commit device by hand", p.us[1], 10.0 + 6.0 + 31808 / 1600.0 + 6.0 + 19248 / 1600.0);
}

// ---- pick_leg -----------------------------------------------------------------------------
static uint32_t picked(double host, double device, double split, double bytes) {
    LegPlan p;
    p.us[0] = host;
    p.us[1] = device;
    p.us[2] = split;
    pick_leg(&p, bytes);
    return p.leg;
}

static void test_pick_leg() {
    const double big = static_cast<double>(kHostCacheBytes) + 1, cached = static_cast<double>(kHostCacheBytes);
    const double eps = 1e-6;
    expect_true("inside kSplitGain", picked(1000, 2000, 1000 * kSplitGain - eps, big) == STORMCK_LEG_SPLIT);
    expect_true("outside kSplitGain", picked(1000, 2000, 1000 * kSplitGain + eps, big) == STORMCK_LEG_HOST);
    expect_true("on kSplitGain", picked(1000, 2000, 1000 * kSplitGain, big) == STORMCK_LEG_HOST);
    expect_true("inside kSplitGainCached", picked(1000, 2000, 1000 * kSplitGainCached - eps, cached) == STORMCK_LEG_SPLIT);
    expect_true("outside kSplitGainCached", picked(1000, 2000, 1000 * kSplitGainCached + eps, cached) == STORMCK_LEG_HOST);
    expect_true("kSplitGain one byte above the cache size", picked(1000, 2000, 900, big) == STORMCK_LEG_SPLIT);
    expect_true("kSplitGainCached at the cache size", picked(1000, 2000, 900, cached) == STORMCK_LEG_HOST);
    // 100 us: the gain allows 95 (80), the saving only 70
    expect_true("inside kSplitMinSaveUs", picked(100, 200, 100 - kSplitMinSaveUs - eps, big) == STORMCK_LEG_SPLIT);
    expect_true("outside kSplitMinSaveUs", picked(100, 200, 100 - kSplitMinSaveUs + eps, big) == STORMCK_LEG_HOST);
    expect_true("on kSplitMinSaveUs", picked(100, 200, 100 - kSplitMinSaveUs, big) == STORMCK_LEG_HOST);
    expect_true("a device that ties the host", picked(1000, 1000, INFINITY, big) == STORMCK_LEG_HOST);
    expect_true("a faster device", picked(1000, 999, INFINITY, big) == STORMCK_LEG_DEVICE);
    expect_true("the split against a faster device", picked(10000, 5000, 5000 * kSplitGain - eps, big) == STORMCK_LEG_SPLIT);
    expect_true("the split loses to a faster device", picked(10000, 5000, 5000 * kSplitGain + eps, big) == STORMCK_LEG_DEVICE);
    expect_true("no device, no split", picked(1000, INFINITY, INFINITY, big) == STORMCK_LEG_HOST);
    expect_near("split_us", split_us(1e6, 40000, 52000, 120, 10, 1e9), (1e6 + 52000 * 120.0) / 92000 + 10);
    expect_true("a split no faster than the host", std::isinf(split_us(1e6, 40000, 52000, 120, 10, 10)));
}

// ---- the host-only bound ------------------------------------------------------------------
static void test_host_only() {
    for (double ht : {40000.0, 48000.0, 24000.0, 40000.03, 39999.97, 1e9 / 3, 6361.6, 2000.0}) {
        const double bound = kHostOnlyUs * ht;
        const uint64_t below = static_cast<uint64_t>(std::ceil(bound)) - 1, above = static_cast<uint64_t>(std::floor(bound)) + 1;
        const std::string what = "host_only ht=" + std::to_string(ht);
        expect_true(what + " one byte below", host_only(ht, below));
        expect_true(what + " one byte above", !host_only(ht, above));
        if (bound == std::floor(bound)) expect_true(what + " on the bound", !host_only(ht, static_cast<uint64_t>(bound)));
        // the form the plan entry points had (a division) and the call's (a byte bound), as the
        // totals cross the bound; the forest form with the total spread over records, and more
        // records behind the bound that the early stop never reads into the sum
        int differ = 0, forest_differ = 0;
        std::vector<stormck_dirty_block> blocks(8);
        std::memset(blocks.data(), 0, blocks.size() * sizeof blocks[0]);
        for (uint64_t total = below - 2000; total <= above + 2000; ++total) {
            const bool division = static_cast<double>(total) / ht < kHostOnlyUs;
            differ += division != host_only(ht, total);
            const uint64_t part = total / 5;
            for (int k = 0; k < 4; ++k) blocks[k].length = static_cast<uint32_t>(std::min<uint64_t>(part, 0xffffffffu));
            const uint64_t rest = total - 4 * uint64_t{blocks[0].length};
            if (rest > 0xffffffffu) continue;
            blocks[4].length = static_cast<uint32_t>(rest);
            forest_differ += host_only(ht, blocks.data(), 5) != host_only(ht, total);
            blocks[5].length = blocks[6].length = blocks[7].length = 0xffffffffu;
            forest_differ += host_only(ht, blocks.data(), 8) != false;
        }
        expect_true(what + " the division and the byte bound agree", differ == 0);
        expect_true(what + " the forest form agrees", forest_differ == 0);
    }
    expect_true("an empty forest is host-only", host_only(40000.0, nullptr, 0) && host_only(40000.0, uint64_t{0}));
    // the decisions hold the shortcut: no device or split time, one thread, whatever the pool
    Pool pool;
    pool.threads = pool.size = pool.cpus = 16;
    Route rt = route_batch(kBase, 3, 399999, 200000, true, true, 1, pool);
    expect_true("route_batch below the bound", rt.plan.leg == STORMCK_LEG_HOST && rt.threads == 1 &&
                                                   std::isinf(rt.plan.us[1]) && std::isinf(rt.plan.us[2]));
    expect_near("route_batch below the bound: host time", rt.plan.us[0], 399999 / 40000.0);
    rt = route_batch(kBase, 3, 400000, 200000, true, true, 1, pool);
    expect_true("route_batch on the bound is planned", std::isfinite(rt.plan.us[1]) && rt.threads == 16);
    CommitShape s = shape({2, 1}, 190000, 19999);
    rt = route_commit(kBase, s, true, 1, pool);
    expect_true("route_commit below the bound", rt.plan.leg == STORMCK_LEG_HOST && rt.threads == 1 &&
                                                    std::isinf(rt.plan.us[1]) && std::isinf(rt.plan.us[2]));
    expect_near("route_commit below the bound: host time", rt.plan.us[0], 399999 / 40000.0);
    s = shape({2, 1}, 190000, 20000);
    rt = route_commit(kBase, s, true, 1, pool);
    expect_true("route_commit on the bound is planned", std::isfinite(rt.plan.us[1]) && rt.threads == 16);
}

// ---- the busy-pool rule -------------------------------------------------------------------
static void test_busy_pool() {
    const PoolCpus pc{16, 16};
    const uint64_t n = 32, L = 32768, B = n * L;  // 1 MiB: four threads' worth
    for (unsigned ndev : {0u, 1u}) {
        const double with_pool = m_batch(kBase, n, B, L, true, true, 16, ndev, pc).best();
        const double alone = m_batch(kBase, n, B, L, true, true, 1, ndev, pc).best();
        expect_true("the pool is faster when free", with_pool + 1 < alone);
        Pool pool;
        pool.threads = pool.size = pool.cpus = 16;
        const double margin = alone - with_pool;
        struct Case {
            double busy;
            unsigned threads;
        } cases[] = {{0.0, 16}, {margin - 0.01, 16}, {margin * 0.5, 16}, {margin + 0.01, 1}, {1e6, 1}};
        for (const Case& c : cases) {
            pool.busy_us = c.busy;
            const Route rt = route_batch(kBase, n, B, L, true, true, ndev, pool);
            const std::string what = "busy batch nd=" + std::to_string(ndev) + " busy=" + std::to_string(c.busy);
            expect_true(what + " threads", rt.threads == c.threads);
            expect_plan(what, rt.plan, m_batch(kBase, n, B, L, true, true, c.threads, ndev, pc));
        }
        pool.threads = 1;  // a call allowed one thread never asks
        pool.busy_us = 0.001;
        expect_true("one thread allowed", route_batch(kBase, n, B, L, true, true, ndev, pool).threads == 1);
        pool.threads = 4;
        pool.busy_us = 0;
        expect_true("four threads allowed", route_batch(kBase, n, B, L, true, true, ndev, pool).threads == 4);
    }
    const CommitShape s = shape({32, 1}, 32768, 19248);
    const double with_pool = m_commit(kBase, s, true, 16, 1, pc).best(), alone = m_commit(kBase, s, true, 1, 1, pc).best();
    expect_true("commit: the pool is faster when free", with_pool + 1 < alone);
    Pool pool;
    pool.threads = pool.size = pool.cpus = 16;
    for (double busy : {0.0, (alone - with_pool) - 0.01, (alone - with_pool) + 0.01}) {
        pool.busy_us = busy;
        const unsigned want = busy < alone - with_pool ? 16 : 1;
        const Route rt = route_commit(kBase, s, true, 1, pool);
        expect_true("busy commit threads busy=" + std::to_string(busy), rt.threads == want);
        expect_plan("busy commit busy=" + std::to_string(busy), rt.plan, m_commit(kBase, s, true, want, 1, pc));
    }
}

// ---- SplitQueue ---------------------------------------------------------------------------
static void test_queue_balanced() {
    const uint64_t n = 1000, huge = UINT64_MAX;
    const double bpb = 32768, r_h = 100000, r_d = 50000;
    uint64_t a = 0, b = 0;
    // the closed form of the header's comment, by hand: R = 32,768,000 bytes, r_o = r_h (one device)
    {
        SplitQueue q(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 1);
        const double R = n * bpb, want = (R / r_h - 120.0 - 0.0 / r_d) / (1.0 / r_d + 1.0 / r_h);
        const uint64_t cnt = static_cast<uint64_t>(want / bpb);
        expect_true("balanced: the first claim by hand is 211 blocks", cnt == 211);
        expect_true("balanced: first claim", q.device(0, 120, huge, &a, &b) && a == n - cnt && b == n);
        // the second, with the first in flight and a chunk's latency
        const double R2 = (n - cnt) * bpb, I = cnt * bpb;
        const double want2 = (R2 / r_h - kSplitChunkUs - I / r_d) / (1.0 / r_d + 1.0 / r_h);
        const uint64_t cnt2 = static_cast<uint64_t>(want2 / bpb);
        expect_true("balanced: second claim", cnt2 > 0 && q.device(I, kSplitChunkUs, huge, &a, &b) && a == n - cnt - cnt2 &&
                                                  b == n - cnt);
        expect_true("balanced: the host takes from the front", q.host(8, &a, &b) && a == 0 && b == 8);
    }
    {  // three devices: the others' rate is the host's and two devices'
        SplitQueue q(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 3);
        const double r_o = r_h + 2 * r_d, want = (n * bpb / r_o - 120.0) / (1.0 / r_d + 1.0 / r_o);
        expect_true("balanced: three devices", q.device(0, 120, huge, &a, &b) && b - a == static_cast<uint64_t>(want / bpb));
    }
    {  // ndev 0 and 1: the same r_o, the same claims
        SplitQueue q0(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 0), q1(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 1);
        for (int k = 0; k < 3; ++k) {
            uint64_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
            const bool g0 = q0.device(k * 1e6, 120, huge, &a0, &b0), g1 = q1.device(k * 1e6, 120, huge, &a1, &b1);
            expect_true("balanced: ndev 0 as ndev 1", g0 == g1 && a0 == a1 && b0 == b1);
        }
    }
    {  // the minimum claim: equal rates of 2^16, no latency: want = R / 2 exactly
        SplitQueue q(64, STORMCK_SPLIT_BALANCED, bpb, 65536, 65536, 1);
        expect_true("balanced: a claim of kSplitMinClaimBytes is taken", q.device(0, 0, huge, &a, &b) && a == 32 && b == 64);
        SplitQueue q2(63, STORMCK_SPLIT_BALANCED, bpb, 65536, 65536, 1);
        expect_true("balanced: a smaller claim ends the device's part", !q2.device(0, 0, huge, &a, &b));
        expect_true("balanced: ... and the host has every block", q2.host(100, &a, &b) && a == 0 && b == 63 && !q2.host(100, &a, &b));
        SplitQueue q3(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 1);
        expect_true("balanced: a latency longer than the call ends it too", !q3.device(0, 1e6, huge, &a, &b));
    }
    {  // max_blocks caps the claim; a claim of less than one block is none
        SplitQueue q(n, STORMCK_SPLIT_BALANCED, bpb, r_h, r_d, 1);
        expect_true("balanced: max_blocks", q.device(0, 120, 10, &a, &b) && a == n - 10 && b == n);
        SplitQueue q2(4, STORMCK_SPLIT_BALANCED, 8.0 * (1 << 20), 65536, 65536, 1);  // want = 16 MiB of 8 MiB blocks: two
        expect_true("balanced: whole blocks", q2.device(0, 0, huge, &a, &b) && a == 2 && b == 4);
        SplitQueue q3(1, STORMCK_SPLIT_BALANCED, 3.0 * (1 << 20), 65536, 65536, 1);  // want = 1.5 MiB: under a block
        expect_true("balanced: under one block", !q3.device(0, 0, huge, &a, &b));
    }
    {  // r_o <= 0: nobody else hashes, the device takes everything (in chunks of max_blocks)
        SplitQueue q(n, STORMCK_SPLIT_BALANCED, bpb, 0, r_d, 1);
        expect_true("balanced: r_o = 0 takes max_blocks", q.device(0, 120, 400, &a, &b) && a == 600 && b == 1000);
        expect_true("balanced: r_o = 0 takes the rest", q.device(0, 120, huge, &a, &b) && a == 0 && b == 600);
        expect_true("balanced: nothing left", !q.device(0, 120, huge, &a, &b) && !q.host(8, &a, &b));
        SplitQueue q2(n, STORMCK_SPLIT_BALANCED, bpb, -1, r_d, 0);
        expect_true("balanced: r_o < 0", q2.device(0, 120, huge, &a, &b) && a == 0 && b == n);
    }
}

static void test_queue_fixed() {
    uint64_t a = 0, b = 0;
    {
        SplitQueue q(100, 37, 32768, 100000, 50000, 1);
        const uint64_t want[][2] = {{90, 100}, {80, 90}, {70, 80}, {63, 70}};
        for (auto& w : want) expect_true("fixed: device chunk", q.device(0, 120, 10, &a, &b) && a == w[0] && b == w[1]);
        expect_true("fixed: the devices' part is over", !q.device(0, 120, 10, &a, &b));
        expect_true("fixed: host piece", q.host(40, &a, &b) && a == 0 && b == 40);
        expect_true("fixed: host piece ends at the boundary", q.host(40, &a, &b) && a == 40 && b == 63);
        expect_true("fixed: the host's part is over", !q.host(40, &a, &b));
    }
    for (uint64_t fixed : {uint64_t{100}, uint64_t{101}, uint64_t{1} << 40, UINT64_MAX - 1}) {  // fixed > n as fixed == n
        SplitQueue q(100, fixed, 32768, 100000, 50000, 1);
        expect_true("fixed >= n: the host gets nothing", !q.host(8, &a, &b));
        expect_true("fixed >= n: the devices get all", q.device(0, 120, 1000, &a, &b) && a == 0 && b == 100 &&
                                                           !q.device(0, 120, 1000, &a, &b));
    }
    {
        SplitQueue q(100, 0, 32768, 100000, 50000, 1);
        expect_true("fixed 0: the devices get nothing", !q.device(0, 120, 10, &a, &b));
        expect_true("fixed 0: the host gets all", q.host(1000, &a, &b) && a == 0 && b == 100 && !q.host(1000, &a, &b));
    }
    {
        SplitQueue q(0, 0, 1, 100000, 50000, 1);
        expect_true("an empty queue", !q.device(0, 120, 10, &a, &b) && !q.host(8, &a, &b));
        SplitQueue q2(0, STORMCK_SPLIT_BALANCED, 1, 100000, 50000, 1);
        expect_true("an empty balanced queue", !q2.device(0, 120, 10, &a, &b) && !q2.host(8, &a, &b));
    }
}

struct Claim {
    uint64_t a, b;
    bool device;
};

// 8 threads call host() and 3 call device() on one queue until each is refused.
static void run_concurrent(const std::string& what, uint64_t n, uint64_t fixed, double r_host, bool covers) {
    SplitQueue q(n, fixed, 32768, r_host, 50000, 3);
    std::vector<std::vector<Claim>> got(11);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 11; ++t)
        th.emplace_back([&, t] {
            uint64_t a = 0, b = 0;
            double inflight = 0;
            if (t < 8) {
                while (q.host(1 + t, &a, &b)) got[t].push_back({a, b, false});
            } else {
                while (q.device(inflight, inflight > 0 ? kSplitChunkUs : 120.0, 64 + t, &a, &b)) {
                    got[t].push_back({a, b, true});
                    inflight = (b - a) * 32768.0;
                }
            }
        });
    for (auto& x : th) x.join();
    std::vector<uint8_t> seen(n, 0);
    uint64_t overlaps = 0, out_of_range = 0, covered = 0, device_blocks = 0, misplaced = 0;
    const uint64_t boundary = fixed == STORMCK_SPLIT_BALANCED ? 0 : n - std::min(fixed, n);
    auto take = [&](const Claim& c) {
        if (c.a >= c.b || c.b > n) {
            ++out_of_range;
            return;
        }
        for (uint64_t i = c.a; i < c.b; ++i) {
            overlaps += seen[i];
            seen[i] = 1;
        }
        covered += c.b - c.a;
        if (c.device) device_blocks += c.b - c.a;
        if (fixed != STORMCK_SPLIT_BALANCED) misplaced += c.device ? c.a < boundary : c.b > boundary;
    };
    for (auto& v : got)
        for (const Claim& c : v) take(c);
    expect_true(what + ": claims in range", out_of_range == 0);
    expect_true(what + ": claims disjoint", overlaps == 0);
    if (covers) expect_true(what + ": the threads' claims cover [0, n)", covered == n);
    if (fixed != STORMCK_SPLIT_BALANCED) {
        expect_true(what + ": the devices got exactly the last blocks", device_blocks == n - boundary && misplaced == 0);
    }
    // what is left is what the host loop would take: drain it, then everything is covered
    uint64_t a = 0, b = 0;
    while (q.host(1000, &a, &b)) take({a, b, false});
    expect_true(what + ": covered after the host drains", covered == n && overlaps == 0);
    expect_true(what + ": the queue is empty", !q.host(1, &a, &b) && (fixed != STORMCK_SPLIT_BALANCED || !q.device(0, 0, 1, &a, &b)));
}

static void test_queue_concurrent() {
    for (uint64_t n : {uint64_t{1}, uint64_t{7}, uint64_t{100003}}) {
        const std::string s = " n=" + std::to_string(n);
        run_concurrent("fixed third" + s, n, n / 3, 100000, true);
        run_concurrent("fixed all" + s, n, n + 5, 100000, true);
        run_concurrent("fixed none" + s, n, 0, 100000, true);
        run_concurrent("balanced, r_o <= 0" + s, n, STORMCK_SPLIT_BALANCED, -200000, true);  // r_o = r_host + 2 r_dev
        run_concurrent("balanced" + s, n, STORMCK_SPLIT_BALANCED, 100000, false);
    }
}

// ---- RouteModel ---------------------------------------------------------------------------
static bool same(const stormck_route_rates& x, const stormck_route_rates& y) {
    return x.host_thread == y.host_thread && x.host_memory == y.host_memory && x.host_cached == y.host_cached &&
           x.link_pinned == y.link_pinned && x.link_pageable == y.link_pageable && x.link_inplace == y.link_inplace &&
           x.device_latency == y.device_latency && x.observations == y.observations;
}
static double m_ewma(double old, double obs) { return old + kLearnWeight * (obs - old); }

static void test_model() {
    const uint64_t MiB = 1 << 20;
    for (bool x4 : {false, true}) {
        RouteModel m(x4);
        const stormck_route_rates p = m.now();
        expect_true("priors", p.host_thread == (x4 ? kPriorHostThreadX4 : kPriorHostThread) && p.host_memory == kPriorHostMemory &&
                                  p.host_cached == kPriorHostMemory && p.link_pinned == kPriorLinkPinned &&
                                  p.link_pageable == kPriorLinkPageable && p.link_inplace == kPriorLinkInplace &&
                                  p.device_latency == kPriorDeviceLatencyUs && p.observations == 0);
        expect_true("host_thread() reads the prior", m.host_thread() == p.host_thread);
        stormck_route_rates r = kBase;
        r.observations = 77;
        m.set(&r, false);
        r.observations = 0;
        expect_true("set with rates", same(m.now(), r) && m.host_thread() == r.host_thread);
        m.learn_host(16 * MiB, 1, 400);
        expect_true("set without freeze learns", m.now().observations == 1);
        m.set(nullptr, false);
        expect_true("set(nullptr) is the priors again", same(m.now(), p) && m.host_thread() == p.host_thread);
    }
    {  // freeze blocks every learner
        RouteModel m(true);
        m.set(&kBase, true);
        m.learn_host(16 * MiB, 1, 400);
        m.learn_host(16 * MiB, 4, 400);
        m.learn_host(128 * MiB, 4, 1e6);
        m.learn_link(Link::kPinned, 128 * MiB, 1000);
        m.learn_link(Link::kPageable, 128 * MiB, 1000);
        m.learn_link(Link::kInplace, 128 * MiB, 1000);
        m.learn_latency(MiB, 50000, 1e6);
        expect_true("a frozen model does not move", same(m.now(), kBase) && m.host_thread() == kBase.host_thread);
    }
    {  // learn_host: the three branches, the 8 MiB floor, the two caps
        RouteModel m(true);
        m.set(&kBase, false);
        stormck_route_rates want = kBase;
        m.learn_host(8 * MiB - 1, 1, 100);
        m.learn_host(16 * MiB, 1, 0);
        m.learn_host(16 * MiB, 4, -5);
        expect_true("learn_host: below 8 MiB or without a time nothing is learned", same(m.now(), want));
        m.learn_host(8 * MiB, 1, 400);  // one thread: the per-thread rate
        want.host_thread = m_ewma(want.host_thread, 8.0 * MiB / 400);
        want.observations++;
        expect_true("learn_host: one thread at the floor", same(m.now(), want) && m.host_thread() == want.host_thread);
        // four threads at more than 0.8 x 4 x host_thread: the threads' rate, and the cap is raised to it
        double rate = 32.0 * MiB / (110 - kHostLevelUs);
        expect_true("(the case runs at the threads' rate)", rate >= 0.8 * 4 * want.host_thread && rate > want.host_cached);
        m.learn_host(32 * MiB, 4, 110);
        want.host_thread = m_ewma(want.host_thread, rate / 4);
        want.host_cached = rate;
        want.observations++;
        expect_true("learn_host: a pool pass at the threads' rate (cached cap)", same(m.now(), want) && m.host_thread() == want.host_thread);
        // the same above 64 MiB: the memory cap, and a cap already higher stays
        rate = 128.0 * MiB / (1000 - kHostLevelUs);
        expect_true("(the case runs at the threads' rate, below the cap)", rate >= 0.8 * 2 * want.host_thread && rate < want.host_memory);
        m.learn_host(128 * MiB, 2, 1000);
        want.host_thread = m_ewma(want.host_thread, rate / 2);
        want.observations++;
        expect_true("learn_host: ... the memory cap is never lowered by it", same(m.now(), want));
        // below the threads' rate: the cap moves, each apart from the other
        rate = 64.0 * MiB / (2000 - kHostLevelUs);
        expect_true("(the case runs below the threads' rate)", rate < 0.8 * 16 * want.host_thread);
        m.learn_host(64 * MiB, 16, 2000);
        want.host_cached = m_ewma(want.host_cached, rate);
        want.observations++;
        expect_true("learn_host: a capped pass of 64 MiB moves host_cached", same(m.now(), want));
        rate = (64.0 * MiB + 1) / (2000 - kHostLevelUs);
        m.learn_host(64 * MiB + 1, 16, 2000);
        want.host_memory = m_ewma(want.host_memory, rate);
        want.observations++;
        expect_true("learn_host: one byte more moves host_memory", same(m.now(), want));
        m.learn_host(64 * MiB + 1, 16, 5);  // a time under the fork/join counts as 1 us
        want.host_thread = m_ewma(want.host_thread, (64.0 * MiB + 1) / 16);
        want.host_memory = 64.0 * MiB + 1;
        want.observations++;
        expect_true("learn_host: at least 1 us", same(m.now(), want));
    }
    for (double share : {0.79, 0.81}) {  // either side of 0.8 x threads x host_thread
        RouteModel m(true);
        m.set(&kBase, false);
        stormck_route_rates want = kBase;
        const double us = 32.0 * MiB / (share * 4 * kBase.host_thread) + kHostLevelUs, rate = 32.0 * MiB / (us - kHostLevelUs);
        m.learn_host(32 * MiB, 4, us);
        if (share > 0.8) want.host_thread = m_ewma(want.host_thread, rate / 4);  // the cap is higher already
        else want.host_cached = m_ewma(want.host_cached, rate);
        want.observations++;
        expect_true("learn_host: " + std::to_string(share) + " of the threads' rate", same(m.now(), want));
    }
    {  // learn_link
        RouteModel m(false);
        m.set(&kBase, false);
        stormck_route_rates want = kBase;
        m.learn_link(Link::kPinned, 64 * MiB - 1, 1000);
        m.learn_link(Link::kInplace, 128 * MiB, 0);
        m.learn_link(Link::kPageable, 128 * MiB, -1);
        expect_true("learn_link: below 64 MiB or without a time nothing is learned", same(m.now(), want));
        m.learn_link(Link::kPinned, 64 * MiB, 1000);
        want.link_pinned = m_ewma(want.link_pinned, 64.0 * MiB / 1000);
        want.observations++;
        expect_true("learn_link: pinned at the floor", same(m.now(), want));
        m.learn_link(Link::kPageable, 128 * MiB, 3000);
        want.link_pageable = m_ewma(want.link_pageable, 128.0 * MiB / 3000);
        want.observations++;
        expect_true("learn_link: pageable", same(m.now(), want));
        m.learn_link(Link::kInplace, 256 * MiB, 4000);
        want.link_inplace = m_ewma(want.link_inplace, 256.0 * MiB / 4000);
        want.observations++;
        expect_true("learn_link: in place", same(m.now(), want) && m.host_thread() == kBase.host_thread);
    }
    {  // learn_latency
        RouteModel m(false);
        m.set(&kBase, false);
        stormck_route_rates want = kBase;
        m.learn_latency(MiB, 50000, 0);
        m.learn_latency(MiB, 0, 100);
        m.learn_latency(MiB, -1, 100);
        expect_true("learn_latency: without a time or a rate nothing is learned", same(m.now(), want));
        m.learn_latency(MiB, 50000, 200);  // an ordinary observation: 200 us less the bytes over the link
        want.device_latency = m_ewma(want.device_latency, 200 - 1.0 * MiB / 50000);
        want.observations++;
        expect_true("learn_latency: the time less the link's", same(m.now(), want));
        const double lat = want.device_latency;
        m.learn_latency(0, 50000, 1e7);  // a spike of 10 s
        const double moved = m.now().device_latency - lat;
        expect_true("learn_latency: a spike moves it by at most kLearnWeight x (lat + 100)",
                    moved > 0 && moved <= kLearnWeight * (2 * lat + 100 - lat) * (1 + 1e-12));
        want.device_latency = m_ewma(lat, 2 * lat + 100);
        want.observations++;
        expect_true("learn_latency: the clamp", same(m.now(), want));
        m.learn_latency(100 * MiB, 50000, 5);  // less than the link's time: the floor of 1 us
        want.device_latency = m_ewma(want.device_latency, 1.0);
        want.observations++;
        expect_true("learn_latency: the floor of 1 us", same(m.now(), want));
        expect_true("observations count the accepted ones", m.now().observations == 3);
    }
    {  // four threads at once: readers and every learner (ThreadSanitizer's case)
        RouteModel m(true);
        const int rounds = 2000;
        std::vector<std::thread> th;
        std::atomic<int> odd{0};
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                for (int k = 0; k < rounds; ++k) {
                    const stormck_route_rates r = m.now();
                    if (!(r.host_thread > 0 && m.host_thread() > 0 && r.device_latency >= 1)) odd.fetch_add(1);
                    switch ((k + t) % 4) {
                        case 0: m.learn_host(16 * MiB, 1 + (k % 3), 300 + k % 7); break;
                        case 1: m.learn_link(static_cast<Link>(k % 3), 128 * MiB, 2000 + k % 11); break;
                        case 2: m.learn_latency(MiB, 50000, 100 + k % 13); break;
                        default: m.learn_host(MiB, 1, 10); break;  // refused: too small
                    }
                }
            });
        for (auto& x : th) x.join();
        expect_true("concurrent: every read saw sane rates", odd.load() == 0);
        expect_true("concurrent: observations count the accepted ones", m.now().observations == 4ull * rounds * 3 / 4);
    }
}

int main() {
    test_batch_times();
    test_commit_times();
    test_pick_leg();
    test_host_only();
    test_busy_pool();
    test_queue_balanced();
    test_queue_fixed();
    test_queue_concurrent();
    test_model();
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
