// The commit's forest planning (storm_amd/csrc/commit_plan.h) against a small reference
// model written here, on a serial executor and on std::thread executors of 1, 2, 5 and 16
// parts; its error rules; and the level-0 chunk schedule against a table worked out by hand
// from the loop the schedule replaced. No GPU and no library.
//     commit_plan_test [big [full]]   big: the largest forest (default 300,000 blocks);
//                                     full: the largest that takes every check (default 16,385)
#include "../../storm_amd/csrc/commit_plan.h"

#include <condition_variable>
#include <cstdio>
#include <functional>
#include <mutex>
#include <numeric>
#include <random>
#include <string>
#include <thread>

using namespace stormck;
using Forest = std::vector<stormck_dirty_block>;

static int failures = 0;
static void expect_true(const std::string& what, bool ok) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
}

static auto serial = [](uint64_t count, auto&& fn) {
    fn(0u, uint64_t{0}, count);
    return 1u;
};
// `parts` parts whatever the count (some may be empty), each on a thread of its own: 16
// workers started once (a thread per part and pass is most of the run time under TSan)
class Workers {
  public:
    Workers() {
        for (unsigned t = 0; t < 16; ++t) th_.emplace_back([this, t] { loop(t); });
    }
    ~Workers() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        go_.notify_all();
        for (auto& x : th_) x.join();
    }
    void run(unsigned parts, const std::function<void(unsigned)>& job) {
        std::unique_lock<std::mutex> g(mu_);
        job_ = &job;
        parts_ = parts;
        left_ = 16;
        ++gen_;
        go_.notify_all();
        done_.wait(g, [&] { return left_ == 0; });
    }

  private:
    void loop(unsigned t) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
            go_.wait(g, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            const std::function<void(unsigned)>* job = job_;
            const bool mine = t < parts_;
            g.unlock();
            if (mine) (*job)(t);
            g.lock();
            if (--left_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable go_, done_;
    const std::function<void(unsigned)>* job_ = nullptr;
    unsigned parts_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};
struct Threads {
    unsigned parts;
    template <class F>
    unsigned operator()(uint64_t count, F&& fn) const {
        static Workers workers;
        workers.run(parts, [&](unsigned t) { fn(t, count * t / parts, count * (t + 1) / parts); });
        return parts;
    }
};

// ---- forests -----------------------------------------------------------------------------
constexpr uint64_t kRevision = 9;

static stormck_dirty_block record(uint64_t i, int64_t parent, std::mt19937_64& rng) {
    stormck_dirty_block b{};
    b.data_offset = 1024 * (i + 1) + (i % 7 == 3 ? 8 : 0);  // some rows off 16 bytes
    b.origin_pointer = parent < 0 ? 32 : 1024 * static_cast<uint64_t>(parent + 1) + 24 * (i % 40);
    b.origin_type = b.origin_pointer + 1000;
    b.parent = parent;
    b.address = 100 + i;
    b.birth_revision = kRevision + 1;
    b.length = static_cast<uint32_t>(rng() % 5 == 0 ? 0 : 72 + rng() % 900);  // some records hash nothing
    b.type = parent < 0 ? STORMCK_POINTER_BLOCK : STORMCK_LEAF_BLOCK;
    return b;
}

// A `fanout`-ary heap with `roots` roots, children first: leaves are a prefix and heights
// never fall with the index, so the commit order is the identity.
static Forest heap(uint64_t n, uint64_t fanout, uint64_t roots, std::mt19937_64& rng) {
    Forest f(n);
    roots = std::min(roots, n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t j = n - 1 - i;  // the root side's index
        f[i] = record(i, j < roots ? STORMCK_NO_PARENT : static_cast<int64_t>(n - 1 - (j - roots) / fanout), rng);
    }
    return f;
}
// Every block's parent is a random later block (or none): leaves at any depth, level 0
// nowhere near a prefix.
static Forest ragged(uint64_t n, std::mt19937_64& rng) {
    Forest f(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t left = n - 1 - i;
        f[i] = record(i, left == 0 || rng() % 16 == 0 ? STORMCK_NO_PARENT : static_cast<int64_t>(i + 1 + rng() % std::min<uint64_t>(left, 40)), rng);
    }
    return f;
}
static Forest chain(uint64_t n, std::mt19937_64& rng) {  // height n - 1
    Forest f(n);
    for (uint64_t i = 0; i < n; ++i) f[i] = record(i, i + 1 < n ? static_cast<int64_t>(i + 1) : STORMCK_NO_PARENT, rng);
    return f;
}
// Permute the blocks from index `from` on and remap the parents.
static Forest shuffled(const Forest& f, uint64_t from, std::mt19937_64& rng) {
    const uint64_t n = f.size();
    std::vector<uint64_t> perm(n), inv(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin() + static_cast<std::ptrdiff_t>(std::min(from, n)), perm.end(), rng);
    for (uint64_t i = 0; i < n; ++i) inv[perm[i]] = i;
    Forest g(n);
    for (uint64_t i = 0; i < n; ++i) {
        g[i] = f[perm[i]];
        if (g[i].parent >= 0) g[i].parent = static_cast<int64_t>(inv[static_cast<uint64_t>(g[i].parent)]);
    }
    return g;
}
static void relocating(Forest* f, int how, std::mt19937_64& rng) {  // 0 none, 1 a third, 2 all
    for (auto& b : *f)
        if (how == 2 || (how == 1 && rng() % 3 == 0)) b.birth_revision = rng() % 2 ? kRevision : 3;
}

// ---- the reference model -------------------------------------------------------------------
struct Model {
    std::vector<uint32_t> height, order;
    std::vector<uint64_t> level_start;
    CommitShape shape;
    Forest after;
    uint64_t last;
};
// height = the longest distance to a descendant (children report to their parent once all of
// theirs have), order = a stable sort by height, relocation in that order
static Model model(const Forest& f, uint64_t last) {
    const uint64_t n = f.size();
    Model m;
    m.height.assign(n, 0);
    std::vector<uint32_t> waiting(n, 0), ready;
    for (const auto& b : f)
        if (b.parent >= 0) waiting[static_cast<uint64_t>(b.parent)]++;
    for (uint64_t i = 0; i < n; ++i)
        if (!waiting[i]) ready.push_back(static_cast<uint32_t>(i));
    for (size_t q = 0; q < ready.size(); ++q) {
        const uint32_t i = ready[q];
        if (f[i].parent < 0) continue;
        const uint64_t p = static_cast<uint64_t>(f[i].parent);
        m.height[p] = std::max(m.height[p], m.height[i] + 1);
        if (--waiting[p] == 0) ready.push_back(static_cast<uint32_t>(p));
    }
    m.order.resize(n);
    std::iota(m.order.begin(), m.order.end(), 0u);
    std::stable_sort(m.order.begin(), m.order.end(), [&](uint32_t a, uint32_t b) { return m.height[a] < m.height[b]; });
    const uint32_t max_h = *std::max_element(m.height.begin(), m.height.end());
    m.level_start.assign(max_h + 2, 0);
    m.shape.cnt.assign(max_h + 1, 0);
    m.shape.bytes.assign(max_h + 1, 0);
    m.shape.longest.assign(max_h + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t h = m.height[i];
        m.level_start[h + 1]++;
        m.shape.cnt[h]++;
        m.shape.bytes[h] += f[i].length;
        m.shape.longest[h] = std::max<uint64_t>(m.shape.longest[h], f[i].length);
    }
    for (uint32_t h = 0; h <= max_h; ++h) m.level_start[h + 1] += m.level_start[h];
    m.after = f;
    m.last = last;
    for (uint32_t i : m.order)
        if (m.after[i].birth_revision <= kRevision) {
            m.after[i].address = ++m.last;
            m.after[i].birth_revision = kRevision + 1;
        }
    return m;
}

static bool same(const Forest& a, const Forest& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(stormck_dirty_block)) == 0;
}

// The planner on one executor against the model. in_chunks: as the device leg runs it (level
// 0's order, its chunks staged one by one, then the upper order and the upper part); else
// as the host legs do (the whole order, one range).
template <class Par>
static void check(const std::string& what, const Forest& given, const Model& m, Par par, bool in_chunks) {
    const uint64_t n = given.size();
    Forest f = given;
    Heights H;
    const CommitError e = commit_heights(f.data(), n, kRevision, par, &H);
    expect_true(what + ": well formed", e == CommitError::Ok);
    if (e != CommitError::Ok) return;
    expect_true(what + ": nothing written by the walk", same(f, given));
    expect_true(what + ": height[]", std::equal(m.height.begin(), m.height.end(), H.height()));
    uint64_t reloc = 0;
    uint32_t longest = 0;
    bool off16 = false;
    for (const auto& b : given) {
        reloc += b.birth_revision <= kRevision;
        longest = std::max(longest, b.length);
        off16 |= (b.data_offset & 15) != 0;
    }
    const uint64_t n0 = m.level_start[1];
    bool prefix = true;
    for (uint64_t i = 0; i < n; ++i) prefix &= (m.height[i] == 0) == (i < n0);
    expect_true(what + ": counts", H.n == n && H.relocating == reloc && H.n0() == n0 && H.longest == longest &&
                                       H.data_off16 == off16 && H.prefix0() == prefix);
    CommitShape s;
    commit_shape(H, f.data(), n, &s);
    expect_true(what + ": shape", s.cnt == m.shape.cnt && s.bytes == m.shape.bytes && s.longest == m.shape.longest);

    CommitOrder O;
    uint64_t last = 1000;
    Forest staged(n);
    std::vector<uint8_t> seen(n, 0);
    auto emit = [&](uint64_t k, const stormck_dirty_block& r) {
        staged[k] = r;
        seen[k]++;
    };
    if (in_chunks) {
        order_level0(H, par, &O);
        expect_true(what + ": level 0's order comes first", O.order.empty() == prefix);
        uint64_t covered = 0;
        for (uint64_t lo = 0, cnt, next = 300; lo < n0; lo += cnt, next = cnt * 2, covered += cnt) {
            cnt = level0_chunk(n0 - lo, next);
            expect_true(what + ": a chunk is some of the rest", cnt > 0 && cnt <= n0 - lo);
            relocate_range(f.data(), O, lo, lo + cnt, kRevision, H.relocating != 0, &last, par, emit);
        }
        expect_true(what + ": chunks cover level 0", covered == n0);
        order_upper(H, par, &O);
        relocate_range(f.data(), O, n0, n, kRevision, H.relocating != 0, &last, par, emit);
    } else {
        commit_order(H, par, &O);
        relocate_range(f.data(), O, 0, n, kRevision, H.relocating != 0, &last, par, emit);
    }
    bool identity = true, order_ok = true, staged_ok = true, once = true;
    for (uint64_t k = 0; k < n; ++k) {
        identity &= m.order[k] == k;
        order_ok &= O.at(k) == m.order[k];
        once &= seen[k] == 1;
        staged_ok &= std::memcmp(&staged[k], &m.after[m.order[k]], sizeof staged[k]) == 0;
    }
    expect_true(what + ": order", order_ok && O.order.empty() == identity);
    expect_true(what + ": level_start", O.level_start == m.level_start && H.max_h + 2 == m.level_start.size());
    expect_true(what + ": relocated records and last", same(f, m.after) && last == m.last);
    expect_true(what + ": every position emitted once, relocated", once && staged_ok);
}

// light: a third relocating, on the serial executor and on 5 and 16 threads only
static void check_all(const std::string& what, Forest f, std::mt19937_64& rng, bool light) {
    for (int how : {1, 0, 2}) {
        relocating(&f, how, rng);
        const Model m = model(f, 1000);
        const std::string w = what + " n=" + std::to_string(f.size()) + " reloc=" + std::to_string(how);
        check(w + " serial", f, m, serial, false);
        check(w + " threads=5 one range", f, m, Threads{5}, false);
        check(w + " threads=16", f, m, Threads{16}, true);
        if (light) return;
        check(w + " serial chunks", f, m, serial, true);
        for (unsigned parts : {1u, 2u, 5u}) check(w + " threads=" + std::to_string(parts), f, m, Threads{parts}, true);
    }
}

// Every kind, relocation and executor up to `full` blocks (1 to 16,385); the big one takes the
// light checks of three kinds.
static void forests(uint64_t big, uint64_t full) {
    std::mt19937_64 rng(7);
    for (uint64_t n : {uint64_t{1}, uint64_t{2}, uint64_t{11}, uint64_t{999}, uint64_t{16383}, uint64_t{16384},
                       uint64_t{16385}, big}) {
        const bool light = n > full;
        for (uint64_t roots : {uint64_t{1}, uint64_t{3}}) {
            const Forest f = heap(n, n > 20000 ? 100 : 10, roots, rng);
            const uint64_t n0 = model(f, 0).level_start[1];
            const std::string r = " roots=" + std::to_string(roots);
            if (!light || roots == 1) check_all("children first" + r, f, rng, light);
            if (!light) check_all("upper shuffled" + r, shuffled(f, n0, rng), rng, light);
            if (!light || roots == 3) check_all("shuffled" + r, shuffled(f, 0, rng), rng, light);
        }
        const Forest g = ragged(n, rng);
        if (!light) check_all("ragged", g, rng, light);
        check_all("ragged shuffled", shuffled(g, 0, rng), rng, light);
        if (!light) {
            const Forest c = chain(n, rng);
            check_all("chain", c, rng, light);
            check_all("chain shuffled", shuffled(c, 0, rng), rng, light);
        }
    }
}

// ---- errors ----------------------------------------------------------------------------------
template <class Par>
static void expect_error(const std::string& what, const Forest& bad, Par par, CommitError want) {
    Forest f = bad;
    Heights H;
    const CommitError e = commit_heights(f.data(), f.size(), kRevision, par, &H);
    expect_true(what + ": " + commit_error_message(want) + " (got '" + commit_error_message(e) + "')", e == want);
    expect_true(what + ": records untouched", same(f, bad));
}
static void expect_error_everywhere(const std::string& what, const Forest& bad, CommitError want) {
    expect_error(what + " serial", bad, serial, want);
    for (unsigned parts : {1u, 2u, 5u, 16u}) expect_error(what + " threads=" + std::to_string(parts), bad, Threads{parts}, want);
}

static void errors() {
    std::mt19937_64 rng(3);
    const Forest good = heap(29, 10, 1, rng);  // 25 leaves, 3 pointer blocks, the root
    const uint64_t root = 28;
    Forest f = good;
    f[3].parent = 1000000;
    expect_error_everywhere("parent too large", f, CommitError::ParentRange);
    f = good;
    f[3].parent = 29;
    expect_error_everywhere("parent = n", f, CommitError::ParentRange);
    f = good;
    f[3].parent = -2;
    expect_error_everywhere("parent -2", f, CommitError::ParentRange);
    f = good;
    f[root].parent = INT64_MIN;
    expect_error_everywhere("an ancestor's parent below zero", f, CommitError::ParentRange);
    f = good;
    f[3].origin_pointer = 1028;
    expect_error_everywhere("origin off 8", f, CommitError::OriginAlign);
    f = good;
    f[3].origin_pointer = STORMCK_NO_ORIGIN;  // not an address: no alignment asked
    expect_error_everywhere("no origin", f, CommitError::Ok);
    f = good;
    f[5].parent = 5;
    expect_error_everywhere("1-cycle", f, CommitError::Cycle);
    f = good;
    f[25].parent = 26;
    f[26].parent = 25;
    expect_error_everywhere("2-cycle", f, CommitError::Cycle);
    f = good;
    f[root].parent = 3;  // root -> leaf 3 -> ... -> root
    expect_error_everywhere("cycle through the root", f, CommitError::Cycle);
    f = good;
    for (uint64_t i = 0; i < f.size(); ++i) f[i].parent = static_cast<int64_t>((i + 1) % f.size());
    expect_error_everywhere("every block has a dirty child", f, CommitError::Cycle);
    f.assign(1, good[0]);
    f[0].parent = 0;
    expect_error_everywhere("one block, its own parent", f, CommitError::Cycle);

    // n > 2^32 - 1 is refused by its argument alone: nothing is read or allocated
    Heights H;
    expect_true("2^32 blocks", commit_heights(nullptr, uint64_t{1} << 32, kRevision, serial, &H) == CommitError::TooMany);
    expect_true("2^40 blocks", commit_heights(nullptr, uint64_t{1} << 40, kRevision, Threads{5}, &H) == CommitError::TooMany);
    expect_true("no height array for them", H.height() == nullptr);

    // two defects, one part: the lower index's
    f = good;
    f[3].origin_pointer = 1028;
    f[7].parent = 1000000;
    expect_error("origin then range", f, serial, CommitError::OriginAlign);
    expect_error("origin then range, one thread", f, Threads{1}, CommitError::OriginAlign);
    f = good;
    f[3].parent = 1000000;
    f[7].origin_pointer = 1028;
    expect_error("range then origin", f, serial, CommitError::ParentRange);
    f = good;
    f[0].parent = 1;
    f[1].parent = 0;
    f[20].parent = 1000000;
    expect_error("cycle then range", f, serial, CommitError::Cycle);
    f = good;
    f[2].parent = 1000000;
    f[10].parent = 11;
    f[11].parent = 10;
    expect_error("range then cycle", f, serial, CommitError::ParentRange);
    f = good;
    f[4].origin_pointer = 1028;
    f[root].parent = 0;  // block 0's walk is the first to fail
    expect_error("cycle through the root then origin", f, serial, CommitError::Cycle);

    expect_true("messages", std::string(commit_error_message(CommitError::TooMany)) == "more than 2^32 dirty blocks" &&
                                std::string(commit_error_message(CommitError::ParentRange)) == "parent index out of range" &&
                                std::string(commit_error_message(CommitError::OriginAlign)) ==
                                    "origin_pointer must be 8-byte aligned (Go blocks.Pointer alignment)" &&
                                std::string(commit_error_message(CommitError::Cycle)) == "parent links form a cycle");
}

// ---- the level-0 chunk schedule ------------------------------------------------------------
static void expect_chunks(uint64_t n0, uint64_t first, uint64_t growth, const std::vector<uint64_t>& want) {
    std::vector<uint64_t> got;  // as the device leg walks level 0
    for (uint64_t lo = 0, cnt, next = first; lo < n0; lo += cnt, next = cnt * growth) {
        cnt = level0_chunk(n0 - lo, next);
        if (cnt == 0 || cnt > n0 - lo) break;
        got.push_back(cnt);
    }
    std::string g;
    for (uint64_t c : got) g += " " + std::to_string(c);
    expect_true("chunks of " + std::to_string(n0) + " from " + std::to_string(first) + " x" + std::to_string(growth) +
                    ": got" + g,
                got == want);
}

static void chunk_table() {
    const Knobs k{};
    expect_true("shipped schedule", k.commit_first == 32768 && k.commit_growth == 3 && kStreamBatch == 16384);
    // a chunk is min(next, rest), or all of the rest when fewer than 16,384 would remain;
    // next = 3 x the chunk
    expect_chunks(1, 32768, 3, {1});
    expect_chunks(16384, 32768, 3, {16384});
    expect_chunks(32768, 32768, 3, {32768});
    expect_chunks(32768 + 16383, 32768, 3, {49151});        // 16,383 would remain: one chunk
    expect_chunks(32768 + 16384, 32768, 3, {32768, 16384});  // 16,384 remain: a chunk of their own
    expect_chunks(140000, 32768, 3, {32768, 107232});        // 98,304 would leave 8,928
    expect_chunks(1048576, 32768, 3, {32768, 98304, 294912, 622592});  // 884,736 is more than the rest
    expect_chunks(20000, 4096, 2, {20000});                  // 4,096 would leave 15,904
    expect_chunks(20480, 4096, 2, {4096, 16384});            // 8,192 would leave 8,192
    expect_chunks(100000, 4096, 2, {4096, 8192, 16384, 32768, 38560});
    expect_true("one piece", !commit_one_piece(0, 4096) && commit_one_piece(1, 4096) && !commit_one_piece(0, 4097) &&
                                 !commit_one_piece(1, 4097) && commit_one_piece(3, 1));
}

int main(int argc, char** argv) {
    const uint64_t big = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300000;
    forests(big, argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 16385);
    errors();
    chunk_table();
    std::printf("ok: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
