// The forest planning of a commit (storm's Cache.Commit), once for every leg of libstormck:
// validation and heights, the per-height shape the router prices, the commit order, the
// relocation in that order and the level-0 chunk schedule. Pure host code (no HIP, no thread
// pool, no error state; tests/cpp/commit_plan_test.cpp compiles it with a plain C++17
// compiler). stormck.hip asks for a plan and runs it: on the device, on the host threads, or
// on both.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/stormck.h"
#include "dispatch.h"

namespace stormck {

// The executor of the threaded passes: parts = par(count, fn) runs fn(t, lo, hi) for every
// t in [0, parts) (an empty range included) over contiguous ascending ranges that cover
// [0, count), at once or one after the other, and returns when all are done. 1 <= parts <=
// kMaxParts, and the same count gives the same ranges on every call (a counting pass and its
// placing pass must agree). Serial:
//     auto serial = [](uint64_t count, auto&& fn) { fn(0u, uint64_t{0}, count); return 1u; };
constexpr unsigned kMaxParts = 16;

enum class CommitError { Ok, TooMany, ParentRange, OriginAlign, Cycle, NoMem };

inline const char* commit_error_message(CommitError e) {
    switch (e) {
        case CommitError::TooMany: return "more than 2^32 dirty blocks";
        case CommitError::ParentRange: return "parent index out of range";
        case CommitError::OriginAlign: return "origin_pointer must be 8-byte aligned (Go blocks.Pointer alignment)";
        case CommitError::Cycle: return "parent links form a cycle";
        case CommitError::NoMem: return "commit: height array";
        default: return "";
    }
}

// What one pass over a well-formed forest finds.
struct Heights {
    struct Free {
        void operator()(void* p) const { std::free(p); }
    };
    std::unique_ptr<uint32_t, Free> mem;
    uint64_t n = 0;
    uint64_t relocating = 0;  // blocks with birth_revision <= revision
    uint64_t n_upper = 0;     // blocks with a dirty child (height >= 1)
    uint64_t upper_min = 0;   // the smallest index among them (n without any)
    uint32_t longest = 0;     // the longest block
    uint32_t max_h = 0;       // the largest height
    bool data_off16 = false;  // some data_offset is not 16-byte aligned
    const uint32_t* height() const { return mem.get(); }  // longest distance to a descendant
    uint64_t n0() const { return n - n_upper; }            // level 0: the blocks without dirty children
    // level 0 is a prefix of the caller's array: the n_upper upper blocks are the last ones
    bool prefix0() const { return n_upper == 0 || upper_min == n0(); }
};

// The only pass over the caller's records before anything runs: per block the parent range
// check, the origin alignment check, then a walk up that raises every ancestor's height to
// >= its distance above the block (atomic max; a walk stops at the first ancestor some walk
// has already raised high enough, which then carries the raise further up). The first raise
// of a block from 0 marks it as an upper block. A part stops at its first failing block, and
// every part stops once one has failed: on one part the error is that of the lowest-index
// block whose check or walk fails. A part that covers all of [0, n) has the heights to itself
// and raises them with plain stores (storm's small commits). A forest in which every block
// has a dirty child is a cycle. Nothing of the caller's is written.
template <class Par>
CommitError commit_heights(const stormck_dirty_block* blocks, uint64_t n, uint64_t revision, Par&& par, Heights* H) {
    if (n > 0xffffffffULL) return CommitError::TooMany;
    // zeroed heights: calloc's fresh pages for a large forest, malloc + memset for a small one
    // (calloc misses the allocator's per-thread cache, about 10 ns of a 3-block commit)
    const bool small = n <= 4096;
    H->mem.reset(static_cast<uint32_t*>(small ? std::malloc(4 * std::max<uint64_t>(n, 1)) : std::calloc(n, 4)));
    if (!H->mem) return CommitError::NoMem;
    uint32_t* height = H->mem.get();
    if (small) std::memset(height, 0, 4 * n);
    struct Acc {
        uint64_t reloc, up, up_min;
        uint32_t longest, max_h;
        bool mis;
    } acc[kMaxParts];  // part t fills acc[t]
    std::atomic<int> bad{0};  // the first CommitError stored
    const unsigned parts = par(n, [&](unsigned t, uint64_t lo, uint64_t hi) {
        Acc a{0, 0, n, 0, 0, false};
        const bool alone = lo == 0 && hi == n;
        auto stop = [&](CommitError e) {
            int none = 0;
            bad.compare_exchange_strong(none, static_cast<int>(e), std::memory_order_relaxed);
        };
        for (uint64_t i = lo; i < hi && !bad.load(std::memory_order_relaxed); ++i) {
            const stormck_dirty_block& b = blocks[i];
            a.mis |= (b.data_offset & 15) != 0;
            a.longest = std::max(a.longest, b.length);
            if (b.parent != STORMCK_NO_PARENT && (b.parent < 0 || static_cast<uint64_t>(b.parent) >= n)) {
                stop(CommitError::ParentRange);
                break;
            }
            if (b.origin_pointer != STORMCK_NO_ORIGIN && (b.origin_pointer & 7) != 0) {
                stop(CommitError::OriginAlign);
                break;
            }
            a.reloc += b.birth_revision <= revision;
            uint64_t cur = i;
            uint32_t hh = 0;
            while (blocks[cur].parent != STORMCK_NO_PARENT) {
                const uint64_t p = static_cast<uint64_t>(blocks[cur].parent);
                if (p >= n) {  // an ancestor whose own check has not run yet
                    stop(CommitError::ParentRange);
                    break;
                }
                if (++hh > n) {
                    stop(CommitError::Cycle);
                    break;
                }
                uint32_t old = alone ? height[p] : __atomic_load_n(&height[p], __ATOMIC_RELAXED);
                if (alone && old < hh) height[p] = hh;
                while (!alone && old < hh &&
                       !__atomic_compare_exchange_n(&height[p], &old, hh, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
                }
                if (old >= hh) break;  // another walk holds p at >= hh and carries it upward
                if (old == 0) {        // this walk raised p first
                    ++a.up;
                    a.up_min = std::min(a.up_min, p);
                }
                a.max_h = std::max(a.max_h, hh);
                cur = p;
            }
        }
        acc[t] = a;
    });
    if (bad.load()) return static_cast<CommitError>(bad.load());
    H->n = n;
    H->relocating = H->n_upper = 0;
    H->upper_min = n;
    H->longest = H->max_h = 0;
    H->data_off16 = false;
    for (unsigned t = 0; t < parts; ++t) {
        H->relocating += acc[t].reloc;
        H->n_upper += acc[t].up;
        H->upper_min = std::min(H->upper_min, acc[t].up_min);
        H->longest = std::max(H->longest, acc[t].longest);
        H->max_h = std::max(H->max_h, acc[t].max_h);
        H->data_off16 |= acc[t].mis;
    }
    if (H->n0() == 0 && n > 0) return CommitError::Cycle;  // every block has a dirty child
    return CommitError::Ok;
}

// What the router's cost model prices: per height the blocks, their bytes and the longest.
struct CommitShape {
    std::vector<uint64_t> cnt, bytes, longest;  // per height
};

inline void commit_shape(const Heights& H, const stormck_dirty_block* blocks, uint64_t n, CommitShape* s) {
    const uint32_t* height = H.height();
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t h = height[i];
        if (h >= s->cnt.size()) {
            s->cnt.resize(h + 1, 0);
            s->bytes.resize(h + 1, 0);
            s->longest.resize(h + 1, 0);
        }
        s->cnt[h]++;
        s->bytes[h] += blocks[i].length;
        s->longest[h] = std::max<uint64_t>(s->longest[h], blocks[i].length);
    }
}

// Commit order: level 0 in index order, then the upper levels by height (index order within
// a height), i.e. a stable sort by height.
struct CommitOrder {
    std::vector<uint32_t> order;        // commit position -> the caller's index; empty: the identity
    std::vector<uint32_t> upper;        // upper blocks in index order (only when level 0 is not a prefix)
    std::vector<uint64_t> level_start;  // height h: commit positions [level_start[h], level_start[h + 1])
    uint64_t at(uint64_t k) const { return order.empty() ? k : order[k]; }
};

// Level 0's part of the order, all that the first launch needs: order[0, n0) and upper[],
// materialised only when level 0 is not a prefix of the caller's array.
template <class Par>
void order_level0(const Heights& H, Par&& par, CommitOrder* O) {
    if (H.prefix0()) return;
    const uint32_t* height = H.height();
    O->order.resize(H.n);
    O->upper.resize(H.n_upper);
    uint64_t z[kMaxParts + 1];  // level-0 blocks before part t
    z[0] = 0;
    const unsigned parts = par(H.n, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t m = 0;
        for (uint64_t i = lo; i < hi; ++i) m += height[i] == 0;
        z[t + 1] = m;
    });
    for (unsigned t = 0; t < parts; ++t) z[t + 1] += z[t];
    par(H.n, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t a = z[t], u = lo - z[t];
        for (uint64_t i = lo; i < hi; ++i) {
            if (height[i] == 0) O->order[a++] = static_cast<uint32_t>(i);
            else O->upper[u++] = static_cast<uint32_t>(i);
        }
    });
}

// The upper part, after order_level0 (the device leg builds it while level 0 hashes):
// level_start[], and a stable counting sort by height of the upper blocks unless they are
// already in that order.
template <class Par>
void order_upper(const Heights& H, Par&& par, CommitOrder* O) {
    const uint32_t* height = H.height();
    const uint64_t n = H.n, nu = H.n_upper, n0 = H.n0();
    const uint32_t max_h = H.max_h;
    auto uidx = [&](uint64_t u) -> uint32_t { return O->upper.empty() ? static_cast<uint32_t>(n0 + u) : O->upper[u]; };
    std::vector<uint64_t>& level_start = O->level_start;
    level_start.assign(static_cast<size_t>(max_h) + 2, 0);
    level_start[1] = n0;
    if (nu == 0) return;
    // per part: its upper blocks of each height, and whether they come in height order; a part
    // that covers all of them counts into level_start itself
    std::vector<uint64_t> hist[kMaxParts];
    bool in_order[kMaxParts];
    const unsigned parts = par(nu, [&](unsigned t, uint64_t lo, uint64_t hi) {
        const bool alone = lo == 0 && hi == nu;
        if (!alone) hist[t].assign(static_cast<size_t>(max_h) + 1, 0);
        uint64_t* cnt = alone ? level_start.data() + 1 : hist[t].data();
        uint32_t prev = lo ? height[uidx(lo - 1)] : 0;
        bool rising = true;
        for (uint64_t u = lo; u < hi; ++u) {
            const uint32_t h = height[uidx(u)];
            rising &= h >= prev;
            prev = h;
            cnt[h]++;
        }
        in_order[t] = rising;
    });
    bool sorted = true;
    for (unsigned t = 0; t < parts; ++t) {
        sorted &= in_order[t];
        for (size_t l = 1; l < hist[t].size(); ++l) level_start[l + 1] += hist[t][l];
    }
    for (uint32_t l = 1; l <= max_h; ++l) level_start[l + 1] += level_start[l];
    if (sorted && O->upper.empty()) return;  // the upper part is in commit order as given
    if (O->order.empty()) {
        O->order.resize(n);
        for (uint64_t k = 0; k < n0; ++k) O->order[k] = static_cast<uint32_t>(k);
    }
    if (sorted) {
        std::memcpy(O->order.data() + n0, O->upper.data(), nu * 4);
        return;
    }
    std::vector<std::vector<uint64_t>> pos(parts, std::vector<uint64_t>(level_start.begin(), level_start.end() - 1));
    for (unsigned t = 1; t < parts; ++t)
        for (size_t l = 1; l <= max_h; ++l) pos[t][l] = pos[t - 1][l] + hist[t - 1][l];
    par(nu, [&](unsigned t, uint64_t lo, uint64_t hi) {
        std::vector<uint64_t>& ps = pos[t];
        for (uint64_t u = lo; u < hi; ++u) {
            const uint32_t i = uidx(u);
            O->order[ps[height[i]]++] = i;
        }
    });
}

// The whole order at once (the host legs).
template <class Par>
void commit_order(const Heights& H, Par&& par, CommitOrder* O) {
    order_level0(H, par, O);
    order_upper(H, par, O);
}

// Relocation (cache/cache.go:114-118: the k-th relocating block in commit order gets address
// last + k and is born in revision + 1) of commit positions [a, b), applied to the caller's
// records, then emit(k, record) for every position (from several threads, each k once).
// relocating: whether the forest has any such block (Heights::relocating); without one it is
// a single pass. The ranges of one commit go through in ascending order, `last` carried along.
template <class Par, class Emit>
void relocate_range(stormck_dirty_block* blocks, const CommitOrder& O, uint64_t a, uint64_t b, uint64_t revision,
                    bool relocating, uint64_t* last, Par&& par, Emit&& emit) {
    if (a >= b) return;
    uint64_t before[kMaxParts + 1];  // relocating blocks of [a, b) before part t
    before[0] = 0;
    unsigned parts = 0;
    if (relocating) {
        parts = par(b - a, [&](unsigned t, uint64_t lo, uint64_t hi) {
            uint64_t m = 0;
            for (uint64_t k = a + lo; k < a + hi; ++k) m += blocks[O.at(k)].birth_revision <= revision;
            before[t + 1] = m;
        });
        for (unsigned t = 0; t < parts; ++t) before[t + 1] += before[t];
    }
    const uint64_t first = *last;
    par(b - a, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t addr = first + (relocating ? before[t] : 0);
        for (uint64_t k = a + lo; k < a + hi; ++k) {
            stormck_dirty_block& rec = blocks[O.at(k)];
            if (relocating && rec.birth_revision <= revision) {
                rec.address = ++addr;
                rec.birth_revision = revision + 1;
            }
            emit(k, rec);
        }
    });
    *last = first + before[parts];
}

// Level 0 on the device goes out in growing chunks: `first` blocks, then `growth` times the
// previous chunk (the caller's `next`), and no runt: a chunk that would leave fewer than
// kStreamBatch of the `rest` takes all of it.
constexpr uint64_t level0_chunk(uint64_t rest, uint64_t next) {
    return rest - std::min(next, rest) < kStreamBatch ? rest : std::min(next, rest);
}

// A small commit with upper levels returns its checksums in one piece after the last level.
constexpr bool commit_one_piece(uint64_t nu, uint64_t n0) { return nu > 0 && n0 <= kCommitOnePiece; }

}  // namespace stormck
