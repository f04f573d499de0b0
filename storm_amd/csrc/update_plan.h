// The planning of an update (include/stormck.h "update", rules C and D), once for both legs: from
// the distinct dirty blocks of a batch it computes their heights, the order, the new addresses, the
// room check, the records the commit engine runs and the new singularity. Pure host code (no HIP,
// no thread pool, no error state; tests/cpp/update_plan_test.cpp compiles it with a plain C++17
// compiler). update.h finds the dirty blocks, asks for a plan and runs it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/stormck.h"

namespace stormck {

// One dirty block as the walks find it. parent: the old address of the dirty block that holds
// its origin, 0 for the topmost block (its origin is the singularity). slot: the entry of a
// pointer block, the space's index k of a spacelist leaf. A spacelist leaf holds two origins per
// space: a child says with kUpdateKeyOrigin in `slot` that its own is the KeyStorePointer; without
// it (every child of an update) it is the ObjectStorePointer.
constexpr uint32_t kUpdateKeyOrigin = 1u << 31;

struct UpdateDirty {
    uint64_t address, parent;
    uint32_t slot, kind;  // STORMCK_SCRUB_*
};

struct UpdateGeometry {
    uint64_t block_size, n_blocks;
    uint32_t fanout;
    uint32_t len[4];  // bytes hashed per kind
};

enum class UpdateError { Ok, NoSpace, Empty, Duplicate, NoParent, ParentKind, Top, Cycle, TooMany };

inline const char* update_error_message(UpdateError e) {
    switch (e) {
        case UpdateError::NoSpace: return "update: the image has no room for the dirty blocks (LastAllocatedBlock + dirty blocks >= n_blocks)";
        case UpdateError::Empty: return "update: no dirty block";
        case UpdateError::Duplicate: return "update: a block is referenced twice on the dirty paths";
        case UpdateError::NoParent: return "update: a dirty block's parent is not dirty";
        case UpdateError::ParentKind: return "update: a dirty block's parent holds no origins";
        case UpdateError::Top: return "update: the dirty blocks do not have exactly one topmost block";
        case UpdateError::Cycle: return "update: the dirty paths form a cycle";
        case UpdateError::TooMany: return "update: more than 2^32 dirty blocks";
        default: return "";
    }
}

// Where the parent's copy of `kind` at arena offset `at` keeps entry `slot`'s Pointer and type.
inline uint64_t update_origin_pointer(uint64_t at, uint32_t kind, uint32_t slot) {
    if (kind == STORMCK_SCRUB_POINTER) return at + 24ull * slot;
    return at + 72ull * (slot & ~kUpdateKeyOrigin) + ((slot & kUpdateKeyOrigin) ? 16 : 40);
}
inline uint64_t update_origin_type(uint64_t at, uint32_t kind, uint32_t slot, uint32_t fanout) {
    if (kind == STORMCK_SCRUB_POINTER) return at + 24ull * fanout + slot;
    return at + 72ull * (slot & ~kUpdateKeyOrigin) + ((slot & kUpdateKeyOrigin) ? 64 : 65);
}

struct UpdatePlan {
    // in commit order (ascending height, ascending old address within a height)
    std::vector<uint64_t> old_address;         // position k moves to first_new + k
    std::vector<uint32_t> kind;
    std::vector<stormck_dirty_block> records;  // for stormck_commit_*; the last one is the topmost block
    uint64_t first_new = 0, last_allocated = 0;
    uint64_t n_dirty[4] = {0, 0, 0, 0};
    uint64_t bytes_hashed = 0;  // of the dirty blocks
    uint32_t heights = 0;       // the number of distinct heights
};

// The plan of the distinct dirty blocks d[0..n) on a store whose singularity holds `revision` and
// last = LastAllocatedBlock. Nothing of the caller's is written.
inline UpdateError update_plan(const UpdateDirty* d, uint64_t n, const UpdateGeometry& G, uint64_t revision, uint64_t last,
                               UpdatePlan* P) {
    if (n == 0) return UpdateError::Empty;
    if (n > 0xffffffffULL) return UpdateError::TooMany;
    if (last >= G.n_blocks || n >= G.n_blocks - last) return UpdateError::NoSpace;  // L + D >= n_blocks, without overflow
    // by old address: a block's index from its address
    std::vector<uint32_t> by(n);
    for (uint64_t i = 0; i < n; ++i) by[i] = static_cast<uint32_t>(i);
    std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return d[a].address < d[b].address; });
    for (uint64_t i = 1; i < n; ++i)
        if (d[by[i]].address == d[by[i - 1]].address) return UpdateError::Duplicate;
    auto find = [&](uint64_t address) -> int64_t {
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (d[by[mid]].address < address) lo = mid + 1;
            else hi = mid;
        }
        return lo < n && d[by[lo]].address == address ? static_cast<int64_t>(by[lo]) : -1;
    };
    std::vector<int64_t> parent(n);
    uint64_t tops = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (d[i].kind > STORMCK_SCRUB_BLOB) return UpdateError::ParentKind;
        if (d[i].parent == 0) {
            parent[i] = -1;
            ++tops;
            continue;
        }
        parent[i] = find(d[i].parent);
        if (parent[i] < 0) return UpdateError::NoParent;
        const uint32_t pk = d[parent[i]].kind;
        if (pk != STORMCK_SCRUB_POINTER && pk != STORMCK_SCRUB_SPACELIST) return UpdateError::ParentKind;
    }
    if (tops != 1) return UpdateError::Top;
    // heights: every block raises its ancestors to their distance above it; a walk stops where an
    // earlier one has raised as high
    std::vector<uint32_t> height(n, 0);
    uint32_t max_h = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t h = 0;
        for (int64_t p = parent[i]; p >= 0; p = parent[p]) {
            if (++h > n) return UpdateError::Cycle;
            if (height[p] >= h) break;
            height[p] = h;
            max_h = std::max(max_h, h);
        }
    }
    // the order: by is ascending in address, and the sort by height is stable
    std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return height[a] < height[b]; });
    std::vector<uint32_t> place(n);
    for (uint64_t k = 0; k < n; ++k) place[by[k]] = static_cast<uint32_t>(k);
    P->first_new = last + 1;
    P->last_allocated = last + n;
    P->heights = max_h + 1;
    P->bytes_hashed = 0;
    for (uint64_t& c : P->n_dirty) c = 0;
    P->old_address.resize(n);
    P->kind.resize(n);
    P->records.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
        const UpdateDirty& b = d[by[k]];
        const uint64_t address = P->first_new + k;
        stormck_dirty_block& r = P->records[k];
        std::memset(&r, 0, sizeof r);
        r.data_offset = address * G.block_size;
        r.address = address;
        r.birth_revision = revision + 1;  // above `revision`: the commit engine relocates nothing itself
        r.length = G.len[b.kind];
        r.type = b.kind == STORMCK_SCRUB_POINTER ? STORMCK_POINTER_BLOCK : STORMCK_LEAF_BLOCK;
        if (parent[by[k]] < 0) {
            r.parent = STORMCK_NO_PARENT;
            r.origin_pointer = STORMCK_NO_ORIGIN;  // the singularity: its checksum comes back to the caller
            r.origin_type = 0;
        } else {
            const uint32_t pk = place[parent[by[k]]];
            const uint64_t at = (P->first_new + pk) * G.block_size;
            r.parent = pk;
            r.origin_pointer = update_origin_pointer(at, d[parent[by[k]]].kind, b.slot);
            r.origin_type = update_origin_type(at, d[parent[by[k]]].kind, b.slot, G.fanout);
        }
        P->old_address[k] = b.address;
        P->kind[k] = b.kind;
        ++P->n_dirty[b.kind];
        P->bytes_hashed += r.length;
    }
    return UpdateError::Ok;
}

// The singularity (72 bytes, blocks/singularity/block.go:8-19) after the commit: the space origin
// names the topmost block's new copy, Revision + 1, LastAllocatedBlock, and Checksum over the 72
// bytes with the field zeroed (hash: XXH64 of (pointer, length)).
template <class Hash>
void update_singularity(uint8_t* sing, uint64_t top_checksum, const UpdatePlan& P, uint64_t revision, Hash&& hash) {
    auto put = [&](uint32_t at, uint64_t v) { std::memcpy(sing + at, &v, 8); };
    const stormck_dirty_block& top = P.records.back();
    put(0, 0);
    put(16, revision + 1);
    put(32, top_checksum);
    put(40, top.address);
    put(48, top.birth_revision);
    sing[56] = top.type;
    put(64, P.last_allocated);
    put(0, hash(sing, 72));
}

}  // namespace stormck
