// Scrub: walk a committed snapshot from its root and verify every reachable block
// (include/stormck.h "scrub"; DESIGN.md "Scrub").
//
// Included by stormck.hip inside its anonymous namespace, after the dispatch it calls
// (launch_checksum), the fault slots (take_fault) and the host pool (ForkJoin).
//
// Three parts:
//   1. the rules: one __host__ __device__ function from a verified block's entry to
//      (address, expected, kind, length, status), which the host leg and the kernel share;
//   2. the device engine: per level, launch_checksum over the frontier, k_scrub_expand over
//      the same rows, one small read-back;
//   3. the host leg: the same walk with the level hashed on pool threads.
//
// The frontier is one append-only queue of rows (structure of arrays): level L is the window
// [start_L, start_L + count_L) and the next level is appended right behind it. A block is
// enqueued at most once (the claim table and the visited bitmap below), so the queue holds
// fewer than n_blocks rows in all and cannot overflow; the two adjacent windows are the ping
// and the pong, and the rows of the level before stay readable, which the first-error detail
// pass uses.
//
// Which reference wins a block that several name is decided by value, not by arrival: within a
// level the smallest (parent, slot) wins, as the rule in the header says. k_scrub_expand runs
// twice per level for that. Pass 0 atomicMin's each in-range candidate's key into claim[address]
// unless the visited bit is already set (the block was won at a shallower level, and claim then
// still holds that winner's key). Pass 1 re-reads the entries: a candidate whose key is in
// claim[address] is the winner, is enqueued and sets the visited bit; any other candidate is a
// DUPLICATE. Keys are unique (a block is a parent once), so "claim[address] == my key" is
// the same in every later pass. The pointer blocks that are read twice are under 0.1 % of an
// image at fanout 1200.

constexpr uint32_t kScrubSkip = 0xff;      // an entry that is neither followed nor an error
constexpr int kScrubSlotBits = 20;         // key = parent << 20 | slot
constexpr uint64_t kScrubMaxBlocks = uint64_t{1} << 36;
constexpr uint64_t kScrubNoKey = UINT64_MAX;
constexpr uint32_t kScrubSingLen = 72;     // singularity.Block (blocks/singularity/block.go:8-19)

struct ScrubParams {
    uint64_t block_size, n_blocks;
    uint32_t fanout, spaces;
    uint32_t len[4];  // bytes hashed per kind (STORMCK_SCRUB_POINTER ..)
};

struct ScrubChild {
    uint64_t address, expected;
    uint32_t len;
    uint8_t kind, leaf;  // leaf: the leaf kind of the tree the child belongs to
    uint8_t status;      // STORMCK_SCRUB_OK / _RANGE / _TYPE, or kScrubSkip
};

__host__ __device__ inline uint64_t scrub_le64(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint64_t*>(p);  // 8-byte aligned: checked by the entry points
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
#endif
}

__host__ __device__ inline uint64_t scrub_key(uint64_t parent, uint32_t slot) {
    return (parent << kScrubSlotBits) | slot;
}

// Entries a verified block of `kind` holds.
__host__ __device__ inline uint32_t scrub_entries(const ScrubParams& P, uint32_t kind) {
    return kind == STORMCK_SCRUB_POINTER ? P.fanout : (kind == STORMCK_SCRUB_SPACELIST ? 2 * P.spaces : 0);
}

// A reference {expected, address} of block type `type` into a tree whose leaves are `leaf`.
__host__ __device__ inline ScrubChild scrub_ref(const ScrubParams& P, uint64_t expected, uint64_t address,
                                                uint8_t type, uint8_t leaf) {
    ScrubChild c{address, expected, 0, 0, leaf, static_cast<uint8_t>(kScrubSkip)};
    if (type == STORMCK_FREE_BLOCK) return c;
    if (type > STORMCK_LEAF_BLOCK) {
        c.status = STORMCK_SCRUB_TYPE;
        return c;
    }
    c.kind = type == STORMCK_POINTER_BLOCK ? static_cast<uint8_t>(STORMCK_SCRUB_POINTER) : leaf;
    c.len = P.len[c.kind];
    // address < n_blocks before anyone multiplies it by block_size
    c.status = (address == 0 || address >= P.n_blocks) ? STORMCK_SCRUB_RANGE : STORMCK_SCRUB_OK;
    return c;
}

// Entry `slot` of the verified block at `blk` (kind pointer or spacelist; `leaf`: the leaf
// kind of a pointer block's tree).
__host__ __device__ inline ScrubChild scrub_child(const ScrubParams& P, const uint8_t* blk, uint32_t kind,
                                                  uint32_t leaf, uint32_t slot) {
    if (kind == STORMCK_SCRUB_POINTER) {
        const uint8_t* ptr = blk + 24 * static_cast<uint64_t>(slot);
        return scrub_ref(P, scrub_le64(ptr), scrub_le64(ptr + 8), blk[24 * static_cast<uint64_t>(P.fanout) + slot],
                         static_cast<uint8_t>(leaf));
    }
    const uint8_t* sp = blk + 72 * static_cast<uint64_t>(slot >> 1);
    const uint32_t which = slot & 1;  // 0: the key tree, 1: the object tree
    const uint8_t state = sp[66];
    ScrubChild c{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
    if (state > 2) {  // reported once per space
        if (which == 0) c.status = STORMCK_SCRUB_TYPE;
        return c;
    }
    if (state != 1) return c;  // only Defined spaces are followed (spacestore/spacestore.go:29)
    const uint8_t* ptr = sp + 16 + 24 * which;
    return scrub_ref(P, scrub_le64(ptr), scrub_le64(ptr + 8), sp[64 + which],
                     static_cast<uint8_t>(which ? STORMCK_SCRUB_BLOB : STORMCK_SCRUB_OBJECTLIST));
}

// ---- what both legs report -----------------------------------------------------------

struct ScrubFirst {
    bool have = false;
    uint32_t level = 0;
    uint64_t key = kScrubNoKey;
    uint32_t error = STORMCK_SCRUB_OK;
    uint64_t address = 0, computed = 0, expected = 0;
};

struct ScrubTotals {
    uint64_t enq[4] = {0, 0, 0, 0};   // rows enqueued per kind
    uint64_t mism[4] = {0, 0, 0, 0};  // of them, rows whose checksum differed
    uint64_t n_structural = 0;
    uint64_t extra_bytes = 0, extra_mismatch = 0;  // the singularity
    uint32_t levels = 0;
    ScrubFirst first;
};

std::string scrub_error_text(const stormck_scrub_report& r) {
    char buf[200];
    const unsigned long long a = r.first_address, p = r.first_parent;
    switch (r.first_error) {
    case STORMCK_SCRUB_MISMATCH:  // blocks/checksum.go:25-26
        std::snprintf(buf, sizeof buf, "checksum mismatch for block %llu, computed: 0x%llx, expected: 0x%llx", a,
                      static_cast<unsigned long long>(r.first_computed),
                      static_cast<unsigned long long>(r.first_expected));
        break;
    case STORMCK_SCRUB_RANGE:  // cache/cache.go:146
        std::snprintf(buf, sizeof buf, "block %llu does not exist (block %llu, slot %u)", a, p, r.first_slot);
        break;
    case STORMCK_SCRUB_TYPE:
        std::snprintf(buf, sizeof buf, "invalid block type or space state in block %llu, slot %u", p, r.first_slot);
        break;
    default:
        std::snprintf(buf, sizeof buf, "block %llu is referenced more than once (block %llu, slot %u)", a, p,
                      r.first_slot);
    }
    return buf;
}

int scrub_finish(const ScrubParams& P, const ScrubTotals& T, stormck_scrub_report* r) {
    std::memset(r, 0, sizeof *r);
    r->bytes_hashed = T.extra_bytes;
    r->n_mismatch = T.extra_mismatch;
    for (int k = 0; k < 4; ++k) {
        r->verified[k] = T.enq[k] - T.mism[k];
        r->bytes_hashed += T.enq[k] * P.len[k];
        r->n_mismatch += T.mism[k];
    }
    r->n_structural = T.n_structural;
    r->levels = T.levels;
    if (T.first.have) {
        r->first_error = T.first.error;
        r->first_level = T.first.level;
        r->first_slot = static_cast<uint32_t>(T.first.key & ((1u << kScrubSlotBits) - 1));
        r->first_parent = T.first.key >> kScrubSlotBits;
        r->first_address = T.first.address;
        r->first_computed = T.first.computed;
        r->first_expected = T.first.expected;
    }
    if (r->n_mismatch + r->n_structural > 0) return fail(STORMCK_EMISMATCH, scrub_error_text(*r));
    return STORMCK_OK;
}

// Argument checks shared by the four entry points; fills P. leaf_kind < 0: a whole store.
int scrub_params(const void* store, const stormck_scrub_layout* L, const stormck_scrub_report* report, int leaf_kind,
                 uint32_t leaf_len, ScrubParams* P) {
    if (!store || !L || !report) return fail(STORMCK_EINVAL, "scrub: null argument");
    if (L->block_size == 0 || (L->block_size & 7)) return fail(STORMCK_EINVAL, "scrub: block_size must be a positive multiple of 8");
    if (L->n_blocks == 0 || L->n_blocks > kScrubMaxBlocks || L->n_blocks > UINT64_MAX / L->block_size)
        return fail(STORMCK_EINVAL, "scrub: n_blocks out of range (1..2^36, image below 2^64 bytes)");
    if (L->pointer_fanout == 0 || L->pointer_fanout > kMaxFanout) return fail(STORMCK_EINVAL, "scrub: pointer_fanout out of range");
    if (L->spaces_per_block == 0 || L->spaces_per_block > (1u << (kScrubSlotBits - 1)))
        return fail(STORMCK_EINVAL, "scrub: spaces_per_block out of range");
    P->block_size = L->block_size;
    P->n_blocks = L->n_blocks;
    P->fanout = L->pointer_fanout;
    P->spaces = L->spaces_per_block;
    const uint64_t plen = (25 * static_cast<uint64_t>(L->pointer_fanout) + 7) & ~uint64_t{7};
    const uint64_t slen = (72 * static_cast<uint64_t>(L->spaces_per_block) + 2 + 7) & ~uint64_t{7};
    uint64_t len[4] = {plen, slen, L->objectlist_len, L->blob_len};
    if (leaf_kind >= 0) {
        if (leaf_kind < STORMCK_SCRUB_SPACELIST || leaf_kind > STORMCK_SCRUB_BLOB)
            return fail(STORMCK_EINVAL, "scrub: leaf_kind must be spacelist, objectlist or blob");
        if (leaf_len) len[leaf_kind] = leaf_len;
        if (leaf_kind == STORMCK_SCRUB_SPACELIST && len[leaf_kind] < 72 * static_cast<uint64_t>(L->spaces_per_block))
            return fail(STORMCK_EINVAL, "scrub: leaf_len does not cover the spaces of a spacelist block");
    }
    for (int k = 0; k < 4; ++k) {
        if (len[k] > L->block_size) return fail(STORMCK_EINVAL, "scrub: a block length is larger than block_size");
        P->len[k] = static_cast<uint32_t>(len[k]);
    }
    return STORMCK_OK;
}

// The root reference (parent 0, slot 0, level 0): counts its structural error, if any.
// Returns true when there is a root block to walk.
bool scrub_root(const ScrubChild& root, ScrubTotals* T) {
    if (root.status == kScrubSkip) return false;  // Free: an empty tree
    if (root.status != STORMCK_SCRUB_OK) {
        T->n_structural = 1;
        T->first.have = true;
        T->first.level = 0;
        T->first.key = scrub_key(0, 0);
        T->first.error = root.status;
        T->first.address = root.address;
        return false;
    }
    return true;
}

// The singularity's 72 bytes: verifies them (Checksum zeroed) and returns the space origin.
// A failure is recorded in T and returns false.
bool scrub_singularity(const ScrubParams& P, const uint8_t* sing, ScrubTotals* T, ScrubChild* root) {
    uint8_t s[kScrubSingLen];
    std::memcpy(s, sing, kScrubSingLen);
    const uint64_t expected = scrub_le64(s);
    std::memset(s, 0, 8);
    const uint64_t computed = stormck::host::xxh64(s, kScrubSingLen);
    T->extra_bytes = kScrubSingLen;
    if (computed != expected) {
        T->extra_mismatch = 1;
        T->first.have = true;
        T->first.key = scrub_key(0, 0);
        T->first.error = STORMCK_SCRUB_MISMATCH;
        T->first.computed = computed;
        T->first.expected = expected;
        return false;
    }
    *root = scrub_ref(P, scrub_le64(s + 32), scrub_le64(s + 40), s[56], STORMCK_SCRUB_SPACELIST);
    return true;
}

// ---- host leg ---------------------------------------------------------------------------

struct ScrubRow {
    uint64_t address, expected, parent, computed;
    uint32_t len, slot;
    uint8_t kind, leaf;
};

int scrub_walk_host(const uint8_t* base, const ScrubParams& P, const ScrubChild& root, ScrubTotals* T,
                    uint32_t* reachable, uint32_t threads) {
    const uint64_t words = (P.n_blocks + 31) / 32;
    std::vector<uint32_t> visited(words, 0);
    visited[0] = 1;
    std::vector<ScrubRow> level, next;
    if (scrub_root(root, T)) {
        level.push_back({root.address, root.expected, 0, 0, root.len, 0, root.kind, root.leaf});
        visited[root.address >> 5] |= 1u << (root.address & 31);
        T->enq[root.kind] = 1;
    }
    ForkJoin& pool = ForkJoin::get();
    const unsigned want = threads ? threads : pool.size();
    // the first error among this walk's candidates: the shallowest level, then the smallest key
    auto note = [&](uint32_t lvl, uint64_t key, uint32_t error, uint64_t address, uint64_t computed, uint64_t expected) {
        ScrubFirst& f = T->first;
        if (f.have && (f.level < lvl || (f.level == lvl && f.key <= key))) return;
        f = ScrubFirst{true, lvl, key, error, address, computed, expected};
    };
    for (uint32_t lvl = 0; !level.empty(); ++lvl) {
        const unsigned parts = static_cast<unsigned>(std::min<uint64_t>(want, level.size()));
        pool.run(parts, [&](unsigned t) {
            for (size_t i = t; i < level.size(); i += parts)
                level[i].computed = stormck::host::xxh64(base + level[i].address * P.block_size, level[i].len);
        });
        T->levels = lvl + 1;
        // parents in address order and their slots in order: keys ascend, so the first
        // candidate to reach an unvisited block is the one with the smallest key
        std::sort(level.begin(), level.end(), [](const ScrubRow& a, const ScrubRow& b) { return a.address < b.address; });
        next.clear();
        for (const ScrubRow& r : level) {
            if (r.computed != r.expected) {
                ++T->mism[r.kind];
                note(lvl, scrub_key(r.parent, r.slot), STORMCK_SCRUB_MISMATCH, r.address, r.computed, r.expected);
                continue;
            }
            const uint8_t* blk = base + r.address * P.block_size;
            const uint32_t entries = scrub_entries(P, r.kind);
            for (uint32_t e = 0; e < entries; ++e) {
                const ScrubChild c = scrub_child(P, blk, r.kind, r.leaf, e);
                if (c.status == kScrubSkip) continue;
                uint32_t err = c.status;
                if (err == STORMCK_SCRUB_OK) {
                    uint32_t& w = visited[c.address >> 5];
                    const uint32_t bit = 1u << (c.address & 31);
                    if (w & bit) {
                        err = STORMCK_SCRUB_DUPLICATE;
                    } else {
                        w |= bit;
                        ++T->enq[c.kind];
                        next.push_back({c.address, c.expected, r.address, 0, c.len, e, c.kind, c.leaf});
                        continue;
                    }
                }
                ++T->n_structural;
                note(lvl + 1, scrub_key(r.address, e), err, c.address, 0, 0);
            }
        }
        level.swap(next);
    }
    if (reachable) std::memcpy(reachable, visited.data(), words * 4);
    return STORMCK_OK;
}

// ---- device engine ------------------------------------------------------------------------

struct ScrubCounters {
    unsigned long long tail;          // rows in the queue
    unsigned long long enq[4];        // rows enqueued per kind
    unsigned long long mism[4];       // rows whose checksum differed, per kind
    unsigned long long n_structural;
    unsigned long long key_mismatch;  // smallest key of this level's mismatching rows
    unsigned long long key_structural;  // smallest key of the errors among this level's entries
    unsigned long long detail[4];     // detail pass: error, address, computed, expected
};
static_assert(sizeof(ScrubCounters) <= 256, "the counters take the first 256 bytes of the workspace");

struct ScrubQueue {
    uint64_t *address, *expected, *parent, *offset, *computed;
    uint32_t *len, *slot;
    uint8_t* tree;  // kind | leaf << 2
    uint64_t cap;
};

uint64_t scrub_bitmap_bytes(uint64_t n_blocks) { return (((n_blocks + 31) / 32) * 4 + 7) & ~uint64_t{7}; }

uint64_t scrub_workspace_bytes(uint64_t n_blocks) {
    return 256 + n_blocks * 56 + ((n_blocks + 7) & ~uint64_t{7}) + scrub_bitmap_bytes(n_blocks);
}

// After the bitmap and the claims were cleared: the counters, bit 0, and with a root to walk
// (0 < root.address < n_blocks) row 0, its claim (key 0: parent 0, slot 0) and its visited bit.
__global__ void k_scrub_seed(ScrubQueue Q, ScrubChild root, bool walk, uint64_t block_size, unsigned long long* claim,
                             uint32_t* bitmap, ScrubCounters* C) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ScrubCounters c = {};
    bitmap[0] |= 1u;
    if (walk) {
        Q.address[0] = root.address;
        Q.expected[0] = root.expected;
        Q.parent[0] = 0;
        Q.offset[0] = root.address * block_size;
        Q.len[0] = root.len;
        Q.slot[0] = 0;
        Q.tree[0] = static_cast<uint8_t>(root.kind | (root.leaf << 2));
        claim[root.address] = scrub_key(0, 0);
        bitmap[root.address >> 5] |= 1u << (root.address & 31);
        c.tail = 1;
        c.enq[root.kind] = 1;
    }
    *C = c;
}

// One wave per frontier row [start, start + count). PASS 0: claims. PASS 1: compare, decide and
// count, then enqueue. PASS 2 (at most once per scrub): the detail of the error whose key is `want`.
template <int PASS>
__global__ void __launch_bounds__(256) k_scrub_expand(const uint8_t* base, ScrubParams P, ScrubQueue Q, uint64_t start,
                                                      uint64_t count, unsigned long long* claim, uint32_t* bitmap,
                                                      ScrubCounters* C, unsigned long long want) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (r >= count) return;  // wave-uniform
    const uint64_t i = start + r;
    const uint64_t addr = Q.address[i], computed = Q.computed[i], expected = Q.expected[i];
    const uint32_t kind = Q.tree[i] & 3, leaf = Q.tree[i] >> 2;
    if (computed != expected) {  // counted, never expanded or dereferenced
        if (PASS != 0 && lane == 0) {
            const unsigned long long key = scrub_key(Q.parent[i], Q.slot[i]);
            if (PASS == 1) {
                atomicAdd(&C->mism[kind], 1ULL);
                atomicMin(&C->key_mismatch, key);
            } else if (key == want) {
                C->detail[0] = STORMCK_SCRUB_MISMATCH;
                C->detail[1] = addr;
                C->detail[2] = computed;
                C->detail[3] = expected;
            }
        }
        return;
    }
    const uint32_t entries = scrub_entries(P, kind);
    if (entries == 0) return;  // objectlist and blob leaves only take the compare
    const uint8_t* blk = base + addr * P.block_size;  // addr < n_blocks: checked before it was enqueued
    uint32_t n_enq[4] = {0, 0, 0, 0}, n_err = 0, n_win = 0;  // wave-uniform sums
    for (uint32_t c = 0; c < entries; c += 64) {
        const uint32_t e = c + lane;
        ScrubChild ch{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
        if (e < entries) ch = scrub_child(P, blk, kind, leaf, e);
        const unsigned long long key = scrub_key(addr, e);
        const bool cand = ch.status == STORMCK_SCRUB_OK;  // 0 < ch.address < n_blocks
        if (PASS == 0) {
            if (cand && !((bitmap[ch.address >> 5] >> (ch.address & 31)) & 1u)) atomicMin(&claim[ch.address], key);
            continue;
        }
        const bool win = cand && claim[ch.address] == key;
        const uint32_t err = cand ? (win ? STORMCK_SCRUB_OK : STORMCK_SCRUB_DUPLICATE)
                                  : (ch.status == kScrubSkip ? STORMCK_SCRUB_OK : ch.status);
        if (PASS == 2) {
            if (err != STORMCK_SCRUB_OK && key == want) {
                C->detail[0] = err;
                C->detail[1] = ch.address;
                C->detail[2] = 0;
                C->detail[3] = 0;
            }
            continue;
        }
        const unsigned long long m = __ballot(win);
        n_win += __popcll(m);
        if (m) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) n_enq[k] += __popcll(__ballot(win && ch.kind == k));
        }
        const bool bad = err != STORMCK_SCRUB_OK;
        n_err += __popcll(__ballot(bad));
        if (bad) atomicMin(&C->key_structural, key);
    }
    if (PASS != 1) return;
    if (n_win) {
        // one atomicAdd per wave claims the row's whole range of the next level; the winners
        // (the same ones: claim does not change in this pass) then write their rows at their
        // prefix positions, with nothing that waits for an atomic's return between the chunks
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&C->tail, static_cast<unsigned long long>(n_win));
        first = __shfl(first, 0);
        for (uint32_t c = 0; c < entries; c += 64) {
            const uint32_t e = c + lane;
            ScrubChild ch{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
            if (e < entries) ch = scrub_child(P, blk, kind, leaf, e);
            const bool win = ch.status == STORMCK_SCRUB_OK && claim[ch.address] == scrub_key(addr, e);
            const unsigned long long m = __ballot(win);
            const uint64_t pos = first + __popcll(m & ((1ULL << lane) - 1));
            if (win && pos < Q.cap) {  // pos < cap always: a block wins once, and address 0 never
                Q.address[pos] = ch.address;
                Q.expected[pos] = ch.expected;
                Q.parent[pos] = addr;
                Q.offset[pos] = ch.address * P.block_size;
                Q.len[pos] = ch.len;
                Q.slot[pos] = e;
                Q.tree[pos] = static_cast<uint8_t>(ch.kind | (ch.leaf << 2));
                atomicOr(&bitmap[ch.address >> 5], 1u << (ch.address & 31));
            }
            first += __popcll(m);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (n_enq[k]) atomicAdd(&C->enq[k], static_cast<unsigned long long>(n_enq[k]));
        if (n_err) atomicAdd(&C->n_structural, static_cast<unsigned long long>(n_err));
    }
}

// A level that holds leaves only: the compare of PASS 1 with one lane per row. A wave per row
// that has nothing to expand cost 132 us per 1M leaves, this 6 (DESIGN_LOG.md "Scrub").
__global__ void __launch_bounds__(256) k_scrub_compare(ScrubQueue Q, uint64_t start, uint64_t count, ScrubCounters* C) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= count) return;
    const uint64_t i = start + r;
    if (Q.computed[i] == Q.expected[i]) return;
    atomicAdd(&C->mism[Q.tree[i] & 3], 1ULL);
    atomicMin(&C->key_mismatch, static_cast<unsigned long long>(scrub_key(Q.parent[i], Q.slot[i])));
}

// The level's two first-error keys start empty.
__global__ void k_scrub_level_begin(ScrubCounters* C) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        C->key_mismatch = kScrubNoKey;
        C->key_structural = kScrubNoKey;
    }
}

// Pinned read-back buffer of the calling thread (kept: a scrub reads it once per level).
int scrub_pinned(ScrubCounters** out) {
    thread_local ScrubCounters* h = nullptr;
    if (!h) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(ScrubCounters), hipHostMallocPortable));
    *out = h;
    return STORMCK_OK;
}

template <int PASS>
int scrub_launch(const uint8_t* base, const ScrubParams& P, const ScrubQueue& Q, uint64_t start, uint64_t count,
                 unsigned long long* claim, uint32_t* bitmap, ScrubCounters* C, uint64_t want, hipStream_t st) {
    const uint64_t wgs = (count + 3) / 4;
    if (wgs > 0x7fffffffULL) return fail(STORMCK_EINVAL, "scrub: level too large for one launch");
    hipLaunchKernelGGL(k_scrub_expand<PASS>, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, st, base, P, Q, start, count,
                       claim, bitmap, C, static_cast<unsigned long long>(want));
    HIP_TRY(hipGetLastError());
    return STORMCK_OK;
}

int scrub_walk_device(const uint8_t* base, const ScrubParams& P, const ScrubChild& root, ScrubTotals* T, void* d_workspace,
                      uint32_t* d_reachable, hipStream_t st) {
    const uint64_t n = P.n_blocks, words = (n + 31) / 32;
    uint8_t* w = static_cast<uint8_t*>(d_workspace);
    ScrubCounters* C = reinterpret_cast<ScrubCounters*>(w);
    w += 256;
    uint64_t* col[6];
    for (auto& c : col) {
        c = reinterpret_cast<uint64_t*>(w);
        w += n * 8;
    }
    unsigned long long* claim = reinterpret_cast<unsigned long long*>(col[0]);
    ScrubQueue Q;
    Q.address = col[1], Q.expected = col[2], Q.parent = col[3], Q.offset = col[4], Q.computed = col[5];
    Q.len = reinterpret_cast<uint32_t*>(w);
    Q.slot = Q.len + n;
    w += n * 8;
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(w);
    w += scrub_bitmap_bytes(n);
    Q.tree = w;
    Q.cap = n;

    ScrubCounters* h = nullptr;
    int rc = scrub_pinned(&h);
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));

    const bool walk = scrub_root(root, T);
    if (walk) T->enq[root.kind] = 1;  // as k_scrub_seed counts it
    HIP_TRY(hipMemsetAsync(bitmap, 0, scrub_bitmap_bytes(n), st));
    if (walk) HIP_TRY(hipMemsetAsync(claim, 0xff, n * 8, st));
    hipLaunchKernelGGL(k_scrub_seed, dim3(1), dim3(64), 0, st, Q, root, walk, P.block_size, claim, bitmap, C);
    HIP_TRY(hipGetLastError());

    const uint32_t max_len = std::max(std::max(P.len[0], P.len[1]), std::max(P.len[2], P.len[3]));
    // the detail of the error with key `want` among the rows [s, s + c): one more pass over them
    auto detail = [&](uint64_t s, uint64_t c, uint64_t want, uint32_t lvl) -> int {
        int r = scrub_launch<2>(base, P, Q, s, c, claim, bitmap, C, want, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        T->first = ScrubFirst{true, lvl, want, static_cast<uint32_t>(h->detail[0]), h->detail[1], h->detail[2],
                              h->detail[3]};
        return STORMCK_OK;
    };
    uint64_t start = 0, count = walk ? 1 : 0, prev_start = 0, prev_count = 0;
    uint64_t pending = kScrubNoKey;  // smallest key of the structural errors that point into this level
    uint64_t expandable = count && root.kind <= STORMCK_SCRUB_SPACELIST ? 1 : 0;
    uint32_t lvl = 0;
    for (; count > 0; ++lvl) {
        rc = launch_checksum(base, 0, Q.len + start, max_len, Q.offset + start, count, Q.computed + start, nullptr, nullptr,
                             nullptr, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_scrub_level_begin, dim3(1), dim3(64), 0, st, C);
        HIP_TRY(hipGetLastError());
        if (expandable) {
            rc = scrub_launch<0>(base, P, Q, start, count, claim, bitmap, C, 0, st);
            if (rc) return rc;
            rc = scrub_launch<1>(base, P, Q, start, count, claim, bitmap, C, 0, st);
            if (rc) return rc;
        } else {  // a level of leaves: nothing to claim or enqueue
            const uint64_t wgs = (count + 255) / 256;
            if (wgs > 0x7fffffffULL) return fail(STORMCK_EINVAL, "scrub: level too large for one launch");
            hipLaunchKernelGGL(k_scrub_compare, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, st, Q, start, count, C);
            HIP_TRY(hipGetLastError());
        }
        const uint64_t before = T->enq[0] + T->enq[1];
        HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rc = take_fault(dev, st);  // a ring kernel of the dispatch that stalled wrote no checksums
        if (rc) return rc;
        for (int k = 0; k < 4; ++k) {
            T->enq[k] = h->enq[k];
            T->mism[k] = h->mism[k];
        }
        T->n_structural = h->n_structural;
        T->levels = lvl + 1;
        const uint64_t km = h->key_mismatch, ks = h->key_structural, tail = h->tail;
        if (tail < start + count || tail > n) return fail(STORMCK_EHIP, "scrub: the frontier queue is inconsistent");
        if (!T->first.have && (pending != kScrubNoKey || km != kScrubNoKey)) {
            rc = pending < km ? detail(prev_start, prev_count, pending, lvl) : detail(start, count, km, lvl);
            if (rc) return rc;
        }
        pending = ks;
        expandable = T->enq[0] + T->enq[1] - before;
        prev_start = start;
        prev_count = count;
        start += count;
        count = tail - start;
    }
    if (!T->first.have && pending != kScrubNoKey) {
        rc = detail(prev_start, prev_count, pending, lvl);
        if (rc) return rc;
    }
    if (d_reachable) HIP_TRY(hipMemcpyAsync(d_reachable, bitmap, words * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // synchronous, also when there was nothing to walk
    return STORMCK_OK;
}

// The checks every device entry makes after its arguments: the device, the stream.
int scrub_device_ready(const void* d_store, const void* d_workspace, uint64_t workspace_bytes, uint64_t n_blocks,
                       hipStream_t st) {
    if (!d_workspace || workspace_bytes < scrub_workspace_bytes(n_blocks))
        return fail(STORMCK_EINVAL, "scrub: workspace too small (stormck_scrub_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace)) & 7)
        return fail(STORMCK_EINVAL, "scrub: d_store and d_workspace must be 8-byte aligned");
    const int rc = device_check();
    if (rc) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "scrub: stream is being captured (a scrub synchronises its stream every level)");
    return STORMCK_OK;
}

int scrub_device(const void* d_store, const stormck_scrub_layout* layout, void* d_workspace, uint64_t workspace_bytes,
                 uint32_t* d_reachable, stormck_scrub_report* report, void* stream) {
    ScrubParams P;
    int rc = scrub_params(d_store, layout, report, -1, 0, &P);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = scrub_device_ready(d_store, d_workspace, workspace_bytes, P.n_blocks, st);
    if (rc) return rc;
    uint8_t sing[kScrubSingLen];
    if (P.block_size < kScrubSingLen) return fail(STORMCK_EINVAL, "scrub: block_size below the singularity's 72 bytes");
    HIP_TRY(hipMemcpyAsync(sing, d_store, kScrubSingLen, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ScrubTotals T;
    ScrubChild root{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
    scrub_singularity(P, sing, &T, &root);  // on a failure the root stays Free: only bit 0 is set
    rc = scrub_walk_device(static_cast<const uint8_t*>(d_store), P, root, &T, d_workspace, d_reachable, st);
    if (rc) return rc;
    return scrub_finish(P, T, report);
}

int scrub_tree_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                      uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, void* d_workspace,
                      uint64_t workspace_bytes, uint32_t* d_reachable, stormck_scrub_report* report, void* stream) {
    if (!root) return fail(STORMCK_EINVAL, "scrub: root is null");
    if (leaf_kind > STORMCK_SCRUB_BLOB) return fail(STORMCK_EINVAL, "scrub: leaf_kind must be spacelist, objectlist or blob");
    ScrubParams P;
    int rc = scrub_params(d_store, layout, report, static_cast<int>(leaf_kind), leaf_len, &P);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = scrub_device_ready(d_store, d_workspace, workspace_bytes, P.n_blocks, st);
    if (rc) return rc;
    ScrubTotals T;
    const ScrubChild r = scrub_ref(P, root->checksum, root->address, root_type, static_cast<uint8_t>(leaf_kind));
    rc = scrub_walk_device(static_cast<const uint8_t*>(d_store), P, r, &T, d_workspace, d_reachable, st);
    if (rc) return rc;
    return scrub_finish(P, T, report);
}

int scrub_host(const void* store, const stormck_scrub_layout* layout, uint32_t* reachable, stormck_scrub_report* report,
               uint32_t threads) {
    ScrubParams P;
    int rc = scrub_params(store, layout, report, -1, 0, &P);
    if (rc) return rc;
    if (P.block_size < kScrubSingLen) return fail(STORMCK_EINVAL, "scrub: block_size below the singularity's 72 bytes");
    ScrubTotals T;
    ScrubChild root{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
    scrub_singularity(P, static_cast<const uint8_t*>(store), &T, &root);
    rc = scrub_walk_host(static_cast<const uint8_t*>(store), P, root, &T, reachable, threads);
    if (rc) return rc;
    return scrub_finish(P, T, report);
}

int scrub_tree_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                    uint32_t leaf_kind, uint32_t leaf_len, uint32_t* reachable, stormck_scrub_report* report,
                    uint32_t threads) {
    if (!root) return fail(STORMCK_EINVAL, "scrub: root is null");
    if (leaf_kind > STORMCK_SCRUB_BLOB) return fail(STORMCK_EINVAL, "scrub: leaf_kind must be spacelist, objectlist or blob");
    ScrubParams P;
    int rc = scrub_params(store, layout, report, static_cast<int>(leaf_kind), leaf_len, &P);
    if (rc) return rc;
    ScrubTotals T;
    const ScrubChild r = scrub_ref(P, root->checksum, root->address, root_type, static_cast<uint8_t>(leaf_kind));
    rc = scrub_walk_host(static_cast<const uint8_t*>(store), P, r, &T, reachable, threads);
    if (rc) return rc;
    return scrub_finish(P, T, report);
}
