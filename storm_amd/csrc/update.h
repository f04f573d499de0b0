// Update: storm.Set for keys that already have an object, as a new revision (include/stormck.h
// "update"; DESIGN.md "Update").
//
// Included by stormck.hip inside an anonymous namespace, after get.h. A call is the get (get_host,
// get_device: called, not restated), the winner of every slot, the walk that finds the dirty
// blocks, the plan (update_plan.h, on the host for both legs), the copy of the dirty blocks to
// their new addresses, the store of the rows, the commit (stormck_commit_host / _device over the
// planned records: called, not restated) and the singularity.
//
// What is here: the step of a walk both legs share (update_descend), the host leg, and the device
// leg with its kernels: k_update_claim and k_update_actions (the winners), k_update_space_walk and
// k_update_walk (the dirty blocks), k_update_copy (the move) and k_object_store (the rows).

static_assert(sizeof(stormck_update_result) == 32 && sizeof(stormck_update_result) == sizeof(stormck_get_result) &&
                  offsetof(stormck_update_result, action) == offsetof(stormck_get_result, reserved),
              "stormck_update_result is stormck_get_result with its reserved field split");
static_assert(sizeof(stormck::UpdateDirty) == 24, "one small record per dirty block");

using stormck::UpdateDirty;
using stormck::UpdateError;
using stormck::UpdateGeometry;
using stormck::UpdatePlan;

constexpr uint32_t kUpdateMaxDepth = 64;  // the trace's DEPTH rule: a FOUND walk verified at most 64 pointer blocks
constexpr uint64_t kUpdateTail = 72;      // records past the level's: the space's path, at most 64 + 1 blocks

struct UpdateParams {
    UpdateGeometry G;
    uint32_t S;
    uint64_t in_stride;
};

// The slot (object_address, index) as one table key: index is below 4096 (objects_per_block is
// at most 4095) and the address below 2^36.
__host__ __device__ inline uint64_t update_slot_key(uint64_t address, uint32_t index) { return (address << 12) | index; }

__host__ __device__ inline bool update_applicable(const stormck_update_result& r) {
    return r.stage == 2 && r.status == STORMCK_TRACE_FOUND;
}

// A reference on a walk: the block it names, its type, and its origin (parent, slot).
struct UpdateStep {
    uint64_t address, parent, rem;
    uint32_t slot;
    uint8_t type;
};

// A reference the get verified names a pointer block or a leaf inside the image.
__host__ __device__ inline bool update_step_ok(const UpdateStep& s, uint64_t n_blocks) {
    return (s.type == STORMCK_POINTER_BLOCK || s.type == STORMCK_LEAF_BLOCK) && s.address != 0 && s.address < n_blocks;
}

// From the pointer block s names to the reference its walk takes there (cache/trace.go:21-33).
__host__ __device__ inline void update_descend(const uint8_t* base, const UpdateGeometry& G, UpdateStep* s) {
    const uint8_t* blk = base + s->address * G.block_size;
    const uint32_t e = static_cast<uint32_t>(s->rem % G.fanout);
    s->rem /= G.fanout;
    s->parent = s->address;
    s->slot = e;
    s->address = scrub_le64(blk + 24ull * e + 8);
    s->type = blk[24ull * G.fanout + e];
}

uint64_t update_table_slots(uint64_t n) { return trace_table_slots(n); }

uint64_t update_workspace_bytes(uint64_t n, uint32_t C) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return ((get_workspace_bytes(n, C) + 7) & ~uint64_t{7}) + 12 * update_table_slots(n) + 24 * (m + kUpdateTail) + 64;
}

void update_report_clear(stormck_update_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    get_report_clear(&r->get, n);
}

// The argument checks both legs share, before any work: the get's, then the call's own.
int update_params(const void* store, const stormck_scrub_layout* layout, const stormck_get_params* params, const void* keys,
                  const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride, uint32_t flags,
                  const stormck_update_result* results, stormck_update_report* report, UpdateParams* P) {
    if (!report) return fail(STORMCK_EINVAL, "update: null argument");
    GetParams gp;
    const int rc = get_params(store, layout, params, keys, lens, len, n, 0, reinterpret_cast<const stormck_get_result*>(results),
                              nullptr, 0, &report->get, &gp);
    if (rc) return rc;
    if (flags != 0) return fail(STORMCK_EINVAL, "update: flags must be 0 (every leaf is verified)");
    if (in_stride < gp.S) return fail(STORMCK_EINVAL, "update: in_stride is below object_size");
    if (n && !objects) return fail(STORMCK_EINVAL, "update: null argument");
    ScrubParams sp;
    const stormck_scrub_report unused{};
    (void)scrub_params(store, layout, &unused, -1, 0, &sp);  // checked before: get_params
    P->G.block_size = layout->block_size;
    P->G.n_blocks = layout->n_blocks;
    P->G.fanout = layout->pointer_fanout;
    for (int k = 0; k < 4; ++k) P->G.len[k] = sp.len[k];
    P->S = gp.S;
    P->in_stride = in_stride;
    return STORMCK_OK;
}

// The walk's first references: the space's from the singularity, the objects' from the space's record.
UpdateStep update_space_root(const uint8_t* sing, uint64_t space_id) {
    return UpdateStep{scrub_le64(sing + 40), 0, space_id, 0, sing[56]};
}
UpdateStep update_object_root(const stormck_space_result& s) {
    return UpdateStep{s.object_root.address, s.address, 0, s.index, s.object_type};
}

int update_plan_fail(UpdateError e) {
    return fail(e == UpdateError::NoSpace ? STORMCK_ENOSPC : STORMCK_EINVAL, stormck::update_error_message(e));
}

void update_report_plan(stormck_update_report* r, const UpdatePlan& plan, const UpdateGeometry& G, uint64_t revision) {
    for (int k = 0; k < 4; ++k) r->n_dirty[k] = plan.n_dirty[k];
    r->bytes_copied = plan.records.size() * G.block_size;
    r->bytes_hashed = plan.bytes_hashed + kScrubSingLen;
    r->revision = revision + 1;
    r->last_allocated = plan.last_allocated;
    r->first_new = plan.first_new;
    r->heights = plan.heights;
}

// ---- host leg ---------------------------------------------------------------------------

int update_host(void* store_v, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
                const void* keys, uint64_t stride, const uint64_t* offsets, const uint32_t* lens, uint32_t len, uint64_t n,
                const void* objects_v, uint64_t in_stride, uint32_t flags, stormck_update_result* results,
                stormck_update_report* report, uint32_t threads) {
    UpdateParams P;
    int rc = update_params(store_v, layout, params, keys, lens, len, n, objects_v, in_stride, flags, results, report, &P);
    if (rc) return rc;
    update_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    uint8_t* base = static_cast<uint8_t*>(store_v);
    const uint8_t* objects = static_cast<const uint8_t*>(objects_v);
    const UpdateGeometry& G = P.G;
    // A. locate
    rc = get_host(store_v, layout, space_id, params, keys, stride, offsets, lens, len, n, 0,
                  reinterpret_cast<stormck_get_result*>(results), nullptr, 0, &report->get, threads);
    if (rc) return rc;  // EMISMATCH with the get's text: every action is NONE as the get left it
    uint8_t sing[kScrubSingLen];
    std::memcpy(sing, base, kScrubSingLen);
    const uint64_t revision = scrub_le64(sing + 16), last = scrub_le64(sing + 64);
    report->revision = revision;
    report->last_allocated = last;
    // B. select: the last key of every slot
    std::unordered_map<uint64_t, uint64_t> winner;
    for (uint64_t i = 0; i < n; ++i)
        if (update_applicable(results[i])) winner[update_slot_key(results[i].object_address, results[i].index)] = i;
    for (uint64_t i = 0; i < n; ++i) {
        if (!update_applicable(results[i])) continue;
        const bool won = winner[update_slot_key(results[i].object_address, results[i].index)] == i;
        results[i].action = won ? STORMCK_UPDATE_WRITTEN : STORMCK_UPDATE_SUPERSEDED;
        ++(won ? report->n_written : report->n_superseded);
    }
    if (report->n_written == 0) return STORMCK_OK;
    // C. the dirty forest
    std::vector<UpdateDirty> dirty;
    std::unordered_set<uint64_t> seen;
    auto walk = [&](UpdateStep s, uint32_t leaf_kind, uint64_t leaf) {
        for (uint32_t depth = 0; depth <= kUpdateMaxDepth; ++depth) {
            if (!update_step_ok(s, G.n_blocks)) return false;
            const bool pointer = s.type == STORMCK_POINTER_BLOCK;
            if (seen.insert(s.address).second)
                dirty.push_back(UpdateDirty{s.address, s.parent, s.slot, pointer ? uint32_t{STORMCK_SCRUB_POINTER} : leaf_kind});
            if (!pointer) return s.address == leaf;
            update_descend(base, G, &s);
        }
        return false;
    };
    bool on_path = walk(update_space_root(sing, space_id), STORMCK_SCRUB_SPACELIST, report->get.space.address);
    for (uint64_t i = 0; i < n && on_path; ++i) {
        if (results[i].action != STORMCK_UPDATE_WRITTEN) continue;
        UpdateStep s = update_object_root(report->get.space);
        s.rem = results[i].object_id;
        on_path = walk(s, STORMCK_SCRUB_BLOB, results[i].object_address);
    }
    if (!on_path) return fail(STORMCK_EINVAL, "update: a walk left the path the get verified");
    UpdatePlan plan;
    const UpdateError e = stormck::update_plan(dirty.data(), dirty.size(), G, revision, last, &plan);
    if (e != UpdateError::Ok) return update_plan_fail(e);
    // D. write: the copies, the rows, the commit, the singularity
    const uint64_t D = plan.records.size();
    std::unordered_map<uint64_t, uint64_t> moved;  // old leaf -> new leaf
    for (uint64_t k = 0; k < D; ++k) {
        std::memcpy(base + (plan.first_new + k) * G.block_size, base + plan.old_address[k] * G.block_size, G.block_size);
        if (plan.kind[k] == STORMCK_SCRUB_BLOB) moved[plan.old_address[k]] = plan.first_new + k;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (results[i].action == STORMCK_UPDATE_WRITTEN) {
            uint8_t* leaf = base + moved[results[i].object_address] * G.block_size;
            std::memcpy(const_cast<uint8_t*>(stormck::blob_object(leaf, P.S, results[i].index)), objects + i * in_stride, P.S);
        }
    std::vector<uint64_t> checksums(D);
    uint64_t unused_last = last;
    rc = stormck_commit_host(base, plan.records.data(), D, revision, &unused_last, checksums.data(), threads);
    if (rc) return rc;
    stormck::update_singularity(sing, checksums[D - 1], plan, revision,
                                [](const uint8_t* p, size_t len) { return stormck::host::xxh64(p, len); });
    std::memcpy(base, sing, kScrubSingLen);
    update_report_plan(report, plan, G, revision);
    return STORMCK_OK;
}

// ---- device engine ------------------------------------------------------------------------

struct UpdateCounters {
    unsigned long long n_written, n_superseded;
    unsigned long long count, alive;  // of one k_update_walk: its records, its lanes that go deeper
    unsigned long long space_count;   // k_update_space_walk's records
    unsigned long long error;         // a full table, a missing key, a walk off the verified path: never
    unsigned long long pad[2];
};
static_assert(sizeof(UpdateCounters) == 64, "the counters take the last 64 bytes of the workspace");

constexpr uint64_t kUpdateNoKey = UINT64_MAX;  // update_slot_key() and addresses stay below 2^48
constexpr uint64_t kUpdateLeafFlag = uint64_t{1} << 63;  // in a copy's source: the block is a blob leaf

struct UpdateTable {
    unsigned long long* keys;  // memset to 0xff before use
    uint32_t* val;
    uint64_t mask;
};

// The position of `key`, inserted when it is not there (*owner: by this lane); kUpdateNoKey for a
// full table, which its size makes impossible. Probing never waits: a slot goes from empty to one
// key, once (as k_trace_step's).
__device__ inline uint64_t update_table_put(const UpdateTable& T, unsigned long long key, bool* owner) {
    uint64_t h = trace_mix(key) & T.mask;
    *owner = false;
    for (uint64_t probe = 0; probe <= T.mask; ++probe, h = (h + 1) & T.mask) {
        unsigned long long cur = T.keys[h];
        if (cur == kUpdateNoKey) {
            cur = atomicCAS(&T.keys[h], static_cast<unsigned long long>(kUpdateNoKey), key);
            if (cur == kUpdateNoKey) {
                *owner = true;
                return h;
            }
        }
        if (cur == key) return h;
    }
    return kUpdateNoKey;
}

// The position of `key` in a table an earlier kernel filled; kUpdateNoKey when it is not there.
__device__ inline uint64_t update_table_find(const UpdateTable& T, unsigned long long key) {
    uint64_t h = trace_mix(key) & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; ++probe, h = (h + 1) & T.mask) {
        const unsigned long long cur = T.keys[h];
        if (cur == key) return h;
        if (cur == kUpdateNoKey) break;
    }
    return kUpdateNoKey;
}

// One lane per key: an applicable key claims its slot with i + 1; the largest stays.
__global__ void __launch_bounds__(256) k_update_claim(const stormck_update_result* __restrict__ results, uint64_t n,
                                                      UpdateTable T, UpdateCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const stormck_update_result r = results[i];
    if (!update_applicable(r)) return;
    bool owner;
    const uint64_t h = update_table_put(T, update_slot_key(r.object_address, r.index), &owner);
    if (h == kUpdateNoKey) {
        atomicOr(&C->error, 1ULL);
        return;
    }
    atomicMax(&T.val[h], static_cast<uint32_t>(i + 1));  // n <= 2^31
}

// After k_update_claim's kernel boundary: each applicable key's action, counted per wave as
// object_count counts (__ballot / __popcll, one atomicAdd per wave per counter).
__global__ void __launch_bounds__(256) k_update_actions(stormck_update_result* __restrict__ results, uint64_t n,
                                                        UpdateTable T, UpdateCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    uint8_t action = STORMCK_UPDATE_NONE;  // no early return: the wave votes below
    if (i < n) {
        const stormck_update_result r = results[i];
        if (update_applicable(r)) {
            const uint64_t h = update_table_find(T, update_slot_key(r.object_address, r.index));
            if (h == kUpdateNoKey) {
                atomicOr(&C->error, 2ULL);
            } else {
                action = T.val[h] == static_cast<uint32_t>(i + 1) ? STORMCK_UPDATE_WRITTEN : STORMCK_UPDATE_SUPERSEDED;
                results[i].action = action;
            }
        }
    }
    const unsigned long long w = __ballot(action == STORMCK_UPDATE_WRITTEN);
    const unsigned long long s = __ballot(action == STORMCK_UPDATE_SUPERSEDED);
    if (lane == 0) {
        if (w) atomicAdd(&C->n_written, static_cast<unsigned long long>(__popcll(w)));
        if (s) atomicAdd(&C->n_superseded, static_cast<unsigned long long>(__popcll(s)));
    }
}

// One lane: the blocks on the space ID's walk, in walk order, into records[0, space_count).
__global__ void __launch_bounds__(64) k_update_space_walk(const uint8_t* __restrict__ base, UpdateGeometry G, UpdateStep s,
                                                          UpdateDirty* __restrict__ records, UpdateCounters* C) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t count = 0;
    bool ok = false;
    for (uint32_t depth = 0; depth <= kUpdateMaxDepth; ++depth) {
        if (!update_step_ok(s, G.n_blocks)) break;
        const bool pointer = s.type == STORMCK_POINTER_BLOCK;
        records[count++] = UpdateDirty{s.address, s.parent, s.slot,
                                       pointer ? uint32_t{STORMCK_SCRUB_POINTER} : uint32_t{STORMCK_SCRUB_SPACELIST}};
        if (!pointer) {
            ok = true;
            break;
        }
        update_descend(base, G, &s);
    }
    if (!ok) atomicOr(&C->error, 4ULL);
    C->space_count = count;
}

// Which items a walk follows, and the tag of each: the update's are its WRITTEN keys with their
// object IDs.
struct UpdatePick {
    const stormck_update_result* results;
    __device__ bool operator()(uint64_t i, uint64_t* tag) const {
        if (results[i].action != STORMCK_UPDATE_WRITTEN) return false;
        *tag = results[i].object_id;
        return true;
    }
};

// One lane per item that `pick` takes (the update: per WRITTEN key): the block at `depth` on its
// tag's walk from `root` (the update: its object ID's, from the object root; the blocks were
// verified before: nothing is hashed). The lane that installs the block in the table, which the
// host clears per level, appends its record, a leaf's with `leaf_kind`; a wave claims its records
// with one atomicAdd. A lane whose block is a pointer block says that a deeper level exists.
template <class Pick>
__global__ void __launch_bounds__(256) k_update_walk(const uint8_t* __restrict__ base, UpdateGeometry G, Pick pick,
                                                     uint64_t n, UpdateStep root, uint32_t depth, uint32_t leaf_kind,
                                                     UpdateTable T, UpdateDirty* __restrict__ records, uint64_t cap,
                                                     UpdateCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool here = false, owner = false, deeper = false;  // no early return: the wave votes below
    UpdateStep s = root;
    uint64_t tag = 0;
    if (i < n && pick(i, &tag)) {
        s.rem = tag;
        here = true;
        for (uint32_t d = 0; d < depth && here; ++d) {
            if (!update_step_ok(s, G.n_blocks)) {
                atomicOr(&C->error, 8ULL);
                here = false;
            } else if (s.type != STORMCK_POINTER_BLOCK) {
                here = false;  // the walk ended at a shallower leaf
            } else {
                update_descend(base, G, &s);
            }
        }
        if (here && !update_step_ok(s, G.n_blocks)) {
            atomicOr(&C->error, 8ULL);
            here = false;
        }
        if (here) {
            deeper = s.type == STORMCK_POINTER_BLOCK;
            if (update_table_put(T, s.address, &owner) == kUpdateNoKey) atomicOr(&C->error, 1ULL);
        }
    }
    const unsigned long long own = __ballot(owner);
    if (own) {
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&C->count, static_cast<unsigned long long>(__popcll(own)));
        first = __shfl(first, 0);
        const uint64_t idx = first + __popcll(own & ((1ULL << lane) - 1));
        if (owner) {
            if (idx < cap)  // always: a level has at most as many distinct blocks as WRITTEN keys
                records[idx] = UpdateDirty{s.address, s.parent, s.slot,
                                           deeper ? uint32_t{STORMCK_SCRUB_POINTER} : leaf_kind};
            else
                atomicOr(&C->error, 16ULL);
        }
    }
    if (__ballot(deeper) && lane == 0) atomicOr(&C->alive, 1ULL);
}

// The block move: one workgroup per dirty block, pairs[2 b] = its old address (with
// kUpdateLeafFlag for a blob leaf), pairs[2 b + 1] = its new one. 16-byte loads and stores, the
// lanes of one instruction on consecutive addresses, when both blocks are 16-byte aligned (the
// last 8 bytes of a block_size that is 8 mod 16 go as one word); 8-byte words otherwise. Lane 0
// of a leaf's workgroup enters old address -> new address - first_new into the table, for
// k_object_store.
__global__ void __launch_bounds__(256) k_update_copy(uint8_t* __restrict__ base, uint64_t block_size,
                                                     const uint64_t* __restrict__ pairs, uint64_t first_new, UpdateTable T,
                                                     UpdateCounters* C) {
    const uint64_t from = pairs[2ull * blockIdx.x], to = pairs[2ull * blockIdx.x + 1];
    const uint64_t old = from & ~kUpdateLeafFlag;
    const uint8_t* src = base + old * block_size;
    uint8_t* dst = base + to * block_size;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const uint64_t quads = block_size / 16;
        const uint4* s = reinterpret_cast<const uint4*>(src);
        uint4* d = reinterpret_cast<uint4*>(dst);
        for (uint64_t q = threadIdx.x; q < quads; q += 256) d[q] = s[q];
        if ((block_size & 8) && threadIdx.x == 0)
            *reinterpret_cast<uint64_t*>(dst + 16 * quads) = *reinterpret_cast<const uint64_t*>(src + 16 * quads);
    } else {
        const uint64_t words = block_size / 8;  // block_size is a multiple of 8, the store 8-byte aligned
        const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
        uint64_t* d = reinterpret_cast<uint64_t*>(dst);
        for (uint64_t w = threadIdx.x; w < words; w += 256) d[w] = s[w];
    }
    if ((from & kUpdateLeafFlag) && threadIdx.x == 0) {
        bool owner;
        const uint64_t h = update_table_put(T, old, &owner);
        if (h == kUpdateNoKey || !owner) atomicOr(&C->error, 32ULL);
        else T.val[h] = static_cast<uint32_t>(to - first_new);  // below D <= 2^32
    }
}

// The mirror of object_row: one row of S bytes from src (any alignment) to dst (8-byte aligned: an
// object slot) by the lanes first, first + step, ...: 8-byte words and then the tail's bytes when
// src is aligned, bytes otherwise.
__device__ inline void object_row_store(uint8_t* dst, const uint8_t* src, uint32_t S, uint32_t first, uint32_t step) {
    if ((reinterpret_cast<uintptr_t>(src) & 7) == 0) {
        const uint32_t words = S / 8;
        uint64_t* d = reinterpret_cast<uint64_t*>(dst);
        const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
        for (uint32_t w = first; w < words; w += step) d[w] = s[w];
        for (uint32_t b = 8 * words + first; b < S; b += step) dst[b] = src[b];
    } else {
        for (uint32_t b = first; b < S; b += step) dst[b] = src[b];
    }
}

// The mirror of object_move: the store of one lane's row (dst null: the lane has none). Every lane
// of the wave calls it. WAVE false: each lane stores its own row. WAVE true: the wave walks its
// rows in lane order and all 64 lanes move the S bytes of one row together.
template <bool WAVE>
__device__ inline void object_put(uint8_t* dst, const uint8_t* src, uint32_t S) {
    if constexpr (!WAVE) {
        if (dst) object_row_store(dst, src, S, 0, 1);
    } else {
        const uint32_t lane = threadIdx.x & 63;
        unsigned long long rows = __ballot(dst != nullptr);  // the same in every lane, and so is the loop
        while (rows) {
            const int from = __ffsll(rows) - 1;
            rows &= rows - 1;
            const uint8_t* s = reinterpret_cast<const uint8_t*>(__shfl(reinterpret_cast<unsigned long long>(src), from));
            uint8_t* d = reinterpret_cast<uint8_t*>(__shfl(reinterpret_cast<unsigned long long>(dst), from));
            object_row_store(d, s, S, lane, 64);
        }
    }
}

// One lane per key, the inverse of k_object_fetch's move: a WRITTEN key's row goes to its slot's
// object in the new copy of its leaf (k_update_copy's table), in the form WAVE names. No two
// WRITTEN keys name one slot.
template <bool WAVE>
__global__ void __launch_bounds__(256) k_object_store(uint8_t* __restrict__ base, UpdateParams P,
                                                      const stormck_update_result* __restrict__ results, uint64_t n,
                                                      const uint8_t* __restrict__ objects, uint64_t first_new,
                                                      uint64_t n_dirty, UpdateTable T, UpdateCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    uint8_t* dst = nullptr;  // no early return: the wave moves its rows together
    if (i < n) {
        const stormck_update_result r = results[i];
        if (r.action == STORMCK_UPDATE_WRITTEN) {
            const uint64_t h = update_table_find(T, r.object_address);
            const uint64_t k = h == kUpdateNoKey ? n_dirty : T.val[h];
            if (k >= n_dirty)  // never: the leaf of a WRITTEN key is dirty
                atomicOr(&C->error, 64ULL);
            else  // index is below N and N slots fit blob_len: the objects call's own bounds
                dst = const_cast<uint8_t*>(stormck::blob_object(base + (first_new + k) * P.G.block_size, P.S, r.index));
        }
    }
    object_put<WAVE>(dst, objects + i * P.in_stride, P.S);
}

// Which form of the store runs: the fetch's rule, until the store direction is measured
// (DESIGN.md "Update").
bool store_wave(uint32_t S) { return S >= kFetchWaveMin; }

int update_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
                  const void* d_keys, uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t len,
                  uint64_t n, const void* d_objects, uint64_t in_stride, uint32_t flags, stormck_update_result* d_results,
                  void* d_workspace, uint64_t workspace_bytes, stormck_update_report* report, void* stream) {
    UpdateParams P;
    int rc = update_params(d_store, layout, params, d_keys, d_lens, len, n, d_objects, in_stride, flags, d_results, report, &P);
    if (rc) return rc;
    const uint32_t chunks = params->keys.chunks_per_block;
    if (n && (!d_workspace || workspace_bytes < update_workspace_bytes(n, chunks)))
        return fail(STORMCK_EINVAL, "update: workspace too small (stormck_update_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_offsets)) & 7)
        return fail(STORMCK_EINVAL, "update: d_store, d_results, d_offsets and d_workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_lens) & 3) return fail(STORMCK_EINVAL, "update: d_lens must be 4-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "update: stream is being captured (the call synchronises its stream)");
    update_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    const UpdateGeometry& G = P.G;
    uint8_t* base = static_cast<uint8_t*>(d_store);

    // A. locate: the get, in the first part of the workspace
    const uint64_t get_bytes = (get_workspace_bytes(n, chunks) + 7) & ~uint64_t{7};
    rc = get_device(d_store, layout, space_id, params, d_keys, stride, d_offsets, d_lens, len, n, 0,
                    reinterpret_cast<stormck_get_result*>(d_results), nullptr, 0, d_workspace, get_bytes, &report->get, stream);
    if (rc) return rc;  // EMISMATCH with the get's text: every action is NONE as the get left it
    uint8_t sing[kScrubSingLen];
    HIP_TRY(hipMemcpyAsync(sing, d_store, kScrubSingLen, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t revision = scrub_le64(sing + 16), last = scrub_le64(sing + 64);
    report->revision = revision;
    report->last_allocated = last;
    if (report->get.n_found == 0) return STORMCK_OK;  // no key is applicable

    // the call's own part of the workspace: the table, the records, the counters
    const uint64_t m = (n + 7) & ~uint64_t{7}, slots = update_table_slots(n);
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + get_bytes;
    UpdateTable T{reinterpret_cast<unsigned long long*>(w), reinterpret_cast<uint32_t*>(w + 8 * slots), slots - 1};
    w += 12 * slots;
    UpdateDirty* records = reinterpret_cast<UpdateDirty*>(w);
    const uint64_t record_cap = m + kUpdateTail;
    w += 24 * record_cap;
    UpdateCounters* C = reinterpret_cast<UpdateCounters*>(w);
    UpdateCounters h;
    const unsigned wgs = static_cast<unsigned>((n + 255) / 256);  // n <= 2^31

    // B. select
    HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
    HIP_TRY(hipMemsetAsync(T.val, 0, 4 * slots, st));
    HIP_TRY(hipMemsetAsync(C, 0, sizeof *C, st));
    hipLaunchKernelGGL(k_update_claim, dim3(wgs), dim3(256), 0, st, d_results, n, T, C);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_update_actions, dim3(wgs), dim3(256), 0, st, d_results, n, T, C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, C, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h.error || h.n_written + h.n_superseded != report->get.n_found)
        return fail(STORMCK_EHIP, "update: the selection is inconsistent");
    report->n_written = h.n_written;
    report->n_superseded = h.n_superseded;
    if (h.n_written == 0) return STORMCK_OK;  // never: some applicable key is the last of its slot

    // C. the dirty forest: the space's path, then the object tree one level per launch
    std::vector<UpdateDirty> dirty;
    auto read_records = [&](const UpdateDirty* from, uint64_t count) -> int {
        const size_t at = dirty.size();
        dirty.resize(at + count);
        HIP_TRY(hipMemcpyAsync(dirty.data() + at, from, count * sizeof(UpdateDirty), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return STORMCK_OK;
    };
    hipLaunchKernelGGL(k_update_space_walk, dim3(1), dim3(64), 0, st, base, G, update_space_root(sing, space_id),
                       records + m, C);
    HIP_TRY(hipGetLastError());
    const UpdateStep object_root = update_object_root(report->get.space);
    for (uint32_t depth = 0;; ++depth) {
        if (depth > kUpdateMaxDepth) return fail(STORMCK_EHIP, "update: a walk left the path the get verified");
        HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
        HIP_TRY(hipMemsetAsync(&C->count, 0, 16, st));  // count and alive
        hipLaunchKernelGGL(k_update_walk<UpdatePick>, dim3(wgs), dim3(256), 0, st, base, G, UpdatePick{d_results}, n,
                           object_root, depth, uint32_t{STORMCK_SCRUB_BLOB}, T, records, m, C);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, C, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h.error || h.count > m || h.space_count > kUpdateTail)
            return fail(STORMCK_EHIP, "update: a walk left the path the get verified");
        if (depth == 0) {
            rc = read_records(records + m, h.space_count);
            if (rc) return rc;
        }
        rc = read_records(records, h.count);
        if (rc) return rc;
        if (!h.alive) break;
    }
    UpdatePlan plan;
    const UpdateError e = stormck::update_plan(dirty.data(), dirty.size(), G, revision, last, &plan);
    if (e != UpdateError::Ok) return update_plan_fail(e);

    // D. write: the copies (in pieces the records' region holds), the rows, the commit, the singularity
    const uint64_t D = plan.records.size();
    std::vector<uint64_t> pairs(2 * D);
    for (uint64_t k = 0; k < D; ++k) {
        pairs[2 * k] = plan.old_address[k] | (plan.kind[k] == STORMCK_SCRUB_BLOB ? kUpdateLeafFlag : 0);
        pairs[2 * k + 1] = plan.first_new + k;
    }
    uint64_t* d_pairs = reinterpret_cast<uint64_t*>(records);
    const uint64_t piece = std::min<uint64_t>(24 * record_cap / 16, 1u << 30);
    HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
    for (uint64_t k = 0; k < D; k += piece) {
        const uint64_t cnt = std::min(piece, D - k);
        HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data() + 2 * k, 16 * cnt, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_update_copy, dim3(static_cast<unsigned>(cnt)), dim3(256), 0, st, base, G.block_size, d_pairs,
                           plan.first_new, T, C);
        HIP_TRY(hipGetLastError());
    }
    const uint8_t* objects = static_cast<const uint8_t*>(d_objects);
    with_consts([&](auto WAVE) {
        hipLaunchKernelGGL((k_object_store<STORMCK_V(WAVE)>), dim3(wgs), dim3(256), 0, st, base, P, d_results, n, objects,
                           plan.first_new, D, T, C);
    }, store_wave(P.S));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, C, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h.error) return fail(STORMCK_EHIP, "update: the store of the rows is inconsistent");  // the old revision stays valid
    std::vector<uint64_t> checksums(D);
    uint64_t unused_last = last;
    rc = stormck_commit_device(d_store, plan.records.data(), D, revision, &unused_last, checksums.data(), stream);
    if (rc) return rc;
    stormck::update_singularity(sing, checksums[D - 1], plan, revision,
                                [](const uint8_t* p, size_t len) { return stormck::host::xxh64(p, len); });
    HIP_TRY(hipMemcpyAsync(d_store, sing, kScrubSingLen, hipMemcpyHostToDevice, st));  // the call's last store
    HIP_TRY(hipStreamSynchronize(st));
    update_report_plan(report, plan, G, revision);
    return STORMCK_OK;
}
