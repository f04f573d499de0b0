// Insert: storm.Set for new keys whose leaves have room, as a new revision (include/stormck.h
// "insert"; DESIGN.md "Insert").
//
// Included by stormck.hip inside an anonymous namespace, after update.h. A call is the locate
// (the singularity's check, spaces_*, lookup_*: called, not restated), the key stage per
// objectlist leaf (objlist_insert.h), the ranks, the object stage (objects_* over the new IDs,
// then blob_insert.h per blob leaf), the cut, the dirty walks, the plan (update_plan.h), the
// write and the commit (stormck_commit_*), and the singularity.
//
// What is here: the result of a key from its lookup (insert_located), the host leg in plain
// loops, and the device leg with its kernels: the grouping by leaf (k_group_*), k_insert_keys,
// the ranks (the get's compaction over InsertRankPick, k_insert_ids), k_insert_slots, k_insert_cut and
// k_insert_tally. The walks and the block move are the update's (k_update_space_walk,
// k_update_walk, k_update_copy).

static_assert(sizeof(stormck_insert_result) == 40 && offsetof(stormck_insert_result, key_index) == 24 &&
                  offsetof(stormck_insert_result, stage) == 32 && offsetof(stormck_insert_result, wrote) == 36,
              "stormck_insert_result is 40 bytes");
static_assert(stormck::objlist_leaf_len(STORMCK_INSERT_MAX_CHUNKS) + 4 * STORMCK_INSERT_MAX_PER_LEAF + 8 <= 65536,
              "a leaf image and the ordering buffer fit 64 KiB of LDS");

constexpr uint32_t kInsertOrderBytes = 4 * STORMCK_INSERT_MAX_PER_LEAF;
static_assert(16 * stormck::kBlobMaxObjects + kInsertOrderBytes <= 160 * 1024,
              "the slots' image of the largest blob leaf and the ordering buffer fit the 160 KiB of LDS of a gfx950 CU");

struct InsertParams {
    UpdateGeometry G;
    uint32_t C, N, S;
    uint32_t leaf_len, blob_len;
    uint64_t in_stride;
    uint64_t first_id;
};

__host__ __device__ inline bool insert_candidate(const stormck_lookup_result& l) {
    return l.status == STORMCK_TRACE_ABSENT && l.probes != 0;
}

// The result of one key as the locate leaves it (rule A). failed: the call returns
// STORMCK_EMISMATCH and gives no reasons.
__host__ __device__ inline stormck_insert_result insert_located(const stormck_lookup_result& l, bool failed) {
    stormck_insert_result r{};
    r.key_address = l.address;
    r.key_index = l.index;
    r.object_index = STORMCK_LOOKUP_NO_SLOT;
    r.stage = 1;
    r.status = l.status;
    if (l.status == STORMCK_TRACE_FOUND) {
        r.object_id = l.object_id;
        r.reason = STORMCK_INSERT_R_EXISTS;
    } else if (l.status == STORMCK_TRACE_ABSENT && l.probes == 0) {
        r.reason = STORMCK_INSERT_R_NO_LEAF;
    }  // a candidate: the key stage gives it its action or its reason
    if (failed) r.reason = STORMCK_INSERT_R_NONE;
    return r;
}

// A key whose walk ended at the space: every key of the call.
__host__ __device__ inline stormck_insert_result insert_at_space(uint8_t status, uint8_t reason) {
    stormck_insert_result r{};
    r.key_index = r.object_index = STORMCK_LOOKUP_NO_SLOT;
    r.status = status;
    r.reason = reason;
    return r;
}

// A key's result after the key stage judged it (rule B). Until the IDs are known object_id holds
// the item's link, which is the key index of the key that was INSERTED there.
__host__ __device__ inline void insert_judged(stormck_insert_result* r, const stormck::InsertOut& o) {
    constexpr uint8_t reason_of[] = {STORMCK_INSERT_R_NONE,    STORMCK_INSERT_R_NONE,     STORMCK_INSERT_R_KEY_SPLIT,
                                     STORMCK_INSERT_R_NO_SLOT, STORMCK_INSERT_R_KEY_FULL, STORMCK_INSERT_R_MALFORMED};
    r->reason = reason_of[o.verdict];
    if (o.verdict == stormck::kInsertPlaced || o.verdict == stormck::kInsertRepeated) {
        r->action = o.verdict == stormck::kInsertPlaced ? STORMCK_INSERT_INSERTED : STORMCK_INSERT_REPEATED;
        r->object_id = o.link;
        r->key_index = o.index;
    }
}

// A placed ID's fields in its key's result (rule D).
__host__ __device__ inline void insert_placed(stormck_insert_result* r, const stormck_object_result& o,
                                              const stormck::SlotOut& s) {
    r->object_address = o.address;
    r->object_index = s.index;
    r->stage = 2;
    r->status = s.defined ? STORMCK_TRACE_FOUND : STORMCK_TRACE_ABSENT;
}

__host__ __device__ inline bool insert_free_reference(const stormck_object_result& o) {
    return o.status == STORMCK_TRACE_ABSENT && o.probes == 0;
}

uint64_t insert_engine_bytes(uint64_t n, uint32_t C) {
    return (std::max({lookup_workspace_bytes(n, C), spaces_workspace_bytes(1, stormck::kSpaceMaxSpaces),
                      objects_workspace_bytes(n)}) + 7) & ~uint64_t{7};
}

uint64_t insert_workspace_bytes(uint64_t n, uint32_t C) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return insert_engine_bytes(n, C) + (32 + 8 + 8 + 32 + 4 + 4 + 4) * m  // L, tags, ids, O, rank_of, key_of, winner
           + 8 * m + 2 * 4 * m + 3 * 8 * (m + 8) + 3 * 4 * (m + 8)        // gkey, seg x 2, leaves x 2 + new, starts x 2 + cursor
           + get_counts_bytes(n) + 12 * update_table_slots(n) + 24 * (m + kUpdateTail) + lookup_table_bytes(C) + 128 + 64 + 128;
}

void insert_report_clear(stormck_insert_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    r->space.index = STORMCK_LOOKUP_NO_SLOT;
    r->lookup.trace.first_bad = r->lookup.first_bad = n;
    r->limit = n;
}

// The argument checks both legs share, before any work: the get's, then the call's own.
int insert_params(const void* store, const stormck_scrub_layout* layout, const stormck_get_params* params, const void* keys,
                  const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride, uint32_t flags,
                  const stormck_insert_result* results, stormck_insert_report* report, InsertParams* P) {
    if (!report) return fail(STORMCK_EINVAL, "insert: null argument");
    GetParams gp;
    stormck_get_report unused_report;
    const int rc = get_params(store, layout, params, keys, lens, len, n, 0, reinterpret_cast<const stormck_get_result*>(results),
                              nullptr, 0, &unused_report, &gp);
    if (rc) return rc;
    if (flags != 0) return fail(STORMCK_EINVAL, "insert: flags must be 0 (every leaf is verified)");
    if (in_stride < gp.S) return fail(STORMCK_EINVAL, "insert: in_stride is below object_size");
    if (n && !objects) return fail(STORMCK_EINVAL, "insert: null argument");
    if (params->keys.chunks_per_block > STORMCK_INSERT_MAX_CHUNKS)
        return fail(STORMCK_EINVAL, "insert: chunks_per_block is above STORMCK_INSERT_MAX_CHUNKS (1024)");
    ScrubParams sp;
    const stormck_scrub_report unused{};
    (void)scrub_params(store, layout, &unused, -1, 0, &sp);  // checked before: get_params
    P->G.block_size = layout->block_size;
    P->G.n_blocks = layout->n_blocks;
    P->G.fanout = layout->pointer_fanout;
    for (int k = 0; k < 4; ++k) P->G.len[k] = sp.len[k];
    P->C = params->keys.chunks_per_block;
    P->N = params->objects.objects_per_block;
    P->S = gp.S;
    P->leaf_len = stormck::objlist_leaf_len(P->C);
    P->blob_len = static_cast<uint32_t>(layout->blob_len);
    P->in_stride = in_stride;
    P->first_id = 0;
    return STORMCK_OK;
}

UpdateStep insert_key_root(const stormck_space_result& s) {
    return UpdateStep{s.key_root.address, s.address, 0, s.index | stormck::kUpdateKeyOrigin, s.key_type};
}

void insert_report_plan(stormck_insert_report* r, const UpdatePlan& plan, const UpdateGeometry& G, uint64_t revision) {
    for (int k = 0; k < 4; ++k) r->n_dirty[k] = plan.n_dirty[k];
    r->bytes_copied = plan.records.size() * G.block_size;
    r->bytes_hashed = plan.bytes_hashed + kScrubSingLen;
    r->revision = revision + 1;
    r->last_allocated = plan.last_allocated;
    r->first_new = plan.first_new;
    r->heights = plan.heights;
    r->next_object_id = r->first_id + r->cut;
}

int insert_plan_fail(UpdateError e) {
    if (e == UpdateError::NoSpace)
        return fail(STORMCK_ENOSPC, "insert: the image has no room for the dirty blocks (LastAllocatedBlock + dirty blocks >= n_blocks)");
    return fail(STORMCK_EINVAL, stormck::update_error_message(e));
}

// ---- host leg ---------------------------------------------------------------------------

int insert_host(void* store_v, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
                const void* keys_v, uint64_t stride, const uint64_t* offsets, const uint32_t* lens, uint32_t len, uint64_t n,
                const void* objects_v, uint64_t in_stride, uint32_t flags, stormck_insert_result* results,
                stormck_insert_report* report, uint32_t threads) {
    InsertParams P;
    int rc = insert_params(store_v, layout, params, keys_v, lens, len, n, objects_v, in_stride, flags, results, report, &P);
    if (rc) return rc;
    insert_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    uint8_t* base = static_cast<uint8_t*>(store_v);
    const uint8_t* keys = static_cast<const uint8_t*>(keys_v);
    const uint8_t* objects = static_cast<const uint8_t*>(objects_v);
    const UpdateGeometry& G = P.G;
    const uint16_t* A = params->keys.addressing_offsets;
    auto tally = [&] {
        for (uint64_t i = 0; i < n; ++i) {
            if (results[i].action == STORMCK_INSERT_INSERTED) ++report->n_inserted;
            else if (results[i].action == STORMCK_INSERT_REPEATED) ++report->n_repeated;
            else ++report->n_none[results[i].reason];
        }
    };
    // A. locate
    stormck_pointer sroot;
    uint8_t stype = 0, status0 = STORMCK_TRACE_MISMATCH;
    std::string text0;
    if (get_singularity(layout, store_v, base, &sroot, &stype, &text0)) {
        stormck_spaces_report srep;
        rc = spaces_host(store_v, layout, &sroot, stype, params->space_offsets, &space_id, 1, 0, &report->space, &srep, threads);
        if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
        text0 = rc ? g_last_error : std::string();
        status0 = report->space.status;
    }
    if (status0 != STORMCK_TRACE_FOUND) {  // the walk of every key ends at the space
        const bool bad = trace_bad(status0);
        for (uint64_t i = 0; i < n; ++i)
            results[i] = insert_at_space(status0, bad ? STORMCK_INSERT_R_NONE : STORMCK_INSERT_R_SPACE);
        tally();
        return bad ? fail(STORMCK_EMISMATCH, text0) : STORMCK_OK;
    }
    std::vector<stormck_lookup_result> L(n);
    std::vector<uint64_t> tags(n);
    rc = lookup_host(store_v, layout, &report->space.key_root, report->space.key_type, &params->keys, keys_v, stride, offsets,
                     lens, len, n, 0, L.data(), nullptr, tags.data(), &report->lookup, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    for (uint64_t i = 0; i < n; ++i) results[i] = insert_located(L[i], rc != STORMCK_OK);
    if (rc) {
        tally();
        return rc;  // with the lookup's text
    }
    uint8_t sing[kScrubSingLen];
    std::memcpy(sing, base, kScrubSingLen);
    const uint64_t revision = scrub_le64(sing + 16), last = scrub_le64(sing + 64);
    report->revision = revision;
    report->last_allocated = last;
    const uint64_t first_id = report->first_id = report->next_object_id = report->space.next_object_id;
    LookupParams lp{P.C, len, stride, G.block_size};
    auto key_of_index = [&](uint64_t i, uint32_t* key_len) { return lookup_key(keys, lp, offsets, lens, i, key_len); };
    // B. the key stage: every leaf's candidates in ascending key index
    std::vector<uint64_t> key_leaves;
    std::unordered_map<uint64_t, std::vector<uint32_t>> key_groups;
    for (uint64_t i = 0; i < n; ++i)
        if (insert_candidate(L[i])) {
            std::vector<uint32_t>& g = key_groups[L[i].address];
            if (g.empty()) key_leaves.push_back(L[i].address);
            g.push_back(static_cast<uint32_t>(i));
        }
    std::vector<uint8_t> image(P.leaf_len);
    for (uint64_t leaf : key_leaves) {
        const std::vector<uint32_t>& g = key_groups[leaf];
        if (g.size() > STORMCK_INSERT_MAX_PER_LEAF) {
            for (uint32_t i : g) results[i].reason = STORMCK_INSERT_R_CROWDED;
            continue;
        }
        std::memcpy(image.data(), base + leaf * G.block_size, P.leaf_len);
        for (uint32_t i : g) {
            uint32_t key_len;
            const uint8_t* key = key_of_index(i, &key_len);
            insert_judged(&results[i], stormck::objlist_insert(image.data(), P.C, A, key, key_len, L[i].reminder, i));
        }
    }
    // C. the IDs
    std::vector<uint64_t> ids;
    std::vector<uint32_t> rank_of(n, kGetNone), key_of;
    for (uint64_t i = 0; i < n; ++i)
        if (results[i].action == STORMCK_INSERT_INSERTED) {
            rank_of[i] = static_cast<uint32_t>(ids.size());
            ids.push_back(first_id + ids.size());
            key_of.push_back(static_cast<uint32_t>(i));
        }
    for (uint64_t i = 0; i < n; ++i)
        if (results[i].action != STORMCK_INSERT_NONE) results[i].object_id = first_id + rank_of[results[i].object_id];
    const uint64_t n_ins = ids.size();
    // D. the object stage
    std::vector<stormck_object_result> O(n_ins);
    stormck_objects_report orep;
    rc = objects_host(store_v, layout, &report->space.object_root, report->space.object_type, &params->objects, ids.data(), 8,
                      n_ins, 0, O.data(), nullptr, 0, &orep, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    if (rc) {
        for (uint64_t i = 0; i < n; ++i) results[i] = insert_located(L[i], true);
        tally();
        return rc;  // with the object trace's text
    }
    uint64_t cut = n_ins;
    std::vector<uint64_t> blob_leaves;
    std::unordered_map<uint64_t, std::vector<uint32_t>> blob_groups;
    for (uint64_t r = 0; r < n_ins; ++r) {
        if (insert_free_reference(O[r])) {
            cut = std::min(cut, r);
            continue;
        }
        std::vector<uint32_t>& g = blob_groups[O[r].address];
        if (g.empty()) blob_leaves.push_back(O[r].address);
        g.push_back(static_cast<uint32_t>(r));
    }
    std::vector<uint8_t> slots(static_cast<size_t>(P.N) * 16);
    auto load_slots = [&](const uint8_t* leaf) {  // the compact image blob_insert.h works on
        std::memset(slots.data(), 0, slots.size());
        for (uint32_t k = 0; k < P.N; ++k) {
            std::memcpy(slots.data() + 16 * k, leaf + k * stormck::blob_stride(P.S), 8);
            slots[16 * k + 8] = leaf[k * stormck::blob_stride(P.S) + 8 + P.S];
        }
    };
    for (uint64_t leaf_address : blob_leaves) {
        const std::vector<uint32_t>& g = blob_groups[leaf_address];
        if (g.size() > STORMCK_INSERT_MAX_PER_LEAF) {
            cut = std::min<uint64_t>(cut, g[0]);
            continue;
        }
        const uint8_t* leaf = base + leaf_address * G.block_size;
        load_slots(leaf);
        uint64_t n_used = scrub_le64(leaf + P.blob_len - 8);
        for (uint32_t r : g) {
            const stormck::SlotOut s = stormck::blob_insert(slots.data(), P.N, 0, O[r].reminder, &n_used);
            if (s.verdict != stormck::kSlotPlaced) {
                cut = std::min<uint64_t>(cut, r);
                break;
            }
            insert_placed(&results[key_of[r]], O[r], s);
        }
    }
    // E. the cut
    const uint64_t limit = cut < n_ins ? key_of[cut] : n;
    for (uint64_t i = limit; i < n; ++i) {
        results[i] = insert_located(L[i], false);
        results[i].reason = STORMCK_INSERT_R_CUT;
    }
    report->cut = cut;
    report->limit = limit;
    tally();
    if (cut == 0) return STORMCK_OK;
    // G. the dirty forest
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
    bool on_path = walk(update_space_root(sing, space_id), STORMCK_SCRUB_SPACELIST, report->space.address);
    for (uint64_t r = 0; r < cut && on_path; ++r) {
        UpdateStep s = insert_key_root(report->space);
        s.rem = tags[key_of[r]];
        on_path = walk(s, STORMCK_SCRUB_OBJECTLIST, L[key_of[r]].address);
        s = update_object_root(report->space);
        s.rem = ids[r];
        on_path = on_path && walk(s, STORMCK_SCRUB_BLOB, O[r].address);
    }
    if (!on_path) return fail(STORMCK_EINVAL, "insert: a walk left the path the locate verified");
    UpdatePlan plan;
    const UpdateError e = stormck::update_plan(dirty.data(), dirty.size(), G, revision, last, &plan);
    if (e != UpdateError::Ok) return insert_plan_fail(e);
    // H. write: the copies, the keys, the slots and rows, NextObjectID, the commit, the singularity
    const uint64_t D = plan.records.size();
    std::unordered_map<uint64_t, uint64_t> moved;  // old address -> new address
    for (uint64_t k = 0; k < D; ++k) {
        std::memcpy(base + (plan.first_new + k) * G.block_size, base + plan.old_address[k] * G.block_size, G.block_size);
        moved[plan.old_address[k]] = plan.first_new + k;
    }
    std::vector<uint32_t> winner(n, kGetNone);
    for (uint64_t leaf : key_leaves) {
        const auto at = moved.find(leaf);
        if (at == moved.end()) continue;  // no INSERTED key below the limit
        uint8_t* copy = base + at->second * G.block_size;
        for (uint32_t i : key_groups[leaf]) {
            if (i >= limit) break;
            uint32_t key_len;
            const uint8_t* key = key_of_index(i, &key_len);
            const stormck::InsertOut o = stormck::objlist_insert(copy, P.C, A, key, key_len, L[i].reminder, results[i].object_id);
            if (o.verdict == stormck::kInsertPlaced) winner[i] = i;
            else if (o.verdict == stormck::kInsertRepeated) winner[key_of[o.link - first_id]] = i;
        }
    }
    for (uint64_t r = 0; r < cut; ++r) results[winner[key_of[r]]].wrote = 1;
    for (uint64_t leaf_address : blob_leaves) {
        const auto at = moved.find(leaf_address);
        if (at == moved.end()) continue;
        uint8_t* copy = base + at->second * G.block_size;
        uint64_t n_used = scrub_le64(copy + P.blob_len - 8);
        for (uint32_t r : blob_groups[leaf_address]) {
            if (r >= cut) break;
            const stormck::SlotOut s = stormck::blob_insert(copy, P.N, P.S, O[r].reminder, &n_used);
            if (s.verdict != stormck::kSlotPlaced) return fail(STORMCK_EINVAL, "insert: the object stage is inconsistent");
            std::memcpy(const_cast<uint8_t*>(stormck::blob_object(copy, P.S, s.index)), objects + winner[key_of[r]] * in_stride, P.S);
        }
        std::memcpy(copy + P.blob_len - 8, &n_used, 8);
    }
    const uint64_t next_id = first_id + cut;
    std::memcpy(base + moved[report->space.address] * G.block_size + 72ull * report->space.index + 8, &next_id, 8);
    std::vector<uint64_t> checksums(D);
    uint64_t unused_last = last;
    rc = stormck_commit_host(base, plan.records.data(), D, revision, &unused_last, checksums.data(), threads);
    if (rc) return rc;
    stormck::update_singularity(sing, checksums[D - 1], plan, revision,
                                [](const uint8_t* p, size_t len) { return stormck::host::xxh64(p, len); });
    std::memcpy(base, sing, kScrubSingLen);
    insert_report_plan(report, plan, G, revision);
    return STORMCK_OK;
}

// ---- device engine ------------------------------------------------------------------------

struct InsertCounters {
    unsigned long long n_groups;  // k_group_ordinals: the distinct leaves
    unsigned long long cut;       // k_insert_slot_keys, k_insert_slots: the smallest failing rank
    unsigned long long error;     // a full table, a missing leaf, a second pass that judges differently: never
    unsigned long long pad;
    unsigned long long tally[2 + STORMCK_INSERT_REASONS];  // n_inserted, n_repeated, n_none[]
};
static_assert(sizeof(InsertCounters) == 128, "the insert's counters take 128 bytes of the workspace");

// One lane per key: its result as the locate leaves it, and the leaf of a candidate as its
// grouping key.
__global__ void __launch_bounds__(256) k_insert_locate(const stormck_lookup_result* __restrict__ L, uint64_t n, bool failed,
                                                       stormck_insert_result* __restrict__ results,
                                                       unsigned long long* __restrict__ gkey) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const stormck_lookup_result l = L[i];
    results[i] = insert_located(l, failed);
    gkey[i] = !failed && insert_candidate(l) ? l.address : kUpdateNoKey;
}

__global__ void __launch_bounds__(256) k_insert_fill(uint8_t status, uint8_t reason, uint64_t n,
                                                     stormck_insert_result* __restrict__ results) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) results[i] = insert_at_space(status, reason);
}

// The grouping of items by leaf. k_group_count: one lane per item enters its leaf into the table
// (keys 0xff, val 0 before) and counts it there.
__global__ void __launch_bounds__(256) k_group_count(const unsigned long long* __restrict__ gkey, uint64_t n, UpdateTable T,
                                                     InsertCounters* IC) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n || gkey[i] == kUpdateNoKey) return;
    bool owner;
    const uint64_t h = update_table_put(T, gkey[i], &owner);
    if (h == kUpdateNoKey) atomicOr(&IC->error, 1ULL);
    else atomicAdd(&T.val[h], 1u);
}

// One lane per table slot: a leaf gets a dense ordinal, which replaces its count in the table;
// the count and the address go to the ordinal's place.
__global__ void __launch_bounds__(256) k_group_ordinals(UpdateTable T, unsigned long long* __restrict__ leaves,
                                                        uint32_t* __restrict__ counts, uint64_t cap, InsertCounters* IC) {
    const uint64_t h = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool have = h <= T.mask && T.keys[h] != kUpdateNoKey;  // no early return: the wave votes below
    const unsigned long long m = __ballot(have);
    unsigned long long first = 0;
    if (m && lane == 0) first = atomicAdd(&IC->n_groups, static_cast<unsigned long long>(__popcll(m)));
    first = __shfl(first, 0);
    if (have) {
        const uint64_t ord = first + __popcll(m & ((1ULL << lane) - 1));
        if (ord < cap) {  // always: at most as many leaves as items
            leaves[ord] = T.keys[h];
            counts[ord] = T.val[h];
            T.val[h] = static_cast<uint32_t>(ord);
        } else {
            atomicOr(&IC->error, 2ULL);
        }
    }
}

// One lane per item: into its leaf's segment at the leaf's cursor. A segment is left unordered.
__global__ void __launch_bounds__(256) k_group_fill(const unsigned long long* __restrict__ gkey, uint64_t n, UpdateTable T,
                                                    const uint32_t* __restrict__ starts, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ seg, InsertCounters* IC) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n || gkey[i] == kUpdateNoKey) return;
    const uint64_t h = update_table_find(T, gkey[i]);
    if (h == kUpdateNoKey) {
        atomicOr(&IC->error, 4ULL);
        return;
    }
    const uint32_t ord = T.val[h];
    const uint32_t at = starts[ord] + atomicAdd(&cursor[ord], 1u);
    if (at < starts[ord + 1]) seg[at] = static_cast<uint32_t>(i);  // always
    else atomicOr(&IC->error, 4ULL);
}

// order[0, size) ascending, size a power of two, by the workgroup's `threads` threads (a bitonic
// network; every thread of the workgroup calls it).
__device__ inline void insert_sort(uint32_t* order, uint32_t size, uint32_t tid, uint32_t threads) {
    for (uint32_t k = 2; k <= size; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < size; t += threads) {
                const uint32_t p = t ^ j;
                if (p > t) {
                    const uint32_t a = order[t], b = order[p];
                    if ((a > b) == ((t & k) == 0)) {
                        order[t] = b;
                        order[p] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// A leaf's segment into the LDS ordering buffer: sorted there and written back (SORTED false), or
// as an earlier launch left it. count <= STORMCK_INSERT_MAX_PER_LEAF.
template <bool SORTED>
__device__ inline void insert_order(uint32_t* order, uint32_t* seg, uint32_t count, uint32_t tid, uint32_t threads) {
    uint32_t size = 1;
    while (size < count) size <<= 1;
    for (uint32_t j = tid; j < size; j += threads) order[j] = j < count ? seg[j] : UINT32_MAX;
    __syncthreads();
    if constexpr (!SORTED) {
        insert_sort(order, size, tid, threads);
        for (uint32_t j = tid; j < count; j += threads) seg[j] = order[j];
    }
}

struct InsertKeys {  // how k_insert_keys finds a key's bytes
    const uint8_t* keys;
    const uint64_t* offsets;
    const uint32_t* lens;
    LookupParams lp;
};

// One workgroup per objectlist leaf, dynamic LDS = the leaf image + the ordering buffer. The old
// leaf is loaded with 16-byte accesses when it is 16-byte aligned (leaf_len is a multiple of 8:
// the tail word goes alone), its segment's key indices are sorted ascending in LDS, and thread 0
// runs rule B over them on the image (objlist_insert.h) while the others wait.
// APPLY false: the results, with the key index of the item as its link; the store is not written.
// APPLY true, after the plan: the same walk over the keys below `limit` with the IDs as links;
// each key's last occurrence (winner, wrote); then the image goes to the leaf's new address and
// the rest of the block is copied behind it. new_leaves[ordinal] == 0: the leaf is not dirty.
template <bool APPLY>
__global__ void __launch_bounds__(256) k_insert_keys(uint8_t* __restrict__ base, InsertParams P, const uint16_t* __restrict__ A,
                                                     InsertKeys K, const stormck_lookup_result* __restrict__ L,
                                                     const unsigned long long* __restrict__ leaves,
                                                     const unsigned long long* __restrict__ new_leaves,
                                                     const uint32_t* __restrict__ starts, uint32_t* __restrict__ seg,
                                                     stormck_insert_result* __restrict__ results,
                                                     const uint32_t* __restrict__ key_of, uint64_t limit,
                                                     uint32_t* __restrict__ winner, InsertCounters* IC) {
    extern __shared__ uint64_t insert_lds[];
    uint8_t* image = reinterpret_cast<uint8_t*>(insert_lds);
    uint32_t* order = reinterpret_cast<uint32_t*>(image + ((P.leaf_len + 15u) & ~15u));
    const uint32_t tid = threadIdx.x;
    const uint32_t first = starts[blockIdx.x], count = starts[blockIdx.x + 1] - first;
    const uint64_t old = leaves[blockIdx.x], to = APPLY ? new_leaves[blockIdx.x] : 0;
    const bool crowded = count > STORMCK_INSERT_MAX_PER_LEAF;
    // every test below is the same in all threads of the workgroup
    if (old == 0 || old >= P.G.n_blocks || (APPLY && to >= P.G.n_blocks)) {
        if (tid == 0) atomicOr(&IC->error, 8ULL);
    } else if (crowded) {
        if constexpr (!APPLY)
            for (uint32_t j = tid; j < count; j += 256) results[seg[first + j]].reason = STORMCK_INSERT_R_CROWDED;
    } else if (!APPLY || to != 0) {
        const uint8_t* src = base + old * P.G.block_size;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const uint32_t quads = P.leaf_len / 16;
            for (uint32_t q = tid; q < quads; q += 256) reinterpret_cast<uint4*>(image)[q] = reinterpret_cast<const uint4*>(src)[q];
            if ((P.leaf_len & 8) && tid == 0) insert_lds[2 * quads] = *reinterpret_cast<const uint64_t*>(src + 16 * quads);
        } else {
            for (uint32_t w = tid; w < P.leaf_len / 8; w += 256) insert_lds[w] = reinterpret_cast<const uint64_t*>(src)[w];
        }
        insert_order<APPLY>(order, seg + first, count, tid, 256);
        __syncthreads();
        if (tid == 0) {
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t i = order[j];
                if (APPLY && i >= limit) break;
                uint32_t key_len;
                const uint8_t* key = lookup_key(K.keys, K.lp, K.offsets, K.lens, i, &key_len);
                const stormck_insert_result was = results[i];
                const stormck::InsertOut o =
                    stormck::objlist_insert(image, P.C, A, key, key_len, L[i].reminder, APPLY ? was.object_id : i);
                if constexpr (!APPLY) {
                    stormck_insert_result r = was;
                    insert_judged(&r, o);
                    results[i] = r;
                } else {
                    const uint8_t action = o.verdict == stormck::kInsertPlaced      ? STORMCK_INSERT_INSERTED
                                           : o.verdict == stormck::kInsertRepeated ? STORMCK_INSERT_REPEATED
                                                                                    : STORMCK_INSERT_NONE;
                    if (action != was.action || (action && o.link != was.object_id)) atomicOr(&IC->error, 16ULL);
                    else if (action == STORMCK_INSERT_INSERTED) winner[i] = i;
                    else if (action == STORMCK_INSERT_REPEATED) winner[key_of[o.link - P.first_id]] = i;
                }
            }
        }
        __syncthreads();
        if constexpr (APPLY) {
            uint8_t* dst = base + to * P.G.block_size;
            if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                const uint32_t quads = P.leaf_len / 16;
                for (uint32_t q = tid; q < quads; q += 256) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(image)[q];
                if ((P.leaf_len & 8) && tid == 0) *reinterpret_cast<uint64_t*>(dst + 16 * quads) = insert_lds[2 * quads];
            } else {
                for (uint32_t w = tid; w < P.leaf_len / 8; w += 256) reinterpret_cast<uint64_t*>(dst)[w] = insert_lds[w];
            }
            for (uint64_t w = P.leaf_len / 8 + tid; w < P.G.block_size / 8; w += 256)  // the block's bytes past the leaf
                reinterpret_cast<uint64_t*>(dst)[w] = reinterpret_cast<const uint64_t*>(src)[w];
        }
    }
}

// What the get's compaction (k_get_count, k_get_scan, k_get_select) keeps here: the INSERTED keys,
// in key order; the ID of rank r is NextObjectID + r.
struct InsertRankPick {
    const stormck_insert_result* results;
    uint64_t first_id;
    __device__ bool operator()(uint64_t i) const { return results[i].action == STORMCK_INSERT_INSERTED; }
    __device__ uint64_t id(uint64_t, uint32_t rank) const { return first_id + rank; }
};

// After the ranks: the link of an INSERTED or REPEATED key (the key index of its item) becomes
// that item's ID.
__global__ void __launch_bounds__(256) k_insert_ids(stormck_insert_result* __restrict__ results, uint64_t n,
                                                    const uint32_t* __restrict__ rank_of, uint64_t first_id,
                                                    InsertCounters* IC) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n || results[i].action == STORMCK_INSERT_NONE) return;
    const uint64_t item = results[i].object_id;
    if (item >= n || rank_of[item] == kGetNone) atomicOr(&IC->error, 32ULL);
    else results[i].object_id = first_id + rank_of[item];
}

// One lane per rank: the blob leaf of its ID as its grouping key; a trace that ended at a Free
// reference fails the rank.
__global__ void __launch_bounds__(256) k_insert_slot_keys(const stormck_object_result* __restrict__ O, uint64_t n_ins,
                                                          unsigned long long* __restrict__ gkey, InsertCounters* IC) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= n_ins) return;
    const stormck_object_result o = O[r];
    const bool free_reference = insert_free_reference(o);
    if (free_reference) atomicMin(&IC->cut, static_cast<unsigned long long>(r));
    gkey[r] = free_reference ? kUpdateNoKey : o.address;
}

struct InsertRows {  // what k_insert_slots<true> needs beyond the judging
    const uint8_t* objects;
    const uint32_t* winner;
    uint64_t n, cut, first_new, n_dirty;
    UpdateTable T;  // k_update_copy's: old blob leaf -> its place among the new copies
};

// One wave per blob leaf, dynamic LDS = a compact image of the leaf's N slots (16 bytes a slot:
// the reminder, the state byte) + the ordering buffer. The segment's ranks are sorted ascending
// in LDS and lane 0 runs rule D's slot step over them on the image (blob_insert.h).
// APPLY false: the verdicts: a placed ID's fields go to its key's result, the first failing rank
// to the cut. APPLY true, after k_update_copy: the same walk over the ranks below the cut; then
// the whole wave moves one row at a time into the leaf's new copy (object_row_store), and the
// slots' reminders and states and NUsedSlots go there from the image.
template <bool APPLY>
__global__ void __launch_bounds__(64) k_insert_slots(uint8_t* __restrict__ base, InsertParams P,
                                                     const stormck_object_result* __restrict__ O,
                                                     const unsigned long long* __restrict__ leaves,
                                                     const uint32_t* __restrict__ starts, uint32_t* __restrict__ seg,
                                                     const uint32_t* __restrict__ key_of,
                                                     stormck_insert_result* __restrict__ results, InsertRows R,
                                                     InsertCounters* IC) {
    extern __shared__ uint64_t insert_lds[];
    uint8_t* slots = reinterpret_cast<uint8_t*>(insert_lds);
    uint32_t* order = reinterpret_cast<uint32_t*>(slots + 16ull * P.N);
    __shared__ unsigned long long used_after;
    const uint32_t lane = threadIdx.x;
    const uint32_t first = starts[blockIdx.x], count = starts[blockIdx.x + 1] - first;
    const uint64_t old = leaves[blockIdx.x];
    const uint64_t stride = stormck::blob_stride(P.S);
    // every test below is the same in all lanes
    if (old == 0 || old >= P.G.n_blocks) {
        if (lane == 0) atomicOr(&IC->error, 64ULL);
    } else if (count > STORMCK_INSERT_MAX_PER_LEAF) {  // fails at its smallest rank
        if constexpr (!APPLY) {
            uint32_t least = UINT32_MAX;
            for (uint32_t j = lane; j < count; j += 64) least = min(least, seg[first + j]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) least = min(least, __shfl_xor(least, off));
            if (lane == 0) atomicMin(&IC->cut, static_cast<unsigned long long>(least));
        }
    } else {
        const uint8_t* leaf = base + old * P.G.block_size;
        for (uint32_t k = lane; k < P.N; k += 64) {  // N slots fit blob_len - 8: the objects call's own bounds
            insert_lds[2 * k] = *reinterpret_cast<const uint64_t*>(leaf + k * stride);
            insert_lds[2 * k + 1] = leaf[k * stride + 8 + P.S];
        }
        insert_order<APPLY>(order, seg + first, count, lane, 64);
        __syncthreads();
        uint32_t placed = 0;  // APPLY: the ranks of the segment below the cut
        if (lane == 0) {
            uint64_t n_used = *reinterpret_cast<const uint64_t*>(leaf + P.blob_len - 8);
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t r = order[j];
                if (APPLY && r >= R.cut) break;
                const stormck_object_result o = O[r];
                const stormck::SlotOut s = stormck::blob_insert(slots, P.N, 0, o.reminder, &n_used);
                if constexpr (!APPLY) {
                    if (s.verdict != stormck::kSlotPlaced) {
                        atomicMin(&IC->cut, static_cast<unsigned long long>(r));
                        break;
                    }
                    stormck_insert_result res = results[key_of[r]];
                    insert_placed(&res, o, s);
                    results[key_of[r]] = res;
                } else {
                    if (s.verdict != stormck::kSlotPlaced || s.index != results[key_of[r]].object_index) atomicOr(&IC->error, 128ULL);
                    ++placed;
                }
            }
            used_after = n_used;
        }
        __syncthreads();
        if constexpr (APPLY) {
            placed = __shfl(placed, 0);
            const uint64_t h = update_table_find(R.T, old);
            const uint64_t k_new = h == kUpdateNoKey ? R.n_dirty : R.T.val[h];
            if (placed == 0) {
                // nothing of this leaf is below the cut: it is not dirty
            } else if (k_new >= R.n_dirty) {  // never: the leaf of a placed ID is dirty
                if (lane == 0) atomicOr(&IC->error, 256ULL);
            } else {
                uint8_t* copy = base + (R.first_new + k_new) * P.G.block_size;
                for (uint32_t j = 0; j < placed; ++j) {
                    const uint32_t key = key_of[order[j]];
                    const uint32_t index = results[key].object_index;
                    if (index >= P.N || R.winner[key] >= R.n) {  // never
                        if (lane == 0) atomicOr(&IC->error, 512ULL);
                    } else {
                        object_row_store(const_cast<uint8_t*>(stormck::blob_object(copy, P.S, index)),
                                         R.objects + static_cast<uint64_t>(R.winner[key]) * P.in_stride, P.S, lane, 64);
                    }
                }
                for (uint32_t k = lane; k < P.N; k += 64) {
                    *reinterpret_cast<uint64_t*>(copy + k * stride) = insert_lds[2 * k];
                    copy[k * stride + 8 + P.S] = slots[16 * k + 8];
                }
                if (lane == 0) *reinterpret_cast<uint64_t*>(copy + P.blob_len - 8) = used_after;
            }
        }
    }
}

// One lane per key at or past the limit: NONE / CUT with the fields the locate left.
__global__ void __launch_bounds__(256) k_insert_cut(const stormck_lookup_result* __restrict__ L, uint64_t n, uint64_t limit,
                                                    stormck_insert_result* __restrict__ results) {
    const uint64_t i = limit + static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    stormck_insert_result r = insert_located(L[i], false);
    r.reason = STORMCK_INSERT_R_CUT;
    results[i] = r;
}

// The report's counts, per wave as k_update_actions counts.
__global__ void __launch_bounds__(256) k_insert_tally(const stormck_insert_result* __restrict__ results, uint64_t n,
                                                      InsertCounters* IC) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t which = UINT32_MAX;  // no early return: the wave votes below
    if (i < n) {
        const stormck_insert_result r = results[i];
        which = r.action == STORMCK_INSERT_INSERTED   ? 0
                : r.action == STORMCK_INSERT_REPEATED ? 1
                : r.reason < STORMCK_INSERT_REASONS   ? 2u + r.reason
                                                      : UINT32_MAX;
    }
#pragma unroll
    for (uint32_t c = 0; c < 2 + STORMCK_INSERT_REASONS; ++c) {
        const unsigned long long m = __ballot(which == c);
        if (m && lane == 0) atomicAdd(&IC->tally[c], static_cast<unsigned long long>(__popcll(m)));
    }
}

// One lane per rank below the cut: its key's winner wrote the slot.
__global__ void __launch_bounds__(256) k_insert_wrote(stormck_insert_result* __restrict__ results, uint64_t cut,
                                                      const uint32_t* __restrict__ key_of, const uint32_t* __restrict__ winner,
                                                      uint64_t n, InsertCounters* IC) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= cut) return;
    const uint32_t w = winner[key_of[r]];
    if (w >= n) atomicOr(&IC->error, 512ULL);
    else results[w].wrote = 1;
}

// The picks of the two walks (k_update_walk): the INSERTED keys with their tags; the placed ranks
// with their IDs.
struct InsertKeyPick {
    const stormck_insert_result* results;
    const uint64_t* tags;
    __device__ bool operator()(uint64_t i, uint64_t* tag) const {
        if (results[i].action != STORMCK_INSERT_INSERTED) return false;
        *tag = tags[i];
        return true;
    }
};
struct InsertIdPick {
    const uint64_t* ids;
    __device__ bool operator()(uint64_t r, uint64_t* tag) const {
        *tag = ids[r];
        return true;
    }
};

struct InsertGroups {  // one grouping's arrays in the workspace
    unsigned long long* leaves;
    uint32_t *starts, *seg;
    uint64_t n_groups = 0;
};

int insert_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
                  const void* d_keys, uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t len,
                  uint64_t n, const void* d_objects, uint64_t in_stride, uint32_t flags, stormck_insert_result* d_results,
                  void* d_workspace, uint64_t workspace_bytes, stormck_insert_report* report, void* stream) {
    InsertParams P;
    int rc = insert_params(d_store, layout, params, d_keys, d_lens, len, n, d_objects, in_stride, flags, d_results, report, &P);
    if (rc) return rc;
    const uint32_t chunks = P.C;
    if (n && (!d_workspace || workspace_bytes < insert_workspace_bytes(n, chunks)))
        return fail(STORMCK_EINVAL, "insert: workspace too small (stormck_insert_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_offsets)) & 7)
        return fail(STORMCK_EINVAL, "insert: d_store, d_results, d_offsets and d_workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_lens) & 3) return fail(STORMCK_EINVAL, "insert: d_lens must be 4-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "insert: stream is being captured (the call synchronises its stream)");
    insert_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    const UpdateGeometry& G = P.G;
    uint8_t* base = static_cast<uint8_t*>(d_store);

    // the workspace (stormck_insert_workspace_bytes, term by term)
    const uint64_t m = (n + 7) & ~uint64_t{7}, slots = update_table_slots(n);
    const uint64_t engine_bytes = insert_engine_bytes(n, chunks);
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + engine_bytes;
    auto take = [&](uint64_t bytes) {
        uint8_t* at = w;
        w += bytes;
        return at;
    };
    stormck_lookup_result* L = reinterpret_cast<stormck_lookup_result*>(take(32 * m));
    uint64_t* tags = reinterpret_cast<uint64_t*>(take(8 * m));
    uint64_t* ids = reinterpret_cast<uint64_t*>(take(8 * m));
    stormck_object_result* O = reinterpret_cast<stormck_object_result*>(take(32 * m));
    unsigned long long* gkey = reinterpret_cast<unsigned long long*>(take(8 * m));
    InsertGroups KG, BG;
    KG.leaves = reinterpret_cast<unsigned long long*>(take(8 * (m + 8)));
    BG.leaves = reinterpret_cast<unsigned long long*>(take(8 * (m + 8)));
    unsigned long long* new_leaves = reinterpret_cast<unsigned long long*>(take(8 * (m + 8)));
    uint32_t* rank_of = reinterpret_cast<uint32_t*>(take(4 * m));
    uint32_t* key_of = reinterpret_cast<uint32_t*>(take(4 * m));
    uint32_t* winner = reinterpret_cast<uint32_t*>(take(4 * m));
    KG.seg = reinterpret_cast<uint32_t*>(take(4 * m));
    BG.seg = reinterpret_cast<uint32_t*>(take(4 * m));
    KG.starts = reinterpret_cast<uint32_t*>(take(4 * (m + 8)));
    BG.starts = reinterpret_cast<uint32_t*>(take(4 * (m + 8)));
    uint32_t* cursor = reinterpret_cast<uint32_t*>(take(4 * (m + 8)));
    uint32_t* counts = reinterpret_cast<uint32_t*>(take(get_counts_bytes(n)));
    UpdateTable T{reinterpret_cast<unsigned long long*>(w), reinterpret_cast<uint32_t*>(w + 8 * slots), slots - 1};
    w += 12 * slots;
    UpdateDirty* records = reinterpret_cast<UpdateDirty*>(take(24 * (m + kUpdateTail)));
    const uint64_t record_cap = m + kUpdateTail;
    uint16_t* d_table = reinterpret_cast<uint16_t*>(take(lookup_table_bytes(chunks)));
    uint64_t* d_space_id = reinterpret_cast<uint64_t*>(w);
    stormck_space_result* d_space = reinterpret_cast<stormck_space_result*>(take(128) + 8);
    UpdateCounters* UC = reinterpret_cast<UpdateCounters*>(take(64));
    InsertCounters* IC = reinterpret_cast<InsertCounters*>(take(128));
    UpdateCounters uh;
    InsertCounters ih;
    const unsigned wgs = static_cast<unsigned>((n + 255) / 256);  // n <= 2^31
    auto grid = [](uint64_t items) { return dim3(static_cast<unsigned>((items + 255) / 256)); };
    auto read_counters = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(&ih, IC, sizeof ih, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ih.error ? fail(STORMCK_EHIP, "insert: the device's bookkeeping is inconsistent") : STORMCK_OK;
    };
    auto finish = [&](int code, const std::string& text) -> int {  // the tally, then the return
        hipLaunchKernelGGL(k_insert_tally, dim3(wgs), dim3(256), 0, st, d_results, n, IC);
        HIP_TRY(hipGetLastError());
        const int bad = read_counters();
        if (bad) return bad;
        report->n_inserted = ih.tally[0];
        report->n_repeated = ih.tally[1];
        for (int k = 0; k < STORMCK_INSERT_REASONS; ++k) report->n_none[k] = ih.tally[2 + k];
        return code ? fail(code, text) : STORMCK_OK;
    };
    std::memset(&ih, 0, sizeof ih);
    ih.cut = n;
    HIP_TRY(hipMemcpyAsync(IC, &ih, sizeof ih, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(UC, 0, sizeof *UC, st));
    HIP_TRY(hipMemcpyAsync(d_table, params->keys.addressing_offsets, 2ull * chunks, hipMemcpyHostToDevice, st));

    // A. locate
    uint8_t sing[kScrubSingLen];
    HIP_TRY(hipMemcpyAsync(sing, d_store, kScrubSingLen, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    stormck_pointer sroot;
    uint8_t stype = 0, status0 = STORMCK_TRACE_MISMATCH;
    std::string text0;
    if (get_singularity(layout, d_store, sing, &sroot, &stype, &text0)) {
        HIP_TRY(hipMemcpyAsync(d_space_id, &space_id, 8, hipMemcpyHostToDevice, st));
        stormck_spaces_report srep;
        rc = spaces_device(d_store, layout, &sroot, stype, params->space_offsets, d_space_id, 1, 0, d_space, d_workspace,
                           engine_bytes, &srep, stream);
        if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
        text0 = rc ? g_last_error : std::string();
        HIP_TRY(hipMemcpyAsync(&report->space, d_space, sizeof report->space, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        status0 = report->space.status;
    }
    if (status0 != STORMCK_TRACE_FOUND) {  // the walk of every key ends at the space
        const bool bad = trace_bad(status0);
        hipLaunchKernelGGL(k_insert_fill, dim3(wgs), dim3(256), 0, st, status0,
                           static_cast<uint8_t>(bad ? STORMCK_INSERT_R_NONE : STORMCK_INSERT_R_SPACE), n, d_results);
        HIP_TRY(hipGetLastError());
        return finish(bad ? STORMCK_EMISMATCH : STORMCK_OK, text0);
    }
    rc = lookup_device(d_store, layout, &report->space.key_root, report->space.key_type, &params->keys, d_keys, stride,
                       d_offsets, d_lens, len, n, 0, L, nullptr, tags, d_workspace, engine_bytes, &report->lookup, stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string lookup_text = rc ? g_last_error : std::string();
    hipLaunchKernelGGL(k_insert_locate, dim3(wgs), dim3(256), 0, st, L, n, rc != STORMCK_OK, d_results, gkey);
    HIP_TRY(hipGetLastError());
    if (rc) return finish(rc, lookup_text);
    const uint64_t revision = scrub_le64(sing + 16), last = scrub_le64(sing + 64);
    report->revision = revision;
    report->last_allocated = last;
    const uint64_t first_id = report->first_id = report->next_object_id = report->space.next_object_id;
    P.first_id = first_id;

    // the grouping of the items whose gkey names a leaf: the table, the ordinals, the scan, the fill
    auto group = [&](uint64_t items, InsertGroups* g) -> int {
        HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
        HIP_TRY(hipMemsetAsync(T.val, 0, 4 * slots, st));
        HIP_TRY(hipMemsetAsync(&IC->n_groups, 0, 8, st));
        hipLaunchKernelGGL(k_group_count, grid(items), dim3(256), 0, st, gkey, items, T, IC);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(g->starts, 0, 4 * (m + 8), st));
        hipLaunchKernelGGL(k_group_ordinals, grid(slots), dim3(256), 0, st, T, g->leaves, g->starts, m, IC);
        HIP_TRY(hipGetLastError());
        const int bad = read_counters();
        if (bad) return bad;
        g->n_groups = ih.n_groups;
        if (g->n_groups > m) return fail(STORMCK_EHIP, "insert: the device's bookkeeping is inconsistent");
        if (g->n_groups == 0) return STORMCK_OK;
        hipLaunchKernelGGL(k_get_scan, dim3(1), dim3(256), 0, st, g->starts, g->n_groups + 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(cursor, 0, 4 * (m + 8), st));
        hipLaunchKernelGGL(k_group_fill, grid(items), dim3(256), 0, st, gkey, items, T, g->starts, cursor, g->seg, IC);
        HIP_TRY(hipGetLastError());
        return STORMCK_OK;
    };

    // B. the key stage
    rc = group(n, &KG);
    if (rc) return rc;
    const InsertKeys K{static_cast<const uint8_t*>(d_keys), d_offsets, d_lens, LookupParams{chunks, len, stride, G.block_size}};
    const uint32_t keys_lds = ((P.leaf_len + 15u) & ~15u) + kInsertOrderBytes;
    if (KG.n_groups) {
        hipLaunchKernelGGL(k_insert_keys<false>, dim3(static_cast<unsigned>(KG.n_groups)), dim3(256), keys_lds, st, base, P,
                           d_table, K, L, KG.leaves, nullptr, KG.starts, KG.seg, d_results, nullptr, n, nullptr, IC);
        HIP_TRY(hipGetLastError());
    }
    // C. the IDs
    HIP_TRY(hipMemsetAsync(counts + wgs, 0, 4, st));
    const InsertRankPick ranks{d_results, first_id};
    hipLaunchKernelGGL(k_get_count<InsertRankPick>, dim3(wgs), dim3(256), 0, st, ranks, n, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_get_scan, dim3(1), dim3(256), 0, st, counts, static_cast<uint64_t>(wgs) + 1);  // counts[wgs]: the total
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_get_select<InsertRankPick>, dim3(wgs), dim3(256), 0, st, ranks, n, counts, ids, rank_of, key_of);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_insert_ids, dim3(wgs), dim3(256), 0, st, d_results, n, rank_of, first_id, IC);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + wgs, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t n_ins = total;
    if (n_ins > n) return fail(STORMCK_EHIP, "insert: the device's bookkeeping is inconsistent");

    // D. the object stage
    uint64_t cut = 0;
    if (n_ins) {
        stormck_objects_report orep;
        rc = objects_device(d_store, layout, &report->space.object_root, report->space.object_type, &params->objects, ids, 8,
                            n_ins, 0, O, nullptr, 0, d_workspace, engine_bytes, &orep, stream);
        if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
        if (rc) {
            const std::string object_text = g_last_error;
            hipLaunchKernelGGL(k_insert_locate, dim3(wgs), dim3(256), 0, st, L, n, true, d_results, gkey);
            HIP_TRY(hipGetLastError());
            return finish(rc, object_text);
        }
        HIP_TRY(hipMemcpyAsync(&IC->cut, &n_ins, 8, hipMemcpyHostToDevice, st));  // no rank has failed yet
        hipLaunchKernelGGL(k_insert_slot_keys, grid(n_ins), dim3(256), 0, st, O, n_ins, gkey, IC);
        HIP_TRY(hipGetLastError());
        rc = group(n_ins, &BG);
        if (rc) return rc;
    }
    const uint32_t slots_lds = 16 * P.N + kInsertOrderBytes;
    if (slots_lds > 65536) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_insert_slots<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(slots_lds)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_insert_slots<true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(slots_lds)));
    }
    InsertRows R{static_cast<const uint8_t*>(d_objects), winner, n, 0, 0, 0, T};
    if (BG.n_groups) {
        hipLaunchKernelGGL(k_insert_slots<false>, dim3(static_cast<unsigned>(BG.n_groups)), dim3(64), slots_lds, st, base, P, O,
                           BG.leaves, BG.starts, BG.seg, key_of, d_results, R, IC);
        HIP_TRY(hipGetLastError());
    }
    // E. the cut
    rc = read_counters();
    if (rc) return rc;
    cut = n_ins ? std::min<uint64_t>(ih.cut, n_ins) : 0;
    uint64_t limit = n;
    if (cut < n_ins) {
        uint32_t at = 0;
        HIP_TRY(hipMemcpyAsync(&at, key_of + cut, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        limit = at;
        hipLaunchKernelGGL(k_insert_cut, grid(n - limit), dim3(256), 0, st, L, n, limit, d_results);
        HIP_TRY(hipGetLastError());
    }
    report->cut = cut;
    report->limit = limit;
    rc = finish(STORMCK_OK, "");
    if (rc || cut == 0) return rc;

    // G. the dirty forest: the space's path, then the two trees one level per launch
    std::vector<UpdateDirty> dirty;
    auto read_records = [&](const UpdateDirty* from, uint64_t count) -> int {
        const size_t at = dirty.size();
        dirty.resize(at + count);
        HIP_TRY(hipMemcpyAsync(dirty.data() + at, from, count * sizeof(UpdateDirty), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return STORMCK_OK;
    };
    hipLaunchKernelGGL(k_update_space_walk, dim3(1), dim3(64), 0, st, base, G, update_space_root(sing, space_id), records + m,
                       UC);
    HIP_TRY(hipGetLastError());
    auto walks = [&](auto pick, uint64_t items, const UpdateStep& root, uint32_t leaf_kind, bool first_tree) -> int {
        for (uint32_t depth = 0;; ++depth) {
            if (depth > kUpdateMaxDepth) return fail(STORMCK_EHIP, "insert: a walk left the path the locate verified");
            HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
            HIP_TRY(hipMemsetAsync(&UC->count, 0, 16, st));  // count and alive
            hipLaunchKernelGGL(k_update_walk<decltype(pick)>, grid(items), dim3(256), 0, st, base, G, pick, items, root, depth,
                               leaf_kind, T, records, m, UC);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&uh, UC, sizeof uh, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (uh.error || uh.count > m || uh.space_count > kUpdateTail)
                return fail(STORMCK_EHIP, "insert: a walk left the path the locate verified");
            if (first_tree && depth == 0) {
                const int bad = read_records(records + m, uh.space_count);
                if (bad) return bad;
            }
            const int bad = read_records(records, uh.count);
            if (bad) return bad;
            if (!uh.alive) return STORMCK_OK;
        }
    };
    rc = walks(InsertKeyPick{d_results, tags}, n, insert_key_root(report->space), uint32_t{STORMCK_SCRUB_OBJECTLIST}, true);
    if (rc) return rc;
    rc = walks(InsertIdPick{ids}, cut, update_object_root(report->space), uint32_t{STORMCK_SCRUB_BLOB}, false);
    if (rc) return rc;
    UpdatePlan plan;
    const UpdateError e = stormck::update_plan(dirty.data(), dirty.size(), G, revision, last, &plan);
    if (e != UpdateError::Ok) return insert_plan_fail(e);

    // H. write: the copies of every dirty block but the key leaves, the key leaves with their
    // inserts, the slots and rows, NextObjectID, the commit, the singularity
    const uint64_t D = plan.records.size();
    std::unordered_map<uint64_t, uint64_t> moved;  // old address -> new address
    std::vector<uint64_t> pairs;
    for (uint64_t k = 0; k < D; ++k) {
        moved[plan.old_address[k]] = plan.first_new + k;
        if (plan.kind[k] == STORMCK_SCRUB_OBJECTLIST) continue;
        pairs.push_back(plan.old_address[k] | (plan.kind[k] == STORMCK_SCRUB_BLOB ? kUpdateLeafFlag : 0));
        pairs.push_back(plan.first_new + k);
    }
    const uint64_t n_pairs = pairs.size() / 2;
    uint64_t* d_pairs = reinterpret_cast<uint64_t*>(records);
    const uint64_t piece = std::min<uint64_t>(24 * record_cap / 16, 1u << 30);
    HIP_TRY(hipMemsetAsync(T.keys, 0xff, 8 * slots, st));
    for (uint64_t k = 0; k < n_pairs; k += piece) {
        const uint64_t cnt = std::min(piece, n_pairs - k);
        HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data() + 2 * k, 16 * cnt, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_update_copy, dim3(static_cast<unsigned>(cnt)), dim3(256), 0, st, base, G.block_size, d_pairs,
                           plan.first_new, T, UC);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));  // the next piece reuses d_pairs, and `pairs` is pageable
    }
    std::vector<unsigned long long> key_leaves(KG.n_groups);
    HIP_TRY(hipMemcpyAsync(key_leaves.data(), KG.leaves, 8 * KG.n_groups, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (unsigned long long& a : key_leaves) {
        const auto at = moved.find(a);
        a = at == moved.end() ? 0 : at->second;
    }
    HIP_TRY(hipMemcpyAsync(new_leaves, key_leaves.data(), 8 * KG.n_groups, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(winner, 0xff, 4 * m, st));
    hipLaunchKernelGGL(k_insert_keys<true>, dim3(static_cast<unsigned>(KG.n_groups)), dim3(256), keys_lds, st, base, P,
                       d_table, K, L, KG.leaves, new_leaves, KG.starts, KG.seg, d_results, key_of, limit, winner, IC);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_insert_wrote, grid(cut), dim3(256), 0, st, d_results, cut, key_of, winner, n, IC);
    HIP_TRY(hipGetLastError());
    R.cut = cut;
    R.first_new = plan.first_new;
    R.n_dirty = D;
    hipLaunchKernelGGL(k_insert_slots<true>, dim3(static_cast<unsigned>(BG.n_groups)), dim3(64), slots_lds, st, base, P, O,
                       BG.leaves, BG.starts, BG.seg, key_of, d_results, R, IC);
    HIP_TRY(hipGetLastError());
    const uint64_t next_id = first_id + cut;
    HIP_TRY(hipMemcpyAsync(base + moved[report->space.address] * G.block_size + 72ull * report->space.index + 8, &next_id, 8,
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(&uh, UC, sizeof uh, hipMemcpyDeviceToHost, st));
    rc = read_counters();  // synchronises: next_id and key_leaves are the host's again
    if (rc || uh.error) return fail(STORMCK_EHIP, "insert: the write of the new copies is inconsistent");  // the old revision stays valid
    std::vector<uint64_t> checksums(D);
    uint64_t unused_last = last;
    rc = stormck_commit_device(d_store, plan.records.data(), D, revision, &unused_last, checksums.data(), stream);
    if (rc) return rc;
    stormck::update_singularity(sing, checksums[D - 1], plan, revision,
                                [](const uint8_t* p, size_t len) { return stormck::host::xxh64(p, len); });
    HIP_TRY(hipMemcpyAsync(d_store, sing, kScrubSingLen, hipMemcpyHostToDevice, st));  // the call's last store
    HIP_TRY(hipStreamSynchronize(st));
    insert_report_plan(report, plan, G, revision);
    return STORMCK_OK;
}
