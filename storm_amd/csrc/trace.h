// Trace: the batched, verified form of storm's read path, cache.TraceTagForReading
// (include/stormck.h "trace"; DESIGN.md "Trace").
//
// Included by stormck.hip inside its anonymous namespace, after scrub.h: the entry layout and
// the TYPE and RANGE rules are the scrub's (ScrubParams, scrub_ref, scrub_child) and are not
// restated here.
//
// Three parts, as in scrub.h:
//   1. the rules: trace_rule (what a reference is) and trace_descend (from a verified pointer
//      block to the tag's entry), __host__ __device__, shared by the host leg and the kernels;
//   2. the device engine: per level, launch_checksum over the level's distinct references,
//      k_trace_step with one lane per live tag, k_trace_link, one small read-back;
//   3. the host leg: the same walk, each level's distinct blocks hashed on pool threads.
//
// A level is the set of distinct references (parent, slot) at one depth that are to be hashed:
// its rows. Every live tag holds the index of its row. Only two levels of rows exist at a time
// (the window of level L is [(L & 1) * m, (L & 1) * m + count)), and a level has at most as
// many rows as live tags, so the rows take 2 * n_tags however large the image is.
//
// The next level's rows are found through an open-addressing table of scrub_key(parent, slot),
// cleared per level. k_trace_step inserts with a 64-bit atomicCAS; the lane whose CAS installed
// the key owns the new row, writes it and publishes its index beside the key. No lane reads
// that index in the same kernel: every continuing tag keeps its table position, and
// k_trace_link turns it into the row index after the kernel boundary.

constexpr uint32_t kTraceMaxDepth = 64;  // pointer blocks a walk may verify: F^64 >= 2^64 for F >= 2
constexpr uint64_t kTraceMaxTags = uint64_t{1} << 31;
constexpr uint8_t kTraceLive = 0xff;     // the reference is to be hashed and the walk goes on
constexpr uint64_t kTraceNoKey = UINT64_MAX;  // scrub_key() stays below 2^56
static_assert(STORMCK_TRACE_MISMATCH == STORMCK_SCRUB_MISMATCH && STORMCK_TRACE_RANGE == STORMCK_SCRUB_RANGE &&
                  STORMCK_TRACE_TYPE == STORMCK_SCRUB_TYPE,
              "trace_rule passes the scrub's RANGE and TYPE through");

// What reference `c` (scrub_ref's answer) is to a walk that has verified `depth` pointer
// blocks: a final status, or kTraceLive. The order is the header's.
__host__ __device__ inline uint8_t trace_rule(const ScrubChild& c, uint32_t depth, uint32_t flags) {
    if (c.status == kScrubSkip) return STORMCK_TRACE_ABSENT;
    if (c.status != STORMCK_SCRUB_OK) return c.status;  // TYPE, RANGE: the scrub's numbers
    if (c.kind == STORMCK_SCRUB_POINTER) return depth >= kTraceMaxDepth ? STORMCK_TRACE_DEPTH : kTraceLive;
    return (flags & STORMCK_TRACE_LEAVES_UNVERIFIED) ? STORMCK_TRACE_FOUND : kTraceLive;
}

// cache/trace.go:38-40 at the verified pointer block `address`: the tag's slot, its new
// reminder, and the entry there.
__host__ __device__ inline ScrubChild trace_descend(const ScrubParams& P, const uint8_t* base, uint64_t address,
                                                    uint32_t leaf, uint64_t* reminder, uint32_t* slot) {
    *slot = static_cast<uint32_t>(*reminder % P.fanout);
    *reminder /= P.fanout;
    return scrub_child(P, base + address * P.block_size, STORMCK_SCRUB_POINTER, leaf, *slot);
}

__host__ __device__ inline stormck_trace_result trace_result(uint64_t address, uint64_t reminder, uint64_t parent,
                                                             uint32_t slot, uint32_t depth, uint8_t status) {
    return stormck_trace_result{address, reminder, parent, slot, static_cast<uint16_t>(depth), status, 0};
}

__host__ __device__ inline bool trace_bad(uint8_t status) {
    return status == STORMCK_TRACE_MISMATCH || status == STORMCK_TRACE_RANGE || status == STORMCK_TRACE_TYPE ||
           status == STORMCK_TRACE_DEPTH;
}

// ---- what both legs report -----------------------------------------------------------

struct TraceFirst {  // the detail of tag first_bad's error
    uint8_t status = 0;
    uint32_t slot = 0;
    uint64_t address = 0, parent = 0, computed = 0, expected = 0;
};

std::string trace_error_text(const TraceFirst& f) {
    if (f.status == STORMCK_TRACE_DEPTH) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "more than %u pointer blocks on the way to block %llu (block %llu, slot %u)",
                      kTraceMaxDepth, static_cast<unsigned long long>(f.address),
                      static_cast<unsigned long long>(f.parent), f.slot);
        return buf;
    }
    stormck_scrub_report r;
    std::memset(&r, 0, sizeof r);
    r.first_error = f.status;  // MISMATCH, RANGE and TYPE have the scrub's numbers
    r.first_slot = f.slot;
    r.first_parent = f.parent;
    r.first_address = f.address;
    r.first_computed = f.computed;
    r.first_expected = f.expected;
    return scrub_error_text(r);
}

int trace_finish(const ScrubParams& P, uint32_t leaf_kind, uint64_t n, const TraceFirst& first,
                 stormck_trace_report* r) {
    r->bytes_hashed = r->blocks_hashed[0] * P.len[STORMCK_SCRUB_POINTER] + r->blocks_hashed[1] * P.len[leaf_kind];
    if (r->first_bad < n) return fail(STORMCK_EMISMATCH, trace_error_text(first));
    return STORMCK_OK;
}

// The argument checks both legs share; fills P and the root reference.
int trace_params(const void* store, const stormck_scrub_layout* L, const stormck_pointer* root, uint8_t root_type,
                 uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* tags, uint64_t n, uint32_t flags,
                 const stormck_trace_result* results, const stormck_trace_report* report, ScrubParams* P,
                 ScrubChild* r) {
    if (!root || !report) return fail(STORMCK_EINVAL, "trace: null argument");
    if (leaf_kind > STORMCK_SCRUB_BLOB) return fail(STORMCK_EINVAL, "trace: leaf_kind must be spacelist, objectlist or blob");
    const stormck_scrub_report unused{};
    const int rc = scrub_params(store, L, &unused, static_cast<int>(leaf_kind), leaf_len, P);
    if (rc) return rc;
    if (flags & ~STORMCK_TRACE_LEAVES_UNVERIFIED) return fail(STORMCK_EINVAL, "trace: unknown flag");
    if (n > kTraceMaxTags) return fail(STORMCK_EINVAL, "trace: more than 2^31 tags in one call");
    if (n && (!tags || !results)) return fail(STORMCK_EINVAL, "trace: null argument");
    *r = scrub_ref(*P, root->checksum, root->address, root_type, static_cast<uint8_t>(leaf_kind));
    return STORMCK_OK;
}

// The root reference (parent 0, slot 0, depth 0). Returns true when there is a root block to
// hash; otherwise *status is what every tag ends with, and the report and `first` say so.
bool trace_root(const ScrubChild& root, uint32_t flags, uint64_t n, uint8_t* status, uint64_t* address,
                stormck_trace_report* r, TraceFirst* first) {
    *status = trace_rule(root, 0, flags);
    if (*status == kTraceLive) return true;
    *address = *status == STORMCK_TRACE_ABSENT ? 0 : root.address;
    r->n_status[*status] = n;
    if (trace_bad(*status) && n) {
        r->first_bad = 0;
        first->status = *status;
        first->address = root.address;
    }
    return false;
}

// ---- host leg ---------------------------------------------------------------------------

struct TraceRow {
    uint64_t address, expected, parent, computed;
    uint32_t len, slot;
    uint8_t kind;
};

int trace_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root_ptr, uint8_t root_type,
               uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* tags, uint64_t n, uint32_t flags,
               stormck_trace_result* results, uint64_t* leaf_checksums, stormck_trace_report* report, uint32_t threads) {
    ScrubParams P;
    ScrubChild root;
    int rc = trace_params(store, layout, root_ptr, root_type, leaf_kind, leaf_len, tags, n, flags, results, report, &P,
                          &root);
    if (rc) return rc;
    std::memset(report, 0, sizeof *report);
    report->first_bad = n;
    if (n == 0) return STORMCK_OK;
    const uint8_t* base = static_cast<const uint8_t*>(store);
    TraceFirst first;
    uint8_t status;
    uint64_t address;
    if (!trace_root(root, flags, n, &status, &address, report, &first)) {
        for (uint64_t t = 0; t < n; ++t) {
            results[t] = trace_result(address, tags[t], 0, 0, 0, status);
            if (leaf_checksums) leaf_checksums[t] = status == STORMCK_TRACE_FOUND ? root.expected : 0;
        }
        return trace_finish(P, leaf_kind, n, first, report);
    }
    std::vector<uint64_t> reminder(tags, tags + n);
    std::vector<uint32_t> row(n, 0), live(n), next_live;
    for (uint64_t t = 0; t < n; ++t) live[t] = static_cast<uint32_t>(t);
    std::vector<TraceRow> level, next;
    level.push_back({root.address, root.expected, 0, 0, root.len, 0, root.kind});
    std::unordered_map<uint64_t, uint32_t> rows_by_key;
    ForkJoin& pool = ForkJoin::get();
    const unsigned want = pool_threads(threads);  // at most the pool: run() takes no more parts than it has threads
    auto end =[&](uint32_t t, const stormck_trace_result& res, uint64_t leaf_cs, uint64_t computed, uint64_t expected) {
        results[t] = res;
        if (leaf_checksums) leaf_checksums[t] = res.status == STORMCK_TRACE_FOUND ? leaf_cs : 0;
        ++report->n_status[res.status];
        if (trace_bad(res.status) && t < report->first_bad) {
            report->first_bad = t;
            first = TraceFirst{res.status, res.slot, res.address, res.parent, computed, expected};
        }
    };
    for (uint32_t depth = 0; !level.empty(); ++depth) {
        const unsigned parts = static_cast<unsigned>(std::min<uint64_t>(want, level.size()));
        pool.run(parts, [&](unsigned p) {
            for (size_t i = p; i < level.size(); i += parts)
                level[i].computed = stormck::host::xxh64(base + level[i].address * P.block_size, level[i].len);
        });
        for (const TraceRow& r : level) ++report->blocks_hashed[r.kind == STORMCK_SCRUB_POINTER ? 0 : 1];
        report->levels = depth + 1;
        next.clear();
        next_live.clear();
        rows_by_key.clear();
        for (const uint32_t t : live) {
            const TraceRow& r = level[row[t]];
            if (r.computed != r.expected) {
                end(t, trace_result(r.address, reminder[t], r.parent, r.slot, depth, STORMCK_TRACE_MISMATCH), 0, r.computed,
                    r.expected);
                continue;
            }
            if (r.kind != STORMCK_SCRUB_POINTER) {
                end(t, trace_result(r.address, reminder[t], r.parent, r.slot, depth, STORMCK_TRACE_FOUND), r.expected, 0, 0);
                continue;
            }
            uint32_t slot;
            const ScrubChild c = trace_descend(P, base, r.address, leaf_kind, &reminder[t], &slot);
            const uint8_t st = trace_rule(c, depth + 1, flags);
            if (st != kTraceLive) {
                end(t, trace_result(c.address, reminder[t], r.address, slot, depth + 1, st), c.expected, 0, 0);
                continue;
            }
            const auto ins = rows_by_key.emplace(scrub_key(r.address, slot), static_cast<uint32_t>(next.size()));
            if (ins.second) next.push_back({c.address, c.expected, r.address, 0, c.len, slot, c.kind});
            row[t] = ins.first->second;
            next_live.push_back(t);
        }
        level.swap(next);
        live.swap(next_live);
    }
    return trace_finish(P, leaf_kind, n, first, report);
}

// ---- device engine ------------------------------------------------------------------------

struct TraceCounters {
    unsigned long long row_tail, live_tail;  // rows and continuing tags so far, over all levels
    unsigned long long n_status[7];
    unsigned long long rows[2];              // rows so far: pointer blocks, leaves
    unsigned long long first_bad;
    unsigned long long error;                // the table or a window overflowed: never, by their sizes
    unsigned long long detail[6];            // of tag first_bad: status, address, computed, expected, parent, slot
};
static_assert(sizeof(TraceCounters) <= 256, "the counters take the first 256 bytes of the workspace");

struct TraceRows {  // two windows of m rows
    uint64_t *address, *expected, *parent, *offset, *computed;
    uint32_t *len, *slot;
    uint8_t* kind;
};

struct TraceState {
    uint64_t* reminder;          // per tag
    uint32_t* row;               // per tag: its row; between k_trace_step and k_trace_link its table position
    unsigned long long* keys;    // the table
    uint32_t* key_row;           // the row of the key at the same position
};

uint64_t trace_table_slots(uint64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

uint64_t trace_workspace_bytes(uint64_t n) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return 256 + 12 * trace_table_slots(n) + 118 * m;
}

__device__ inline uint64_t trace_mix(uint64_t k) {  // splitmix64's finalizer
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ULL;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebULL;
    return k ^ (k >> 31);
}

// Every tag starts at row 0, the root, with its tag as the reminder.
__global__ void __launch_bounds__(256) k_trace_seed(const uint64_t* tags, uint64_t n, TraceRows Q, TraceState S,
                                                    uint32_t* live, ScrubChild root, uint64_t block_size,
                                                    TraceCounters* C) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t < n) {
        S.reminder[t] = tags[t];
        S.row[t] = 0;
        live[t] = static_cast<uint32_t>(t);
    }
    if (t == 0) {
        Q.address[0] = root.address;
        Q.expected[0] = root.expected;
        Q.parent[0] = 0;
        Q.offset[0] = root.address * block_size;
        Q.len[0] = root.len;
        Q.slot[0] = 0;
        Q.kind[0] = root.kind;
        TraceCounters c = {};
        c.row_tail = 1;
        c.live_tail = n;
        c.rows[root.kind == STORMCK_SCRUB_POINTER ? 0 : 1] = 1;
        c.first_bad = n;
        *C = c;
    }
}

// A root that is not hashed: every tag ends at it.
__global__ void __launch_bounds__(256) k_trace_fill(const uint64_t* tags, uint64_t n, uint64_t address, uint8_t status,
                                                    uint64_t leaf_cs, stormck_trace_result* results, uint64_t* leaf_checksums) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    results[t] = trace_result(address, tags[t], 0, 0, 0, status);
    if (leaf_checksums) leaf_checksums[t] = leaf_cs;
}

struct TraceStep {
    uint64_t live, m;                      // live tags of this level; rows per window
    uint64_t next_window;                  // first row of the next level's window
    uint64_t row_tail_base, live_tail_base;  // the counters' values before this level
    uint64_t mask;                         // table slots of this level - 1
    uint32_t depth, leaf_kind, flags;
};

// One lane per live tag of level `depth`, whose rows were just hashed.
__global__ void __launch_bounds__(256) k_trace_step(const uint8_t* base, ScrubParams P, TraceRows Q, TraceState S,
                                                    TraceStep L, const uint32_t* live_in, uint32_t* live_out,
                                                    stormck_trace_result* results, uint64_t* leaf_checksums,
                                                    TraceCounters* C) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < L.live;  // no early return: the wave votes below
    uint32_t t = 0;
    uint8_t status = kTraceLive;
    bool go_on = false, owner = false;
    uint64_t reminder = 0, leaf_cs = 0, pos = 0;
    ScrubChild c{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
    uint64_t parent = 0;
    uint32_t slot = 0;
    if (valid) {
        t = live_in[i];
        const uint32_t r = S.row[t];
        reminder = S.reminder[t];
        const uint64_t address = Q.address[r], expected = Q.expected[r];
        stormck_trace_result res;
        if (Q.computed[r] != expected) {
            status = STORMCK_TRACE_MISMATCH;
            res = trace_result(address, reminder, Q.parent[r], Q.slot[r], L.depth, status);
        } else if (Q.kind[r] != STORMCK_SCRUB_POINTER) {
            status = STORMCK_TRACE_FOUND;
            leaf_cs = expected;
            res = trace_result(address, reminder, Q.parent[r], Q.slot[r], L.depth, status);
        } else {  // address < n_blocks: checked before the row was made
            c = trace_descend(P, base, address, L.leaf_kind, &reminder, &slot);
            parent = address;
            status = trace_rule(c, L.depth + 1, L.flags);
            if (status == STORMCK_TRACE_FOUND) leaf_cs = c.expected;
            res = trace_result(c.address, reminder, parent, slot, L.depth + 1, status);
        }
        go_on = status == kTraceLive;
        if (!go_on) {
            results[t] = res;
            if (leaf_checksums) leaf_checksums[t] = leaf_cs;
        }
    }
    if (go_on) {
        // insert the key; probing never waits: a slot goes from empty to one key, once
        const unsigned long long key = scrub_key(parent, slot);
        uint64_t h = trace_mix(key) & L.mask;
        bool placed = false;
        for (uint64_t probe = 0; probe <= L.mask; ++probe, h = (h + 1) & L.mask) {
            unsigned long long cur = S.keys[h];
            if (cur == kTraceNoKey) cur = atomicCAS(&S.keys[h], static_cast<unsigned long long>(kTraceNoKey), key);
            if (cur == kTraceNoKey) owner = true;
            if (cur == kTraceNoKey || cur == key) {
                placed = true;
                break;
            }
        }
        pos = h;
        if (!placed) {  // a full table: its size makes this impossible
            atomicOr(&C->error, 1ULL);
            go_on = owner = false;
        }
    }
    // the owners' rows: one atomicAdd per wave claims their range of the next window
    const unsigned long long own = __ballot(owner);
    if (own) {
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&C->row_tail, static_cast<unsigned long long>(__popcll(own)));
        first = __shfl(first, 0);
        const uint64_t idx = first - L.row_tail_base + __popcll(own & ((1ULL << lane) - 1));
        if (owner) {
            if (idx < L.m) {  // always: a level has at most as many rows as live tags
                const uint64_t q = L.next_window + idx;
                Q.address[q] = c.address;
                Q.expected[q] = c.expected;
                Q.parent[q] = parent;
                Q.offset[q] = c.address * P.block_size;  // c.address < n_blocks: trace_rule
                Q.len[q] = c.len;
                Q.slot[q] = slot;
                Q.kind[q] = c.kind;
                S.key_row[pos] = static_cast<uint32_t>(q);
            } else {
                atomicOr(&C->error, 2ULL);
            }
        }
        const unsigned long long ptr = __ballot(owner && c.kind == STORMCK_SCRUB_POINTER);
        if (lane == 0) {
            if (ptr) atomicAdd(&C->rows[0], static_cast<unsigned long long>(__popcll(ptr)));
            if (own != ptr) atomicAdd(&C->rows[1], static_cast<unsigned long long>(__popcll(own) - __popcll(ptr)));
        }
    }
    // the tags that go on, compacted
    const unsigned long long on = __ballot(go_on);
    if (on) {
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&C->live_tail, static_cast<unsigned long long>(__popcll(on)));
        first = __shfl(first, 0);
        const uint64_t idx = first - L.live_tail_base + __popcll(on & ((1ULL << lane) - 1));
        if (go_on) {
            if (idx < L.m) {
                live_out[idx] = t;
                S.row[t] = static_cast<uint32_t>(pos);
                S.reminder[t] = reminder;
            } else {
                atomicOr(&C->error, 4ULL);
            }
        }
    }
    // the tags that ended, counted per wave
    const bool ended = valid && status != kTraceLive;
    if (__ballot(ended)) {
#pragma unroll
        for (uint32_t s = 0; s < 7; ++s) {
            if (s == 4) continue;  // no such status
            const unsigned long long m = __ballot(ended && status == s);
            if (m && lane == 0) atomicAdd(&C->n_status[s], static_cast<unsigned long long>(__popcll(m)));
        }
        const bool bad = ended && trace_bad(status);
        if (__ballot(bad)) {
            uint32_t v = bad ? t : UINT32_MAX;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
            if (lane == 0) atomicMin(&C->first_bad, static_cast<unsigned long long>(v));
        }
    }
}

// After k_trace_step's kernel boundary: each continuing tag's table position becomes its row.
__global__ void __launch_bounds__(256) k_trace_link(TraceState S, const uint32_t* live_out, uint64_t live_tail_base,
                                                    uint64_t m, const TraceCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t count = C->live_tail - live_tail_base;
    if (i >= count || i >= m) return;
    const uint32_t t = live_out[i];
    S.row[t] = S.key_row[S.row[t]];
}

// The detail of tag first_bad, while the rows of the level it ended on are still there.
__global__ void k_trace_detail(const stormck_trace_result* results, TraceRows Q, TraceState S, TraceCounters* C) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const stormck_trace_result r = results[C->first_bad];
    C->detail[0] = r.status;
    C->detail[1] = r.address;
    C->detail[2] = C->detail[3] = 0;
    if (r.status == STORMCK_TRACE_MISMATCH) {
        const uint32_t row = S.row[C->first_bad];
        C->detail[2] = Q.computed[row];
        C->detail[3] = Q.expected[row];
    }
    C->detail[4] = r.parent;
    C->detail[5] = r.slot;
}

int trace_pinned(TraceCounters** out) {
    thread_local TraceCounters* h = nullptr;
    if (!h) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(TraceCounters), hipHostMallocPortable));
    *out = h;
    return STORMCK_OK;
}

int trace_walk_device(const uint8_t* base, const ScrubParams& P, const ScrubChild& root, uint32_t leaf_kind,
                      const uint64_t* d_tags, uint64_t n, uint32_t flags, stormck_trace_result* d_results,
                      uint64_t* d_leaf_checksums, void* d_workspace, stormck_trace_report* report, TraceFirst* first,
                      hipStream_t st) {
    const uint64_t m = (n + 7) & ~uint64_t{7}, cap = trace_table_slots(n);
    uint8_t* w = static_cast<uint8_t*>(d_workspace);
    TraceCounters* C = reinterpret_cast<TraceCounters*>(w);
    w += 256;
    TraceState S;
    S.keys = reinterpret_cast<unsigned long long*>(w);
    w += cap * 8;
    uint64_t* col[5];
    for (auto& c : col) {
        c = reinterpret_cast<uint64_t*>(w);
        w += 2 * m * 8;
    }
    TraceRows Q;
    Q.address = col[0], Q.expected = col[1], Q.parent = col[2], Q.offset = col[3], Q.computed = col[4];
    S.reminder = reinterpret_cast<uint64_t*>(w);
    w += m * 8;
    S.key_row = reinterpret_cast<uint32_t*>(w);
    w += cap * 4;
    Q.len = reinterpret_cast<uint32_t*>(w);
    Q.slot = Q.len + 2 * m;
    w += 2 * m * 8;
    S.row = reinterpret_cast<uint32_t*>(w);
    uint32_t* live[2] = {S.row + m, S.row + 2 * m};
    w += 3 * m * 4;
    Q.kind = w;

    TraceCounters* h = nullptr;
    int rc = trace_pinned(&h);
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const unsigned tag_wgs = static_cast<unsigned>((n + 255) / 256);  // n <= 2^31
    hipLaunchKernelGGL(k_trace_seed, dim3(tag_wgs), dim3(256), 0, st, d_tags, n, Q, S, live[0], root, P.block_size, C);
    HIP_TRY(hipGetLastError());

    const uint32_t max_len = std::max(P.len[STORMCK_SCRUB_POINTER], P.len[leaf_kind]);
    uint64_t count = 1, alive = n, row_tail = 1, live_tail = n;
    for (uint32_t depth = 0; count > 0; ++depth) {
        if (depth > kTraceMaxDepth) return fail(STORMCK_EHIP, "trace: the walk is inconsistent");
        const uint64_t window = (depth & 1) * m;
        rc = launch_checksum(base, 0, Q.len + window, max_len, Q.offset + window, count, Q.computed + window, nullptr,
                             nullptr, nullptr, st);
        if (rc) return rc;
        TraceStep L;
        L.live = alive, L.m = m;
        L.next_window = ((depth + 1) & 1) * m;
        L.row_tail_base = row_tail, L.live_tail_base = live_tail;
        L.mask = trace_table_slots(alive) - 1;
        L.depth = depth, L.leaf_kind = leaf_kind, L.flags = flags;
        HIP_TRY(hipMemsetAsync(S.keys, 0xff, (L.mask + 1) * 8, st));
        const unsigned wgs = static_cast<unsigned>((alive + 255) / 256);
        hipLaunchKernelGGL(k_trace_step, dim3(wgs), dim3(256), 0, st, base, P, Q, S, L, live[depth & 1],
                           live[(depth + 1) & 1], d_results, d_leaf_checksums, C);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_trace_link, dim3(wgs), dim3(256), 0, st, S, live[(depth + 1) & 1], live_tail, m, C);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rc = take_fault(dev, st);  // a ring kernel of the dispatch that stalled wrote no checksums
        if (rc) return rc;
        const uint64_t rows = h->row_tail - row_tail, on = h->live_tail - live_tail;
        if (h->error || rows > on || on > alive) return fail(STORMCK_EHIP, "trace: the level queue is inconsistent");
        report->levels = depth + 1;
        if (h->first_bad < report->first_bad) {  // the rows this tag ended on are still in their window
            report->first_bad = h->first_bad;
            hipLaunchKernelGGL(k_trace_detail, dim3(1), dim3(64), 0, st, d_results, Q, S, C);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            *first = TraceFirst{static_cast<uint8_t>(h->detail[0]), static_cast<uint32_t>(h->detail[5]), h->detail[1],
                                h->detail[4], h->detail[2], h->detail[3]};
        }
        row_tail = h->row_tail;
        live_tail = h->live_tail;
        count = rows;
        alive = on;
    }
    uint64_t total = 0;
    for (int s = 0; s < 7; ++s) total += (report->n_status[s] = h->n_status[s]);
    report->blocks_hashed[0] = h->rows[0];
    report->blocks_hashed[1] = h->rows[1];
    if (total != n) return fail(STORMCK_EHIP, "trace: the level queue is inconsistent");
    return STORMCK_OK;
}

int trace_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root_ptr,
                 uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* d_tags, uint64_t n,
                 uint32_t flags, stormck_trace_result* d_results, uint64_t* d_leaf_checksums, void* d_workspace,
                 uint64_t workspace_bytes, stormck_trace_report* report, void* stream) {
    ScrubParams P;
    ScrubChild root;
    int rc = trace_params(d_store, layout, root_ptr, root_type, leaf_kind, leaf_len, d_tags, n, flags, d_results, report,
                          &P, &root);
    if (rc) return rc;
    if (n && (!d_workspace || workspace_bytes < trace_workspace_bytes(n)))
        return fail(STORMCK_EINVAL, "trace: workspace too small (stormck_trace_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_tags) | reinterpret_cast<uintptr_t>(d_results) |
         reinterpret_cast<uintptr_t>(d_leaf_checksums)) & 7)
        return fail(STORMCK_EINVAL, "trace: d_store, d_tags, d_results, d_leaf_checksums and d_workspace must be 8-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "trace: stream is being captured (a trace synchronises its stream every level)");
    std::memset(report, 0, sizeof *report);
    report->first_bad = n;
    if (n == 0) return STORMCK_OK;
    TraceFirst first;
    uint8_t status;
    uint64_t address;
    if (!trace_root(root, flags, n, &status, &address, report, &first)) {
        hipLaunchKernelGGL(k_trace_fill, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, d_tags, n, address,
                           status, status == STORMCK_TRACE_FOUND ? root.expected : uint64_t{0}, d_results,
                           d_leaf_checksums);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        rc = trace_walk_device(static_cast<const uint8_t*>(d_store), P, root, leaf_kind, d_tags, n, flags, d_results,
                               d_leaf_checksums, d_workspace, report, &first, st);
        if (rc) return rc;
    }
    return trace_finish(P, leaf_kind, n, first, report);
}
