// Lookup: the batched, verified form of keystore.GetObjectID (keystore/keystore.go:18-45;
// include/stormck.h "lookup"; DESIGN.md "Lookup").
//
// Included by stormck.hip inside an anonymous namespace, after trace.h and after
// stormck_key_tags_device: a lookup is the key-tag launch, the trace engine (trace_device,
// trace_host: called, not restated) and the probe of each key's leaf. The probe's rules live in
// objlist_probe.h, one function for k_lookup_probe, the host leg and the stand-alone test.
//
// What is here: the final status of a key (lookup_finish: KEY, then the trace's status, then the
// probe's outcome), the report both legs fill, k_lookup_probe, and the two legs.

static_assert(sizeof(stormck_lookup_result) == 32, "stormck_lookup_result is 32 bytes");
static_assert(STORMCK_LOOKUP_KEY == 7 && STORMCK_TRACE_DEPTH < STORMCK_LOOKUP_KEY, "KEY follows the trace's statuses");
static_assert(STORMCK_LOOKUP_NO_SLOT == stormck::kObjlistNoSlot, "the probe's no-slot value is the header's");

struct LookupParams {
    uint32_t C;           // ChunksPerBlock
    uint32_t len;         // the uniform key length when there are no lens
    uint64_t stride;
    uint64_t block_size;
};

__host__ __device__ inline bool lookup_bad(uint8_t status) { return trace_bad(status) || status == STORMCK_LOOKUP_KEY; }

// The result of one key from its length, its trace and its leaf. *probed and *malformed say
// what the report counts.
template <bool BATCHED = stormck::kObjlistBatched>
__host__ __device__ inline stormck_lookup_result lookup_finish(const uint8_t* base, const LookupParams& P,
                                                               const uint16_t* A, const uint8_t* key, uint32_t key_len,
                                                               const stormck_trace_result& t, bool* probed,
                                                               bool* malformed) {
    *probed = *malformed = false;
    if (key_len == 0 || key_len > stormck::kObjlistMaxKey)
        return stormck_lookup_result{0, 0, 0, STORMCK_LOOKUP_NO_SLOT, 0, STORMCK_LOOKUP_KEY, 0};
    if (t.status != STORMCK_TRACE_FOUND)
        return stormck_lookup_result{0, t.address, t.reminder, STORMCK_LOOKUP_NO_SLOT, 0, t.status, 0};
    // FOUND: t.address is below n_blocks (trace_rule), so the leaf lies inside the image
    const stormck::ProbeOut o = stormck::objlist_probe<BATCHED>(base + t.address * P.block_size, P.C, A, key, key_len, t.reminder);
    *probed = true;
    *malformed = o.malformed != 0;
    return stormck_lookup_result{o.object_id, t.address, t.reminder, o.index, o.probes,
                                 static_cast<uint8_t>(o.found ? STORMCK_TRACE_FOUND : STORMCK_TRACE_ABSENT), 0};
}

__host__ __device__ inline const uint8_t* lookup_key(const uint8_t* keys, const LookupParams& P, const uint64_t* offsets,
                                                     const uint32_t* lens, uint64_t i, uint32_t* key_len) {
    *key_len = lens ? lens[i] : P.len;
    return keys + (offsets ? offsets[i] : i * P.stride);
}

std::string lookup_key_text(uint32_t key_len) {  // keystore.go:23-28
    if (key_len == 0) return "key cannot be empty";
    return "maximum key component length exceeded, maximum: " + std::to_string(stormck::kObjlistMaxKey) +
           ", actual: " + std::to_string(key_len);
}

uint64_t lookup_table_bytes(uint32_t C) { return (2ull * C + 7) & ~7ull; }

uint64_t lookup_workspace_bytes(uint64_t n, uint32_t C) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return trace_workspace_bytes(n) + 40 * m + lookup_table_bytes(C) + 256;
}

// The argument checks both legs share, before any work.
int lookup_params(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                  const stormck_objectlist_params* params, const void* keys, const uint32_t* lens, uint32_t len,
                  uint64_t n, uint32_t flags, const stormck_lookup_result* results, const stormck_lookup_report* report,
                  LookupParams* P) {
    if (!params || !report || !layout) return fail(STORMCK_EINVAL, "lookup: null argument");
    const uint32_t C = params->chunks_per_block;
    if (C == 0 || C > stormck::kObjlistMaxChunks) return fail(STORMCK_EINVAL, "lookup: chunks_per_block out of range (1..4096)");
    if (!params->addressing_offsets) return fail(STORMCK_EINVAL, "lookup: addressing_offsets is null");
    if (layout->objectlist_len != stormck::objlist_leaf_len(C))
        return fail(STORMCK_EINVAL, "lookup: layout->objectlist_len is not the leaf of chunks_per_block chunks, (53 * C + 11) & ~7");
    std::vector<bool> seen(C, false);
    for (uint32_t i = 0; i < C; ++i) {
        const uint16_t a = params->addressing_offsets[i];
        if (a >= C || seen[a]) return fail(STORMCK_EINVAL, "lookup: addressing_offsets is not a permutation of 0..chunks_per_block-1");
        seen[a] = true;
    }
    if (n > kTraceMaxTags) return fail(STORMCK_EINVAL, "lookup: more than 2^31 keys in one call");
    if (n && (!keys || !results)) return fail(STORMCK_EINVAL, "lookup: null argument");
    ScrubParams sp;
    ScrubChild r;  // the trace's checks of the store, the layout, the root and the flags; its arrays come later (n = 0)
    const int rc = trace_params(store, layout, root, root_type, STORMCK_SCRUB_OBJECTLIST, 0, nullptr, 0, flags, nullptr,
                                &report->trace, &sp, &r);
    if (rc) return rc;
    if (n && !lens && (len == 0 || len > stormck::kObjlistMaxKey))
        return fail(STORMCK_EINVAL, "lookup: " + lookup_key_text(len));
    P->C = C;
    P->len = len;
    P->block_size = layout->block_size;
    return STORMCK_OK;
}

void lookup_report_clear(stormck_lookup_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    r->trace.first_bad = r->first_bad = n;
}

// The call's return code once the report is whole. trace_text: what the trace left in
// stormck_last_error(); key_len: of key first_bad.
int lookup_return(const stormck_lookup_report& r, uint64_t n, uint8_t first_status, uint32_t key_len,
                  const std::string& trace_text) {
    if (r.first_bad >= n) return STORMCK_OK;
    // a key that is not KEY and ends badly is the trace's own first_bad: no smaller tag ended badly in the trace
    return fail(STORMCK_EMISMATCH, first_status == STORMCK_LOOKUP_KEY ? lookup_key_text(key_len) : trace_text);
}

// ---- host leg ---------------------------------------------------------------------------

int lookup_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                const stormck_objectlist_params* params, const void* keys_v, uint64_t stride, const uint64_t* offsets,
                const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags, stormck_lookup_result* results,
                stormck_trace_result* trace_results, uint64_t* tags, stormck_lookup_report* report, uint32_t threads) {
    LookupParams P;
    int rc = lookup_params(store, layout, root, root_type, params, keys_v, lens, len, n, flags, results, report, &P);
    if (rc) return rc;
    P.stride = stride;
    lookup_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    const uint8_t* base = static_cast<const uint8_t*>(store);
    const uint8_t* keys = static_cast<const uint8_t*>(keys_v);
    std::vector<uint64_t> own_tags;
    std::vector<stormck_trace_result> own_trace;
    if (!tags) {
        own_tags.resize(n);
        tags = own_tags.data();
    }
    if (!trace_results) {
        own_trace.resize(n);
        trace_results = own_trace.data();
    }
    ForkJoin& pool = ForkJoin::get();
    const unsigned parts = static_cast<unsigned>(std::min<uint64_t>(pool_threads(threads), (n + 1023) / 1024));
    auto range = [&](unsigned p, uint64_t* lo, uint64_t* hi) {
        *lo = n * p / parts;
        *hi = n * (p + 1) / parts;
    };
    pool.run(parts, [&](unsigned p) {
        uint64_t lo, hi;
        range(p, &lo, &hi);
        for (uint64_t i = lo; i < hi; ++i) {
            uint32_t key_len;
            const uint8_t* key = lookup_key(keys, P, offsets, lens, i, &key_len);
            tags[i] = stormck::host::xxh64(key, key_len);
        }
    });
    rc = trace_host(store, layout, root, root_type, STORMCK_SCRUB_OBJECTLIST, 0, tags, n, flags, trace_results, nullptr,
                    &report->trace, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();
    std::vector<stormck_lookup_report> part(parts);
    pool.run(parts, [&](unsigned p) {
        uint64_t lo, hi;
        range(p, &lo, &hi);
        stormck_lookup_report& r = part[p];
        lookup_report_clear(&r, n);
        for (uint64_t i = lo; i < hi; ++i) {
            uint32_t key_len;
            const uint8_t* key = lookup_key(keys, P, offsets, lens, i, &key_len);
            bool probed, malformed;
            results[i] = lookup_finish(base, P, params->addressing_offsets, key, key_len, trace_results[i], &probed, &malformed);
            ++r.n_status[results[i].status];
            r.n_probed += probed;
            r.probes += results[i].probes;
            r.n_malformed += malformed;
            if (lookup_bad(results[i].status) && i < r.first_bad) r.first_bad = i;
        }
    });
    for (const stormck_lookup_report& r : part) {
        for (int s = 0; s < 8; ++s) report->n_status[s] += r.n_status[s];
        report->n_probed += r.n_probed;
        report->probes += r.probes;
        report->n_malformed += r.n_malformed;
        report->first_bad = std::min(report->first_bad, r.first_bad);
    }
    const uint64_t fb = report->first_bad;
    return lookup_return(*report, n, fb < n ? results[fb].status : 0, fb < n && lens ? lens[fb] : len, trace_text);
}

// ---- device engine ------------------------------------------------------------------------

struct LookupCounters {
    unsigned long long n_status[8];
    unsigned long long n_probed, probes, n_malformed, first_bad;
};
static_assert(sizeof(LookupCounters) <= 256, "the counters take the last 256 bytes of the workspace");

// One lane per key. While the lanes of a wave run in step the probe's table index is the same
// in every lane, so A[i] is one address per wave. LDS_TABLE: the workgroup copies the table
// (at most 8 KiB) into LDS first and probes from there. BATCHED: objlist_probe.h.
// The shipped pair is kLookupLdsTable, kObjlistBatched; the others are compiled into the probe
// build only, where STORMCK_LOOKUP_VARIANT = LDS_TABLE + 2 * BATCHED picks one (DESIGN_LOG.md
// section 21 has the four measured).
constexpr bool kLookupLdsTable = false;

template <bool LDS_TABLE, bool BATCHED>
__global__ void __launch_bounds__(256) k_lookup_probe(const uint8_t* __restrict__ base, LookupParams P,
                                                      const uint16_t* __restrict__ A, const uint8_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ lens, uint64_t n,
                                                      const stormck_trace_result* __restrict__ trace_results,
                                                      stormck_lookup_result* __restrict__ results, LookupCounters* C) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;  // no early return: the wave votes below
    bool probed = false, malformed = false;
    uint8_t status = 0xff;
    uint32_t probes = 0;
    const uint16_t* table = A;
    if constexpr (LDS_TABLE) {
        __shared__ uint16_t lds_table[stormck::kObjlistMaxChunks];
        for (uint32_t j = threadIdx.x; j < P.C; j += 256) lds_table[j] = A[j];
        __syncthreads();
        table = lds_table;
    }
    if (valid) {
        uint32_t key_len;
        const uint8_t* key = lookup_key(keys, P, offsets, lens, i, &key_len);
        const stormck_lookup_result r =
            lookup_finish<BATCHED>(base, P, table, key, key_len, trace_results[i], &probed, &malformed);
        results[i] = r;
        status = r.status;
        probes = r.probes;
    }
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s) {
        if (s == 4) continue;  // no such status
        const unsigned long long m = __ballot(valid && status == s);
        if (m && lane == 0) atomicAdd(&C->n_status[s], static_cast<unsigned long long>(__popcll(m)));
    }
    const unsigned long long pm = __ballot(probed);
    if (pm) {
        uint32_t sum = probes;  // at most 64 * 4096
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        const unsigned long long mm = __ballot(malformed);
        if (lane == 0) {
            atomicAdd(&C->n_probed, static_cast<unsigned long long>(__popcll(pm)));
            atomicAdd(&C->probes, static_cast<unsigned long long>(sum));
            if (mm) atomicAdd(&C->n_malformed, static_cast<unsigned long long>(__popcll(mm)));
        }
    }
    const bool bad = valid && lookup_bad(status);
    if (__ballot(bad)) {
        uint32_t v = bad ? static_cast<uint32_t>(i) : UINT32_MAX;  // n <= 2^31
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
        if (lane == 0) atomicMin(&C->first_bad, static_cast<unsigned long long>(v));
    }
}

int lookup_variant() {
    constexpr int shipped = (kLookupLdsTable ? 1 : 0) + (stormck::kObjlistBatched ? 2 : 0);
#ifdef STORMCK_PROBES
    static const int v = [] {
        const char* e = std::getenv("STORMCK_LOOKUP_VARIANT");
        return e && e[0] >= '0' && e[0] <= '3' && !e[1] ? e[0] - '0' : shipped;
    }();
    return v;
#else
    return shipped;
#endif
}

// The pinned block the lookup's counters travel through is the trace's own (one per calling
// thread): every use of it is ordered on the one stream, the trace's between the lookup's two.
static_assert(sizeof(LookupCounters) <= sizeof(TraceCounters), "the lookup's counters fit the trace's pinned block");

int lookup_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                  const stormck_objectlist_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                  const uint32_t* d_lens, uint32_t len, uint64_t n, uint32_t flags, stormck_lookup_result* d_results,
                  stormck_trace_result* d_trace_results, uint64_t* d_tags, void* d_workspace, uint64_t workspace_bytes,
                  stormck_lookup_report* report, void* stream) {
    LookupParams P;
    int rc = lookup_params(d_store, layout, root, root_type, params, d_keys, d_lens, len, n, flags, d_results, report, &P);
    if (rc) return rc;
    P.stride = stride;
    if (n && (!d_workspace || workspace_bytes < lookup_workspace_bytes(n, P.C)))
        return fail(STORMCK_EINVAL, "lookup: workspace too small (stormck_lookup_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_trace_results) |
         reinterpret_cast<uintptr_t>(d_tags) | reinterpret_cast<uintptr_t>(d_offsets)) & 7)
        return fail(STORMCK_EINVAL, "lookup: d_store, d_results, d_trace_results, d_tags, d_offsets and d_workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_lens) & 3) return fail(STORMCK_EINVAL, "lookup: d_lens must be 4-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "lookup: stream is being captured (a lookup synchronises its stream)");
    lookup_report_clear(report, n);
    if (n == 0) return STORMCK_OK;

    // the workspace: the trace's, then the tags, the trace results, the table, the counters
    const uint64_t m = (n + 7) & ~uint64_t{7};
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + trace_workspace_bytes(n);
    if (!d_tags) d_tags = reinterpret_cast<uint64_t*>(w);
    w += 8 * m;
    if (!d_trace_results) d_trace_results = reinterpret_cast<stormck_trace_result*>(w);
    w += 32 * m;
    uint16_t* d_table = reinterpret_cast<uint16_t*>(w);
    w += lookup_table_bytes(P.C);
    LookupCounters* C = reinterpret_cast<LookupCounters*>(w);

    TraceCounters* pinned = nullptr;
    rc = trace_pinned(&pinned);
    if (rc) return rc;
    LookupCounters* h = reinterpret_cast<LookupCounters*>(pinned);
    std::memset(h, 0, sizeof *h);
    h->first_bad = n;
    HIP_TRY(hipMemcpyAsync(C, h, sizeof *h, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_table, params->addressing_offsets, 2ull * P.C, hipMemcpyHostToDevice, st));
    rc = stormck_key_tags_device(d_keys, stride, d_offsets, d_lens, len, n, d_tags, stream);
    if (rc) return rc;
    rc = trace_device(d_store, layout, root, root_type, STORMCK_SCRUB_OBJECTLIST, 0, d_tags, n, flags, d_trace_results,
                      nullptr, d_workspace, workspace_bytes, &report->trace, stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();

    with_int<0, 1, 2, 3>(lookup_variant(), [&](auto V) {
        constexpr bool lds = (STORMCK_V(V) & 1) != 0, batched = (STORMCK_V(V) & 2) != 0;
        if constexpr (kProbes || (lds == kLookupLdsTable && batched == stormck::kObjlistBatched))
            hipLaunchKernelGGL((k_lookup_probe<lds, batched>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                               st, static_cast<const uint8_t*>(d_store), P, d_table, static_cast<const uint8_t*>(d_keys),
                               d_offsets, d_lens, n, d_trace_results, d_results, C);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t total = 0;
    for (int s = 0; s < 8; ++s) total += (report->n_status[s] = h->n_status[s]);
    report->n_probed = h->n_probed;
    report->probes = h->probes;
    report->n_malformed = h->n_malformed;
    report->first_bad = h->first_bad;
    if (total != n || report->first_bad > n) return fail(STORMCK_EHIP, "lookup: the counters are inconsistent");
    uint8_t first_status = 0;
    uint32_t key_len = len;
    if (report->first_bad < n) {  // the error path alone reads more: that key's status and its length
        stormck_lookup_result first;
        HIP_TRY(hipMemcpyAsync(&first, d_results + report->first_bad, sizeof first, hipMemcpyDeviceToHost, st));
        if (d_lens) HIP_TRY(hipMemcpyAsync(&key_len, d_lens + report->first_bad, sizeof key_len, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        first_status = first.status;
    }
    return lookup_return(*report, n, first_status, key_len, trace_text);
}
