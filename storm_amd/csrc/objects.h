// Objects: the batched, verified form of objectstore.GetObject (objectstore/objectstore.go:15-38;
// include/stormck.h "objects"; DESIGN.md "Objects").
//
// Included by stormck.hip inside an anonymous namespace, after lookup.h: a call is the trace
// engine with blob leaves (trace_device, trace_host: called, not restated), the probe of each
// ID's leaf and the move of the found objects into the caller's rows. The probe's rules live in
// blob_probe.h, one function for k_object_fetch, the host leg and the stand-alone test.
//
// What is here: the final result of an ID (object_finish: the trace's status, then the probe's
// outcome), the report both legs fill, k_object_fetch with its two forms of the move, and the
// two legs.

static_assert(sizeof(stormck_object_result) == 32, "stormck_object_result is 32 bytes");
static_assert(sizeof(stormck_object_result) == sizeof(stormck_lookup_result) &&
                  offsetof(stormck_lookup_result, object_id) == 0,
              "id_stride 32 reads the object IDs of a lookup result array in place");
static_assert(STORMCK_LOOKUP_NO_SLOT == stormck::kBlobNoSlot, "the probe's no-slot value is the header's");

struct ObjectParams {
    uint32_t N, S;          // objectsPerBlock, unsafe.Sizeof(T)
    uint64_t block_size;
    uint64_t id_stride;     // in u64 words
    uint64_t out_stride;
};

// The result of one ID from its trace and its leaf. *src: where its object lies, or null when
// the ID is not FOUND; *probed says what the report counts.
__host__ __device__ inline stormck_object_result object_finish(const uint8_t* base, const ObjectParams& P, uint64_t id,
                                                               const stormck_trace_result& t, const uint8_t** src,
                                                               bool* probed) {
    *src = nullptr;
    *probed = false;
    if (t.status != STORMCK_TRACE_FOUND)
        return stormck_object_result{id, t.address, t.reminder, STORMCK_LOOKUP_NO_SLOT, 0, t.status, 0};
    // FOUND: t.address is below n_blocks (trace_rule), so the leaf lies inside the image
    const uint8_t* leaf = base + t.address * P.block_size;
    const stormck::BlobProbeOut o = stormck::blob_probe(leaf, P.N, P.S, t.reminder);
    *probed = true;
    if (o.found) *src = stormck::blob_object(leaf, P.S, o.index);
    return stormck_object_result{id, t.address, t.reminder, o.index, o.probes,
                                 static_cast<uint8_t>(o.found ? STORMCK_TRACE_FOUND : STORMCK_TRACE_ABSENT), 0};
}

uint64_t objects_workspace_bytes(uint64_t n) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return trace_workspace_bytes(n) + 32 * m + 256;
}

// The argument checks both legs share, before any work.
int objects_params(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                   const stormck_blob_params* params, const void* ids, uint64_t id_stride, uint64_t n, uint32_t flags,
                   const stormck_object_result* results, const void* objects, uint64_t out_stride,
                   const stormck_objects_report* report, ObjectParams* P) {
    if (!params || !report || !layout) return fail(STORMCK_EINVAL, "objects: null argument");
    const uint32_t N = params->objects_per_block, S = params->object_size;
    if (N == 0 || N > stormck::kBlobMaxObjects) return fail(STORMCK_EINVAL, "objects: objects_per_block out of range (1..4095)");
    if (S == 0) return fail(STORMCK_EINVAL, "objects: object_size is 0");
    if (!stormck::blob_fits(N, S, layout->blob_len))
        return fail(STORMCK_EINVAL, "objects: objects_per_block slots of (8 + object_size + 1 + 7) & ~7 bytes do not fit layout->blob_len - 8");
    if (objects && out_stride < S) return fail(STORMCK_EINVAL, "objects: out_stride is below object_size");
    if (id_stride < 8 || (id_stride & 7)) return fail(STORMCK_EINVAL, "objects: id_stride must be a multiple of 8, at least 8");
    if (n > kTraceMaxTags) return fail(STORMCK_EINVAL, "objects: more than 2^31 IDs in one call");
    if (n && (!ids || !results)) return fail(STORMCK_EINVAL, "objects: null argument");
    ScrubParams sp;
    ScrubChild r;  // the trace's checks of the store, the layout, the root and the flags; its arrays come later (n = 0)
    const int rc = trace_params(store, layout, root, root_type, STORMCK_SCRUB_BLOB, 0, nullptr, 0, flags, nullptr,
                                &report->trace, &sp, &r);
    if (rc) return rc;
    P->N = N;
    P->S = S;
    P->block_size = layout->block_size;
    P->id_stride = id_stride / 8;
    P->out_stride = out_stride;
    return STORMCK_OK;
}

void objects_report_clear(stormck_objects_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    r->trace.first_bad = r->first_bad = n;
}

// The call's return code once the report is whole. An ID that ends badly ends so in the trace,
// and the smallest such ID is the trace's own first_bad: trace_text is its message.
int objects_return(const stormck_objects_report& r, uint64_t n, const std::string& trace_text) {
    if (r.first_bad >= n) return STORMCK_OK;
    return fail(STORMCK_EMISMATCH, trace_text);
}

// ---- host leg ---------------------------------------------------------------------------

int objects_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                 const stormck_blob_params* params, const void* ids_v, uint64_t id_stride, uint64_t n, uint32_t flags,
                 stormck_object_result* results, void* objects_v, uint64_t out_stride, stormck_objects_report* report,
                 uint32_t threads) {
    ObjectParams P;
    int rc = objects_params(store, layout, root, root_type, params, ids_v, id_stride, n, flags, results, objects_v,
                            out_stride, report, &P);
    if (rc) return rc;
    objects_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    const uint8_t* base = static_cast<const uint8_t*>(store);
    const uint8_t* ids = static_cast<const uint8_t*>(ids_v);
    uint8_t* objects = static_cast<uint8_t*>(objects_v);
    std::vector<uint64_t> tags(n);  // the trace reads its tags densely
    for (uint64_t i = 0; i < n; ++i) std::memcpy(&tags[i], ids + i * id_stride, 8);
    std::vector<stormck_trace_result> trace_results(n);
    rc = trace_host(store, layout, root, root_type, STORMCK_SCRUB_BLOB, 0, tags.data(), n, flags, trace_results.data(),
                    nullptr, &report->trace, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();
    ForkJoin& pool = ForkJoin::get();
    const unsigned parts = static_cast<unsigned>(std::min<uint64_t>(pool_threads(threads), (n + 1023) / 1024));
    std::vector<stormck_objects_report> part(parts);
    pool.run(parts, [&](unsigned p) {
        stormck_objects_report& r = part[p];
        objects_report_clear(&r, n);
        for (uint64_t i = n * p / parts; i < n * (p + 1) / parts; ++i) {
            const uint8_t* src;
            bool probed;
            results[i] = object_finish(base, P, tags[i], trace_results[i], &src, &probed);
            ++r.n_status[results[i].status];
            r.n_probed += probed;
            r.probes += results[i].probes;
            if (trace_bad(results[i].status) && i < r.first_bad) r.first_bad = i;
            if (!objects) continue;
            if (src)
                std::memcpy(objects + i * out_stride, src, P.S);
            else
                std::memset(objects + i * out_stride, 0, P.S);
        }
    });
    for (const stormck_objects_report& r : part) {
        for (int s = 0; s < 8; ++s) report->n_status[s] += r.n_status[s];
        report->n_probed += r.n_probed;
        report->probes += r.probes;
        report->first_bad = std::min(report->first_bad, r.first_bad);
    }
    return objects_return(*report, n, trace_text);
}

// ---- device engine ------------------------------------------------------------------------

struct ObjectCounters {
    unsigned long long n_status[8];
    unsigned long long n_probed, probes, first_bad;
};
static_assert(sizeof(ObjectCounters) <= 256, "the counters take the last 256 bytes of the workspace");
static_assert(sizeof(ObjectCounters) <= sizeof(TraceCounters), "the counters fit the trace's pinned block");

// The IDs at their stride into a dense array, which is what the trace reads.
__global__ void __launch_bounds__(256) k_object_ids(const uint64_t* __restrict__ ids, uint64_t id_stride, uint64_t n,
                                                    uint64_t* __restrict__ dense) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) dense[i] = ids[i * id_stride];
}

// One row of S bytes from src (8-byte aligned; null: zeros) to dst (any alignment) by the
// lanes first, first + step, ...: 8-byte words and then the tail's bytes when dst is aligned,
// bytes otherwise. Lane form: first 0, step 1. Wave form: first = the lane, step 64, so that
// the lanes of one instruction touch consecutive words.
__device__ inline void object_row(uint8_t* dst, const uint8_t* src, uint32_t S, uint32_t first, uint32_t step) {
    if ((reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
        const uint32_t words = S / 8;
        uint64_t* d = reinterpret_cast<uint64_t*>(dst);
        const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
        for (uint32_t w = first; w < words; w += step) d[w] = src ? s[w] : 0;
        for (uint32_t b = 8 * words + first; b < S; b += step) dst[b] = src ? src[b] : 0;
    } else {
        for (uint32_t b = first; b < S; b += step) dst[b] = src ? src[b] : 0;
    }
}

// The form of the move that ships for objects of S bytes: the wave form from kFetchWaveMin
// bytes on, the lane form below. Measured at S = 8, 64, 256 and 1024 (DESIGN.md "Objects",
// profiles/get/forms.json): the lane form is the faster one at 8 and 64, 256 is the smallest size
// at which the wave form's median beats it by more than the repeats of either form spread.
constexpr uint32_t kFetchWaveMin = 256;

// The report's counters for one lane's ID, per wave as k_lookup_probe counts: __ballot / __popcll
// per status, one atomicAdd per wave per counter, atomicMin for first_bad. Every lane of the
// wave calls it (valid false past the end). k_object_fetch and k_space_probe share it.
__device__ inline void object_count(bool valid, uint64_t i, uint8_t status, bool probed, uint32_t probes,
                                    ObjectCounters* C) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (uint32_t s = 0; s < 7; ++s) {
        if (s == 4) continue;  // no such status
        const unsigned long long m = __ballot(valid && status == s);
        if (m && lane == 0) atomicAdd(&C->n_status[s], static_cast<unsigned long long>(__popcll(m)));
    }
    const unsigned long long pm = __ballot(probed);
    if (pm) {
        uint32_t sum = probes;  // at most 64 * 32768
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) {
            atomicAdd(&C->n_probed, static_cast<unsigned long long>(__popcll(pm)));
            atomicAdd(&C->probes, static_cast<unsigned long long>(sum));
        }
    }
    const bool bad = valid && trace_bad(status);
    if (__ballot(bad)) {
        uint32_t v = bad ? static_cast<uint32_t>(i) : UINT32_MAX;  // n <= 2^31
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
        if (lane == 0) atomicMin(&C->first_bad, static_cast<unsigned long long>(v));
    }
}

// The move of one lane's row (dst null: the lane has none; src null: zeros). Every lane of the
// wave calls it. WAVE false: each lane copies its own object, or zeros, to its row. WAVE true: the
// wave walks its rows in lane order; source and destination of a row come from its lane by a
// broadcast, and all 64 lanes move the S bytes together, or zero them. k_object_fetch and
// k_get_scatter share it.
template <bool WAVE>
__device__ inline void object_move(uint8_t* dst, const uint8_t* src, uint32_t S) {
    if constexpr (!WAVE) {
        if (dst) object_row(dst, src, S, 0, 1);
    } else {
        const uint32_t lane = threadIdx.x & 63;
        unsigned long long rows = __ballot(dst != nullptr);  // the same in every lane, and so is the loop
        while (rows) {
            const int from = __ffsll(rows) - 1;
            rows &= rows - 1;
            const uint8_t* s = reinterpret_cast<const uint8_t*>(__shfl(reinterpret_cast<unsigned long long>(src), from));
            uint8_t* d = reinterpret_cast<uint8_t*>(__shfl(reinterpret_cast<unsigned long long>(dst), from));
            object_row(d, s, S, lane, 64);
        }
    }
}

// One lane per ID: the probe, the report's counters, then the move of the objects in the form
// WAVE names.
template <bool WAVE>
__global__ void __launch_bounds__(256) k_object_fetch(const uint8_t* __restrict__ base, ObjectParams P,
                                                      const uint64_t* __restrict__ ids, uint64_t n,
                                                      const stormck_trace_result* __restrict__ trace_results,
                                                      stormck_object_result* __restrict__ results,
                                                      uint8_t* __restrict__ objects, ObjectCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;  // no early return: the wave votes below
    bool probed = false;
    uint8_t status = 0xff;
    uint32_t probes = 0;
    const uint8_t* src = nullptr;
    if (valid) {
        const stormck_object_result r = object_finish(base, P, ids[i * P.id_stride], trace_results[i], &src, &probed);
        results[i] = r;
        status = r.status;
        probes = r.probes;
    }
    object_count(valid, i, status, probed, probes, C);
    if (!objects) return;  // the same in every lane
    object_move<WAVE>(valid ? objects + i * P.out_stride : nullptr, src, P.S);
}

// Which form runs: the shipped rule, or in the probe build the one STORMCK_FETCH_COPY names
// (0: lane, 1: wave) at every size. Read at every call, so that tools/get_bench.py times both
// forms in turn in one process on one arena.
bool fetch_wave(uint32_t S) {
#ifdef STORMCK_PROBES
    const char* e = std::getenv("STORMCK_FETCH_COPY");
    if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
#endif
    return S >= kFetchWaveMin;
}

int objects_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                   const stormck_blob_params* params, const void* d_ids, uint64_t id_stride, uint64_t n, uint32_t flags,
                   stormck_object_result* d_results, void* d_objects, uint64_t out_stride, void* d_workspace,
                   uint64_t workspace_bytes, stormck_objects_report* report, void* stream) {
    ObjectParams P;
    int rc = objects_params(d_store, layout, root, root_type, params, d_ids, id_stride, n, flags, d_results, d_objects,
                            out_stride, report, &P);
    if (rc) return rc;
    if (n && (!d_workspace || workspace_bytes < objects_workspace_bytes(n)))
        return fail(STORMCK_EINVAL, "objects: workspace too small (stormck_objects_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_ids)) & 7)
        return fail(STORMCK_EINVAL, "objects: d_store, d_ids, d_results and d_workspace must be 8-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "objects: stream is being captured (the call synchronises its stream)");
    objects_report_clear(report, n);
    if (n == 0) return STORMCK_OK;

    // the workspace: the trace's, then the trace results, the counters
    const uint64_t m = (n + 7) & ~uint64_t{7};
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + trace_workspace_bytes(n);
    stormck_trace_result* d_trace_results = reinterpret_cast<stormck_trace_result*>(w);
    w += 32 * m;
    ObjectCounters* C = reinterpret_cast<ObjectCounters*>(w);

    const uint64_t* ids = static_cast<const uint64_t*>(d_ids);
    const unsigned wgs = static_cast<unsigned>((n + 255) / 256);  // n <= 2^31
    const uint64_t* d_tags = ids;
    // The trace reads its tags densely. The workspace formula is fixed (the trace's, the trace results, the
    // counters) and none of the three can hold 8 n more bytes while the trace runs: the trace owns its own
    // part, the counters are 256 bytes, and k_trace_fill (a root that ends every tag at once) reads tag t and
    // writes trace result t in one kernel, so IDs laid anywhere into the trace-results region would race with
    // it. The first 8 n bytes of d_results are free until k_object_fetch writes them, and that kernel reads
    // the IDs from d_ids again: hence the header's rule that d_results does not overlap d_ids, and that
    // d_results is unspecified after a call that fails.
    if (P.id_stride != 1) {
        uint64_t* dense = reinterpret_cast<uint64_t*>(d_results);
        hipLaunchKernelGGL(k_object_ids, dim3(wgs), dim3(256), 0, st, ids, P.id_stride, n, dense);
        HIP_TRY(hipGetLastError());
        d_tags = dense;
    }
    rc = trace_device(d_store, layout, root, root_type, STORMCK_SCRUB_BLOB, 0, d_tags, n, flags, d_trace_results,
                      nullptr, d_workspace, workspace_bytes, &report->trace, stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();

    // the trace has synchronised: its pinned block (one per calling thread) is free again
    TraceCounters* pinned = nullptr;
    rc = trace_pinned(&pinned);
    if (rc) return rc;
    ObjectCounters* h = reinterpret_cast<ObjectCounters*>(pinned);
    // no upload: the counters start at 0 and first_bad at all ones, which atomicMin lowers and the host caps at n
    HIP_TRY(hipMemsetAsync(C, 0, sizeof *C, st));
    HIP_TRY(hipMemsetAsync(&C->first_bad, 0xff, sizeof C->first_bad, st));
    with_consts([&](auto WAVE) {
        hipLaunchKernelGGL((k_object_fetch<STORMCK_V(WAVE)>), dim3(wgs), dim3(256), 0, st,
                           static_cast<const uint8_t*>(d_store), P, ids, n, d_trace_results, d_results,
                           static_cast<uint8_t*>(d_objects), C);
    }, fetch_wave(P.S));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t total = 0;
    for (int s = 0; s < 8; ++s) total += (report->n_status[s] = h->n_status[s]);
    report->n_probed = h->n_probed;
    report->probes = h->probes;
    report->first_bad = std::min<uint64_t>(h->first_bad, n);
    if (total != n || (h->first_bad >= n && h->first_bad != UINT64_MAX))
        return fail(STORMCK_EHIP, "objects: the counters are inconsistent");
    return objects_return(*report, n, trace_text);
}
