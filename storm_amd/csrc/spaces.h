// Spaces: the batched, verified form of spacestore.GetSpace (spacestore/spacestore.go:14-42;
// include/stormck.h "spaces"; DESIGN.md "Spaces").
//
// Included by stormck.hip inside an anonymous namespace, after objects.h: a call is the trace
// engine with spacelist leaves (trace_device, trace_host: called, not restated) and the probe of
// each ID's leaf, whose rules live in space_probe.h, one function for k_space_probe, the host leg
// and the stand-alone test. The report's counters are the objects call's (ObjectCounters).

static_assert(sizeof(stormck_space_result) == 88, "stormck_space_result is 88 bytes");
static_assert(STORMCK_LOOKUP_NO_SLOT == stormck::kSpaceNoSlot, "the probe's no-slot value is the header's");

struct SpaceParams {
    uint32_t S;  // SpacesPerBlock
    uint64_t block_size;
};

// The result of one space ID from its trace and its leaf.
__host__ __device__ inline stormck_space_result space_finish(const uint8_t* base, const SpaceParams& P, const uint16_t* A,
                                                             const stormck_trace_result& t, bool* probed) {
    stormck_space_result r;
    memset(&r, 0, sizeof r);
    r.address = t.address;
    r.reminder = t.reminder;
    r.index = STORMCK_LOOKUP_NO_SLOT;
    r.status = t.status;
    *probed = false;
    if (t.status != STORMCK_TRACE_FOUND) return r;
    // FOUND: t.address is below n_blocks (trace_rule), so the leaf lies inside the image
    const uint8_t* leaf = base + t.address * P.block_size;
    const stormck::SpaceProbeOut o = stormck::space_probe(leaf, P.S, A, t.reminder);
    *probed = true;
    r.index = o.index;
    r.probes = o.probes;
    r.status = o.found ? STORMCK_TRACE_FOUND : STORMCK_TRACE_ABSENT;
    if (!o.found) return r;
    const uint8_t* space = leaf + o.index * stormck::kSpaceSize;
    r.next_object_id = stormck::space_u64(space + 8);
    r.key_root = stormck_pointer{stormck::space_u64(space + 16), stormck::space_u64(space + 24), stormck::space_u64(space + 32)};
    r.object_root = stormck_pointer{stormck::space_u64(space + 40), stormck::space_u64(space + 48), stormck::space_u64(space + 56)};
    r.key_type = space[64];
    r.object_type = space[65];
    return r;
}

uint64_t spaces_table_bytes(uint32_t S) { return (2ull * S + 7) & ~7ull; }

uint64_t spaces_workspace_bytes(uint64_t n, uint32_t S) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return trace_workspace_bytes(n) + 32 * m + spaces_table_bytes(S) + 256;
}

// The argument checks both legs share, before any work.
int spaces_params(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                  const uint16_t* A, const uint64_t* ids, uint64_t n, uint32_t flags, const stormck_space_result* results,
                  const stormck_spaces_report* report, SpaceParams* P) {
    if (!report || !layout) return fail(STORMCK_EINVAL, "spaces: null argument");
    const uint32_t S = layout->spaces_per_block;
    if (S == 0 || S > stormck::kSpaceMaxSpaces) return fail(STORMCK_EINVAL, "spaces: spaces_per_block out of range (1..32768)");
    if (!A) return fail(STORMCK_EINVAL, "spaces: addressing_offsets is null");
    std::vector<bool> seen(S, false);
    for (uint32_t i = 0; i < S; ++i) {
        if (A[i] >= S || seen[A[i]]) return fail(STORMCK_EINVAL, "spaces: addressing_offsets is not a permutation of 0..spaces_per_block-1");
        seen[A[i]] = true;
    }
    if (n > kTraceMaxTags) return fail(STORMCK_EINVAL, "spaces: more than 2^31 IDs in one call");
    if (n && (!ids || !results)) return fail(STORMCK_EINVAL, "spaces: null argument");
    ScrubParams sp;
    ScrubChild r;  // the trace's checks of the store, the layout, the root and the flags; its arrays come later (n = 0)
    const int rc = trace_params(store, layout, root, root_type, STORMCK_SCRUB_SPACELIST, 0, nullptr, 0, flags, nullptr,
                                &report->trace, &sp, &r);
    if (rc) return rc;
    P->S = S;
    P->block_size = layout->block_size;
    return STORMCK_OK;
}

void spaces_report_clear(stormck_spaces_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    r->trace.first_bad = r->first_bad = n;
}

// ---- host leg ---------------------------------------------------------------------------

int spaces_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                const uint16_t* A, const uint64_t* ids, uint64_t n, uint32_t flags, stormck_space_result* results,
                stormck_spaces_report* report, uint32_t threads) {
    SpaceParams P;
    int rc = spaces_params(store, layout, root, root_type, A, ids, n, flags, results, report, &P);
    if (rc) return rc;
    spaces_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    std::vector<stormck_trace_result> trace_results(n);
    rc = trace_host(store, layout, root, root_type, STORMCK_SCRUB_SPACELIST, 0, ids, n, flags, trace_results.data(), nullptr,
                    &report->trace, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();
    const uint8_t* base = static_cast<const uint8_t*>(store);
    for (uint64_t i = 0; i < n; ++i) {  // a call has few space IDs: one thread
        bool probed;
        results[i] = space_finish(base, P, A, trace_results[i], &probed);
        ++report->n_status[results[i].status];
        report->n_probed += probed;
        report->probes += results[i].probes;
        if (trace_bad(results[i].status) && i < report->first_bad) report->first_bad = i;
    }
    if (report->first_bad >= n) return STORMCK_OK;
    return fail(STORMCK_EMISMATCH, trace_text);  // an ID that ends badly ends so in the trace
}

// ---- device engine ------------------------------------------------------------------------

// One lane per ID; the counters through object_count, as k_object_fetch counts them.
__global__ void __launch_bounds__(256) k_space_probe(const uint8_t* __restrict__ base, SpaceParams P,
                                                     const uint16_t* __restrict__ A, uint64_t n,
                                                     const stormck_trace_result* __restrict__ trace_results,
                                                     stormck_space_result* __restrict__ results, ObjectCounters* C) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;  // no early return: the wave votes in object_count
    bool probed = false;
    uint8_t status = 0xff;
    uint32_t probes = 0;
    if (valid) {
        const stormck_space_result r = space_finish(base, P, A, trace_results[i], &probed);
        results[i] = r;
        status = r.status;
        probes = r.probes;
    }
    object_count(valid, i, status, probed, probes, C);
}

int spaces_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root, uint8_t root_type,
                  const uint16_t* A, const uint64_t* d_ids, uint64_t n, uint32_t flags, stormck_space_result* d_results,
                  void* d_workspace, uint64_t workspace_bytes, stormck_spaces_report* report, void* stream) {
    SpaceParams P;
    int rc = spaces_params(d_store, layout, root, root_type, A, d_ids, n, flags, d_results, report, &P);
    if (rc) return rc;
    if (n && (!d_workspace || workspace_bytes < spaces_workspace_bytes(n, P.S)))
        return fail(STORMCK_EINVAL, "spaces: workspace too small (stormck_spaces_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_ids)) & 7)
        return fail(STORMCK_EINVAL, "spaces: d_store, d_ids, d_results and d_workspace must be 8-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "spaces: stream is being captured (the call synchronises its stream)");
    spaces_report_clear(report, n);
    if (n == 0) return STORMCK_OK;

    // the workspace: the trace's, then the trace results, the table, the counters
    const uint64_t m = (n + 7) & ~uint64_t{7};
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + trace_workspace_bytes(n);
    stormck_trace_result* d_trace_results = reinterpret_cast<stormck_trace_result*>(w);
    w += 32 * m;
    uint16_t* d_table = reinterpret_cast<uint16_t*>(w);
    w += spaces_table_bytes(P.S);
    ObjectCounters* C = reinterpret_cast<ObjectCounters*>(w);

    HIP_TRY(hipMemcpyAsync(d_table, A, 2ull * P.S, hipMemcpyHostToDevice, st));
    rc = trace_device(d_store, layout, root, root_type, STORMCK_SCRUB_SPACELIST, 0, d_ids, n, flags, d_trace_results, nullptr,
                      d_workspace, workspace_bytes, &report->trace, stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string trace_text = rc ? g_last_error : std::string();

    TraceCounters* pinned = nullptr;  // the trace has synchronised: its pinned block is free again
    rc = trace_pinned(&pinned);
    if (rc) return rc;
    ObjectCounters* h = reinterpret_cast<ObjectCounters*>(pinned);
    HIP_TRY(hipMemsetAsync(C, 0, sizeof *C, st));
    HIP_TRY(hipMemsetAsync(&C->first_bad, 0xff, sizeof C->first_bad, st));
    hipLaunchKernelGGL(k_space_probe, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st,
                       static_cast<const uint8_t*>(d_store), P, d_table, n, d_trace_results, d_results, C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, C, sizeof *h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t total = 0;
    for (int s = 0; s < 8; ++s) total += (report->n_status[s] = h->n_status[s]);
    report->n_probed = h->n_probed;
    report->probes = h->probes;
    report->first_bad = std::min<uint64_t>(h->first_bad, n);
    if (total != n || (h->first_bad >= n && h->first_bad != UINT64_MAX))
        return fail(STORMCK_EHIP, "spaces: the counters are inconsistent");
    if (report->first_bad >= n) return STORMCK_OK;
    return fail(STORMCK_EMISMATCH, trace_text);
}
