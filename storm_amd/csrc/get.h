// Get: storm.Get (storm.go:32-58) for many keys of one space (include/stormck.h "get";
// DESIGN.md "Get").
//
// Included by stormck.hip inside an anonymous namespace, after spaces.h. A call is the
// singularity's check (scrub_singularity, as the scrub makes it), then the three engines, called
// and not restated: spaces with n = 1, the lookup over the keys, the objects call over the IDs of
// the keys that were FOUND. What is here: the order-preserving compaction between the last two
// (k_get_count, k_get_scan, k_get_select), the way back to key order with the move of the objects
// (get_finish, k_get_scatter), the report, and the two legs.

static_assert(sizeof(stormck_get_result) == 32, "stormck_get_result is 32 bytes");

constexpr uint32_t kGetNone = UINT32_MAX;  // a key that is not among the object stage's IDs

struct GetParams {
    uint32_t S;           // unsafe.Sizeof(T)
    uint64_t block_size;
    uint64_t out_stride;
};

// A key whose walk ended at the space: every key of the call.
__host__ __device__ inline stormck_get_result get_at_space(uint8_t status) {
    return stormck_get_result{0, 0, 0, STORMCK_LOOKUP_NO_SLOT, 0, status, 0};
}

// The result of one key from its lookup and, when that was FOUND, the object stage's result of its
// ID. *src: where the object lies, or null.
__host__ __device__ inline stormck_get_result get_finish(const uint8_t* base, const GetParams& P,
                                                         const stormck_lookup_result& l, const stormck_object_result* o,
                                                         const uint8_t** src) {
    *src = nullptr;
    if (l.status != STORMCK_TRACE_FOUND || !o) return stormck_get_result{l.object_id, l.address, 0, l.index, 1, l.status, 0};
    if (o->status == STORMCK_TRACE_FOUND)  // index is below N and the leaf below n_blocks: the objects call's own bounds
        *src = stormck::blob_object(base + o->address * P.block_size, P.S, o->index);
    return stormck_get_result{l.object_id, l.address, o->address, o->index, 2, o->status, 0};
}

uint64_t get_counts_bytes(uint64_t n) { return 8 * (n / 256 + 2); }

uint64_t get_workspace_bytes(uint64_t n, uint32_t C) {
    const uint64_t m = (n + 7) & ~uint64_t{7};
    return std::max(lookup_workspace_bytes(n, C), spaces_workspace_bytes(1, stormck::kSpaceMaxSpaces)) + 80 * m +
           get_counts_bytes(n) + 128;
}

void get_report_clear(stormck_get_report* r, uint64_t n) {
    std::memset(r, 0, sizeof *r);
    r->space.index = STORMCK_LOOKUP_NO_SLOT;
    r->lookup.trace.first_bad = r->lookup.first_bad = r->first_bad = n;
}

// The argument checks both legs share, before any work: the call's own, then those of the three
// calls it contains (with a Free root in the place of the roots the store will give).
int get_params(const void* store, const stormck_scrub_layout* layout, const stormck_get_params* params, const void* keys,
               const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags, const stormck_get_result* results,
               const void* objects, uint64_t out_stride, stormck_get_report* report, GetParams* P) {
    if (!params || !report || !layout) return fail(STORMCK_EINVAL, "get: null argument");
    if (n && !results) return fail(STORMCK_EINVAL, "get: null argument");
    const stormck_pointer none{0, 0, 0};
    const uint64_t id = 0;
    stormck_space_result sr;
    stormck_spaces_report srep;
    SpaceParams sp;
    int rc = spaces_params(store, layout, &none, 0, params->space_offsets, &id, 1, 0, &sr, &srep, &sp);
    if (rc) return rc;
    LookupParams lp;
    rc = lookup_params(store, layout, &none, 0, &params->keys, keys, lens, len, n, flags,
                       reinterpret_cast<const stormck_lookup_result*>(results), &report->lookup, &lp);
    if (rc) return rc;
    stormck_objects_report orep;
    ObjectParams op;
    rc = objects_params(store, layout, &none, 0, &params->objects, results, 8, n, flags,
                        reinterpret_cast<const stormck_object_result*>(results), objects, out_stride, &orep, &op);
    if (rc) return rc;
    if (layout->block_size < kScrubSingLen) return fail(STORMCK_EINVAL, "get: block_size below the singularity's 72 bytes");
    P->S = params->objects.object_size;
    P->block_size = layout->block_size;
    P->out_stride = out_stride;
    return STORMCK_OK;
}

// Stage 0 from the singularity's 72 bytes: true when there is a space tree to look the space up
// in (*root, *root_type); otherwise every key ends MISMATCH and *text says why.
bool get_singularity(const stormck_scrub_layout* layout, const void* store, const uint8_t* sing, stormck_pointer* root,
                     uint8_t* root_type, std::string* text) {
    ScrubParams P;
    const stormck_scrub_report unused{};
    (void)scrub_params(store, layout, &unused, -1, 0, &P);  // checked before: get_params
    ScrubTotals T;
    ScrubChild child{0, 0, 0, 0, 0, static_cast<uint8_t>(kScrubSkip)};
    if (!scrub_singularity(P, sing, &T, &child)) {
        stormck_scrub_report r;
        (void)scrub_finish(P, T, &r);  // the scrub's words for it
        *text = g_last_error;
        return false;
    }
    *root = stormck_pointer{scrub_le64(sing + 32), scrub_le64(sing + 40), scrub_le64(sing + 48)};
    *root_type = sing[56];
    return true;
}

// The report and the return code once the three stages have run.
int get_return(stormck_get_report* r, uint64_t n, const stormck_objects_report& o, uint64_t n_selected,
               uint64_t object_first_bad_key, const std::string& lookup_text, const std::string& object_text) {
    r->n_selected = n_selected;
    for (int s = 0; s < 8; ++s) r->n_status[s] = o.n_status[s];
    r->blocks_hashed[0] = o.trace.blocks_hashed[0];
    r->blocks_hashed[1] = o.trace.blocks_hashed[1];
    r->bytes_hashed = o.trace.bytes_hashed;
    r->levels = o.trace.levels;
    r->probes = o.probes;
    r->n_found = o.n_status[STORMCK_TRACE_FOUND];
    r->first_bad = std::min(r->lookup.first_bad, object_first_bad_key);
    if (r->first_bad >= n) return STORMCK_OK;
    return fail(STORMCK_EMISMATCH, r->first_bad == r->lookup.first_bad ? lookup_text : object_text);
}

// ---- host leg ---------------------------------------------------------------------------

int get_host(const void* store, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
             const void* keys, uint64_t stride, const uint64_t* offsets, const uint32_t* lens, uint32_t len, uint64_t n,
             uint32_t flags, stormck_get_result* results, void* objects_v, uint64_t out_stride, stormck_get_report* report,
             uint32_t threads) {
    GetParams P;
    int rc = get_params(store, layout, params, keys, lens, len, n, flags, results, objects_v, out_stride, report, &P);
    if (rc) return rc;
    get_report_clear(report, n);
    if (n == 0) return STORMCK_OK;
    const uint8_t* base = static_cast<const uint8_t*>(store);
    uint8_t* objects = static_cast<uint8_t*>(objects_v);
    stormck_pointer sroot;
    uint8_t stype = 0, status0 = STORMCK_TRACE_MISMATCH;
    std::string text0;
    if (get_singularity(layout, store, base, &sroot, &stype, &text0)) {
        stormck_spaces_report srep;
        rc = spaces_host(store, layout, &sroot, stype, params->space_offsets, &space_id, 1, 0, &report->space, &srep, threads);
        if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
        text0 = rc ? g_last_error : std::string();
        status0 = report->space.status;
    }
    if (status0 != STORMCK_TRACE_FOUND) {  // the walk of every key ends at the space
        for (uint64_t i = 0; i < n; ++i) {
            results[i] = get_at_space(status0);
            if (objects) std::memset(objects + i * out_stride, 0, P.S);
        }
        if (!trace_bad(status0)) return STORMCK_OK;
        report->first_bad = 0;
        return fail(STORMCK_EMISMATCH, text0);
    }
    std::vector<stormck_lookup_result> L(n);
    rc = lookup_host(store, layout, &report->space.key_root, report->space.key_type, &params->keys, keys, stride, offsets,
                     lens, len, n, flags, L.data(), nullptr, nullptr, &report->lookup, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string lookup_text = rc ? g_last_error : std::string();
    std::vector<uint64_t> ids;
    std::vector<uint32_t> pos(n, kGetNone), key_of;
    for (uint64_t i = 0; i < n; ++i)
        if (L[i].status == STORMCK_TRACE_FOUND) {
            pos[i] = static_cast<uint32_t>(ids.size());
            ids.push_back(L[i].object_id);
            key_of.push_back(static_cast<uint32_t>(i));
        }
    const uint64_t n_sel = ids.size();
    std::vector<stormck_object_result> O(n_sel);
    stormck_objects_report orep;
    rc = objects_host(store, layout, &report->space.object_root, report->space.object_type, &params->objects, ids.data(), 8,
                      n_sel, flags, O.data(), nullptr, 0, &orep, threads);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string object_text = rc ? g_last_error : std::string();
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* src;
        results[i] = get_finish(base, P, L[i], pos[i] == kGetNone ? nullptr : &O[pos[i]], &src);
        if (!objects) continue;
        if (src)
            std::memcpy(objects + i * out_stride, src, P.S);
        else
            std::memset(objects + i * out_stride, 0, P.S);
    }
    return get_return(report, n, orep, n_sel, orep.first_bad < n_sel ? key_of[orep.first_bad] : n, lookup_text, object_text);
}

// ---- device engine ------------------------------------------------------------------------

// Which items the compaction keeps, and the ID of a kept item at its place: the get's are the keys
// whose lookup ended FOUND, with their object IDs.
struct GetPick {
    const stormck_lookup_result* L;
    __device__ bool operator()(uint64_t i) const { return L[i].status == STORMCK_TRACE_FOUND; }
    __device__ uint64_t id(uint64_t i, uint32_t) const { return L[i].object_id; }
};

// Items that `pick` keeps (the get: keys that were FOUND), per workgroup of 256 items.
template <class Pick>
__global__ void __launch_bounds__(256) k_get_count(Pick pick, uint64_t n, uint32_t* __restrict__ counts) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int c = __syncthreads_count(i < n && pick(i));
    if (threadIdx.x == 0) counts[blockIdx.x] = static_cast<uint32_t>(c);
}

// counts[0..nb) become their exclusive prefix sums, in place; one workgroup, 256 counts a round.
__global__ void __launch_bounds__(256) k_get_scan(uint32_t* counts, uint64_t nb) {
    __shared__ uint32_t lds[256];
    uint32_t carry = 0;
    for (uint64_t first = 0; first < nb; first += 256) {
        const uint64_t j = first + threadIdx.x;
        const uint32_t own = j < nb ? counts[j] : 0;
        lds[threadIdx.x] = own;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {  // inclusive sums, Hillis and Steele's
            const uint32_t add = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
            __syncthreads();
            lds[threadIdx.x] += add;
            __syncthreads();
        }
        if (j < nb) counts[j] = carry + lds[threadIdx.x] - own;
        carry += lds[255];
        __syncthreads();
    }
}

// Each kept item's place among the kept items, in item order (the get: each FOUND key's among the
// FOUND keys): its ID goes there (ids), the item remembers the place (pos, kGetNone for every other
// item) and the place the item (key_of).
template <class Pick>
__global__ void __launch_bounds__(256) k_get_select(Pick pick, uint64_t n, const uint32_t* __restrict__ counts,
                                                    uint64_t* __restrict__ ids, uint32_t* __restrict__ pos,
                                                    uint32_t* __restrict__ key_of) {
    __shared__ uint32_t waves[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool found = i < n && pick(i);
    const unsigned long long m = __ballot(found);
    if (lane == 0) waves[wave] = static_cast<uint32_t>(__popcll(m));
    __syncthreads();
    uint32_t at = counts[blockIdx.x] + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1)));
    for (uint32_t w = 0; w < wave; ++w) at += waves[w];
    if (i < n) pos[i] = found ? at : kGetNone;
    if (found) {
        ids[at] = pick.id(i, at);
        key_of[at] = static_cast<uint32_t>(i);  // n <= 2^31
    }
}

// One lane per key: its result from the lookup's and the object stage's, and the move of its
// object into its row in the form WAVE names (objects.h object_move).
template <bool WAVE>
__global__ void __launch_bounds__(256) k_get_scatter(const uint8_t* __restrict__ base, GetParams P,
                                                     const stormck_lookup_result* __restrict__ L,
                                                     const stormck_object_result* __restrict__ O,
                                                     const uint32_t* __restrict__ pos, uint64_t n,
                                                     stormck_get_result* __restrict__ results,
                                                     uint8_t* __restrict__ objects) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;  // no early return: the wave moves its rows together
    const uint8_t* src = nullptr;
    if (valid) {
        const uint32_t at = pos[i];
        stormck_object_result o;
        if (at != kGetNone) o = O[at];
        results[i] = get_finish(base, P, L[i], at != kGetNone ? &o : nullptr, &src);
    }
    if (!objects) return;  // the same in every lane
    object_move<WAVE>(valid ? objects + i * P.out_stride : nullptr, src, P.S);
}

// Every key ends at the space: one result for all, rows zeroed.
__global__ void __launch_bounds__(256) k_get_fill(uint8_t status, uint64_t n, GetParams P,
                                                  stormck_get_result* __restrict__ results, uint8_t* __restrict__ objects) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    results[i] = get_at_space(status);
    if (objects) object_row(objects + i * P.out_stride, nullptr, P.S, 0, 1);
}

int get_device(const void* d_store, const stormck_scrub_layout* layout, uint64_t space_id, const stormck_get_params* params,
               const void* d_keys, uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t len,
               uint64_t n, uint32_t flags, stormck_get_result* d_results, void* d_objects, uint64_t out_stride,
               void* d_workspace, uint64_t workspace_bytes, stormck_get_report* report, void* stream) {
    GetParams P;
    int rc = get_params(d_store, layout, params, d_keys, d_lens, len, n, flags, d_results, d_objects, out_stride, report, &P);
    if (rc) return rc;
    const uint32_t C = params->keys.chunks_per_block;
    if (n && (!d_workspace || workspace_bytes < get_workspace_bytes(n, C)))
        return fail(STORMCK_EINVAL, "get: workspace too small (stormck_get_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(d_store) | reinterpret_cast<uintptr_t>(d_workspace) |
         reinterpret_cast<uintptr_t>(d_results) | reinterpret_cast<uintptr_t>(d_offsets)) & 7)
        return fail(STORMCK_EINVAL, "get: d_store, d_results, d_offsets and d_workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_lens) & 3) return fail(STORMCK_EINVAL, "get: d_lens must be 4-byte aligned");
    rc = device_check();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(STORMCK_EINVAL, "get: stream is being captured (the call synchronises its stream)");
    get_report_clear(report, n);
    if (n == 0) return STORMCK_OK;

    // the workspace: the part the three engines use in turn, then the lookup's results, the dense IDs,
    // the object stage's results, each key's place, each place's key, the counts, the space
    const uint64_t m = (n + 7) & ~uint64_t{7};
    const uint64_t shared_bytes = std::max(lookup_workspace_bytes(n, C), spaces_workspace_bytes(1, stormck::kSpaceMaxSpaces));
    uint8_t* w = static_cast<uint8_t*>(d_workspace) + shared_bytes;
    stormck_lookup_result* L = reinterpret_cast<stormck_lookup_result*>(w);
    w += 32 * m;
    uint64_t* ids = reinterpret_cast<uint64_t*>(w);
    w += 8 * m;
    stormck_object_result* O = reinterpret_cast<stormck_object_result*>(w);
    w += 32 * m;
    uint32_t* pos = reinterpret_cast<uint32_t*>(w);
    w += 4 * m;
    uint32_t* key_of = reinterpret_cast<uint32_t*>(w);
    w += 4 * m;
    uint32_t* counts = reinterpret_cast<uint32_t*>(w);
    w += get_counts_bytes(n);
    uint64_t* d_space_id = reinterpret_cast<uint64_t*>(w);
    stormck_space_result* d_space = reinterpret_cast<stormck_space_result*>(w + 8);

    const uint8_t* base = static_cast<const uint8_t*>(d_store);
    uint8_t* objects = static_cast<uint8_t*>(d_objects);
    const unsigned wgs = static_cast<unsigned>((n + 255) / 256);  // n <= 2^31
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
                           workspace_bytes, &srep, stream);
        if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
        text0 = rc ? g_last_error : std::string();
        HIP_TRY(hipMemcpyAsync(&report->space, d_space, sizeof report->space, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        status0 = report->space.status;
    }
    if (status0 != STORMCK_TRACE_FOUND) {  // the walk of every key ends at the space
        hipLaunchKernelGGL(k_get_fill, dim3(wgs), dim3(256), 0, st, status0, n, P, d_results, objects);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        if (!trace_bad(status0)) return STORMCK_OK;
        report->first_bad = 0;
        return fail(STORMCK_EMISMATCH, text0);
    }
    rc = lookup_device(d_store, layout, &report->space.key_root, report->space.key_type, &params->keys, d_keys, stride,
                       d_offsets, d_lens, len, n, flags, L, nullptr, nullptr, d_workspace, workspace_bytes, &report->lookup,
                       stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string lookup_text = rc ? g_last_error : std::string();
    const uint64_t n_sel = report->lookup.n_status[STORMCK_TRACE_FOUND];
    hipLaunchKernelGGL(k_get_count<GetPick>, dim3(wgs), dim3(256), 0, st, GetPick{L}, n, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_get_scan, dim3(1), dim3(256), 0, st, counts, static_cast<uint64_t>(wgs));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_get_select<GetPick>, dim3(wgs), dim3(256), 0, st, GetPick{L}, n, counts, ids, pos, key_of);
    HIP_TRY(hipGetLastError());
    stormck_objects_report orep;
    rc = objects_device(d_store, layout, &report->space.object_root, report->space.object_type, &params->objects, ids, 8,
                        n_sel, flags, O, nullptr, 0, d_workspace, workspace_bytes, &orep, stream);
    if (rc != STORMCK_OK && rc != STORMCK_EMISMATCH) return rc;
    const std::string object_text = rc ? g_last_error : std::string();
    with_consts([&](auto WAVE) {
        hipLaunchKernelGGL((k_get_scatter<STORMCK_V(WAVE)>), dim3(wgs), dim3(256), 0, st, base, P, L, O, pos, n, d_results,
                           objects);
    }, fetch_wave(P.S));
    HIP_TRY(hipGetLastError());
    uint32_t bad_key = 0;
    if (orep.first_bad < n_sel)  // the error path alone reads more: the key of the object stage's first bad ID
        HIP_TRY(hipMemcpyAsync(&bad_key, key_of + orep.first_bad, sizeof bad_key, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return get_return(report, n, orep, n_sel, orep.first_bad < n_sel ? bad_key : n, lookup_text, object_text);
}
