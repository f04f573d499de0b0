// Test-only entry points to the gather's locality order (kernels.h k_order_*), so that
// tests/test_gather_order_gpu.py can run the order pass on bare numbers: every buffer is
// the caller's device memory, nothing is copied and no offset is dereferenced.
// Compiled with -DSTORMCK_PROBES (k_order_rank, the index-only placement):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DSTORMCK_PROBES
//         -o tests/hip/liborderpass.so tests/hip/order_pass.hip
#include <hip/hip_runtime.h>

#include "../../storm_amd/csrc/kernels.h"

namespace {
int done(hipError_t e) {
    const hipError_t l = hipGetLastError();
    return e != hipSuccess ? static_cast<int>(e) : static_cast<int>(l);
}
}  // namespace

// launch_checksum's order pass: bounds 2 * 4096 words, cursor 4096 words, order / s_offs /
// s_lens n entries each (lens and s_lens may both be null).
extern "C" int orderpass_run(const uint64_t* offs, const uint32_t* lens, uint64_t n, uint32_t* bounds, uint32_t* cursor,
                             uint32_t* order, uint64_t* s_offs, uint32_t* s_lens, int idx, void* stream) {
    if (!offs || !bounds || !cursor || !order || !s_offs || n == 0 || n >= (uint64_t{1} << 32) || (lens && !s_lens)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return done(idx ? stormck::order_pass<true>(offs, lens, n, bounds, cursor, order, s_offs, s_lens, st)
                    : stormck::order_pass<false>(offs, lens, n, bounds, cursor, order, s_offs, s_lens, st));
}

// out[order[k]] = s_out[k], in launch_checksum's grid.
extern "C" int orderpass_scatter(const uint32_t* order, const uint64_t* s_out, uint64_t* out, uint64_t n, void* stream) {
    if (!order || !s_out || !out) return -1;
    hipLaunchKernelGGL(stormck::k_order_scatter, dim3(2048), dim3(256), 0, static_cast<hipStream_t>(stream), order, s_out,
                       out, n);
    return done(hipSuccess);
}

// The full groups of 128 re-dealt by length rank; G: the hash kernel's grid (its group step).
extern "C" int orderpass_rank(uint32_t* order, uint64_t* s_offs, uint32_t* s_lens, uint64_t n, uint64_t G, void* stream) {
    if (!order || !s_offs || !s_lens || G == 0 || n / 128 == 0 || n / 128 > 0x7fffffffULL) return -1;
    hipLaunchKernelGGL(stormck::k_order_rank, dim3(static_cast<unsigned>(n / 128)), dim3(128), 0,
                       static_cast<hipStream_t>(stream), order, s_offs, s_lens, G);
    return done(hipSuccess);
}
