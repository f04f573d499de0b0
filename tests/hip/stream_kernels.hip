// Test-only direct launches of the two persistent streaming kernels (kernels.h
// k_xxh64_glds_skew, k_xxh64_glds_var) on the caller's device buffers and on a grid the
// caller chooses, so that tests/test_stream_kernels_gpu.py can reach with a few MiB the
// paths the shipped dispatch takes only from tens of GB (tests/stream_cases.py). Only
// template instances that launch_checksum (stormck.hip) ships are launched. These are
// separately compiled instances of the same source, not the kernels inside libstormck.so.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared
//         -o tests/hip/libstreamkernels.so tests/hip/stream_kernels.hip
// With -DSTORMCK_DEBUG_QUAD (tests/hip/libstreamkernels_debug.so) every quad merge counts a
// partially active quad (kernels.h quad_bcast) and streamk_debug_partial_quads reads the count.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../storm_amd/csrc/kernels.h"

namespace {
using namespace stormck;

// dispatch.h's launch constants, restated (tests/test_stream_cases.py compares them with
// that header's text); what kernels.h derives from them is asserted here
constexpr int kTileStripes = 16;
constexpr int kAuxNT = 2;
constexpr int kGldsWaves = 8;
constexpr int kSkewTiles = 8;
static_assert(GldsTile<kTileStripes, kGldsWaves>::BPW == 128 && GldsTile<kTileStripes, kGldsWaves>::ROW == 512 &&
                  GldsTile<kTileStripes, kGldsWaves>::TILE == 64 * 1024 && GldsTile<kTileStripes, 3>::PER_WAVE == 8,
              "128-block groups of 512-byte rows, a wave's 8 pieces its own 16 rows");

constexpr int kRefused = -1;

int done() {
    const hipError_t l = hipGetLastError();
    return static_cast<int>(l);
}

// {first_bad, n_bad} of a verify launch before any mismatch: {n, 0}
__global__ void k_result_init(unsigned long long* result, unsigned long long n) {
    result[0] = n;
    result[1] = 0;
}

template <bool V>
using Bool = std::integral_constant<bool, V>;

template <class F>
void with_bool(bool v, F&& f) {
    if (v) f(Bool<true>{});
    else f(Bool<false>{});
}

template <bool VERIFY, int W, int SKEW, bool LENS, bool OFFS, bool ORD>
void launch_var(unsigned grid, hipStream_t st, const uint8_t* base, uint64_t stride, const uint32_t* lens, uint32_t len,
                const uint64_t* offs, uint64_t n, uint64_t* out, const uint64_t* expected, unsigned long long* result,
                const uint32_t* order) {
    hipLaunchKernelGGL((k_xxh64_glds_var<kTileStripes, kAuxNT, VERIFY, W, SKEW, LENS, OFFS, ORD>), dim3(grid), dim3(64 * W),
                       0, st, base, stride, lens, len, offs, n, out, expected, result, result ? result + 1 : nullptr, order);
}
}  // namespace

// k_xxh64_glds_skew<16, 2, VERIFY, 8, 8> on `grid` workgroups of 512 threads. expected:
// verify into result = {first_bad, n_bad}, set to {n, 0} on the stream first. < 0: refused,
// nothing launched; > 0: a hipError_t.
extern "C" int streamk_skew(const void* base, uint64_t stride, uint32_t len, uint64_t n, uint64_t* out,
                            const uint64_t* expected, uint64_t* result, uint32_t grid, void* stream) {
    if (!base || n == 0 || grid == 0 || grid > 0x7fffffffu) return kRefused;
    if (expected ? !result : !out) return kRefused;
    if (len < 32u * kTileStripes || stride < len) return kRefused;
    if ((reinterpret_cast<uintptr_t>(base) & 15) || (stride & 15)) return kRefused;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* b = static_cast<const uint8_t*>(base);
    unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
    if (expected) {
        hipLaunchKernelGGL(k_result_init, dim3(1), dim3(1), 0, st, r, static_cast<unsigned long long>(n));
        hipLaunchKernelGGL((k_xxh64_glds_skew<kTileStripes, kAuxNT, true, kGldsWaves, kSkewTiles>), dim3(grid),
                           dim3(64 * kGldsWaves), 0, st, b, stride, len, n, out, expected, r, r + 1);
    } else {
        hipLaunchKernelGGL((k_xxh64_glds_skew<kTileStripes, kAuxNT, false, kGldsWaves, kSkewTiles>), dim3(grid),
                           dim3(64 * kGldsWaves), 0, st, b, stride, len, n, out, nullptr, nullptr, nullptr);
    }
    return done();
}

// k_xxh64_glds_var<16, 2, VERIFY, W, persistent ? 8 : 0, lens != null, offs != null, order != null>.
// Non-persistent: ceil(n / (16 * W)) workgroups, `grid` ignored; persistent (8 waves only):
// `grid` workgroups. order (the ordered gather's instances: 8 waves, offsets, no verify):
// out[order[i]] is block i's checksum. Returns as streamk_skew.
extern "C" int streamk_var(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, const uint64_t* offs,
                           const uint32_t* order, uint64_t n, uint64_t* out, const uint64_t* expected, uint64_t* result,
                           int waves, int persistent, uint32_t grid, void* stream) {
    if (!base || n == 0 || grid == 0 || grid > 0x7fffffffu) return kRefused;
    if (expected ? !result : !out) return kRefused;
    if (!lens && !offs) return kRefused;
    if (waves != 1 && waves != 3 && waves != kGldsWaves) return kRefused;
    if (persistent && waves != kGldsWaves) return kRefused;
    if (order && (!offs || expected || waves != kGldsWaves)) return kRefused;
    if (!offs && ((reinterpret_cast<uintptr_t>(base) & 15) || (stride & 15))) return kRefused;
    const uint64_t wgs = (n + 16 * static_cast<uint64_t>(waves) - 1) / (16 * static_cast<uint64_t>(waves));
    if (!persistent && wgs > 0x7fffffffULL) return kRefused;
    const unsigned g = persistent ? grid : static_cast<unsigned>(wgs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* b = static_cast<const uint8_t*>(base);
    unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
    if (expected) hipLaunchKernelGGL(k_result_init, dim3(1), dim3(1), 0, st, r, static_cast<unsigned long long>(n));
    if (order) {
        with_bool(persistent != 0, [&](auto P) {
            with_bool(lens != nullptr, [&](auto L) {
                launch_var<false, kGldsWaves, decltype(P)::value ? kSkewTiles : 0, decltype(L)::value, true, true>(
                    g, st, b, stride, lens, len, offs, n, out, nullptr, nullptr, order);
            });
        });
        return done();
    }
    with_bool(expected != nullptr, [&](auto V) {
        with_bool(lens != nullptr, [&](auto L) {
            with_bool(offs != nullptr, [&](auto O) {
                constexpr bool v = decltype(V)::value, l = decltype(L)::value, o = decltype(O)::value;
                if constexpr (l || o) {
                    if (persistent) launch_var<v, kGldsWaves, kSkewTiles, l, o, false>(g, st, b, stride, lens, len, offs, n, out, expected, r, nullptr);
                    else if (waves == 1) launch_var<v, 1, 0, l, o, false>(g, st, b, stride, lens, len, offs, n, out, expected, r, nullptr);
                    else if (waves == 3) launch_var<v, 3, 0, l, o, false>(g, st, b, stride, lens, len, offs, n, out, expected, r, nullptr);
                    else launch_var<v, kGldsWaves, 0, l, o, false>(g, st, b, stride, lens, len, offs, n, out, expected, r, nullptr);
                }
            });
        });
    });
    return done();
}

// hipGetLastError of the calling thread (the runtime this library is linked to), for the
// check after a stream sync.
extern "C" int streamk_last_error() { return static_cast<int>(hipGetLastError()); }

#ifdef STORMCK_DEBUG_QUAD
// This translation unit's count of quad merges made with a partially active quad
// (kernels.h g_partial_quads), after a device sync; reset: zero it.
extern "C" int streamk_debug_partial_quads(uint64_t* count, int reset) {
    if (!count) return kRefused;
    unsigned long long v = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_partial_quads), sizeof v);
    if (e == hipSuccess && reset) {
        const unsigned long long z = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_partial_quads), &z, sizeof z);
    }
    *count = v;
    return static_cast<int>(e);
}
#endif
