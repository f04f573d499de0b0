// The open-addressing probe of a blob leaf: findObject of objectstore.GetObject
// (objectstore/objectstore.go:92-123), as one function for the device kernel, the host leg and
// a stand-alone test program (include/stormck.h "objects"; DESIGN.md "Objects").
// Plain C++ with no HIP include: under hipcc the function is __host__ __device__ through
// STORMCK_PROBE_HD, under any other compiler the macro is empty
// (tests/blob_probe_main.cpp compiles it with the host compiler and sanitizers).
//
// The leaf is blob.Block (blocks/blob/block.go:25-29): Data[blob_len - 8], then NUsedSlots as
// u64. findObject views Data as N = objectsPerBlock values of Go's blob.Object[T]:
//   ObjectIDTagReminder u64 at 0 | Object T at 8 | State byte at 8 + S,   S = unsafe.Sizeof(T).
// Go lays a struct's fields out in order, each at the next multiple of its alignment, and
// rounds the struct's size up to its largest alignment. The reminder puts that at 8. T follows
// at 8, a multiple of every alignment up to 8; S is itself a multiple of T's alignment, so the
// one-byte State sits right behind T at 8 + S; and the size rounds 8 + S + 1 up to 8:
//   stride = (8 + S + 1 + 7) & ~7
// for every T of alignment at most 8 (Go has no wider one on storm's platforms).
// The leaf must be 8-byte aligned; every slot's reminder and object then are.
//
// The probe never reads outside the leaf, whatever the leaf holds: the only index into it is
// below N, and the caller has checked N * stride <= blob_len - 8. Its one loop sees at most N
// slots.
#pragma once

#include <cstdint>
#include <cstring>

#ifndef STORMCK_PROBE_HD
#if defined(__HIPCC__)
#define STORMCK_PROBE_HD __host__ __device__
#else
#define STORMCK_PROBE_HD
#endif
#endif

namespace stormck {

constexpr uint32_t kBlobMaxObjects = 4095;  // the largest objectsPerBlock the library takes: probes fits a u16
constexpr uint32_t kBlobNoSlot = UINT32_MAX;
enum : uint8_t { kObjectFree = 0, kObjectDefined = 1, kObjectInvalid = 2 };  // blob.ObjectState

struct BlobProbeOut {
    uint32_t index;   // found: the slot; not found: the slot findObject hands SetObject, or kBlobNoSlot
    uint16_t probes;  // slots examined
    uint8_t found;    // a Defined slot with the reminder
};

// unsafe.Sizeof(blob.Object[T]) for unsafe.Sizeof(T) == S (the derivation is above)
STORMCK_PROBE_HD constexpr uint64_t blob_stride(uint32_t S) { return (8ull + S + 1 + 7) & ~7ull; }

// Do N slots of S-byte objects fit the Data of a leaf of blob_len bytes?
STORMCK_PROBE_HD constexpr bool blob_fits(uint32_t N, uint32_t S, uint64_t blob_len) {
    return blob_len >= 8 && N * blob_stride(S) <= blob_len - 8;
}

STORMCK_PROBE_HD inline uint64_t blob_u64(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint64_t*>(p);
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
#endif
}

// Where slot k's object lies in the leaf: S bytes, 8-byte aligned.
STORMCK_PROBE_HD inline const uint8_t* blob_object(const uint8_t* leaf, uint32_t S, uint32_t k) {
    return leaf + k * blob_stride(S) + 8;
}

// findObject for an object ID whose tag reminder at this leaf is `reminder`.
STORMCK_PROBE_HD inline BlobProbeOut blob_probe(const uint8_t* leaf, uint32_t N, uint32_t S, uint64_t reminder) {
    BlobProbeOut out{kBlobNoSlot, 0, 0};
    const uint64_t stride = blob_stride(S);
    const uint32_t start = static_cast<uint32_t>(reminder % N);
    uint32_t invalid = kBlobNoSlot;
    for (uint32_t j = 0; j < N; ++j) {
        const uint32_t k = start + j < N ? start + j : start + j - N;  // (start + j) % N: both are below N
        const uint8_t* slot = leaf + k * stride;
        out.probes = static_cast<uint16_t>(j + 1);
        const uint8_t state = slot[8 + S];
        if (state == kObjectDefined) {
            if (blob_u64(slot) == reminder) {
                out.index = k;
                out.found = 1;
                return out;
            }
        } else if (state == kObjectInvalid) {
            if (invalid == kBlobNoSlot) invalid = k;
        } else if (state == kObjectFree) {
            out.index = invalid != kBlobNoSlot ? invalid : k;
            return out;
        }  // any other state byte: storm's switch has no case for it
    }
    return out;  // every slot seen: findObject returns nil whatever Invalid slot it passed
}

}  // namespace stormck
