// The open-addressing probe of a spacelist leaf: findSpace of spacestore.GetSpace
// (spacestore/spacestore.go:92-121), as one function for the device kernel, the host leg and a
// stand-alone test program (include/stormck.h "spaces"; DESIGN.md "Spaces").
// Plain C++ with no HIP include, like blob_probe.h.
//
// The leaf is spacelist.Block with S = SpacesPerBlock (blocks/spacelist/block.go:21-36): S spaces
// of 72 bytes, then NUsedSpaces as u16; (72 S + 2 + 7) & ~7 bytes. A space:
//   SpaceIDTagReminder 0 | NextObjectID 8 | KeyStorePointer 16 | ObjectStorePointer 40 |
//   KeyStoreBlockType 64 | ObjectStoreBlockType 65 | State 66.
// The leaf must be 8-byte aligned.
//
// The probe never reads outside the leaf, whatever the leaf holds: the only index into it is
// below S. Its one loop sees at most S slots. storm computes the index in uint16; for S up to
// 32768, which the library requires, seed + A[i] stays below 65536 and the arithmetic here is
// storm's.
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

constexpr uint32_t kSpaceSize = 72;            // unsafe.Sizeof(spacelist.Space)
constexpr uint32_t kSpaceStateOffset = 66;
constexpr uint32_t kSpaceMaxSpaces = 32768;    // the largest SpacesPerBlock the probe takes
constexpr uint32_t kSpaceNoSlot = UINT32_MAX;
enum : uint8_t { kSpaceFree = 0, kSpaceDefined = 1, kSpaceInvalid = 2 };  // spacelist.SpaceState

struct SpaceProbeOut {
    uint32_t index;   // found: the slot; not found: the slot findSpace hands EnsureSpace, or kSpaceNoSlot
    uint16_t probes;  // slots examined
    uint8_t found;    // a Defined slot with the reminder
};

STORMCK_PROBE_HD inline uint64_t space_u64(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint64_t*>(p);
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
#endif
}

// findSpace for a space ID whose tag reminder at this leaf is `reminder`; A is
// spacelist.AddressingOffsets, S entries below S.
STORMCK_PROBE_HD inline SpaceProbeOut space_probe(const uint8_t* leaf, uint32_t S, const uint16_t* A, uint64_t reminder) {
    SpaceProbeOut out{kSpaceNoSlot, 0, 0};
    const uint32_t seed = static_cast<uint32_t>(reminder % S);
    uint32_t invalid = kSpaceNoSlot;
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t index = (seed + A[i]) % S;
        const uint8_t* space = leaf + index * kSpaceSize;
        out.probes = static_cast<uint16_t>(i + 1);  // at most kSpaceMaxSpaces
        const uint8_t state = space[kSpaceStateOffset];
        if (state == kSpaceDefined) {
            if (space_u64(space) == reminder) {
                out.index = index;
                out.found = 1;
                return out;
            }
        } else if (state == kSpaceInvalid) {
            if (invalid == kSpaceNoSlot) invalid = index;
        } else if (state == kSpaceFree) {
            out.index = invalid != kSpaceNoSlot ? invalid : index;
            return out;
        }  // any other state byte: storm's switch has no case for it
    }
    return out;  // every slot seen: findSpace returns nil whatever Invalid slot it passed
}

}  // namespace stormck
