// The slot step of objectstore.SetObject without a split (objectstore/objectstore.go:59-85:
// findObject, the 3/4 test, the slot's reminder and state), as one function for the device
// kernel, the host leg and a stand-alone test program (include/stormck.h "insert", rule D;
// DESIGN.md "Insert"). Plain C++ with no HIP include, as blob_probe.h, whose probe it calls.
//
// It works on any image of N slots that blob_probe can read: a whole blob leaf with its S, or a
// compact image with S = 0 (16 bytes a slot: the reminder, then the state byte) that holds only
// what the step reads and writes. The object's bytes and NUsedSlots are the caller's.
#pragma once

#include "blob_probe.h"

namespace stormck {

enum : uint8_t { kSlotPlaced = 0, kSlotSplit = 1, kSlotNone = 2 };

struct SlotOut {
    uint32_t index;   // kSlotPlaced: the slot
    uint8_t verdict;  // kSlot*
    uint8_t defined;  // kSlotPlaced: the slot was Defined with the reminder already (nothing is counted)
};

STORMCK_PROBE_HD inline void blob_put64(uint8_t* p, uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint64_t*>(p) = v;
#else
    memcpy(p, &v, 8);
#endif
}

// One ID against the slots as they are now; *n_used is NUsedSlots as it is now.
STORMCK_PROBE_HD inline SlotOut blob_insert(uint8_t* slots, uint32_t N, uint32_t S, uint64_t reminder, uint64_t* n_used) {
    const BlobProbeOut o = blob_probe(slots, N, S, reminder);
    if (o.found) return SlotOut{o.index, kSlotPlaced, 1};
    if (*n_used >= static_cast<uint64_t>(N) * 3 / 4) return SlotOut{kBlobNoSlot, kSlotSplit, 0};  // storm splits
    if (o.index == kBlobNoSlot) return SlotOut{kBlobNoSlot, kSlotNone, 0};                         // storm errors
    uint8_t* slot = slots + o.index * blob_stride(S);
    ++*n_used;
    blob_put64(slot, reminder);
    slot[8 + S] = kObjectDefined;
    return SlotOut{o.index, kSlotPlaced, 0};
}

}  // namespace stormck
