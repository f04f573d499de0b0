// The insert of one key into an objectlist leaf without a split: keystore.EnsureObjectID after
// its trace (keystore/keystore.go:72-109: findChunkPointerForKey, the SplitTrigger test,
// setKeyInChunks, initFreeChunkList), as one function for the device kernel, the host leg and a
// stand-alone test program (include/stormck.h "insert", rule B; DESIGN.md "Insert").
// Plain C++ with no HIP include, as objlist_probe.h, whose probe it calls.
//
// The leaf image is written in place. Nothing outside it is read or written, whatever it holds:
// every index into it is checked against C first, and where storm would index out of range the
// key is refused (kInsertMalformed) with the image as it was.
#pragma once

#include "objlist_probe.h"

namespace stormck {

enum : uint8_t { kInsertPlaced = 0, kInsertRepeated, kInsertSplit, kInsertNoSlot, kInsertFull, kInsertMalformed };

struct InsertOut {
    uint64_t link;    // kInsertRepeated: ObjectLinks[index] of the item that holds the key
    uint32_t index;   // kInsertPlaced, kInsertRepeated: the item
    uint8_t verdict;  // kInsert*
};

STORMCK_PROBE_HD inline void objlist_put16(uint8_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(v);
#else
    const uint16_t w = static_cast<uint16_t>(v);
    memcpy(p, &w, 2);
#endif
}

STORMCK_PROBE_HD inline void objlist_put64(uint8_t* p, uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint64_t*>(p) = v;
#else
    memcpy(p, &v, 8);
#endif
}

// NUsedChunks and FreeChunkIndex lie at 53 C and 53 C + 2, which is odd for an odd C (every other
// 16-bit field of the leaf is at an even offset): they are read and written byte by byte.
STORMCK_PROBE_HD inline uint32_t objlist_header16(const uint8_t* p) { return p[0] | static_cast<uint32_t>(p[1]) << 8; }
STORMCK_PROBE_HD inline void objlist_put_header16(uint8_t* p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v);
    p[1] = static_cast<uint8_t>(v >> 8);
}

// objectlist.SplitTrigger
STORMCK_PROBE_HD constexpr uint32_t objlist_split_trigger(uint32_t C) { return C * 3 / 4; }

// One key against the leaf as it is now. `link` goes into ObjectLinks[index] when the key is
// placed. key_len is 1..256 (the lookup refused every other length).
STORMCK_PROBE_HD inline InsertOut objlist_insert(uint8_t* leaf, uint32_t C, const uint16_t* A, const uint8_t* key,
                                                 uint32_t key_len, uint64_t reminder, uint64_t link) {
    uint8_t* next_pointers = leaf + 50u * C;
    // 1. findChunkPointerForKey: a Defined match is an item an earlier key of the batch put there
    const ProbeOut o = objlist_probe(leaf, C, A, key, key_len, reminder);
    if (o.found) return InsertOut{o.object_id, o.index, kInsertRepeated};
    // 2. the split trigger
    uint32_t n_used = objlist_header16(leaf + 53u * C);
    if (n_used >= objlist_split_trigger(C)) return InsertOut{0, kObjlistNoSlot, kInsertSplit};
    // 3. no slot was handed out
    if (o.index == kObjlistNoSlot) return InsertOut{0, kObjlistNoSlot, kInsertNoSlot};
    // 4. setKeyInChunks's room test
    const uint32_t need = (key_len + kObjlistChunkSize - 1) / kObjlistChunkSize;
    if (n_used + need > C) return InsertOut{0, kObjlistNoSlot, kInsertFull};
    // 5. the walk of the free list before anything changes: storm indexes NextChunkPointers[FreeChunkIndex]
    const bool fresh = n_used == 0;  // initFreeChunkList: NextChunkPointers[i] = i + 1
    uint32_t free_index = objlist_header16(leaf + 53u * C + 2);
    uint32_t f = free_index;
    for (uint32_t s = 0; s < need; ++s) {
        if (f >= C) return InsertOut{0, kObjlistNoSlot, kInsertMalformed};
        f = fresh ? f + 1 : objlist_u16(next_pointers + 2u * f);
    }
    if (fresh)
        for (uint32_t i = 0; i < C; ++i) objlist_put16(next_pointers + 2u * i, i + 1);
    leaf[52u * C + o.index] = kChunkDefined;
    objlist_put16(leaf + 48u * C + 2u * o.index, free_index);
    objlist_put64(leaf + 32u * C + 8u * o.index, reminder);
    uint32_t last = 0, copied = 0, left = key_len;
    while (left > 0) {  // `need` rounds, every index checked by the walk above
        ++n_used;
        last = free_index;
        free_index = objlist_u16(next_pointers + 2u * last);
        copied = left < kObjlistChunkSize ? left : kObjlistChunkSize;
        uint8_t* chunk = leaf + last * kObjlistChunkSize;
        for (uint32_t b = 0; b < copied; ++b) chunk[b] = key[b];
        key += copied;
        left -= copied;
    }
    objlist_put16(next_pointers + 2u * last, C + copied);
    objlist_put_header16(leaf + 53u * C, n_used);
    objlist_put_header16(leaf + 53u * C + 2, free_index);
    objlist_put64(leaf + 40u * C + 8u * o.index, link);
    return InsertOut{link, o.index, kInsertPlaced};
}

}  // namespace stormck
