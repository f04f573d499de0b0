// The open-addressing probe of an objectlist leaf: the third stage of keystore.GetObjectID
// (keystore/keystore.go:39-42: findChunkPointerForKey and verifyKeyInChunks, :112-133 and
// :178-208), as one function for the device kernel, the host leg and a stand-alone test program
// (include/stormck.h "lookup"; DESIGN.md "Lookup").
// Plain C++ with no HIP include: under hipcc the function is __host__ __device__ through
// STORMCK_PROBE_HD, under any other compiler the macro is empty
// (tests/lookup_probe_main.cpp compiles it with the host compiler and sanitizers).
//
// The leaf is objectlist.Block with C = ChunksPerBlock (blocks/objectlist/block.go:29-40):
//   Blob 0 | KeyTagReminders 32C | ObjectLinks 40C | ChunkPointers 48C | NextChunkPointers 50C |
//   ChunkPointerStates 52C | NUsedChunks 53C | FreeChunkIndex 53C+2;   (53C + 4 + 7) & ~7 bytes.
// It must be 8-byte aligned (every field is then aligned to its own size).
//
// The probe never reads outside the leaf, whatever the leaf holds: every index into it is
// checked against C first. Where storm would index or slice out of range (and panic), the item
// does not match, `malformed` is set and the probe goes on. Every loop is bounded: at most C
// slots, and per item at most 8 chunks that consume 32 key bytes each plus the one that ends
// the chain.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define STORMCK_PROBE_HD __host__ __device__
#else
#define STORMCK_PROBE_HD
#endif

namespace stormck {

constexpr uint32_t kObjlistChunkSize = 32;      // objectlist.ChunkSize
constexpr uint32_t kObjlistMaxKey = 256;        // objectlist.MaxKeyComponentLength
constexpr uint32_t kObjlistMaxChunks = 4096;    // the largest ChunksPerBlock the library takes
constexpr uint32_t kObjlistNoSlot = UINT32_MAX;
enum : uint8_t { kChunkFree = 0, kChunkDefined = 1, kChunkInvalid = 2 };
constexpr bool kObjlistBatched = false;         // the shipped form of the probe's reads: batching them measured no faster (DESIGN_LOG.md section 21)

struct ProbeOut {
    uint64_t object_id;  // found: ObjectLinks[index]; otherwise 0
    uint32_t index;      // found: the item; not found: the slot findChunkPointerForKey would hand out, or kObjlistNoSlot
    uint16_t probes;     // slots examined
    uint8_t found;
    uint8_t malformed;   // at least one item's chain would have taken storm out of range
};

STORMCK_PROBE_HD constexpr uint32_t objlist_leaf_len(uint32_t C) { return (53u * C + 4u + 7u) & ~7u; }

STORMCK_PROBE_HD inline uint64_t objlist_u64(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint64_t*>(p);
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
#endif
}

STORMCK_PROBE_HD inline uint32_t objlist_u16(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint16_t*>(p);
#else
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
#endif
}

// A key is at any alignment: on the device an unaligned load, or byte loads that do not wait
// for one another, where the leaf's own fields take one aligned load.
STORMCK_PROBE_HD inline uint64_t objlist_key64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// bytes.Equal(stored[:n], key[:n]) for n <= 32, stored 8-byte aligned. Compared in 8-byte words
// with no exit on the way: the loads are independent, where a byte loop that stops at the first
// difference waits for memory once per byte.
STORMCK_PROBE_HD inline bool objlist_bytes_equal(const uint8_t* stored, const uint8_t* key, uint32_t n) {
    uint64_t diff = 0;
    uint32_t j = 0;
    for (; j + 8 <= n; j += 8) diff |= objlist_u64(stored + j) ^ objlist_key64(key + j);
    for (; j < n; ++j) diff |= static_cast<uint64_t>(stored[j] ^ key[j]);
    return diff == 0;
}

// The same for a chunk whose 32 bytes are already in four words (little-endian, as storm's
// hosts and the device are): the full words, then the tail's bytes out of their word.
STORMCK_PROBE_HD inline bool objlist_words_equal(const uint64_t* stored, const uint8_t* key, uint32_t n) {
    uint64_t diff = 0;
    uint32_t j = 0;
    for (; j + 8 <= n; j += 8) diff |= stored[j / 8] ^ objlist_key64(key + j);
    for (; j < n; ++j) diff |= ((stored[j / 8] >> (8 * (j % 8))) & 0xff) ^ key[j];
    return diff == 0;
}

// verifyKeyInChunks after its reminder test: does the chunk chain at `chunk` spell the key?
// BATCHED: a chunk's 32 bytes are read together with its next pointer, before the pointer says
// how many of them count (they are inside the leaf whatever it says), so the two reads do not
// wait for one another.
template <bool BATCHED>
STORMCK_PROBE_HD inline bool objlist_chain_equals(const uint8_t* leaf, uint32_t C, uint32_t chunk, const uint8_t* key,
                                                  uint32_t key_len, uint8_t* malformed) {
    const uint8_t* next_pointers = leaf + 50u * C;
    uint32_t left = key_len;
    for (uint32_t step = 0; step <= kObjlistMaxKey / kObjlistChunkSize; ++step) {
        if (chunk >= C) break;  // storm indexes NextChunkPointers[chunk]
        const uint8_t* stored = leaf + chunk * kObjlistChunkSize;
        const uint32_t next = objlist_u16(next_pointers + 2u * chunk);
        uint64_t words[4] = {0, 0, 0, 0};
        if (BATCHED)
            for (uint32_t w = 0; w < 4; ++w) words[w] = objlist_u64(stored + 8u * w);
        if (next > C) {  // the last chunk: next - C bytes of it
            const uint32_t rest = next - C;
            if (rest > kObjlistChunkSize) break;
            if (rest != left) return false;
            return BATCHED ? objlist_words_equal(words, key, rest) : objlist_bytes_equal(stored, key, rest);
        }
        if (left < kObjlistChunkSize) break;  // storm slices key[:ChunkSize]
        if (!(BATCHED ? objlist_words_equal(words, key, kObjlistChunkSize)
                      : objlist_bytes_equal(stored, key, kObjlistChunkSize)))
            return false;
        key += kObjlistChunkSize;
        left -= kObjlistChunkSize;
        chunk = next;
    }
    *malformed = 1;  // a key of at most 256 bytes cannot pass 8 full chunks, so the loop ends by a break
    return false;
}

// findChunkPointerForKey for a key whose tag reminder at this leaf is `reminder`; A is
// objectlist.AddressingOffsets, C entries below C.
// BATCHED: a slot's state, reminder, chunk pointer and object link are read together (all four
// are inside the leaf for any index below C), and so are a chunk's bytes and its next pointer;
// the answer is the same, the reads of one step do not wait for one another.
template <bool BATCHED = kObjlistBatched>
STORMCK_PROBE_HD inline ProbeOut objlist_probe(const uint8_t* leaf, uint32_t C, const uint16_t* A, const uint8_t* key,
                                               uint32_t key_len, uint64_t reminder) {
    ProbeOut out{0, kObjlistNoSlot, 0, 0, 0};
    const uint8_t* reminders = leaf + 32u * C;
    const uint8_t* links = leaf + 40u * C;
    const uint8_t* chunk_pointers = leaf + 48u * C;
    const uint8_t* states = leaf + 52u * C;
    const uint32_t seed = static_cast<uint32_t>(reminder % C);
    uint32_t invalid = kObjlistNoSlot;
    for (uint32_t i = 0; i < C; ++i) {
        const uint32_t index = (seed + A[i]) % C;
        out.probes = static_cast<uint16_t>(i + 1);
        const uint8_t state = states[index];
        uint64_t slot_reminder = 0, slot_link = 0;
        uint32_t slot_chunk = 0;
        if (BATCHED) {
            slot_reminder = objlist_u64(reminders + 8u * index);
            slot_chunk = objlist_u16(chunk_pointers + 2u * index);
            slot_link = objlist_u64(links + 8u * index);
        }
        if (state == kChunkDefined) {
            if (!BATCHED) {
                slot_reminder = objlist_u64(reminders + 8u * index);
                if (slot_reminder == reminder) slot_chunk = objlist_u16(chunk_pointers + 2u * index);
            }
            if (slot_reminder == reminder &&
                objlist_chain_equals<BATCHED>(leaf, C, slot_chunk, key, key_len, &out.malformed)) {
                out.object_id = BATCHED ? slot_link : objlist_u64(links + 8u * index);
                out.index = index;
                out.found = 1;
                return out;
            }
        } else if (state == kChunkInvalid) {
            if (invalid == kObjlistNoSlot) invalid = index;
        } else if (state == kChunkFree) {
            out.index = invalid != kObjlistNoSlot ? invalid : index;
            return out;
        }  // any other state byte: storm's switch has no case for it
    }
    return out;  // every slot seen: storm returns (0, false) whatever Invalid slot it passed
}

}  // namespace stormck
