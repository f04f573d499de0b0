// GetObjectIDs (include/storm_blocks.hpp) on the host leg: a key tree whose root is directly an
// objectlist leaf of 10 chunks, built here with ObjectListBlock<10>; tests/test_lookup.py compiles
// and runs it. Exit code 0 and "ok" on success.
#include <cstdio>
#include <cstring>
#include <vector>

#include "storm_blocks.hpp"

using namespace storm::blocks;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    constexpr uint32_t C = 10;
    const uint64_t bs = 1024, n_blocks = 2;
    const uint16_t A[C] = {3, 0, 7, 1, 9, 4, 2, 8, 6, 5};
    const char stored[] = "a key of forty bytes, held in two chunks";  // 40 bytes
    const uint32_t len = 40;
    static_assert(sizeof stored == 41);
    const uint64_t tag = stormck_xxh64(stored, len);  // the root is the leaf: the reminder is the tag

    std::vector<uint8_t> img(bs * n_blocks, 0);
    auto* leaf = reinterpret_cast<ObjectListBlock<C>*>(img.data() + bs);
    const uint32_t index = (tag % C + A[1]) % C;  // the second slot of the key's sequence; the first holds another item
    leaf->ChunkPointerStates[(tag % C + A[0]) % C] = 1;
    leaf->KeyTagReminders[(tag % C + A[0]) % C] = tag + 1;
    leaf->ChunkPointerStates[index] = 1;
    leaf->KeyTagReminders[index] = tag;
    leaf->ObjectLinks[index] = 4242;
    leaf->ChunkPointers[index] = 5;
    std::memcpy(leaf->Blob + 5 * 32, stored, 32);
    leaf->NextChunkPointers[5] = 2;
    std::memcpy(leaf->Blob + 2 * 32, stored + 32, 8);
    leaf->NextChunkPointers[2] = C + 8;
    leaf->NUsedChunks = 2;

    const stormck_scrub_layout layout{bs, n_blocks, 10, 10, sizeof(ObjectListBlock<C>), 728};
    Pointer root{stormck_xxh64(leaf, sizeof *leaf), 1, 1};
    char keys[3][48] = {};
    std::memcpy(keys[0], stored, len);
    std::memcpy(keys[1], stored, len);
    keys[1][39] ^= 1;
    std::memcpy(keys[2], stored, len);
    stormck_lookup_result res[3];
    LookupResult r = GetObjectIDs(img.data(), layout, root, LeafBlockType, A, C, keys, 48, nullptr, nullptr, len, 3, res,
                                  false);
    EXPECT(r.ok(3) && r.message.empty());
    EXPECT(res[0].status == STORMCK_TRACE_FOUND && res[0].object_id == 4242 && res[0].index == index && res[0].probes == 2);
    EXPECT(res[0].address == 1 && res[0].reminder == tag);
    EXPECT(res[1].status == STORMCK_TRACE_ABSENT && res[1].object_id == 0);
    EXPECT(std::memcmp(&res[2], &res[0], sizeof res[0]) == 0);
    EXPECT(r.report.n_status[STORMCK_TRACE_FOUND] == 2 && r.report.n_probed == 3 && r.report.n_malformed == 0);
    EXPECT(r.report.trace.blocks_hashed[1] == 1 && r.report.trace.n_status[STORMCK_TRACE_FOUND] == 3);

    const uint32_t lens[3] = {len, 0, len};  // an empty key: KEY, storm's message
    r = GetObjectIDs(img.data(), layout, root, LeafBlockType, A, C, keys, 48, nullptr, lens, 0, 3, res, false);
    EXPECT(!r.ok(3) && r.report.first_bad == 1 && res[1].status == STORMCK_LOOKUP_KEY && res[1].index == STORMCK_LOOKUP_NO_SLOT);
    EXPECT(r.message == "key cannot be empty" && res[2].object_id == 4242);
    std::puts("ok");
    return 0;
}
