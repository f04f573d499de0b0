// GetObjects (include/storm_blocks.hpp) on the host leg: an object tree whose root is directly a
// blob leaf of 10 slots, built here with BlobObject<T>; the IDs are the results of GetObjectIDs
// over a key leaf, read in place; GetSpaces over a spacelist leaf that holds both roots, whose
// result feeds GetObjects; and Get over the whole store, singularity included.
// tests/test_objects_cpp.py compiles and runs it. Exit code 0 and "ok" on success.
#include <cstddef>
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

struct Item {  // a Go struct { A uint32; B [12]byte }: 16 bytes, alignment 4, no padding
    uint32_t a;
    uint8_t b[12];
};
static_assert(sizeof(Item) == 16 && sizeof(BlobObject<Item>) == 32 && sizeof(BlobObject<uint8_t>) == 16 &&
              sizeof(BlobObject<uint64_t>) == 24 && offsetof(BlobObject<Item>, State) == 24);

int main() {
    constexpr uint32_t N = 10, C = 10;
    const uint64_t bs = 1024, n_blocks = 4;  // the singularity, a key leaf, a blob leaf, a spacelist leaf
    std::vector<uint8_t> img(bs * n_blocks, 0);

    // block 2: the blob leaf, the root of the object tree: the reminder of an ID is the ID
    auto* slots = reinterpret_cast<BlobObject<Item>*>(img.data() + 2 * bs);
    const Item first{7, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}}, second{8, {12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1}};
    slots[9] = {4239, first, 1};   // start 9
    slots[0] = {4249, second, 1};  // start 9, probes on to 0: the probe wraps
    slots[1] = {4259, second, 2};  // Invalid: never a match
    const stormck_scrub_layout layout{bs, n_blocks, 10, 10, sizeof(ObjectListBlock<C>), 728};
    const Pointer objects_root{stormck_xxh64(img.data() + 2 * bs, 728), 2, 1};

    const ObjectID ids[4] = {4249, 4239, 4259, 4269};
    stormck_object_result res[4];
    Item got[4];
    std::memset(got, 0xEE, sizeof got);
    ObjectsResult r = GetObjects(img.data(), layout, objects_root, LeafBlockType, N, ids, 4, res, got, false);
    EXPECT(r.ok(4) && r.message.empty());
    EXPECT(res[0].status == STORMCK_TRACE_FOUND && res[0].index == 0 && res[0].probes == 2 && res[0].object_id == 4249);
    EXPECT(res[1].status == STORMCK_TRACE_FOUND && res[1].index == 9 && res[1].probes == 1 && res[1].address == 2);
    EXPECT(res[2].status == STORMCK_TRACE_ABSENT && res[2].index == 1 && res[2].probes == 4);  // 9, 0, 1 (Invalid), 2 (Free)
    EXPECT(res[3].status == STORMCK_TRACE_ABSENT && res[3].index == 1 && res[3].probes == 4);
    EXPECT(std::memcmp(&got[0], &second, sizeof second) == 0 && std::memcmp(&got[1], &first, sizeof first) == 0);
    const Item zero{};
    EXPECT(std::memcmp(&got[2], &zero, sizeof zero) == 0 && std::memcmp(&got[3], &zero, sizeof zero) == 0);
    EXPECT(r.report.n_status[STORMCK_TRACE_FOUND] == 2 && r.report.n_probed == 4 && r.report.probes == 11);
    EXPECT(r.report.trace.blocks_hashed[1] == 1);

    // block 1: a key leaf whose one key has the object ID 4239; its lookup result is the ID array
    const uint16_t A[C] = {3, 0, 7, 1, 9, 4, 2, 8, 6, 5};
    const char key[] = "a key";
    const uint64_t tag = stormck_xxh64(key, 5);
    auto* leaf = reinterpret_cast<ObjectListBlock<C>*>(img.data() + bs);
    const uint32_t index = (tag % C + A[0]) % C;
    leaf->ChunkPointerStates[index] = 1;
    leaf->KeyTagReminders[index] = tag;
    leaf->ObjectLinks[index] = 4239;
    leaf->ChunkPointers[index] = 4;
    std::memcpy(leaf->Blob + 4 * 32, key, 5);
    leaf->NextChunkPointers[4] = C + 5;
    leaf->NUsedChunks = 1;
    const Pointer keys_root{stormck_xxh64(leaf, sizeof *leaf), 1, 1};
    stormck_lookup_result looked_up[2];
    const char keys[2][8] = {"a key", "b key"};
    LookupResult l = GetObjectIDs(img.data(), layout, keys_root, LeafBlockType, A, C, keys, 8, nullptr, nullptr, 5, 2,
                                  looked_up, false);
    EXPECT(l.ok(2) && looked_up[0].object_id == 4239 && looked_up[1].status == STORMCK_TRACE_ABSENT);
    uint8_t rows[2][24];
    std::memset(rows, 0xEE, sizeof rows);
    r = GetObjects(img.data(), layout, objects_root, LeafBlockType, N, sizeof(Item), looked_up, sizeof looked_up[0], 1, res,
                   rows, 24, false);
    EXPECT(r.ok(1) && res[0].status == STORMCK_TRACE_FOUND && res[0].object_id == 4239);
    EXPECT(std::memcmp(rows[0], &first, 16) == 0 && rows[0][16] == 0xEE && rows[0][23] == 0xEE && rows[1][0] == 0xEE);

    // a space tree whose root is directly a spacelist leaf of 10 spaces (in an image of its own): the space
    // holds the two roots above, and GetSpaces hands them back ready for GetObjectIDs and GetObjects
    {
        std::vector<uint8_t> simg(bs * 2, 0);
        auto* sl = reinterpret_cast<SpaceListBlock<10>*>(simg.data() + bs);
        const uint64_t space_id = 57;  // seed 7
        Space& s = sl->Spaces[(7 + A[1]) % 10];
        sl->Spaces[(7 + A[0]) % 10].State = 2;  // Invalid, in the way
        s.SpaceIDTagReminder = space_id;
        s.NextObjectID = 4270;
        s.KeyStorePointer = keys_root;
        s.ObjectStorePointer = objects_root;
        s.KeyStoreBlockType = s.ObjectStoreBlockType = LeafBlockType;
        s.State = 1;
        const stormck_scrub_layout slayout{bs, 2, 10, 10, sizeof(ObjectListBlock<C>), 728};
        const Pointer spaces_root{stormck_xxh64(sl, sizeof *sl), 1, 1};
        const uint64_t space_ids[2] = {space_id, 67};
        stormck_space_result sres[2];
        SpacesResult sr = GetSpaces(simg.data(), slayout, spaces_root, LeafBlockType, A, space_ids, 2, sres, false);
        EXPECT(sr.ok(2) && sres[0].status == STORMCK_TRACE_FOUND && sres[0].probes == 2 && sres[0].next_object_id == 4270);
        EXPECT(std::memcmp(&sres[0].key_root, &keys_root, 24) == 0 && std::memcmp(&sres[0].object_root, &objects_root, 24) == 0);
        EXPECT(sres[0].key_type == LeafBlockType && sres[0].object_type == LeafBlockType);
        EXPECT(sres[1].status == STORMCK_TRACE_ABSENT && sres[1].index == (7u + A[0]) % 10 && sres[1].key_root.address == 0);
        Pointer back;
        std::memcpy(&back, &sres[0].object_root, sizeof back);
        r = GetObjects(img.data(), layout, back, static_cast<BlockType>(sres[0].object_type), N, ids, 4, res, got, false);
        EXPECT(r.ok(4) && std::memcmp(&got[1], &first, sizeof first) == 0);

        // the same spacelist leaf as block 3 of the store and a singularity that names it: Get is the
        // three calls in one
        std::memcpy(img.data() + 3 * bs, sl, sizeof *sl);
        SingularityBlock sing{};
        sing.StormID = 1;
        sing.Revision = 1;
        sing.NBlocks = n_blocks;
        sing.SpacePointer = Pointer{spaces_root.Checksum, 3, 1};
        sing.SpaceBlockType = LeafBlockType;
        sing.LastAllocatedBlock = 3;
        sing.Checksum = stormck_xxh64(&sing, sizeof sing);  // over the block with a zero Checksum
        std::memcpy(img.data(), &sing, sizeof sing);
        stormck_get_result gres[2];
        Item gobj[2];
        std::memset(gobj, 0xEE, sizeof gobj);
        GetResult g = Get(img.data(), layout, space_id, A, A, C, N, sizeof(Item), keys, 8, nullptr, nullptr, 5, 2, gres, gobj,
                          sizeof(Item), false);
        EXPECT(g.ok(2) && g.message.empty() && g.report.n_selected == 1 && g.report.n_found == 1);
        EXPECT(gres[0].stage == 2 && gres[0].status == STORMCK_TRACE_FOUND && gres[0].object_id == 4239 &&
               gres[0].key_address == 1 && gres[0].object_address == 2 && gres[0].index == 9);
        EXPECT(gres[1].stage == 1 && gres[1].status == STORMCK_TRACE_ABSENT && gres[1].object_address == 0);
        EXPECT(std::memcmp(&gobj[0], &first, sizeof first) == 0 && std::memcmp(&gobj[1], &zero, sizeof zero) == 0);
        EXPECT(g.report.space.next_object_id == 4270 && g.report.lookup.n_status[STORMCK_TRACE_FOUND] == 1);
        g = Get(img.data(), layout, 67, A, A, C, N, sizeof(Item), keys, 8, nullptr, nullptr, 5, 2, gres, gobj, sizeof(Item),
                false);  // storm's "space does not exist"
        EXPECT(g.ok(2) && gres[0].stage == 0 && gres[0].status == STORMCK_TRACE_ABSENT && gres[1].stage == 0);
        img[20] ^= 1;  // the singularity's Revision
        g = Get(img.data(), layout, space_id, A, A, C, N, sizeof(Item), keys, 8, nullptr, nullptr, 5, 2, gres, gobj,
                sizeof(Item), false);
        EXPECT(!g.ok(2) && g.report.first_bad == 0 && gres[1].stage == 0 && gres[1].status == STORMCK_TRACE_MISMATCH);
        EXPECT(g.message.rfind("checksum mismatch for block 0", 0) == 0);
        img[20] ^= 1;
    }

    // a flipped byte in the leaf: MISMATCH, the trace's words, the rows zeroed
    img[2 * bs + 700] ^= 1;
    r = GetObjects(img.data(), layout, objects_root, LeafBlockType, N, ids, 4, res, got, false);
    EXPECT(!r.ok(4) && r.report.first_bad == 0 && res[1].status == STORMCK_TRACE_MISMATCH && !r.message.empty());
    EXPECT(std::memcmp(&got[1], &zero, sizeof zero) == 0);
    r = GetObjects(img.data(), layout, objects_root, LeafBlockType, N, ids, 4, res, got, false, STORMCK_TRACE_LEAVES_UNVERIFIED);
    EXPECT(r.ok(4) && std::memcmp(&got[1], &first, sizeof first) == 0);
    std::puts("ok");
    return 0;
}
