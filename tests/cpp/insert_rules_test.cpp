// The insert's rule functions and the planner's two spacelist origins, alone (tests/test_insert_rules.py):
// storm_amd/csrc/objlist_insert.h (rule B of include/stormck.h "insert"), blob_insert.h (rule D's
// slot step) and update_plan.h, on heap leaves of exactly their size, so that a sanitizer sees
// every byte read or written outside them. A stand-alone program with its own main.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../storm_amd/csrc/blob_insert.h"
#include "../../storm_amd/csrc/objlist_insert.h"
#include "../../storm_amd/csrc/update_plan.h"

using namespace stormck;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Leaf {  // objectlist.Block of C chunks on the heap, exactly objlist_leaf_len(C) bytes
    uint32_t C;
    uint8_t* b;
    std::vector<uint16_t> A;
    explicit Leaf(uint32_t c) : C(c), b(static_cast<uint8_t*>(std::calloc(objlist_leaf_len(c), 1))), A(c) {
        for (uint32_t i = 0; i < c; ++i) A[i] = static_cast<uint16_t>((i * 7 + 3) % c);  // a permutation: 7 and 10 are coprime
    }
    ~Leaf() { std::free(b); }
    Leaf(const Leaf&) = delete;
    uint32_t u16(uint32_t at) const { return objlist_u16(b + at); }
    uint32_t n_used() const { return objlist_header16(b + 53 * C); }
    uint32_t free_index() const { return objlist_header16(b + 53 * C + 2); }
    uint32_t next(uint32_t i) const { return u16(50 * C + 2 * i); }
    std::vector<uint8_t> bytes() const { return std::vector<uint8_t>(b, b + objlist_leaf_len(C)); }
    InsertOut insert(const std::string& key, uint64_t reminder, uint64_t link) {
        return objlist_insert(b, C, A.data(), reinterpret_cast<const uint8_t*>(key.data()), static_cast<uint32_t>(key.size()),
                              reminder, link);
    }
};

static std::string key_of(char c, size_t n) { return std::string(n, c); }

static void key_rules() {
    {  // an empty leaf: initFreeChunkList, two chunks, the last next pointer = C + 8
        Leaf l(10);
        const InsertOut o = l.insert(key_of('a', 40), 1234, 77);
        CHECK(o.verdict == kInsertPlaced && o.link == 77 && o.index == (1234u % 10u + l.A[0]) % 10u);
        CHECK(l.n_used() == 2 && l.free_index() == 2 && l.next(0) == 1 && l.next(1) == 10 + 8 && l.next(2) == 3 && l.next(9) == 10);
        CHECK(l.b[52 * 10 + o.index] == kChunkDefined && l.u16(48 * 10 + 2 * o.index) == 0);
        CHECK(objlist_u64(l.b + 32 * 10 + 8 * o.index) == 1234 && objlist_u64(l.b + 40 * 10 + 8 * o.index) == 77);
        CHECK(std::memcmp(l.b, key_of('a', 40).data(), 40) == 0 && l.b[40] == 0);
        // the same key again: the item, with its link
        const InsertOut again = l.insert(key_of('a', 40), 1234, 78);
        CHECK(again.verdict == kInsertRepeated && again.link == 77 && again.index == o.index && l.n_used() == 2);
        // lengths 1, 32, 33: one, one and two chunks; the chunk's other bytes keep what they held
        std::memset(l.b + 2 * 32, 0x5a, 32);
        CHECK(l.insert(key_of('b', 1), 1235, 1).verdict == kInsertPlaced && l.n_used() == 3 && l.next(2) == 10 + 1);
        CHECK(l.b[2 * 32] == 'b' && l.b[2 * 32 + 1] == 0x5a);
        CHECK(l.insert(key_of('c', 32), 1236, 2).verdict == kInsertPlaced && l.n_used() == 4 && l.next(3) == 10 + 32);
        CHECK(l.insert(key_of('d', 33), 1237, 3).verdict == kInsertPlaced && l.n_used() == 6 && l.next(4) == 5 && l.next(5) == 10 + 1);
        // 6 of 10 used: a 256-byte key needs 8 (KEY_FULL), a short one after it goes in, then the trigger
        const std::vector<uint8_t> before = l.bytes();
        CHECK(l.insert(key_of('e', 256), 1238, 4).verdict == kInsertFull && l.bytes() == before);
        CHECK(l.insert(key_of('f', 5), 1239, 5).verdict == kInsertPlaced && l.n_used() == 7);
        const std::vector<uint8_t> at_trigger = l.bytes();
        CHECK(l.insert(key_of('g', 5), 1240, 6).verdict == kInsertSplit && l.bytes() == at_trigger);
        CHECK(l.insert(key_of('f', 5), 1239, 9).verdict == kInsertRepeated);  // the match comes before the trigger
    }
    {  // a 256-byte key into an empty leaf: 8 chunks, the last one full
        Leaf l(10);
        CHECK(l.insert(key_of('k', 256), 5, 1).verdict == kInsertPlaced && l.n_used() == 8 && l.next(7) == 10 + 32 && l.free_index() == 8);
    }
    {  // no slot: no state storm knows anywhere
        Leaf l(10);
        std::memset(l.b + 52 * 10, 7, 10);
        const std::vector<uint8_t> before = l.bytes();
        CHECK(l.insert(key_of('a', 3), 9, 1).verdict == kInsertNoSlot && l.bytes() == before);
    }
    {  // the first Invalid slot on the sequence is reused, before the Free one behind it
        Leaf l(10);
        const uint32_t s0 = (1u + l.A[0]) % 10u, s1 = (1u + l.A[1]) % 10u;
        l.b[52 * 10 + s0] = kChunkInvalid;
        l.b[52 * 10 + s1] = kChunkInvalid;
        CHECK(l.insert(key_of('a', 3), 21, 1).index == s0);
        CHECK(l.insert(key_of('b', 3), 21, 2).index == s1);
    }
    {  // a free list that leaves the leaf: the key is refused and the leaf is as it was
        Leaf l(10);
        CHECK(l.insert(key_of('a', 3), 1, 1).verdict == kInsertPlaced);  // NUsedChunks 1, FreeChunkIndex 1
        objlist_put16(l.b + 50 * 10 + 2 * 1, 60000);
        const std::vector<uint8_t> before = l.bytes();
        CHECK(l.insert(key_of('b', 40), 2, 2).verdict == kInsertMalformed && l.bytes() == before);
        CHECK(l.insert(key_of('c', 5), 3, 3).verdict == kInsertPlaced && l.free_index() == 60000 && l.n_used() == 2);
        const std::vector<uint8_t> after = l.bytes();
        CHECK(l.insert(key_of('d', 5), 4, 4).verdict == kInsertMalformed && l.bytes() == after);  // FreeChunkIndex itself
    }
    {  // FreeChunkIndex of an empty leaf near the end: initFreeChunkList's list runs out
        Leaf l(10);
        objlist_put16(l.b + 53 * 10 + 2, 9);
        const std::vector<uint8_t> before = l.bytes();
        CHECK(l.insert(key_of('a', 40), 1, 1).verdict == kInsertMalformed && l.bytes() == before);
        CHECK(l.insert(key_of('a', 30), 1, 1).verdict == kInsertPlaced && l.free_index() == 10 && l.next(9) == 10 + 30);
    }
    {  // an odd C: NUsedChunks and FreeChunkIndex lie at odd offsets
        Leaf l(9);
        for (uint32_t i = 0; i < 9; ++i) l.A[i] = static_cast<uint16_t>((i * 2 + 1) % 9);
        CHECK(l.insert(key_of('a', 40), 4, 1).verdict == kInsertPlaced && l.n_used() == 2 && l.free_index() == 2);
        CHECK(l.b[53 * 9] == 2 && l.b[53 * 9 + 1] == 0 && l.b[53 * 9 + 2] == 2 && l.next(1) == 9 + 8);
        CHECK(l.insert(key_of('b', 3), 5, 2).verdict == kInsertPlaced && l.n_used() == 3);
    }
    {  // one chunk a leaf: SplitTrigger is 0, storm always splits
        Leaf l(1);
        CHECK(l.insert(key_of('a', 3), 1, 1).verdict == kInsertSplit);
    }
    {  // the largest leaf the insert takes, filled to its trigger with one-chunk keys
        Leaf l(1024);
        for (uint32_t i = 0; i < 1024; ++i) l.A[i] = static_cast<uint16_t>((i * 5 + 1) % 1024);
        uint32_t placed = 0;
        for (uint32_t i = 0; i < 800; ++i) {
            const std::string k = "key" + std::to_string(i);
            const InsertOut o = l.insert(k, 1000 + 13 * i, i);
            if (o.verdict == kInsertPlaced) ++placed;
            else CHECK(o.verdict == kInsertSplit && i >= 768);
        }
        CHECK(placed == 768 && l.n_used() == 768);
    }
}

static void slot_rules() {
    const uint32_t N = 10, S = 13;
    const uint64_t stride = blob_stride(S);
    const size_t len = N * stride + 8;
    uint8_t* leaf = static_cast<uint8_t*>(std::calloc(len, 1));
    uint8_t* compact = static_cast<uint8_t*>(std::calloc(16 * N, 1));
    uint64_t used = 0, used_c = 0;
    leaf[3 * stride + 8 + S] = compact[16 * 3 + 8] = kObjectInvalid;
    for (uint64_t r = 0; r < 9; ++r) {  // the whole leaf and the compact image go the same way
        const uint64_t reminder = 100 + 10 * r + 2;  // all start at slot 2
        const SlotOut a = blob_insert(leaf, N, S, reminder, &used), b = blob_insert(compact, N, 0, reminder, &used_c);
        CHECK(a.verdict == b.verdict && a.index == b.index && a.defined == b.defined && used == used_c);
        if (r < 7) {
            CHECK(a.verdict == kSlotPlaced && !a.defined && used == r + 1);
            CHECK(a.index == (r == 0 ? 2u : r == 1 ? 3u : r + 2));  // slot 2 is Free; then the Invalid slot 3 is passed and handed out; then 4, 5, ...
            CHECK(blob_u64(leaf + a.index * stride) == reminder && leaf[a.index * stride + 8 + S] == kObjectDefined);
        } else {
            CHECK(a.verdict == kSlotSplit && used == 7);  // N * 3 / 4
        }
    }
    const SlotOut again = blob_insert(leaf, N, S, 102, &used);  // Defined with its reminder: nothing is counted
    CHECK(again.verdict == kSlotPlaced && again.defined && again.index == 2 && used == 7);
    used = 0;
    for (uint32_t k = 0; k < N; ++k) leaf[k * stride + 8 + S] = 7;  // no state storm knows: findObject's nil
    CHECK(blob_insert(leaf, N, S, 5, &used).verdict == kSlotNone && used == 0);
    used = 7;
    CHECK(blob_insert(leaf, N, S, 5, &used).verdict == kSlotSplit);  // the 3/4 test comes first
    std::free(leaf);
    std::free(compact);
}

static void two_origins() {  // the spacelist leaf's two children: the key tree's root and the object tree's
    const UpdateGeometry G{1024, 100, 10, {256, 728, 536, 728}};
    const UpdateDirty d[] = {{5, 0, 0, STORMCK_SCRUB_POINTER},
                             {9, 5, 3, STORMCK_SCRUB_SPACELIST},
                             {20, 9, 4 | kUpdateKeyOrigin, STORMCK_SCRUB_OBJECTLIST},
                             {21, 9, 4, STORMCK_SCRUB_BLOB}};
    UpdatePlan P;
    CHECK(update_plan(d, 4, G, 3, 30, &P) == UpdateError::Ok);
    CHECK(P.first_new == 31 && P.heights == 3 && P.old_address == (std::vector<uint64_t>{20, 21, 9, 5}));
    const uint64_t at = 33 * 1024;  // the spacelist leaf's new copy
    CHECK(P.records[0].origin_pointer == at + 72 * 4 + 16 && P.records[0].origin_type == at + 72 * 4 + 64 && P.records[0].length == 536);
    CHECK(P.records[1].origin_pointer == at + 72 * 4 + 40 && P.records[1].origin_type == at + 72 * 4 + 65);
    CHECK(P.records[2].origin_pointer == 34 * 1024 + 24 * 3 && P.n_dirty[STORMCK_SCRUB_OBJECTLIST] == 1);
}

int main() {
    key_rules();
    slot_rules();
    two_origins();
    std::printf("ok\n");
    return 0;
}
