// storm_amd/csrc/update_plan.h alone, with a plain C++17 compiler (tests/test_update_plan.py): the
// heights, the order, the new addresses, the origins, the room check and the singularity on
// hand-made dirty forests. A stand-alone program: it runs as built and under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../storm_amd/csrc/update_plan.h"

using namespace stormck;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const UpdateGeometry G{1024, 200, 10, {256, 728, 536, 728}};
enum { P = STORMCK_SCRUB_POINTER, SL = STORMCK_SCRUB_SPACELIST, B = STORMCK_SCRUB_BLOB };

// The irregular forest: space root 9 -> spacelist 8 (space 3) -> object root 7 -> leaf 2 (slot 2)
// and pointer block 6 (slot 5) -> leaves 4 (slot 0) and 5 (slot 4). Given in no order.
static std::vector<UpdateDirty> irregular() {
    return {{5, 6, 4, B}, {7, 8, 3, P}, {2, 7, 2, B}, {9, 0, 0, P}, {6, 7, 5, P}, {8, 9, 1, SL}, {4, 6, 0, B}};
}

static void test_irregular() {
    const auto d = irregular();
    UpdatePlan p;
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::Ok);
    const uint64_t order[] = {2, 4, 5, 6, 7, 8, 9};  // heights 0 0 0 1 2 3 4
    CHECK(p.records.size() == 7 && p.first_new == 101 && p.last_allocated == 107 && p.heights == 5);
    for (int k = 0; k < 7; ++k) {
        CHECK(p.old_address[k] == order[k]);
        CHECK(p.records[k].address == 101u + k && p.records[k].data_offset == (101u + k) * 1024);
        CHECK(p.records[k].birth_revision == 4);
    }
    CHECK(p.n_dirty[P] == 3 && p.n_dirty[SL] == 1 && p.n_dirty[B] == 3 && p.n_dirty[STORMCK_SCRUB_OBJECTLIST] == 0);
    CHECK(p.bytes_hashed == 3 * 256 + 728 + 3 * 728);
    // leaf 2 under the object root (new 105), slot 2
    CHECK(p.records[0].parent == 4 && p.records[0].origin_pointer == 105 * 1024 + 24 * 2 &&
          p.records[0].origin_type == 105 * 1024 + 240 + 2 && p.records[0].type == STORMCK_LEAF_BLOCK &&
          p.records[0].length == 728);
    // leaf 5 under pointer block 6 (new 104), slot 4
    CHECK(p.records[2].parent == 3 && p.records[2].origin_pointer == 104 * 1024 + 24 * 4);
    // pointer block 6 under the object root, slot 5
    CHECK(p.records[3].parent == 4 && p.records[3].origin_type == 105 * 1024 + 240 + 5 && p.records[3].type == STORMCK_POINTER_BLOCK &&
          p.records[3].length == 256);
    // the object root under the spacelist leaf (new 106), space 3: ObjectStorePointer @72k+40, its type @72k+65
    CHECK(p.records[4].parent == 5 && p.records[4].origin_pointer == 106 * 1024 + 72 * 3 + 40 &&
          p.records[4].origin_type == 106 * 1024 + 72 * 3 + 65);
    // the spacelist leaf under the space root (new 107), slot 1
    CHECK(p.records[5].parent == 6 && p.records[5].origin_pointer == 107 * 1024 + 24 && p.records[5].type == STORMCK_LEAF_BLOCK);
    // the topmost block: the singularity is its origin
    CHECK(p.records[6].parent == STORMCK_NO_PARENT && p.records[6].origin_pointer == STORMCK_NO_ORIGIN);
    for (const stormck_dirty_block& r : p.records)
        if (r.parent != STORMCK_NO_PARENT) CHECK(static_cast<uint64_t>(r.parent) > static_cast<uint64_t>(&r - p.records.data()));

    uint8_t sing[72];
    for (int i = 0; i < 72; ++i) sing[i] = static_cast<uint8_t>(i + 1);
    auto sum = [](const uint8_t* q, size_t n) {
        uint64_t s = 0;
        for (size_t i = 0; i < n; ++i) s = s * 31 + q[i];
        return s;
    };
    uint8_t want[72];
    std::memcpy(want, sing, 72);
    update_singularity(sing, 0xABCDEF, p, 3, sum);
    auto put = [&](int at, uint64_t v) { std::memcpy(want + at, &v, 8); };
    put(0, 0), put(16, 4), put(32, 0xABCDEF), put(40, 107), put(48, 4), put(64, 107);
    want[56] = STORMCK_POINTER_BLOCK;
    put(0, sum(want, 72));
    CHECK(std::memcmp(sing, want, 72) == 0);  // StormID @8, NBlocks @24 and byte 57.. are kept
}

static void test_depth0_and_room() {
    // depth 0: the object root is a leaf whose origin is the space's record; the space root is the spacelist leaf
    const std::vector<UpdateDirty> d = {{3, 0, 0, SL}, {2, 3, 7, B}};
    UpdatePlan p;
    CHECK(update_plan(d.data(), 2, G, 9, 197, &p) == UpdateError::Ok);  // L + D = 199 < 200
    CHECK(p.old_address[0] == 2 && p.old_address[1] == 3 && p.heights == 2 && p.last_allocated == 199);
    CHECK(p.records[0].origin_pointer == 199 * 1024 + 72 * 7 + 40 && p.records[1].origin_pointer == STORMCK_NO_ORIGIN);
    CHECK(p.records[1].type == STORMCK_LEAF_BLOCK);
    CHECK(update_plan(d.data(), 2, G, 9, 198, &p) == UpdateError::NoSpace);  // L + D == n_blocks
    CHECK(update_plan(d.data(), 2, G, 9, 200, &p) == UpdateError::NoSpace);  // L >= n_blocks
    CHECK(update_plan(d.data(), 2, G, 9, UINT64_MAX, &p) == UpdateError::NoSpace);
    CHECK(update_plan(d.data(), 1, G, 9, 198, &p) == UpdateError::Ok);
}

static void test_errors() {
    UpdatePlan p;
    CHECK(update_plan(nullptr, 0, G, 3, 100, &p) == UpdateError::Empty);
    auto d = irregular();
    d.push_back({4, 6, 0, B});
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::Duplicate);
    d = irregular();
    d[0].parent = 77;
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::NoParent);
    d = irregular();
    d[4].parent = 4;  // a blob leaf holds no origins
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::ParentKind);
    d = irregular();
    d[1].parent = 0;  // two topmost blocks
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::Top);
    d = irregular();
    d[1].parent = 6;  // 7 -> 6 -> 7
    d[4].kind = P;
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::Cycle);
    d = irregular();
    d[0].kind = 9;
    CHECK(update_plan(d.data(), d.size(), G, 3, 100, &p) == UpdateError::ParentKind);
    for (int e = 1; e <= 8; ++e) CHECK(update_error_message(static_cast<UpdateError>(e))[0] != 0);
}

// A wide forest in heap memory of exactly its size: 300 leaves under 30 pointer blocks under one root.
static void test_wide() {
    std::vector<UpdateDirty> d;
    d.push_back({1000, 0, 0, SL});
    d.push_back({999, 1000, 2, P});
    for (uint32_t b = 0; b < 30; ++b) {
        d.push_back({500 + b, 999, b % 10, P});
        for (uint32_t l = 0; l < 10; ++l) d.push_back({10 + 10 * b + l, 500 + b, l, B});
    }
    UpdateGeometry g = G;
    g.n_blocks = 5000;
    UpdatePlan p;
    CHECK(update_plan(d.data(), d.size(), g, 1, 2000, &p) == UpdateError::Ok);
    CHECK(p.records.size() == 332 && p.heights == 4);
    for (size_t k = 0; k + 1 < 300; ++k) CHECK(p.old_address[k] < p.old_address[k + 1] && p.kind[k] == B);
    for (size_t k = 300; k < 330; ++k) CHECK(p.old_address[k] == 500 + (k - 300));
    CHECK(p.old_address[330] == 999 && p.old_address[331] == 1000);
    CHECK(p.records[15].parent == 301 && p.records[15].origin_pointer == (2001 + 301) * 1024 + 24 * 5);
}

int main() {
    test_irregular();
    test_depth0_and_room();
    test_errors();
    test_wide();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
