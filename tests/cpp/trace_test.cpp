// TraceTags (include/storm_blocks.hpp) on the host leg: a pointer block of fan-out 4 over two
// leaves, built here; tests/test_trace.py compiles and runs it. Exit code 0 and "ok" on success.
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
    const uint64_t bs = 128, n_blocks = 4, fanout = 4, leaf_len = 64;
    std::vector<uint8_t> img(bs * n_blocks, 0);
    for (uint64_t a = 1; a <= 2; ++a)
        for (uint64_t i = 0; i < leaf_len; ++i) img[a * bs + i] = static_cast<uint8_t>(a * 31 + i * 7);
    uint8_t* node = img.data() + 3 * bs;  // slots 1 and 3 hold the leaves at addresses 1 and 2
    const uint64_t plen = (25 * fanout + 7) & ~uint64_t{7};
    for (uint64_t k = 0; k < 2; ++k) {
        const uint64_t slot = 1 + 2 * k, address = 1 + k, cs = stormck_xxh64(img.data() + address * bs, leaf_len);
        std::memcpy(node + 24 * slot, &cs, 8);
        std::memcpy(node + 24 * slot + 8, &address, 8);
        node[24 * fanout + slot] = STORMCK_LEAF_BLOCK;
    }
    Pointer root{stormck_xxh64(node, plen), 3, 1};
    const stormck_scrub_layout layout{bs, n_blocks, static_cast<uint32_t>(fanout), 1, 64, static_cast<uint32_t>(leaf_len)};
    const uint64_t tags[4] = {1, 3, 2, 7};  // 7 = slot 3, reminder 1
    stormck_trace_result res[4];
    uint64_t cs[4];
    TraceResult r = TraceTags(img.data(), layout, root, PointerBlockType, STORMCK_SCRUB_BLOB, 0,
                              tags, 4, res, false, 0, cs);
    EXPECT(r.ok(4) && r.message.empty());
    EXPECT(r.report.n_status[STORMCK_TRACE_FOUND] == 3 && r.report.n_status[STORMCK_TRACE_ABSENT] == 1);
    EXPECT(r.report.blocks_hashed[0] == 1 && r.report.blocks_hashed[1] == 2 && r.report.levels == 2);
    EXPECT(r.report.bytes_hashed == plen + 2 * leaf_len);
    EXPECT(res[0].status == STORMCK_TRACE_FOUND && res[0].address == 1 && res[0].parent == 3 && res[0].slot == 1);
    EXPECT(res[2].status == STORMCK_TRACE_ABSENT && res[2].depth == 1 && res[2].slot == 2 && cs[2] == 0);
    EXPECT(res[3].status == STORMCK_TRACE_FOUND && res[3].address == 2 && res[3].reminder == 1 && res[3].depth == 1);
    EXPECT(cs[3] == stormck_xxh64(img.data() + 2 * bs, leaf_len));

    img[2 * bs + 5] ^= 1;  // leaf 2 no longer matches
    r = TraceTags(img.data(), layout, root, PointerBlockType, STORMCK_SCRUB_BLOB, 0, tags, 4, res,
                  false);
    EXPECT(!r.ok(4) && r.report.first_bad == 1 && res[1].status == STORMCK_TRACE_MISMATCH && res[3].status == STORMCK_TRACE_MISMATCH);
    EXPECT(r.message.find("checksum mismatch for block 2,") == 0);
    r = TraceTags(img.data(), layout, root, PointerBlockType, STORMCK_SCRUB_BLOB, 0, tags, 4, res,
                  false, STORMCK_TRACE_LEAVES_UNVERIFIED);
    EXPECT(r.ok(4) && r.report.blocks_hashed[1] == 0 && res[1].status == STORMCK_TRACE_FOUND);
    std::puts("ok");
    return 0;
}
