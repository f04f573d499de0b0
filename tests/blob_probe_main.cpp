// blob_probe (storm_amd/csrc/blob_probe.h) alone, under ASan + UBSan
// (tests/test_objects_sanitize.py): the designed probe cases on leaves that each live in a heap
// allocation of exactly their size, N * stride + 8 bytes wherever the case allows, so that a
// read past the last slot's State byte is a report; then space_probe
// (storm_amd/csrc/space_probe.h) likewise. A plain C++17 program: no HIP, no library.
// With a file name as its argument it also runs that corpus of recorded probes (the random
// leaves of tests/objects_util.py leaf_fuzz_case, answered by the Python probe; `corpus` below
// has the format) and prints "ok" and the number of records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../storm_amd/csrc/blob_probe.h"
#include "../storm_amd/csrc/space_probe.h"

using stormck::BlobProbeOut;
using stormck::kBlobNoSlot;

namespace {

int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

struct Leaf {  // blob.Block with N slots of S-byte objects in exactly N * stride + 8 bytes
    uint32_t N, S;
    uint64_t stride;
    std::unique_ptr<uint8_t[]> b;
    Leaf(uint32_t n, uint32_t s) : N(n), S(s), stride(stormck::blob_stride(s)), b(new uint8_t[n * stormck::blob_stride(s) + 8]()) {}
    void slot(uint32_t k, uint8_t state, uint64_t reminder) {
        std::memcpy(&b[k * stride], &reminder, 8);
        std::memset(&b[k * stride + 8], static_cast<int>(0x40 + k % 64), S);  // the object: every byte of it is read back below
        b[k * stride + 8 + S] = state;
    }
    // the object of slot k through blob_object: S bytes, all of them inside the allocation
    bool object_is(uint32_t k) const {
        const uint8_t* p = stormck::blob_object(b.get(), S, k);
        for (uint32_t i = 0; i < S; ++i)
            if (p[i] != 0x40 + k % 64) return false;
        return true;
    }
};

bool same(const BlobProbeOut& o, uint32_t index, uint32_t probes, bool found) {
    return o.index == index && o.probes == probes && (o.found != 0) == found;
}

void designed(uint32_t N, uint32_t S) {
    CHECK(stormck::blob_fits(N, S, N * stormck::blob_stride(S) + 8));
    CHECK(!stormck::blob_fits(N, S, N * stormck::blob_stride(S) + 7));
    CHECK(!stormck::blob_fits(N + 1, S, N * stormck::blob_stride(S) + 8));
    for (uint32_t start : {0u, N / 2, N - 1}) {  // N - 1: the probe wraps at its second slot
        const uint64_t reminder = 7 * static_cast<uint64_t>(N) + start;
        auto at = [&](uint32_t j) { return (start + j) % N; };
        for (uint32_t position : {1u, 2u, N}) {  // the ID's slot behind Defined slots of other reminders
            if (position > N) continue;
            Leaf leaf(N, S);
            for (uint32_t j = 0; j + 1 < position; ++j) leaf.slot(at(j), 1, reminder + N * (1 + j));
            leaf.slot(at(position - 1), 1, reminder);
            const BlobProbeOut o = stormck::blob_probe(leaf.b.get(), N, S, reminder);
            CHECK(same(o, at(position - 1), position, true));
            CHECK(leaf.object_is(o.index));
        }
        {  // Free first
            Leaf leaf(N, S);
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), at(0), 1, false));
        }
        {  // a Free slot that holds the reminder: no match, the slot is handed out
            Leaf leaf(N, S);
            leaf.slot(at(0), 0, reminder);
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), at(0), 1, false));
        }
        if (N >= 5) {
            Leaf leaf(N, S);  // state 3, Invalid, state 255, Invalid, then Free: the first Invalid is the slot
            leaf.slot(at(0), 3, reminder);
            leaf.slot(at(1), 2, reminder);
            leaf.slot(at(2), 255, reminder);
            leaf.slot(at(3), 2, reminder);
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), at(1), 5, false));
            leaf.slot(at(4), 1, reminder);  // a Defined match behind them
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), at(4), 5, true));
            CHECK(leaf.object_is(at(4)));
            for (uint32_t k = 0; k < N; ++k) leaf.slot(k, static_cast<uint8_t>(k % 2 ? 255 : 2), reminder);
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), kBlobNoSlot, N, false));  // no Free and no match
            for (uint32_t k = 0; k < N; ++k) leaf.slot(k, 1, reminder + N * (1 + k));
            CHECK(same(stormck::blob_probe(leaf.b.get(), N, S, reminder), kBlobNoSlot, N, false));  // every slot another's
        }
    }
}

// space_probe (storm_amd/csrc/space_probe.h) on a spacelist leaf of S spaces in exactly
// (72 S + 2 + 7) & ~7 bytes and a table in exactly S entries.
struct SpaceLeaf {
    uint32_t S;
    std::unique_ptr<uint8_t[]> b;
    explicit SpaceLeaf(uint32_t s) : S(s), b(new uint8_t[(72 * s + 2 + 7) & ~7u]()) {}
    void space(uint32_t k, uint8_t state, uint64_t reminder) {
        std::memcpy(&b[72 * k], &reminder, 8);
        b[72 * k + 66] = state;
    }
};

void spaces_designed(uint32_t S) {
    std::unique_ptr<uint16_t[]> A(new uint16_t[S]);
    for (uint32_t i = 0; i < S; ++i) A[i] = static_cast<uint16_t>(S % 7 ? (7 * i + 3) % S : (i + 3) % S);  // a permutation
    for (uint32_t seed : {0u, S - 1}) {  // S - 1: seed + A[i] wraps for every A[i] > 0
        const uint64_t reminder = 5 * static_cast<uint64_t>(S) + seed;
        auto at = [&](uint32_t i) { return (seed + A[i]) % S; };
        auto probe = [&](const SpaceLeaf& leaf) {
            const stormck::SpaceProbeOut o = stormck::space_probe(leaf.b.get(), S, A.get(), reminder);
            return BlobProbeOut{o.index, o.probes, o.found};
        };
        for (uint32_t position : {1u, 2u, S}) {
            if (position > S) continue;
            SpaceLeaf leaf(S);
            for (uint32_t i = 0; i + 1 < position; ++i) leaf.space(at(i), 1, reminder + S * (1 + i));
            leaf.space(at(position - 1), 1, reminder);
            CHECK(same(probe(leaf), at(position - 1), position, true));
        }
        {
            SpaceLeaf leaf(S);  // Free first, also when it holds the reminder
            leaf.space(at(0), 0, reminder);
            CHECK(same(probe(leaf), at(0), 1, false));
        }
        if (S >= 5) {
            SpaceLeaf leaf(S);  // state 3, Invalid, state 255, Invalid, then Free: the first Invalid is the slot
            leaf.space(at(0), 3, reminder);
            leaf.space(at(1), 2, reminder);
            leaf.space(at(2), 255, reminder);
            leaf.space(at(3), 2, reminder);
            CHECK(same(probe(leaf), at(1), 5, false));
            leaf.space(at(4), 1, reminder);  // a Defined match behind them
            CHECK(same(probe(leaf), at(4), 5, true));
            for (uint32_t k = 0; k < S; ++k) leaf.space(k, static_cast<uint8_t>(k % 2 ? 255 : 2), reminder);
            CHECK(same(probe(leaf), stormck::kSpaceNoSlot, S, false));  // no Free and no match
        }
    }
}

// The corpus file tests/test_objects_sanitize.py writes: records one after another with no
// padding, every number little-endian. A record is a 32-byte head
//   u32 N | u32 S | u64 reminder | u64 leaf_len | u32 index | u16 probes | u8 found | u8 zero
// (index, probes, found: what find_object of tests/objects_util.py answers, index 2^32 - 1 for
// its nil), then the leaf (leaf_len bytes).
struct CorpusHead {
    uint32_t N, S;
    uint64_t reminder, leaf_len;
    uint32_t index;
    uint16_t probes;
    uint8_t found, zero;
};
static_assert(sizeof(CorpusHead) == 32, "the head of a corpus record is 32 bytes");

// Every record through the probe, its leaf in a heap allocation of exactly its size. Returns
// the number of records, -1 for a file that is not a corpus.
long corpus(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return -1;
    long n = 0;
    CorpusHead h;
    size_t got;
    while ((got = std::fread(&h, 1, sizeof h, f)) == sizeof h) {
        if (h.N == 0 || h.N > stormck::kBlobMaxObjects || h.S == 0 || h.leaf_len > (1u << 20) ||
            !stormck::blob_fits(h.N, h.S, h.leaf_len) || h.zero)
            break;
        std::unique_ptr<uint8_t[]> leaf(new uint8_t[h.leaf_len]);
        if (std::fread(leaf.get(), 1, h.leaf_len, f) != h.leaf_len) break;
        const BlobProbeOut o = stormck::blob_probe(leaf.get(), h.N, h.S, h.reminder);
        if (!same(o, h.index, h.probes, h.found != 0)) {
            std::printf("record %ld: want index %u probes %u found %u; got %u %u %u\n", n, h.index, h.probes, h.found,
                        o.index, o.probes, o.found);
            ++failures;
        }
        if (o.found) {  // the object's S bytes are read, as the fetch reads them
            const uint8_t* p = stormck::blob_object(leaf.get(), h.S, o.index);
            unsigned sum = 0;
            for (uint32_t i = 0; i < h.S; ++i) sum += p[i];
            if (sum == 0xffffffffu) ++failures;
        }
        ++n;
    }
    const bool whole = got == 0 && std::feof(f);  // the file ends where a record ends
    std::fclose(f);
    return whole ? n : -1;
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(stormck::blob_stride(1) == 16 && stormck::blob_stride(7) == 16 && stormck::blob_stride(8) == 24 &&
                      stormck::blob_stride(13) == 24 && stormck::blob_stride(16) == 32 && stormck::blob_stride(1024) == 1040 &&
                      stormck::blob_stride(UINT32_MAX) == (uint64_t{1} << 32) + 8,
                  "unsafe.Sizeof(blob.Object[T])");
    for (uint32_t S : {1u, 7u, 8u, 9u, 13u, 16u, 24u, 100u, 1024u, 4000u})
        for (uint32_t N : {1u, 2u, 10u, 100u}) designed(N, S);
    designed(4095, 1);
    for (uint32_t S : {1u, 2u, 10u, 400u, 32768u}) spaces_designed(S);
    long records = 0;
    if (argc > 1 && (records = corpus(argv[1])) < 0) {
        std::printf("%s is not a corpus of whole records\n", argv[1]);
        return 1;
    }
    if (failures) return 1;
    if (argc > 1)
        std::printf("ok %ld\n", records);
    else
        std::printf("ok\n");
    return 0;
}
