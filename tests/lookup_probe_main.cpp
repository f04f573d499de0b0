// objlist_probe (storm_amd/csrc/objlist_probe.h) alone, under ASan + UBSan
// (tests/test_lookup_sanitize.py): the malformed-chain and the probe-order cases on leaves, keys
// and tables that each live in a heap allocation of exactly their size, so that a read past
// any of them is a report. A plain C++17 program: no HIP, no library.
// With a file name as its argument it also runs that corpus of recorded probes (the random
// leaves of tests/lookup_util.py leaf_fuzz_case, answered by the Python probe; `corpus` below
// has the format) and prints "ok" and the number of records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../storm_amd/csrc/objlist_probe.h"

using stormck::kObjlistNoSlot;
using stormck::ProbeOut;

namespace {

int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

struct Leaf {  // objectlist.Block of C chunks in exactly objlist_leaf_len(C) bytes
    uint32_t C;
    std::unique_ptr<uint8_t[]> b;
    uint16_t next_free = 0;
    explicit Leaf(uint32_t c) : C(c), b(new uint8_t[stormck::objlist_leaf_len(c)]()) {}
    void u64(uint32_t base, uint32_t i, uint64_t v) { std::memcpy(&b[base * C + 8 * i], &v, 8); }
    void u16(uint32_t base, uint32_t i, uint16_t v) { std::memcpy(&b[base * C + 2 * i], &v, 2); }
    uint16_t next(uint32_t chunk) const {
        uint16_t v;
        std::memcpy(&v, &b[50 * C + 2 * chunk], 2);
        return v;
    }
    // the key into consecutive fresh chunks; returns the first
    uint16_t store(const std::vector<uint8_t>& key) {
        const uint16_t first = next_free;
        size_t done = 0;
        while (done < key.size()) {
            const size_t n = key.size() - done < 32 ? key.size() - done : 32;
            std::memcpy(&b[32 * next_free], key.data() + done, n);
            done += n;
            u16(50, next_free, static_cast<uint16_t>(done < key.size() ? next_free + 1 : C + n));
            ++next_free;
        }
        return first;
    }
    void item(uint32_t index, uint8_t state, uint64_t reminder, uint64_t id, uint16_t chunk) {
        b[52 * C + index] = state;
        u64(32, index, reminder);
        u64(40, index, id);
        u16(48, index, chunk);
    }
};

std::vector<uint8_t> key_of(size_t n, uint8_t salt) {
    std::vector<uint8_t> k(n);
    for (size_t i = 0; i < n; ++i) k[i] = static_cast<uint8_t>(salt + 7 * i + (i >> 5));
    return k;
}

// the key in an allocation of exactly its length, through both forms of the probe's reads
ProbeOut probe(const Leaf& leaf, const uint16_t* A, const std::vector<uint8_t>& key, uint64_t reminder) {
    std::unique_ptr<uint8_t[]> k(new uint8_t[key.size()]);
    std::memcpy(k.get(), key.data(), key.size());
    const uint32_t n = static_cast<uint32_t>(key.size());
    const ProbeOut plain = stormck::objlist_probe<false>(leaf.b.get(), leaf.C, A, k.get(), n, reminder);
    const ProbeOut batched = stormck::objlist_probe<true>(leaf.b.get(), leaf.C, A, k.get(), n, reminder);
    CHECK(std::memcmp(&plain, &batched, sizeof plain) == 0);  // both forms of the reads, one answer
    return batched;
}

void malformed_chains(uint32_t C, const uint16_t* A) {
    const uint64_t reminder = 3 * C + 1;  // seed 1
    auto slot = [&](uint32_t i) { return (1 + A[i]) % C; };
    const std::vector<uint8_t> key = key_of(40, 9);
    for (int what = 0; what < 5; ++what) {
        Leaf leaf(C);
        const uint16_t bad = leaf.store(key), good = leaf.store(key);
        leaf.item(slot(0), 1, reminder, 66, bad);
        leaf.item(slot(1), 1, reminder, 67, good);
        if (what == 0) leaf.u16(48, slot(0), static_cast<uint16_t>(C));       // ChunkPointers[index] = C
        if (what == 1) leaf.u16(48, slot(0), 65535);
        if (what == 2) leaf.u16(50, bad, static_cast<uint16_t>(C));           // a next pointer = C
        if (what == 3) leaf.u16(50, bad + 1, static_cast<uint16_t>(C + 33));  // a remaining length of 33
        if (what == 4) leaf.u16(50, bad + 1, 65535);                          // ... of 65535 - C
        const ProbeOut o = probe(leaf, A, key, reminder);
        CHECK(o.found && o.malformed && o.object_id == 67 && o.index == slot(1) && o.probes == 2);
    }
    {  // the last chunk of the leaf's Blob named with 33 bytes: the read would leave the Blob
        Leaf leaf(C);
        leaf.next_free = static_cast<uint16_t>(C - 1);
        const std::vector<uint8_t> one = key_of(32, 3);
        const uint16_t chunk = leaf.store(one);
        leaf.u16(50, chunk, static_cast<uint16_t>(C + 33));
        leaf.item(slot(0), 1, reminder, 5, chunk);
        std::vector<uint8_t> longer = one;
        longer.push_back(0);
        const ProbeOut o = probe(leaf, A, longer, reminder);
        CHECK(!o.found && o.malformed && o.index == slot(1) && o.probes == 2);
    }
    {  // a chain that points at itself under a 256-byte key of eight equal chunks
        Leaf leaf(C);
        const std::vector<uint8_t> piece = key_of(32, 1);
        std::vector<uint8_t> k;
        for (int i = 0; i < 8; ++i) k.insert(k.end(), piece.begin(), piece.end());
        const uint16_t chunk = leaf.store(piece);
        leaf.u16(50, chunk, chunk);
        leaf.item(slot(0), 1, reminder, 5, chunk);
        const ProbeOut o = probe(leaf, A, k, reminder);
        CHECK(!o.found && o.malformed && o.object_id == 0 && o.index == slot(1) && o.probes == 2);
        // ... and under a key that ends inside the second round: fewer than 32 bytes remain
        k.resize(40);
        const ProbeOut p = probe(leaf, A, k, reminder);
        CHECK(!p.found && p.malformed && p.probes == 2);
    }
    {  // a key shorter than a chunk against a chunk that is not the last
        Leaf leaf(C);
        const uint16_t chunk = leaf.store(key);
        leaf.item(slot(0), 1, reminder, 5, chunk);
        const ProbeOut o = probe(leaf, A, key_of(1, 9), reminder);
        CHECK(!o.found && o.malformed);
    }
}

void probe_order(uint32_t C, const uint16_t* A) {
    const std::vector<uint8_t> key = key_of(20, 4);
    for (uint32_t seed : {0u, C - 1}) {  // C - 1: seed + A[i] wraps for every A[i] > 0
        const uint64_t reminder = 5 * static_cast<uint64_t>(C) + seed;
        auto slot = [&](uint32_t i) { return (seed + A[i]) % C; };
        for (uint32_t position : {1u, 2u, C}) {
            if (position > C) continue;
            Leaf leaf(C);
            for (uint32_t i = 0; i + 1 < position; ++i) leaf.item(slot(i), 1, reminder + 1 + i, 1000 + i, 0);
            leaf.item(slot(position - 1), 1, reminder, 42, leaf.store(key));
            const ProbeOut o = probe(leaf, A, key, reminder);
            CHECK(o.found && !o.malformed && o.object_id == 42 && o.index == slot(position - 1) && o.probes == position);
        }
        if (C >= 4) {
            Leaf leaf(C);  // Invalid, state 3, Invalid, then Free: the first Invalid is the slot
            leaf.item(slot(0), 2, reminder, 1, 0);
            leaf.item(slot(1), 3, reminder, 1, 0);
            leaf.item(slot(2), 2, reminder, 1, 0);
            ProbeOut o = probe(leaf, A, key, reminder);
            CHECK(!o.found && o.index == slot(0) && o.probes == 4 && o.object_id == 0);
            for (uint32_t i = 0; i < C; ++i) leaf.b[52 * C + i] = static_cast<uint8_t>(i % 2 ? 255 : 2);
            o = probe(leaf, A, key, reminder);  // no Free and no match
            CHECK(!o.found && o.index == kObjlistNoSlot && o.probes == C);
        }
    }
}

// The corpus file tests/test_lookup_sanitize.py writes: records one after another with no
// padding, every number little-endian. A record is a 32-byte head
//   u32 C | u32 key_len | u64 reminder | u64 object_id | u32 index | u16 probes | u8 found | u8 malformed
// (the last five: what the Python probe of tests/lookup_util.py answers), then the table (C
// u16), the leaf (objlist_leaf_len(C) bytes) and the key (key_len bytes).
struct CorpusHead {
    uint32_t C, key_len;
    uint64_t reminder, object_id;
    uint32_t index;
    uint16_t probes;
    uint8_t found, malformed;
};
static_assert(sizeof(CorpusHead) == 32, "the head of a corpus record is 32 bytes");

// Every record through both forms of the probe, its table, leaf and key each in a heap
// allocation of exactly its size. Returns the number of records, -1 for a file that is not a corpus.
long corpus(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return -1;
    long n = 0;
    CorpusHead h;
    size_t got;
    while ((got = std::fread(&h, 1, sizeof h, f)) == sizeof h) {
        if (h.C == 0 || h.C > stormck::kObjlistMaxChunks || h.key_len == 0 || h.key_len > stormck::kObjlistMaxKey) break;
        const size_t leaf_len = stormck::objlist_leaf_len(h.C);
        std::unique_ptr<uint16_t[]> A(new uint16_t[h.C]);
        std::unique_ptr<uint8_t[]> leaf(new uint8_t[leaf_len]);
        std::unique_ptr<uint8_t[]> key(new uint8_t[h.key_len]);
        if (std::fread(A.get(), 2, h.C, f) != h.C || std::fread(leaf.get(), 1, leaf_len, f) != leaf_len ||
            std::fread(key.get(), 1, h.key_len, f) != h.key_len)
            break;
        const ProbeOut want{h.object_id, h.index, h.probes, h.found, h.malformed};
        const ProbeOut plain = stormck::objlist_probe<false>(leaf.get(), h.C, A.get(), key.get(), h.key_len, h.reminder);
        const ProbeOut batched = stormck::objlist_probe<true>(leaf.get(), h.C, A.get(), key.get(), h.key_len, h.reminder);
        if (std::memcmp(&plain, &want, sizeof want) != 0 || std::memcmp(&batched, &want, sizeof want) != 0) {
            std::printf("record %ld: want id %llu index %u probes %u found %u malformed %u; plain %llu %u %u %u %u; batched %llu %u %u %u %u\n",
                        n, static_cast<unsigned long long>(want.object_id), want.index, want.probes, want.found,
                        want.malformed, static_cast<unsigned long long>(plain.object_id), plain.index, plain.probes,
                        plain.found, plain.malformed, static_cast<unsigned long long>(batched.object_id), batched.index,
                        batched.probes, batched.found, batched.malformed);
            ++failures;
        }
        ++n;
    }
    const bool whole = got == 0 && std::feof(f);  // the file ends where a record ends
    std::fclose(f);
    return whole ? n : -1;
}

}  // namespace

int main(int argc, char** argv) {
    for (uint32_t C : {1u, 2u, 10u, 600u, 4096u}) {
        // a permutation in an allocation of exactly C entries: i -> (7 i + 3) mod C, rotated for C = 1, 2
        std::unique_ptr<uint16_t[]> A(new uint16_t[C]);
        for (uint32_t i = 0; i < C; ++i) A[i] = static_cast<uint16_t>(C % 7 ? (7 * i + 3) % C : (i + 3) % C);
        probe_order(C, A.get());
        if (C >= 10) malformed_chains(C, A.get());
    }
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
