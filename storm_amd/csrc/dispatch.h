// Which kernel runs, in which workgroup shape and on which grid, for every device entry
// point of libstormck: pure host code (no HIP; tests/cpp/dispatch_plan_test.cpp compiles it
// with a plain C++17 compiler). stormck.hip checks arguments, asks for a plan and launches it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/stormck.h"

namespace stormck {

// Stripe-loop unroll of the general quad kernel: 16 x 8-byte loads in flight per
// lane per pipelined group (design probe, profiles/r01_probe.txt: U=16 with plain
// loads is the fastest quad variant; non-temporal loads cost 35%).
constexpr int kU = 16;
constexpr int kQuadSpreadDepth = 4;  // groups of kU loads in flight, one-wave quad workgroups
// LDS-staged fast path: 8-wave (512-thread) workgroups of 128 blocks, tiles of 16
// stripes (512 B per block, 64 KiB per tile), a ring of 2 tiles (128 KiB LDS, one
// workgroup per CU), non-temporal LDS-DMA (aux = 2). Measured best of the swept
// waves x tile x ring grid (profiles/r01_probe_8wave.txt: 0.886 of 8 TB/s median vs
// 0.840 for 4 waves / 3 x 32 KiB); 16 stripes divide storm's 32 KiB blocks.
constexpr int kTileStripes = 16;
constexpr int kRing = 2;
constexpr int kGldsWaves = 8;
constexpr unsigned kGldsThreads = 64 * kGldsWaves;
constexpr unsigned kGldsBlocks = 16 * kGldsWaves;
constexpr int kAuxNT = 2;
constexpr uint64_t kMultiBpw = 5;          // blocks per workgroup of k_xxh64_wide_multi
constexpr uint64_t kMultiBpwRing = 8;      // ring staging, batches above kMultiBpw per CU (133 KiB of LDS)
constexpr uint64_t kMultiBpwWide = 16;     // ring staging in 2 KiB chunks, batches above 8 per CU (133 KiB)
constexpr uint32_t kChunkPiecesWide = 128;  // the 2 KiB chunk of kMultiBpwWide (probe build)
constexpr uint64_t kWideBatch = 128;      // batches up to this many blocks: k_xxh64_wide
constexpr uint64_t kCommitWide = 256;     // f1 levels up to this many blocks: k_commit_level_wide
constexpr uint64_t kStreamBatch = 16384;  // f1 commit levels from this many blocks: k_commit_level_glds
constexpr uint64_t kCommitOnePiece = 4096; // f1 commits with at most this many leaves: one checksum copy-back
// Uniform batches take the LDS-staged kernel from kMidBatch blocks. Below kBigBatch its
// workgroups are 2 waves (32 blocks, 16 KiB of ring) rather than 8 (128 blocks, 128 KiB):
// 16,384 blocks in 8-wave workgroups fill only 128 of the 256 CUs
// (profiles/r01_chain/mid_sweep.txt: 16,384 blocks in 84 us instead of 110; 12,288 in 67
// instead of the register quad's 76).
constexpr uint64_t kMidBatch = 10240;
constexpr uint64_t kBigW = 131072;  // uniform batches below this many blocks choose their workgroup size
constexpr uint64_t kBigBatch = 24576;
constexpr int kMidWaves = 2;
constexpr unsigned kThreads = 256;
constexpr uint32_t kMaxFanout = 1u << 16;
// Merkle levels of at most this many nodes take one workgroup per node (k_pointer_level_wide):
// a node is then about one XXH64 chain (~26 us for 30,000 B); larger levels put a quad
// on each node, 64 nodes per workgroup, to keep every CU busy.
constexpr uint64_t kWideNodes = 256;
// k_pointer_level_pc: tiles of 15 stripes (20 child slots) per node; the producer wave
// loads child checksums 6 tiles (90 chain rounds) ahead of the tile it writes
// (profiles/r02_merkle/: 38 us for 13,982 nodes against 41 at 4 tiles and 52 at 12).
constexpr uint32_t kRingTile = 15;
constexpr int kRingPrefetch = 6;

// Skewed persistent streaming kernel (k_xxh64_glds_skew): wave v starts kSkewTiles*v
// tiles late, 4 KiB apart at 16-stripe tiles (profiles/r01_probe_phase_skew.txt). Its
// first and last 7*kSkewTiles steps leave waves idle, so it runs only when every
// workgroup has at least kSkewMinSteps tile steps (idle share <= 1.6%): for 32 KiB
// blocks, batches of about 1.8M blocks and up (the bench's 4M-block passes).
constexpr int kSkewTiles = 8;
constexpr uint64_t kSkewMinSteps = 3584;

// Per-block-length and gathered batches whose longest block is at most this many bytes
// stay on the register quad kernel: k_xxh64_glds_var streams 512-byte rows in lock step,
// and short blocks leave most of a step's rows empty (storm's `-tags test` sizes 256 / 536
// / 728 B: 3.7 against 6.4 G blocks/s strided, 2.8 against 6.2 shuffled, 1M blocks).
// One length L per batch, strided, var / quad in G blocks/s: 1 KiB 4.29 / 5.73, 2 KiB
// 2.82 / 2.99, 4 KiB 1.56 / 1.59, 8 KiB 0.85 / 0.76, 16 KiB 0.41 / 0.37 (DESIGN_LOG.md §5
// "Short blocks", profiles/r04_small_blocks/, r04_small_crossover/).
constexpr uint64_t kVarMinLen = 4096;
// Gathers of at least this many blocks visit them in a locality order (k_order_*).
constexpr uint64_t kOrderMinBlocks = 1u << 20;

// Blocks per CU from which the LDS-DMA ring takes a batch below kBigBatch. The three paths
// were measured apart and keep their own floors.
// Per-block lengths / gathers, from 44 per CU (11,264 on 256 CUs): storm-mix batches in us,
// var kernel / register quad: 9,216 69.5 / 53.4, 10,240 70.0 / 62.9, 12,288 71.8 / 79.9,
// 16,384 82.1 / 124, 49,152 238 / 299 (profiles/r03_mid/varlo*, varhi*).
constexpr uint64_t kVarFloorPerCu = 44;
// Uniform batches, from 36 per CU: see plan_checksum.
constexpr uint64_t kMidFloorPerCu = 36;
// Commit levels, from 39 per CU.
constexpr uint64_t kCommitFloorPerCu = 39;
// A CU count the runtime could not tell (0) is planned as this many on the per-block-length
// and pointer-level paths; the uniform, spread and commit paths skip their CU rules instead.
constexpr uint64_t kAssumedCus = 256;

// What the plans need to know of kernels.h (stormck.hip asserts that the two agree).
constexpr uint32_t kPlanRingSlots = 4;       // kRingSlots
constexpr uint64_t kPlanPipePieces = 4096;   // kPipeMaxChunks * kChunkPieces: pipelined staging covers 64 KiB
constexpr uint64_t kPlanMultiPieces = 2034;  // kMultiPieces: whole-block staging
constexpr uint32_t kPlanOrderBuckets = 4096;  // kOrderBuckets
constexpr uint32_t kPlanNodeLds = 32768;     // kNodeLds
constexpr uint32_t plan_pointer_block_size(uint32_t fanout) { return (fanout * 25u + 7u) & ~7u; }  // pointer_block_size

// Probe knobs. The shipped library has one dispatch, fixed at compile time. The variants
// measured and rejected in DESIGN.md, and the environment switches that select them, are
// compiled only into the probe build (-DSTORMCK_PROBES: tools/libstormck_probes.so, which
// the design tools and tests/test_probe_build.py load). In this build knobs() is a
// constant, so each switch folds to its default and the rejected kernels are not
// instantiated. A field's default is the shipped value.
#ifdef STORMCK_PROBES
constexpr bool kProbes = true;
#else
constexpr bool kProbes = false;
#endif

struct Knobs {
    // Ring depth of the pipelined staging in the wide-multi kernels (kernels.h
    // multi_stage_hash_pipe): kRingSlots; STORMCK_STAGE_PIPE=0 stages whole blocks
    // first (A/B). 6- and 7-slot rings were measured slower (DESIGN_LOG.md §5).
    uint32_t ring_slots = kPlanRingSlots;
    // STORMCK_WIDE16=1: 16 blocks per workgroup (one full chain wave) through 4-slot rings of
    // 2 KiB chunks with double-buffered stagers, for batches of 9..16 blocks per CU: measured
    // no faster than the register-quad kernel (2,049 / 3,072 / 4,096 blocks of 31,808 B: 33.2 /
    // 35.3 / 38.1 against 34.7 / 35.0 / 35.1 us in a round-3 probe; two 8-block rings per CU
    // lost the same way, profiles/r03_multi16/), so off.
    bool wide16 = false;
    bool wide_multi = true;    // STORMCK_WIDE_MULTI=0 disables k_xxh64_wide_multi
    bool glds_var = true;      // STORMCK_GLDS_VAR=0 restores the quad kernel for per-block lengths / gathers (A/B)
    uint64_t var_lo = 0;       // STORMCK_VAR_LO: the smallest batch for the var kernel (0: kVarFloorPerCu per CU)
    uint64_t var_min_len = kVarMinLen;  // STORMCK_VAR_MIN_LEN: another threshold (A/B)
    // STORMCK_MID_WAVES = 1-4 forces W for every uniform batch above one wave per CU; 5 = the
    // kernels before (2-wave workgroups, on the var path too).
    int mid_waves = 0;
    bool big_w = true;         // STORMCK_BIG_W=0: batches from kBigBatch on always take 8-wave workgroups
    // STORMCK_SKEW_MIN_STEPS: the skewed kernel's threshold (A/B of the two kernels at the c3
    // arena's 2M-block launches)
    uint64_t skew_min_steps = kSkewMinSteps;
    uint64_t quad_spread = 1;  // STORMCK_QUAD_SPREAD = waves per CU the one-wave quad workgroups cover (0 disables)
    bool gather_order = true;  // STORMCK_GATHER_ORDER=0 turns the locality order off (A/B)
    // STORMCK_GATHER_RANK=1: large gathers with per-block lengths deal each group's rows by
    // length rank (k_order_rank; measured slower, DESIGN_LOG.md §10).
    bool gather_rank = false;
    // STORMCK_GATHER_DEFER=1: hash into the sorted positions (coalesced stores), then one
    // scatter pass to the caller's indices (A/B)
    bool gather_defer = false;
    bool order_idx = false;      // STORMCK_ORDER_IDX=1: place the indices only, the sort gathers the offsets (A/B)
    bool gather_contig = false;  // STORMCK_GATHER_CONTIG=1: contiguous group runs per workgroup
    uint64_t commit_wide = kCommitWide;  // STORMCK_COMMIT_WIDE: levels up to this many blocks take k_commit_level_wide
    bool commit_multi = true;  // STORMCK_COMMIT_MULTI=0 disables k_commit_level_multi
    bool commit_midw = true;   // STORMCK_COMMIT_MIDW=0: the launches before the 1- / 3-wave levels (A/B)
    // STORMCK_COMMIT_CHUNKS="first,growth": the level-0 chunk schedule (tuning probe)
    uint64_t commit_first = 2 * kStreamBatch, commit_growth = 3;
    // STORMCK_POINTER_RING: "0" = the register-quad kernel; default: the producer / chain
    // wave pair (k_pointer_level_pc). Measured alternatives (one wave producing and hashing,
    // 30- and 45-stripe tiles, prefetch 4 and 12 tiles, two pairs per workgroup, one producer
    // for two chain waves): DESIGN_LOG.md §5, profiles/r02_merkle/.
    int pointer_ring = 2;
    // STORMCK_POINTER_C = 2 / 4 chain waves per workgroup (or 0: the fewest C that keeps one
    // workgroup per CU); STORMCK_POINTER_SIMD=0 takes roles by wave index. See plan_pointer_level.
    int pointer_c = 1;
    bool pointer_simd = true;
    // STORMCK_SINGLE_GPU_MIN=<bytes> sends single calls of at least that many bytes to the
    // device (A/B measurement only; stormck_checksum).
    uint64_t single_gpu_min = UINT64_MAX;
};

#ifdef STORMCK_PROBES
inline const Knobs& knobs() {  // filled once from the environment
    static const Knobs once = [] {
        Knobs k;
        auto env = [](const char* name) { return std::getenv(name); };
        auto is = [&](const char* name, char c) { return env(name) && env(name)[0] == c; };
        auto num = [&](const char* name, uint64_t dflt) { return env(name) ? std::strtoull(env(name), nullptr, 10) : dflt; };
        auto integer = [&](const char* name, int dflt) { return env(name) ? std::atoi(env(name)) : dflt; };
        if (is("STORMCK_STAGE_PIPE", '0')) k.ring_slots = 0;
        k.wide16 = is("STORMCK_WIDE16", '1');
        k.wide_multi = !is("STORMCK_WIDE_MULTI", '0');
        k.glds_var = !is("STORMCK_GLDS_VAR", '0');
        k.var_lo = num("STORMCK_VAR_LO", 0);
        k.var_min_len = num("STORMCK_VAR_MIN_LEN", kVarMinLen);
        k.mid_waves = integer("STORMCK_MID_WAVES", 0);
        k.big_w = !is("STORMCK_BIG_W", '0');
        k.skew_min_steps = num("STORMCK_SKEW_MIN_STEPS", kSkewMinSteps);
        k.quad_spread = static_cast<uint64_t>(integer("STORMCK_QUAD_SPREAD", 1));
        k.gather_order = !is("STORMCK_GATHER_ORDER", '0');
        k.gather_rank = is("STORMCK_GATHER_RANK", '1');
        k.gather_defer = is("STORMCK_GATHER_DEFER", '1');
        k.order_idx = is("STORMCK_ORDER_IDX", '1');
        k.gather_contig = is("STORMCK_GATHER_CONTIG", '1');
        k.commit_multi = !is("STORMCK_COMMIT_MULTI", '0');
        k.commit_midw = !is("STORMCK_COMMIT_MIDW", '0');
        k.pointer_ring = integer("STORMCK_POINTER_RING", 2);
        k.pointer_c = integer("STORMCK_POINTER_C", 1);
        k.pointer_simd = !is("STORMCK_POINTER_SIMD", '0');
        k.single_gpu_min = num("STORMCK_SINGLE_GPU_MIN", UINT64_MAX);
        return k;
    }();
    return once;
}
// The commit's wide threshold and chunk schedule are read on every call
// (tools/commit_chunks.py changes the schedule within one process).
inline Knobs commit_knobs() {
    Knobs k = knobs();
    if (const char* e = std::getenv("STORMCK_COMMIT_WIDE")) k.commit_wide = std::strtoull(e, nullptr, 10);
    unsigned long long f = 0, gr = 0;
    if (const char* e = std::getenv("STORMCK_COMMIT_CHUNKS"))
        if (std::sscanf(e, "%llu,%llu", &f, &gr) == 2 && f >= 1 && gr >= 1) {
            k.commit_first = f;
            k.commit_growth = gr;
        }
    return k;
}
#else
constexpr Knobs knobs() { return Knobs{}; }
constexpr Knobs commit_knobs() { return Knobs{}; }
#endif

enum class Kernel {
    Wide,            // one workgroup per block (k_xxh64_wide, k_commit_level_wide, k_pointer_level_wide)
    WideMulti,       // k_xxh64_wide_multi / k_commit_level_multi: Plan::multi
    GldsVar,         // k_xxh64_glds_var
    GldsVarOrdered,  // the locality-ordered gather: k_order_* then k_xxh64_glds_var<ORD>
    Glds,            // k_xxh64_glds / k_commit_level_glds in Plan::waves-wave workgroups
    GldsSkew,        // k_xxh64_glds_skew, one persistent workgroup per CU
    QuadSpread,      // k_xxh64_quad in one-wave workgroups
    Quad,            // the register quad kernels (k_xxh64_quad, k_commit_level, k_pointer_level)
    PointerPc,       // k_pointer_level_pc: Plan::waves chain waves per workgroup
    TooLarge,        // more workgroups than one launch takes
};

// Workgroup shape of the wide-multi kernels: bpw blocks per workgroup (0: not this kernel),
// staged through rings of `ring` slots of `chunk` 16-byte pieces (ring 0: whole blocks first),
// dbl: double-buffered stagers.
struct MultiShape {
    uint64_t bpw = 0;
    uint32_t ring = 0, chunk = 256;
    bool dbl = false;
};

struct Plan {
    Kernel kernel = Kernel::Quad;
    uint32_t grid = 0, block = kThreads;  // workgroups, threads per workgroup
    int waves = 0;                        // Glds, GldsVar*, PointerPc
    bool persistent = false;              // GldsVar*: the skewed persistent form, one workgroup per CU
    bool simd_roles = false;              // PointerPc with 2 or 4 chain waves
    MultiShape multi;                     // WideMulti
    // GldsVarOrdered: bytes of the stream-ordered workspace, and the probe variants
    uint64_t ws_bytes = 0;
    bool defer = false, idx = false, rank = false, contig = false;
};

inline Plan make_plan(Kernel k, uint64_t grid, unsigned block, int waves = 0) {
    Plan p;
    p.kernel = grid > 0x7fffffffULL ? Kernel::TooLarge : k;
    p.grid = static_cast<uint32_t>(grid);
    p.block = block;
    p.waves = waves;
    return p;
}

// Blocks on the busiest CU when n blocks run in `waves`-wave workgroups (16 blocks a wave)
// dealt round-robin to ncu CUs: ceil(workgroups / CUs) * 16 * waves.
constexpr uint64_t busiest_cu_blocks(uint64_t n, uint64_t waves, uint64_t ncu) {
    return (((n + 16 * waves - 1) / (16 * waves)) + ncu - 1) / ncu * 16 * waves;
}
// Below kBigBatch: 3- or 1-wave workgroups, whichever loads the busiest CU least (ties: 3).
constexpr int mid_waves_for(uint64_t n, uint64_t ncu) {
    return busiest_cu_blocks(n, 1, ncu) < busiest_cu_blocks(n, 3, ncu) ? 1 : 3;
}
// From kBigBatch up to kBigW: 3-wave workgroups instead of 8-wave ones when that puts at most
// 3/4 of the blocks on the busiest CU.
constexpr bool big_takes_3_waves(uint64_t n, uint64_t ncu) {
    return 4 * busiest_cu_blocks(n, 3, ncu) <= 3 * busiest_cu_blocks(n, 8, ncu);
}

// Blocks per workgroup of the wide-multi kernels for a batch of n on ncu CUs: kMultiBpw
// up to kMultiBpw per CU; with ring staging, kMultiBpwRing up to that many per CU. One
// wave walks all of a workgroup's chains, so 8 cost about what 5 do (1,600 / 2,048 blocks:
// 24.2 / 25.4 us against 34.5 / 34.8 on the quad kernel); at or below 5 per CU the
// 5-block workgroups are about 1 us faster (profiles/r02_pipe/bpw_ab/). bpw 0: not this kernel.
inline MultiShape multi_shape(uint64_t n, uint64_t ncu, const Knobs& k) {
    MultiShape s;
    if (ncu == 0) return s;
    if (n <= kMultiBpw * ncu) s.bpw = kMultiBpw;
    else if (k.ring_slots && n <= kMultiBpwRing * ncu) s.bpw = kMultiBpwRing;
    else if (k.ring_slots && n <= kMultiBpwWide * ncu && k.wide16) s.bpw = kMultiBpwWide;  // probe knob only
    else return s;
    s.ring = k.ring_slots;
    s.dbl = s.bpw == kMultiBpwWide;
    s.chunk = s.dbl ? kChunkPiecesWide : 256;
    return s;
}

// One batch of stormck_checksum_batch_device and its kin. len: the block length, or with
// per-block lengths (on the device) the caller's upper bound, 0 = unknown. base_low4: the
// low four bits of the base address. remote: the blocks are host memory read in place over
// PCIe (the split leg). The link carries a kernel's loads as read requests of the loads'
// size, so the kernels that read 16 bytes per lane in wave-wide runs (LDS-DMA) keep it at
// its rate, while the register quad kernel's 32-byte reads run it at ~36 GB/s against ~54
// (profiles/r05_rates/): gathers past the wide-multi range then take the LDS-DMA var kernel
// at any size.
struct Query {
    uint64_t n = 0;
    uint32_t len = 0;
    bool lens = false, offs = false, verify = false, remote = false;
    unsigned base_low4 = 0;
    uint64_t stride = 0;
};

inline Plan plan_checksum(const Query& q, uint64_t ncu, const Knobs& k) {
    const uint64_t n = q.n;
    // The longest block the dispatch plans for: len for uniform lengths; with per-block
    // lengths the caller's upper bound, 0 = unknown, planned as storm's 32 KiB. Results
    // never depend on it, only the kernel choice does.
    const uint64_t plan_len = q.lens ? (q.len ? q.len : uint64_t{32768}) : q.len;
    const bool rows16 = q.base_low4 == 0 && (q.stride & 15) == 0;  // 16-byte aligned rows
    // Batch-size dispatch (profiles/r01_probe_small.txt, us per launch at 32 KiB):
    //  * n <= kWideBatch: one workgroup per block, whole block staged in one round trip
    //  * n <  kMidBatch: register quad kernel (64 blocks per workgroup spread the
    //    batch over the chip; the streaming kernel's 128-block workgroups would occupy
    //    fewer than half of the CUs)
    //  * otherwise, uniform length, 16-byte aligned blocks at a fixed stride, at least
    //    one LDS tile per block: LDS-staged streaming kernel (global_load_lds, nt), in
    //    2-wave workgroups below kBigBatch; its persistent 4 KiB-skewed form when the
    //    batch gives every CU thousands of tiles
    if (n <= kWideBatch) return make_plan(Kernel::Wide, n, kThreads);
    // up to 5 blocks per CU (8 with ring staging): k_xxh64_wide_multi, one workgroup per
    // CU staging 5 (8) premultiplied blocks (the c5 commit batch is one such launch); a
    // uniform batch takes it when its blocks can be staged (pipelined: covers up to 64 KiB)
    const uint64_t multi_pieces = k.ring_slots ? kPlanPipePieces : kPlanMultiPieces;
    const MultiShape ms = multi_shape(n, ncu, k);
    if (k.wide_multi && ms.bpw > 0 &&
        (q.offs || q.lens ||
         ((q.base_low4 & 7) == 0 && (q.stride & 7) == 0 && (uint64_t{q.base_low4} + q.len + 15) / 16 <= multi_pieces))) {
        Plan p = make_plan(Kernel::WideMulti, (n + ms.bpw - 1) / ms.bpw, kThreads);
        p.multi = ms;
        return p;
    }
    // Per-block lengths and/or gathered offsets (storm's dirty slots with mixed Sizeof(T)):
    // the LDS-DMA ring with per-wave tile counts, k_xxh64_glds_var, in the same
    // workgroup shapes as the uniform path below. base + stride batches need 16-byte
    // aligned rows (else the quad kernel); gathered blocks are checked per block in the
    // kernel, which hashes an unaligned one from global memory.
    const uint64_t var_min_n = k.var_lo ? k.var_lo : q.remote ? 0 : std::max<uint64_t>(kMidBatch, kVarFloorPerCu * ncu);
    if (k.glds_var && n >= var_min_n && n > (q.remote ? kMultiBpwRing : 16) * ncu && (q.lens || q.offs) &&
        plan_len > k.var_min_len && (q.offs || rows16)) {
        // below kBigBatch: 3- or 1-wave workgroups, whichever loads the busiest CU least;
        // up to kBigW, 3-wave workgroups where they cut the busiest CU's blocks by a
        // quarter against 8-wave ones (as the uniform path below)
        const uint64_t ncu_v = ncu ? ncu : kAssumedCus;
        const bool big3 = n >= kBigBatch && n < kBigW && k.big_w && big_takes_3_waves(n, ncu_v);
        const bool big = n >= kBigBatch && !big3;
        const int vw = k.mid_waves == 5 ? 2 : (big3 || mid_waves_for(n, ncu_v) == 3) ? 3 : 1;
        const int waves = big ? kGldsWaves : vw;
        const uint64_t wgs = (n + 16 * waves - 1) / (16 * waves);
        if (wgs > 0x7fffffffULL) return make_plan(Kernel::TooLarge, 0, 0);
        // tile steps per workgroup, from the planning length
        const uint64_t tiles = (plan_len / 32 + kTileStripes - 1) / kTileStripes;
        const bool persistent = big && ncu > 0 && wgs >= ncu && (wgs + ncu - 1) / ncu * tiles >= kSkewMinSteps;
        Plan p = make_plan(Kernel::GldsVar, persistent ? ncu : wgs, 64u * waves, waves);
        p.persistent = persistent;
        // large gathers visit their blocks in a locality order (kernels.h k_order_*): a
        // stream-ordered workspace from the library's own pool (the count matrix, the
        // order, the offsets and lengths in that order: 16 bytes per block), freed on the
        // stream after the launch
        if (q.offs && !q.verify && big && n >= kOrderMinBlocks && n < (uint64_t{1} << 32) && k.gather_order) {
            p.kernel = Kernel::GldsVarOrdered;
            p.defer = k.gather_defer;
            p.idx = k.order_idx;
            // rejected (round 4): each group's rows re-dealt by length rank, rotated per
            // workgroup step (kernels.h k_order_rank): 0.794 against 0.848 of 8 TB/s
            p.rank = q.lens && persistent && k.gather_rank && n / kGldsBlocks > 0;
            p.contig = persistent && k.gather_contig;
            const uint64_t words = (uint64_t{kPlanOrderBuckets} * 3 + n + 1) & ~uint64_t{1};
            p.ws_bytes = words * 4 + n * 8 + (q.lens ? n * 4 : 0) + (p.defer ? n * 8 + 8 : 0);
        }
        return p;
    }
    // Uniform batches from 36 blocks per CU up to kBigBatch: the LDS-DMA kernel in
    // W-wave workgroups (16*W blocks each), W in {1, 3} chosen to minimise the blocks of
    // the busiest CU, ceil(workgroups / CUs) * 16W (ties: 3). us per launch of 31,808 B
    // blocks, against the 256-thread quad / 2-wave LDS-DMA kernels before (rocprof-free
    // HIP events, profiles/r03_mid/w*): 10,000 54.2 (60.9), 10,240 54.6 (60.1), 12,288
    // 60.3 (65.6), 16,384 77.7 (81.8), 20,000 101.7 (112.2), 24,575 122.1 (126.3). Below
    // it the quad kernels win (8,192 / 8,704: 39.9 / 47.9 against 51.6 / 52.2 for 3 waves;
    // 9,216 / 9,728: 54.0 / 58.7 against 53.0 / 53.8, profiles/r03_mid/unilo*).
    // From kBigBatch up to kBigW blocks: 3-wave workgroups instead of the big path's
    // 8-wave ones when that puts at most 3/4 of the blocks on the busiest CU (a batch a
    // little above a multiple of 128 blocks per CU would leave most CUs with one 8-wave
    // workgroup and some with two). 36,864 / 40,000 blocks: 179.8 / ~222 us against
    // 237.3 / 240.7; 1-wave workgroups lost there (24,641: 132 against 119.6 us; 57,344:
    // 291 against 264), profiles/r03_mid/bigw*.
    int mid_waves = 0;
    if (ncu > 0 && n < kBigBatch) {
        if (k.mid_waves >= 1 && k.mid_waves <= 4) {
            if (n > 16 * ncu) mid_waves = k.mid_waves;
        } else if (k.mid_waves == 0 && n >= kMidFloorPerCu * ncu) {
            mid_waves = mid_waves_for(n, ncu);
        }
    } else if (ncu > 0 && n < kBigW && k.mid_waves == 0 && k.big_w) {
        if (big_takes_3_waves(n, ncu)) mid_waves = 3;
    }
    const bool streamable = !q.lens && !q.offs && rows16 && q.len >= 32u * kTileStripes;
    if (mid_waves > 0 && streamable)
        return make_plan(Kernel::Glds, (n + 16 * mid_waves - 1) / (16 * mid_waves), 64u * mid_waves, mid_waves);
    if (n >= kMidBatch && streamable) {
        if (n < kBigBatch)
            return make_plan(Kernel::Glds, (n + 16 * kMidWaves - 1) / (16 * kMidWaves), 64u * kMidWaves, kMidWaves);
        const uint64_t wgs = (n + kGldsBlocks - 1) / kGldsBlocks;
        if (wgs > 0x7fffffffULL) return make_plan(Kernel::TooLarge, 0, 0);
        // large batch: persistent workgroups, one per CU, waves' streams 4 KiB apart
        if (ncu > 0 && wgs >= ncu && (wgs + ncu - 1) / ncu * ((q.len / 32) / kTileStripes) >= k.skew_min_steps)
            return make_plan(Kernel::GldsSkew, ncu, kGldsThreads, kGldsWaves);
        return make_plan(Kernel::Glds, wgs, kGldsThreads, kGldsWaves);
    }
    // General path (per-block lengths / explicit offsets / any alignment): register quad
    // kernel. A batch of at most one wave per CU (16 blocks a wave) runs in one-wave
    // workgroups, so every wave has a CU of its own, with four groups of loads in flight:
    // the quad kernel's 16 scattered 32-byte pieces per load instruction make a CU's
    // address path the limit, 2 waves on a CU cost as much as 4 (profiles/r03_quad/:
    // 2,049 / 3,072 / 4,096 blocks of 31,808 B in 25.2 / 27.9 / 31.8 us against 34.6 /
    // 35.0 / 35.1 in 256-thread workgroups). Past one wave per CU it loses (6,144 /
    // 8,192 blocks: 38.5 / 48.8 us against 35.8 / 39.7 in 256-thread workgroups,
    // profiles/r03_mid/spread_*.txt), and so does a one-wave LDS-DMA ring of 4-9 tile
    // slots (38-60 us over 2,064-8,192 blocks, profiles/r03_mid/probe_*).
    if (ncu > 0 && n <= 16 * k.quad_spread * ncu) return make_plan(Kernel::QuadSpread, (n + 15) / 16, 64);
    const uint64_t wgs = (n * 4 + kThreads - 1) / kThreads;
    return make_plan(wgs == 0 ? Kernel::TooLarge : Kernel::Quad, wgs, kThreads);
}

// One level of a commit: cnt blocks in commit order. glds_levels: the forest's rows are
// 16-byte aligned and its longest block is past kVarMinLen.
inline Plan plan_commit_level(uint64_t cnt, uint64_t ncu, bool glds_levels, const Knobs& k) {
    // mid-size levels: the LDS-DMA ring in 3- or 1-wave workgroups, whichever puts
    // fewer blocks on the busiest CU; from kBigBatch, 3-wave ones where they cut the
    // busiest CU's blocks by a quarter (as plan_checksum's uniform path)
    if (k.commit_midw && glds_levels && ncu > 0 && cnt >= kCommitFloorPerCu * ncu &&
        (cnt < kBigBatch || (cnt < kBigW && k.big_w && big_takes_3_waves(cnt, ncu)))) {
        const int w = cnt < kBigBatch ? mid_waves_for(cnt, ncu) : 3;
        return make_plan(Kernel::Glds, (cnt + 16 * w - 1) / (16 * w), 64u * w, w);
    }
    // LDS-DMA ring, 8 waves x 128 blocks per workgroup (as the uniform fast path)
    if (glds_levels && cnt >= kStreamBatch)
        return make_plan(Kernel::Glds, (cnt + kGldsBlocks - 1) / kGldsBlocks, kGldsThreads, kGldsWaves);
    // one workgroup per block, premultiplied staging: the chain wave is alone on its SIMD
    if (cnt <= k.commit_wide) return make_plan(Kernel::Wide, cnt, kThreads);
    // up to 5 (ring staging: 8) blocks per CU (a storm commit's leaves): wide-multi staging
    const MultiShape ms = multi_shape(cnt, ncu, k);
    if (k.commit_multi && ms.bpw > 0) {
        Plan p = make_plan(Kernel::WideMulti, (cnt + ms.bpw - 1) / ms.bpw, kThreads);
        p.multi = ms;
        return p;
    }
    const uint64_t wgs = (cnt * 4 + kThreads - 1) / kThreads;
    return make_plan(wgs == 0 ? Kernel::TooLarge : Kernel::Quad, wgs, kThreads);
}

// One Merkle level of pm parent nodes with `fanout` children each.
inline Plan plan_pointer_level(uint64_t pm, uint32_t fanout, uint64_t ncu, const Knobs& k) {
    // a few nodes: one workgroup each, words synthesised into LDS by all its threads
    if (pm <= kWideNodes && plan_pointer_block_size(fanout) <= kPlanNodeLds) return make_plan(Kernel::Wide, pm, kThreads);
    if (k.pointer_ring != 0 && fanout == STORMCK_POINTERS_PER_BLOCK) {
        // storm's fan-out: 16 nodes per workgroup, premultiplied words staged in LDS
        // C chain waves per workgroup (and C producers). C = 1: the dispatcher already
        // puts the chain waves of 2-wave workgroups on distinct SIMDs at every level size
        // (tools/hwid_probe.hip), and one workgroup per CU with C = 2 / 4 (chains on
        // distinct SIMDs by pc_role) measured slower: 35.2 / 41.0 us against 31.7 / 37.9
        // for the 6,991- / 13,982-node levels (profiles/r03_merkle_simd/).
        const uint64_t chains = (pm + 15) / 16, cus = ncu ? ncu : kAssumedCus;
        const int c = k.pointer_c == 1 || k.pointer_c == 2 || k.pointer_c == 4 ? k.pointer_c
                      : chains <= cus ? 1 : chains <= 2 * cus ? 2 : 4;
        Plan p = make_plan(Kernel::PointerPc, (chains + c - 1) / c, 128u * c, c);
        p.simd_roles = c > 1 && k.pointer_simd;  // one chain wave: its producer cannot take its SIMD
        return p;
    }
    const uint64_t wgs = (pm * 4 + kThreads - 1) / kThreads;
    return make_plan(wgs == 0 ? Kernel::TooLarge : Kernel::Quad, wgs, kThreads);
}

// Key tags: whole batches of 64 keys through a per-wave LDS-DMA prefetch ring: keys up to
// 64 bytes (storm's 48-byte keys) take the 4-slot ring with a compile-time stride (and a
// compile-time length when keys fill their stride), longer ones the runtime-stride double
// buffer; the keys that remain, or every key of a batch that does not qualify, k_key_tags.
constexpr uint32_t kKeysPerWave = 8;  // batches of 64 keys per wave
constexpr int kKeyRing = 4;
struct KeyTagsPlan {
    bool too_large = false;
    uint64_t batches = 0;      // whole 64-key batches on the ring / LDS kernel (0: none)
    int pieces = 0;            // stride / 16: up to 4 k_key_tags_ring<pieces>, above k_key_tags_lds
    bool fixed_len = false;    // len == stride: compiled into k_key_tags_ring
    uint32_t grid = 0, lds = 0;
    uint64_t tail = 0;         // keys left for k_key_tags
    uint32_t tail_grid = 0;    // in kThreads-thread workgroups
};

inline KeyTagsPlan plan_key_tags(uint64_t stride, uint32_t len, uint64_t n, bool offs, bool lens, unsigned base_low4) {
    KeyTagsPlan p;
    auto grid_for = [&](uint64_t threads, uint32_t* grid) {
        const uint64_t wgs = (threads + kThreads - 1) / kThreads;
        *grid = static_cast<uint32_t>(wgs);
        if (wgs == 0 || wgs > 0x7fffffffULL) p.too_large = true;
    };
    p.tail = n;
    grid_for(n, &p.tail_grid);
    if (p.too_large) return p;
    if (!offs && !lens && stride >= 16 && stride <= 256 && (stride & 15) == 0 && len <= stride && base_low4 == 0 && n >= 64) {
        p.batches = n / 64;
        p.pieces = static_cast<int>(stride / 16);
        p.fixed_len = len == stride;
        const uint64_t waves = (p.batches + kKeysPerWave - 1) / kKeysPerWave;
        p.grid = static_cast<uint32_t>((waves + 3) / 4);
        p.lds = static_cast<uint32_t>(4 * (p.pieces <= 4 ? kKeyRing : 2) * 64 * stride);
        p.tail = n - p.batches * 64;
        if (p.tail) grid_for(p.tail, &p.tail_grid);
    }
    return p;
}

}  // namespace stormck
