// The device dispatch's decisions (storm_amd/csrc/dispatch.h) against a table of plans
// worked out by hand from the rules and measurements in its comments, for 256 CUs (MI355X)
// and the shipped knobs. No GPU and no library: a wrong threshold shows here, where the
// parity tests only see that the answer is still right.
#include "../../storm_amd/csrc/dispatch.h"

#include <cstdio>
#include <string>

using namespace stormck;

static int failures = 0;
static const Knobs kShipped{};

static const char* name_of(Kernel k) {
    static const char* names[] = {"wide", "wide-multi", "glds-var", "glds-var-ordered", "glds", "glds-skew",
                                  "quad-spread", "quad", "pointer-pc", "too-large"};
    return names[static_cast<int>(k)];
}

// kernel, grid x block, and waves (0 where the kernel has no such choice)
static void expect(const std::string& what, const Plan& p, Kernel kernel, uint32_t grid, uint32_t block, int waves = 0) {
    if (p.kernel == kernel && (kernel == Kernel::TooLarge || (p.grid == grid && p.block == block && p.waves == waves))) return;
    ++failures;
    std::printf("FAIL %s: got %s %u x %u, %d waves; want %s %u x %u, %d waves\n", what.c_str(), name_of(p.kernel), p.grid,
                p.block, p.waves, name_of(kernel), grid, block, waves);
}
static void expect_true(const std::string& what, bool ok) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
}

static Query uniform(uint64_t n, uint32_t len = 32768, unsigned base_low4 = 0) {
    Query q;
    q.n = n;
    q.len = len;
    q.stride = 32768;
    q.base_low4 = base_low4;
    return q;
}
static Query with_lens(uint64_t n, uint32_t bound = 0) {  // per-block lengths, strided
    Query q = uniform(n, bound);
    q.lens = true;
    return q;
}
static Query gather(uint64_t n, bool remote = false) {
    Query q = uniform(n);
    q.offs = true;
    q.remote = remote;
    return q;
}
static Plan plan(const Query& q, uint64_t ncu = 256) { return plan_checksum(q, ncu, kShipped); }

static void expect_multi(const std::string& what, const Plan& p, uint64_t bpw, uint32_t grid) {
    expect(what, p, Kernel::WideMulti, grid, 256);
    expect_true(what + ": shape", p.multi.bpw == bpw && p.multi.ring == 4 && p.multi.chunk == 256 &&
                                      !p.multi.dbl);
}

static void uniform_batches() {
    expect("n=128", plan(uniform(128)), Kernel::Wide, 128, 256);
    expect_multi("n=129", plan(uniform(129)), 5, 26);      // up to 5 per CU: 1,280
    expect_multi("n=1280", plan(uniform(1280)), 5, 256);
    expect_multi("n=1281", plan(uniform(1281)), 8, 161);   // up to 8 per CU: 2,048
    expect_multi("n=2048", plan(uniform(2048)), 8, 256);
    expect("n=2049", plan(uniform(2049)), Kernel::QuadSpread, 129, 64);  // one wave (16 blocks) per CU: 4,096
    expect("n=4096", plan(uniform(4096)), Kernel::QuadSpread, 256, 64);
    expect("n=4097", plan(uniform(4097)), Kernel::Quad, 65, 256);  // ceil(4n / 256)
    expect("n=9215", plan(uniform(9215)), Kernel::Quad, 144, 256);
    // 36 per CU = 9,216: 576 one-wave workgroups put 3 x 16 blocks on the busiest CU, 192
    // three-wave ones 1 x 48: a tie, which goes to 3 waves
    expect("n=9216", plan(uniform(9216)), Kernel::Glds, 192, 192, 3);
    // 12,289: 769 one-wave workgroups -> 4 x 16 = 64; 257 three-wave ones -> 2 x 48 = 96
    expect("n=12289", plan(uniform(12289)), Kernel::Glds, 769, 64, 1);
    // 24,575: 1,536 -> 6 x 16 = 96; 512 -> 2 x 48 = 96: the tie again
    expect("n=24575", plan(uniform(24575)), Kernel::Glds, 512, 192, 3);
    // 32,768: 683 three-wave workgroups -> 3 x 48 = 144 against 256 eight-wave ones -> 128
    expect("n=32768", plan(uniform(32768)), Kernel::Glds, 256, 512, 8);
    // 36,864: 768 -> 3 x 48 = 144 against 288 -> 2 x 128 = 256: at most 3/4
    expect("n=36864", plan(uniform(36864)), Kernel::Glds, 768, 192, 3);
    expect("n=131072", plan(uniform(131072)), Kernel::Glds, 1024, 512, 8);  // kBigW: no choice
    // 2M blocks: 16,384 workgroups, 64 per CU x 64 tile steps = 4,096 >= 3,584
    expect("n=2097152", plan(uniform(2097152)), Kernel::GldsSkew, 256, 512, 8);
    expect("n=1835008", plan(uniform(1835008)), Kernel::GldsSkew, 256, 512, 8);   // 56 x 64 = 3,584
    expect("n=1802241", plan(uniform(1802241)), Kernel::GldsSkew, 256, 512, 8);   // 14,081 workgroups: 56 on the busiest CU
    expect("n=1802240", plan(uniform(1802240)), Kernel::Glds, 14080, 512, 8);     // 55 x 64 = 3,520
    // rows off 16 bytes, or shorter than one LDS tile: the register quad kernel
    expect("n=2097152 base+8", plan(uniform(2097152, 32768, 8)), Kernel::Quad, 32768, 256);
    expect("n=2097152 len=511", plan(uniform(2097152, 511)), Kernel::Quad, 32768, 256);
    expect("n=36864 base+8", plan(uniform(36864, 32768, 8)), Kernel::Quad, 576, 256);
    expect("n=36864 len=511", plan(uniform(36864, 511)), Kernel::Quad, 576, 256);
    expect("n=36864 len=512", plan(uniform(36864, 512)), Kernel::Glds, 768, 192, 3);
    // wide-multi stages 8-byte aligned blocks of up to 64 KiB
    expect_multi("n=2048 base+8", plan(uniform(2048, 32768, 8)), 8, 256);
    expect("n=2048 base+4", plan(uniform(2048, 32768, 4)), Kernel::QuadSpread, 128, 64);
    expect_multi("n=2048 len=65536", plan(uniform(2048, 65536)), 8, 256);
    expect("n=2048 len=65537", plan(uniform(2048, 65537)), Kernel::QuadSpread, 128, 64);
    expect("n=2^40", plan(uniform(uint64_t{1} << 40)), Kernel::TooLarge, 0, 0);
    expect("n=2^40 base+8", plan(uniform(uint64_t{1} << 40, 32768, 8)), Kernel::TooLarge, 0, 0);
}

static void lengths_and_gathers() {
    // 44 per CU = 11,264; there 704 one-wave workgroups -> 3 x 16 and 235 three-wave ones -> 48: the tie
    expect("lens n=11263", plan(with_lens(11263)), Kernel::Quad, 176, 256);
    expect("lens n=11264", plan(with_lens(11264)), Kernel::GldsVar, 235, 192, 3);
    expect("lens n=12289", plan(with_lens(12289)), Kernel::GldsVar, 769, 64, 1);
    expect("lens n=36864", plan(with_lens(36864)), Kernel::GldsVar, 768, 192, 3);
    expect("lens n=32768", plan(with_lens(32768)), Kernel::GldsVar, 256, 512, 8);
    expect_true("lens n=32768 not persistent", !plan(with_lens(32768)).persistent);
    const Plan big = plan(with_lens(2097152));
    expect("lens n=2097152", big, Kernel::GldsVar, 256, 512, 8);
    expect_true("lens n=2097152 persistent", big.persistent);
    expect("lens n=11264 base+8", plan([] { Query q = with_lens(11264); q.base_low4 = 8; return q; }()), Kernel::Quad, 176, 256);
    // the planning length: past kVarMinLen only
    expect("lens bound 4096", plan(with_lens(11264, 4096)), Kernel::Quad, 176, 256);
    expect("lens bound 4097", plan(with_lens(11264, 4097)), Kernel::GldsVar, 235, 192, 3);
    // small batches with lengths or offsets stage through wide-multi whatever their alignment
    expect_multi("gather n=2048", plan(gather(2048)), 8, 256);
    expect("gather n=2049", plan(gather(2049)), Kernel::QuadSpread, 129, 64);
    // host memory read in place: the LDS-DMA kernel past the wide-multi range (129 one-wave
    // workgroups -> 16 blocks on the busiest CU, 43 three-wave ones -> 48)
    expect_multi("remote gather n=2048", plan(gather(2048, true)), 8, 256);
    expect("remote gather n=2049", plan(gather(2049, true)), Kernel::GldsVar, 129, 64, 1);
    // the locality order from 2^20 blocks: 8,192 workgroups, 32 per CU x 64 steps < 3,584
    expect("gather n=2^20-1", plan(gather((1u << 20) - 1)), Kernel::GldsVar, 8192, 512, 8);
    const Plan ord = plan(gather(1u << 20));
    expect("gather n=2^20", ord, Kernel::GldsVarOrdered, 8192, 512, 8);
    // 3 x 4,096 bucket words + 2^20 order words (even), 8 bytes of offset per block
    expect_true("gather n=2^20 workspace", ord.ws_bytes == (12288u + 1048576u) * 4u + 1048576u * 8u && !ord.persistent &&
                                               !ord.defer && !ord.idx && !ord.rank && !ord.contig);
    Query gl = gather(1u << 20);
    gl.lens = true;
    gl.len = 0;
    expect("gather+lens n=2^20", plan(gl), Kernel::GldsVarOrdered, 8192, 512, 8);
    expect_true("gather+lens n=2^20 workspace", plan(gl).ws_bytes == 12632064u + 4194304u);
    Query gv = gather(1u << 20);
    gv.verify = true;
    expect("gather verify n=2^20", plan(gv), Kernel::GldsVar, 8192, 512, 8);
    expect("gather n=2^32", plan(gather(uint64_t{1} << 32)), Kernel::GldsVar, 256, 512, 8);
    // offsets with one length for all blocks: the classes of the uniform batches up to 16 per CU,
    // whatever the alignment (tests/test_dispatch_fuzz.py, tests/test_far_offsets_gpu.py)
    expect("gather n=128", plan(gather(128)), Kernel::Wide, 128, 256);
    expect_multi("gather n=1280", plan(gather(1280)), 5, 256);
    expect_multi("gather n=1281", plan(gather(1281)), 8, 161);
    expect("gather n=4096", plan(gather(4096)), Kernel::QuadSpread, 256, 64);
    expect("gather n=4097", plan(gather(4097)), Kernel::Quad, 65, 256);
    // 4,200-byte blocks are past kVarMinLen: the var kernel from 44 per CU, below it the quad
    auto short_gather = [](uint64_t n, uint32_t len, bool lens) {
        Query q = gather(n);
        q.len = len;
        q.lens = lens;
        return q;
    };
    expect("gather n=11263 len=4200", plan(short_gather(11263, 4200, false)), Kernel::Quad, 176, 256);
    expect("gather n=11264 len=4200", plan(short_gather(11264, 4200, false)), Kernel::GldsVar, 235, 192, 3);
    expect("gather n=12289 len=4200", plan(short_gather(12289, 4200, false)), Kernel::GldsVar, 769, 64, 1);
    expect("gather+lens n=11264 bound 4200", plan(short_gather(11264, 4200, true)), Kernel::GldsVar, 235, 192, 3);
    expect("gather+lens n=12289 bound 4200", plan(short_gather(12289, 4200, true)), Kernel::GldsVar, 769, 64, 1);
    expect("gather n=11264 len=4096", plan(short_gather(11264, 4096, false)), Kernel::Quad, 176, 256);
    // a scrub level of 11,300 leaves and two pointer blocks (tests/test_scrub_damage_gpu.py): offsets and
    // lengths bounded by 32 KiB; 707 one-wave workgroups -> 3 x 16 and 236 three-wave ones -> 48: the tie
    expect("scrub level n=11302", plan(short_gather(11302, 32768, true)), Kernel::GldsVar, 236, 192, 3);
    // the four ordered gathers of tests/test_gather_order_gpu.py, n = 2^20 + 37: 8,193 workgroups,
    // 33 on the busiest CU. Per-block lengths: bound 0 plans 32 KiB = 64 tile steps, 33 x 64 = 2,112 <
    // 3,584; bound 65,536 = 128 steps, 4,224: persistent. One length: 4,112 B = 9 steps; 60,000 B =
    // 118 steps, 3,894: persistent.
    const uint64_t n_ord = (uint64_t{1} << 20) + 37;
    struct { const char* what; uint32_t len; bool lens, persistent; } ordered[] = {
        {"ordered gather+lens bound 0", 0, true, false},
        {"ordered gather+lens bound 65536", 65536, true, true},
        {"ordered gather len=4112", 4112, false, false},
        {"ordered gather len=60000", 60000, false, true},
    };
    for (const auto& c : ordered) {
        const Plan p = plan(short_gather(n_ord, c.len, c.lens));
        expect(c.what, p, Kernel::GldsVarOrdered, c.persistent ? 256 : 8193, 512, 8);
        expect_true(std::string(c.what) + ": persistent flag, shipped variants",
                    p.persistent == c.persistent && !p.defer && !p.idx && !p.rank && !p.contig);
    }
    // strided rows 512 KiB apart, 4,099 bytes each
    auto far_rows = [](uint64_t n) {
        Query q = uniform(n, 4099);
        q.stride = 524288;
        return q;
    };
    expect("n=9215 stride 512K", plan(far_rows(9215)), Kernel::Quad, 144, 256);
    expect("n=9216 stride 512K", plan(far_rows(9216)), Kernel::Glds, 192, 192, 3);
    expect("lens n=11264 bound 4200", plan(with_lens(11264, 4200)), Kernel::GldsVar, 235, 192, 3);
}

static void commit_levels() {
    auto level = [](uint64_t cnt, bool glds = true, uint64_t ncu = 256) { return plan_commit_level(cnt, ncu, glds, kShipped); };
    expect("commit 256", level(256), Kernel::Wide, 256, 256);
    const Plan m = level(257);
    expect("commit 257", m, Kernel::WideMulti, 52, 256);
    expect_true("commit 257 shape", m.multi.bpw == 5 && m.multi.ring == 4 && m.multi.chunk == 256 && !m.multi.dbl);
    expect("commit 2048", level(2048), Kernel::WideMulti, 256, 256);
    expect("commit 2049", level(2049), Kernel::Quad, 33, 256);
    expect("commit 9983", level(39 * 256 - 1), Kernel::Quad, 156, 256);
    expect("commit 9984", level(39 * 256), Kernel::Glds, 208, 192, 3);  // 624 -> 3 x 16, 208 -> 48: the tie
    expect("commit 16384", level(16384), Kernel::Glds, 1024, 64, 1);    // 1,024 -> 4 x 16 = 64, 342 -> 2 x 48 = 96
    expect("commit 16384 short or unaligned", level(16384, false), Kernel::Quad, 256, 256);
    expect("commit 32768", level(32768), Kernel::Glds, 256, 512, 8);
    expect("commit 36864", level(36864), Kernel::Glds, 768, 192, 3);
    expect("commit 131072", level(131072), Kernel::Glds, 1024, 512, 8);
    // kBigBatch itself: 512 three-wave workgroups -> 2 x 48 = 96 against 192 eight-wave ones -> 128: 3/4
    expect("commit 24576", level(24576), Kernel::Glds, 512, 192, 3);
    // the second level-0 chunk of a 140,000-leaf commit: 2,234 -> 9 x 48 = 432 against 838 -> 4 x 128 = 512
    expect("commit 107232", level(107232), Kernel::Glds, 838, 512, 8);
    expect("commit 14000", level(14000), Kernel::Glds, 875, 64, 1);  // 875 -> 4 x 16 = 64, 292 -> 2 x 48 = 96
    expect("commit 140", level(140), Kernel::Wide, 140, 256);
    const Plan m8 = level(1400);
    expect("commit 1400", m8, Kernel::WideMulti, 175, 256);
    expect_true("commit 1400 shape", m8.multi.bpw == 8 && m8.multi.ring == 4 && m8.multi.chunk == 256 && !m8.multi.dbl);
    expect("commit 1500", level(1500), Kernel::WideMulti, 188, 256);
    expect("commit 375", level(375), Kernel::WideMulti, 75, 256);
    expect("commit 1125", level(1125), Kernel::WideMulti, 225, 256);
    expect("commit 6000", level(6000), Kernel::Quad, 94, 256);
    expect("commit 9000", level(9000), Kernel::Quad, 141, 256);
    // an arena off 16 bytes: no LDS-DMA levels
    expect("commit 12000 unaligned", level(12000, false), Kernel::Quad, 188, 256);
    expect("commit 1500 unaligned", level(1500, false), Kernel::WideMulti, 188, 256);
    expect("commit 9984 ncu=0", level(9984, true, 0), Kernel::Quad, 156, 256);
    expect("commit 16384 ncu=0", level(16384, true, 0), Kernel::Glds, 128, 512, 8);
}

static void pointer_levels() {
    auto level = [](uint64_t pm, uint32_t fanout, uint64_t ncu = 256) { return plan_pointer_level(pm, fanout, ncu, kShipped); };
    expect("pointer 256 x 1200", level(256, 1200), Kernel::Wide, 256, 256);
    expect("pointer 257 x 1200", level(257, 1200), Kernel::PointerPc, 17, 128, 1);  // 16 nodes per chain wave
    expect_true("pointer 257 x 1200 roles", !level(257, 1200).simd_roles);
    expect("pointer 13982 x 1200", level(13982, 1200), Kernel::PointerPc, 874, 128, 1);
    expect("pointer 256 x 10", level(256, 10), Kernel::Wide, 256, 256);
    expect("pointer 257 x 10", level(257, 10), Kernel::Quad, 5, 256);
    expect("pointer 10 x 2000", level(10, 2000), Kernel::Quad, 1, 256);  // a 50,000-byte node does not fit the LDS
    expect("pointer 257 x 1200 ncu=0", level(257, 1200, 0), Kernel::PointerPc, 17, 128, 1);
    // kNodeLds: 1,310 children are 32,752 bytes, 1,311 are 32,776 and take the quad even for one node
    expect_true("node sizes", plan_pointer_block_size(1310) == 32752 && plan_pointer_block_size(1311) == 32776 &&
                                  plan_pointer_block_size(2) == 56 && plan_pointer_block_size(1) == 32);
    expect("pointer 1 x 1310", level(1, 1310), Kernel::Wide, 1, 256);
    expect("pointer 2 x 1310", level(2, 1310), Kernel::Wide, 2, 256);
    expect("pointer 1 x 1311", level(1, 1311), Kernel::Quad, 1, 256);
    expect("pointer 2 x 1311", level(2, 1311), Kernel::Quad, 1, 256);
    expect("pointer 258 x 1311", level(258, 1311), Kernel::Quad, 5, 256);
    expect("pointer 2 x 4096", level(2, 4096), Kernel::Quad, 1, 256);
    expect("pointer 2 x 65536", level(2, 65536), Kernel::Quad, 1, 256);
    expect("pointer 513 x 2", level(513, 2), Kernel::Quad, 9, 256);
    expect("pointer 129 x 2", level(129, 2), Kernel::Wide, 129, 256);
    expect("pointer 258 x 41", level(258, 41), Kernel::Quad, 5, 256);
    expect("pointer 300 x 1", level(300, 1), Kernel::Quad, 5, 256);
    expect("pointer 7 x 1", level(7, 1), Kernel::Wide, 7, 256);
}

static void key_tags() {
    auto keys = [](uint64_t stride, uint32_t len, uint64_t n) { return plan_key_tags(stride, len, n, false, false, 0); };
    auto is = [](const KeyTagsPlan& p, uint64_t batches, int pieces, bool fixed, uint32_t grid, uint32_t lds, uint64_t tail,
                 uint32_t tail_grid) {
        return !p.too_large && p.batches == batches && p.pieces == pieces && p.fixed_len == fixed && p.grid == grid &&
               p.lds == lds && p.tail == tail && (tail == 0 || p.tail_grid == tail_grid);
    };
    // ring kernel: 4 waves x 4 slots x 64 keys of LDS; the runtime-stride kernel: 2 slots
    expect_true("keys 16/16", is(keys(16, 16, 64), 1, 1, true, 1, 16384, 0, 0));
    expect_true("keys 16/8", is(keys(16, 8, 64), 1, 1, false, 1, 16384, 0, 0));
    expect_true("keys 48/48", is(keys(48, 48, 64), 1, 3, true, 1, 49152, 0, 0));
    expect_true("keys 48/40", is(keys(48, 40, 64), 1, 3, false, 1, 49152, 0, 0));
    expect_true("keys 64/64", is(keys(64, 64, 64), 1, 4, true, 1, 65536, 0, 0));
    expect_true("keys 64/33", is(keys(64, 33, 64), 1, 4, false, 1, 65536, 0, 0));
    expect_true("keys 80/80", is(keys(80, 80, 64), 1, 5, true, 1, 40960, 0, 0));
    expect_true("keys 80/72", is(keys(80, 72, 64), 1, 5, false, 1, 40960, 0, 0));
    expect_true("keys n=63", is(keys(48, 48, 63), 0, 0, false, 0, 0, 63, 1));
    // 33 batches: 5 waves of 8, 2 workgroups of 4 waves; 5 keys remain
    expect_true("keys n=2117", is(keys(48, 48, 2117), 33, 3, true, 2, 49152, 5, 1));
    expect_true("keys 48/49", is(keys(48, 49, 1000), 0, 0, false, 0, 0, 1000, 4));
    expect_true("keys stride 40", is(keys(40, 40, 1000), 0, 0, false, 0, 0, 1000, 4));
    expect_true("keys stride 272", is(keys(272, 272, 1000), 0, 0, false, 0, 0, 1000, 4));
    expect_true("keys base+8", is(plan_key_tags(48, 48, 1000, false, false, 8), 0, 0, false, 0, 0, 1000, 4));
    expect_true("keys gathered", is(plan_key_tags(48, 48, 1000, true, false, 0), 0, 0, false, 0, 0, 1000, 4));
    expect_true("keys with lengths", is(plan_key_tags(48, 48, 1000, false, true, 0), 0, 0, false, 0, 0, 1000, 4));
    // 1,223 keys = 19 batches (3 waves, one workgroup) and 7 keys for the lane kernel
    expect_true("keys 256/256 n=1223", is(keys(256, 256, 1223), 19, 16, true, 1, 131072, 7, 1));
    expect_true("keys 240/100 n=1223", is(keys(240, 100, 1223), 19, 15, false, 1, 122880, 7, 1));
    expect_true("keys 96/0 n=1223", is(keys(96, 0, 1223), 19, 6, false, 1, 49152, 7, 1));
    expect_true("keys stride 72", is(keys(72, 72, 1223), 0, 0, false, 0, 0, 1223, 5));
    expect_true("keys 80/80 n=63", is(keys(80, 80, 63), 0, 0, false, 0, 0, 63, 1));
    expect_true("keys 2^24+4133 at 256", is(keys(256, 256, (1u << 24) + 4133), 262208, 16, true, 8194, 131072, 37, 1));
    expect_true("keys 2^40", keys(48, 48, uint64_t{1} << 40).too_large);
}

// A CU count the runtime could not tell: the per-block-length path plans as for 256 CUs
// (its floor of 44 per CU falls away), the uniform mid path, the wide-multi and the spread
// path are skipped.
static void unknown_cu_count() {
    expect("ncu=0 lens n=11264", plan(with_lens(11264), 0), Kernel::GldsVar, 235, 192, 3);
    expect("ncu=0 lens n=12289", plan(with_lens(12289), 0), Kernel::GldsVar, 769, 64, 1);
    expect("ncu=0 lens n=10240", plan(with_lens(10240), 0), Kernel::GldsVar, 214, 192, 3);  // 640 -> 3 x 16, 214 -> 48: the tie
    expect("ncu=0 lens n=10239", plan(with_lens(10239), 0), Kernel::Quad, 160, 256);
    expect("ncu=0 n=129", plan(uniform(129), 0), Kernel::Quad, 3, 256);
    expect("ncu=0 n=2049", plan(uniform(2049), 0), Kernel::Quad, 33, 256);
    expect("ncu=0 n=9216", plan(uniform(9216), 0), Kernel::Quad, 144, 256);
    expect("ncu=0 n=12289", plan(uniform(12289), 0), Kernel::Glds, 385, 128, 2);  // kMidBatch: 2-wave workgroups
    expect("ncu=0 n=36864", plan(uniform(36864), 0), Kernel::Glds, 288, 512, 8);
    expect("ncu=0 n=2097152", plan(uniform(2097152), 0), Kernel::Glds, 16384, 512, 8);
}

int main() {
    uniform_batches();
    lengths_and_gathers();
    commit_levels();
    pointer_levels();
    key_tags();
    unknown_cu_count();
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
