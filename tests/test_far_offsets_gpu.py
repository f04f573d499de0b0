"""Blocks more than 4 GiB from the base pointer, and blocks that straddle byte offset 2^32.

Every kernel computes base + offs[i], base + i * stride or address * block_size in 64 bits.
A 32-bit intermediate anywhere would read (or, in a commit, write) the wrong block and pass
the rest of the default suite, whose arenas end a few hundred MiB from their base. One arena
of about 5 GiB is allocated once (torch.empty: nothing is touched but the windows a test
writes); each test fills its windows, copies them back, and compares every checksum with the
oracle on that copy. Batch sizes come from the thresholds of dispatch.h at this device's CU
count; the docstrings name the kernels for 256 CUs (MI355X). Before a launch every range is
checked on the host to lie inside the arena.
"""
import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from storm_amd import _lib, commit as sc, engine, scrub  # noqa: E402

G4 = 1 << 32
VAR_STRIDE = 479232                          # 468 KiB rows: 11,264 of them span 5.03 GiB
ARENA_BYTES = 11264 * VAR_STRIDE + (1 << 20)
WINDOW = 4224                                # bytes written per strided row
LOW0, LOW_BYTES = 1 << 20, 16 << 20          # gathered blocks far below 2^32 ...
HIGH0, HIGH_BYTES = G4 - (8 << 20), 16 << 20  # ... and a region with 2^32 in its middle
K_WIDE, K_MID, K_BIG = 128, 10240, 24576     # dispatch.h kWideBatch, kMidBatch, kBigBatch


@pytest.fixture(scope="module")
def arena():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda:0")
    assert a.data_ptr() % 16 == 0
    yield a
    del a
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return g


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def _mixed_lengths(rng, n, longest):
    lens = rng.integers(0, longest + 1, size=n).astype(np.uint32)
    lens[rng.permutation(n)[:min(n, 40)]] = np.resize(np.array([0, 31, 32, 33, longest], dtype=np.uint32), min(n, 40))
    return lens


# ---------------------------------------------------------------------------
# gathered batches
# ---------------------------------------------------------------------------

def _fill_regions(arena, seed):
    """Random bytes in the two gather regions; returns their host copy (low then high)."""
    g = _gen(seed)
    for lo, size in ((LOW0, LOW_BYTES), (HIGH0, HIGH_BYTES)):
        assert lo + size <= arena.numel()
        arena[lo:lo + size] = torch.randint(0, 256, (size,), dtype=torch.uint8, device=arena.device, generator=g)
    return np.concatenate([arena[LOW0:LOW0 + LOW_BYTES].cpu().numpy(), arena[HIGH0:HIGH0 + HIGH_BYTES].cpu().numpy()])


def _host_offsets(offs):
    """Arena offsets -> offsets into the host copy of the two regions."""
    offs = offs.astype(np.int64)
    return np.where(offs < HIGH0, offs - LOW0, offs - HIGH0 + LOW_BYTES).astype(np.uint64)


def _gather_offsets(rng, lens, straddle_lens):
    """Offsets alternating below / above 2^32, half of them 16-byte aligned, the others at any
    byte; then, at the front, the middle and the end of the batch, blocks that straddle 2^32:
    starts at 2^32 - {1, 8, 16, 100, len - 1}. Sets the straddlers' lengths in `lens`."""
    n = len(lens)
    longest = int(lens.max()) if n else 0
    span = (8 << 20) - longest - 16
    r = rng.integers(0, span, size=n)
    r = np.where(rng.random(n) < 0.5, r & ~15, r)
    offs = np.where(np.arange(n) % 2 == 0, LOW0 + r, G4 + 16 + r).astype(np.uint64)
    k = len(straddle_lens)
    for first in sorted({0, max(0, n // 2 - k), max(0, n - k)}):
        for t, ln in enumerate(straddle_lens):
            if first + t >= n:
                break
            lens[first + t] = ln
            offs[first + t] = G4 - (1, 8, 16, 100, ln - 1)[t]
    for i in range(n):  # what the library will read, checked before any launch
        assert LOW0 <= offs[i] and (offs[i] + lens[i] <= LOW0 + LOW_BYTES or
                                    (HIGH0 <= offs[i] and offs[i] + lens[i] <= HIGH0 + HIGH_BYTES))
    return offs


def _gather_classes():
    cu = engine._cu_count()
    var = max(K_MID, 44 * cu)
    assert 5 * cu > K_WIDE and 16 * cu + 1 < var and var + 4 * cu + 1 < K_BIG
    return [("Wide", K_WIDE), ("WideMulti 5", 5 * cu), ("WideMulti 8", 8 * cu), ("QuadSpread", 16 * cu),
            ("Quad", 16 * cu + 1), ("GldsVar", var), ("GldsVar", var + 4 * cu + 1)]


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "uniform"])
def test_gathered_blocks_on_both_sides_of_4gib(arena, with_lens):
    """Offsets only (uniform 4,200 bytes) and offsets with per-block lengths (0..4,200 with 0, 31,
    32, 33), one batch per class: k_xxh64_wide (128), k_xxh64_wide_multi at 5 (1,280) and 8 per
    workgroup (2,048), k_xxh64_quad in one-wave (4,096) and 256-thread workgroups (4,097),
    k_xxh64_glds_var<.., LENS, OFFS> in 3-wave (11,264) and 1-wave workgroups (12,289); the
    16-byte aligned blocks stream through its LDS-DMA rows, the others from global memory."""
    dev = arena.device
    host = _fill_regions(arena, 11 + with_lens)
    rng = np.random.default_rng(4296 + with_lens)
    for name, n in _gather_classes():
        lens = _mixed_lengths(rng, n, 4200) if with_lens else np.full(n, 4200, dtype=np.uint32)
        offs = _gather_offsets(rng, lens, [4200, 1000, 4200, 333, 4200] if with_lens else [4200] * 5)
        assert int((offs + lens).max()) <= arena.numel() and int(lens.max()) == 4200
        assert (offs >= G4).sum() >= n // 2 - 10 and ((offs < G4) & (offs + lens > G4)).sum() >= min(n, 5)
        d_offs, d_lens = _i64(offs, dev), _i32(lens, dev)
        out = torch.zeros(n, dtype=torch.int64, device=dev)
        engine.checksum_gather_device(arena.data_ptr(), d_offs.data_ptr(), n, out.data_ptr(), 4200,
                                      d_lens.data_ptr() if with_lens else 0)
        torch.cuda.synchronize()
        want = o.checksum_gather(host, _host_offsets(offs), 4200, lens if with_lens else None)
        bad = np.nonzero(_u64(out) != want)[0]
        assert len(bad) == 0, (name, n, bad[:8], offs[bad[:8]])


# ---------------------------------------------------------------------------
# strided batches
# ---------------------------------------------------------------------------

def _strided_classes():
    """(name, n, stride, per-block lengths?) with n * stride just inside the arena, so that
    i * stride passes 2^32 inside every batch."""
    cu = engine._cu_count()

    def stride_for(n):
        return (ARENA_BYTES - (1 << 16)) // n // 16 * 16

    var = max(K_MID, 44 * cu)
    assert 36 * cu > 16 * cu + 1 and 36 * cu < K_BIG and var * VAR_STRIDE <= ARENA_BYTES
    return [("Wide", K_WIDE, stride_for(K_WIDE), False), ("WideMulti 5", 5 * cu, stride_for(5 * cu), False),
            ("WideMulti 8", 8 * cu, stride_for(8 * cu), False), ("Quad", 36 * cu - 1, 524288, False),
            ("Glds", 36 * cu, 524288, False), ("GldsVar", var, VAR_STRIDE, True)]


def test_strided_batches_past_4gib(arena):
    """base + i * stride with the product past 2^32 inside the batch: k_xxh64_wide (128 blocks,
    40 MiB apart), k_xxh64_wide_multi at 5 and 8 per workgroup (1,280 and 2,048 blocks, 4 and
    2.5 MiB apart), the 256-thread k_xxh64_quad (9,215 blocks, 512 KiB apart: block 8,192 starts
    at 2^32 exactly), k_xxh64_glds in 3-wave workgroups (9,216) and k_xxh64_glds_var with
    per-block lengths in 3-wave workgroups (11,264 blocks, 468 KiB apart). Checksum, then
    verify with mismatches planted below 2^32, above it and at n - 1."""
    dev = arena.device
    g = _gen(77)
    rng = np.random.default_rng(77)
    for name, n, stride, with_lens in _strided_classes():
        length = 4099
        lens = _mixed_lengths(rng, n, 4200) if with_lens else None
        longest = 4200 if with_lens else length
        assert stride % 16 == 0 and longest <= WINDOW <= stride and (n - 1) * stride + WINDOW <= arena.numel()
        assert (n - 1) * stride >= G4, name
        rows = arena.as_strided((n, WINDOW), (stride, 1))
        rows.copy_(torch.randint(0, 256, (n, WINDOW), dtype=torch.uint8, device=dev, generator=g))
        host = rows.cpu().numpy()
        want = o.checksum_batch(host, n, WINDOW, length, lens=lens, threads=8)
        d_lens = _i32(lens, dev) if with_lens else None
        lp = d_lens.data_ptr() if with_lens else 0
        out = torch.zeros(n, dtype=torch.int64, device=dev)
        engine.checksum_device(arena.data_ptr(), stride, n, out.data_ptr(), longest, lp)
        torch.cuda.synchronize()
        bad = np.nonzero(_u64(out) != want)[0]
        assert len(bad) == 0, (name, n, stride, bad[:8])
        first_far = -(-G4 // stride)  # the first block that starts at or past 2^32
        planted = sorted({first_far // 2, first_far - 1, first_far, min(first_far + 1, n - 1), n - 1})
        assert planted[0] * stride < G4 <= planted[-1] * stride
        exp = want.copy()
        exp[planted] ^= np.uint64(1) << np.uint64(63)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        d_exp = _i64(exp, dev)
        assert d_exp.numel() == n
        engine.verify_device(arena.data_ptr(), stride, n, d_exp.data_ptr(), res.data_ptr(), longest, lp)
        torch.cuda.synchronize()
        assert _u64(res).tolist() == [planted[0], len(planted)], (name, n, stride)
        exp[planted[:-1]] = want[planted[:-1]]  # only the last block, far past 2^32, is wrong
        res.zero_()
        d_exp = _i64(exp, dev)
        engine.verify_device(arena.data_ptr(), stride, n, d_exp.data_ptr(), res.data_ptr(), longest, lp)
        torch.cuda.synchronize()
        assert _u64(res).tolist() == [n - 1, 1], (name, n, stride)


# ---------------------------------------------------------------------------
# key tags
# ---------------------------------------------------------------------------

def test_gathered_key_tags_on_both_sides_of_4gib(arena):
    """k_key_tags<true, true>: 20,000 keys of 1..256 bytes at offsets alternating below and
    above 2^32, some straddling it."""
    dev = arena.device
    host = _fill_regions(arena, 31)
    rng = np.random.default_rng(31)
    n = 20000
    lens = rng.integers(1, 257, size=n).astype(np.uint32)
    offs = _gather_offsets(rng, lens, [256, 255, 200, 150, 101])
    assert int((offs + lens).max()) <= arena.numel()
    d_offs, d_lens = _i64(offs, dev), _i32(lens, dev)
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    engine.key_tags_device(arena.data_ptr(), n, out.data_ptr(), d_offsets=d_offs.data_ptr(), d_lens=d_lens.data_ptr())
    torch.cuda.synchronize()
    want = o.checksum_gather(host, _host_offsets(offs), 0, lens)
    bad = np.nonzero(_u64(out) != want)[0]
    assert len(bad) == 0, (bad[:8], offs[bad[:8]])


def test_strided_key_tags_past_4gib(arena):
    """k_key_tags_lds at stride 256 over 2^24 + 4,096 whole keys and 37 more for k_key_tags:
    key 2^24 starts at byte 2^32. Synthetic keys filled on the device; the tags of the first,
    the last and the 4,096 keys around 2^24 against the oracle."""
    dev = arena.device
    n, stride = (1 << 24) + 4096 + 37, 256
    assert n * stride <= arena.numel() and n * stride > G4
    engine.fill_synthetic_device(arena.data_ptr(), stride, n, 0, o.SYNTH_SEED)
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    engine.key_tags_device(arena.data_ptr(), n, out.data_ptr(), stride=stride, length=stride)
    torch.cuda.synchronize()
    for lo, cnt in ((0, 4096), ((1 << 24) - 2048, 4096), (n - 4096, 4096)):
        keys = o.fill_synthetic(cnt, stride, first=lo)
        assert np.array_equal(arena[lo * stride:(lo + cnt) * stride].cpu().numpy(), keys), lo
        bad = np.nonzero(_u64(out[lo:lo + cnt]) != o.checksum_batch(keys, cnt, stride, stride))[0]
        assert len(bad) == 0, (lo, bad[:8] + lo)


# ---------------------------------------------------------------------------
# commit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,fanout,slot,choices", [
    (6000, 4, 32768, [72, 28808, 30000, 31808, 32768, 4097]),
    (9000, 8, 1024, [72, 256, 536, 728, 1000, 1024, 0])], ids=["long", "short"])
def test_commit_on_blocks_past_4gib(arena, n, fanout, slot, choices):
    """A forest whose blocks and origins all lie 4 GiB further into the arena than the records
    of the reference forest say (the root's origin stays in slot 0): pointer blocks hold no
    offsets, so checksums, addresses, births, the bytes of the shifted window and slot 0 must
    equal the oracle's commit of the unshifted forest in a small host arena. Long leaves,
    fan-out 4: levels of 6,000 (k_commit_level), 1,500 (k_commit_level_multi, 8 per workgroup),
    375 (5 per workgroup), 94, 24, 6, 2 and 1 blocks (k_commit_level_wide). Short leaves,
    fan-out 8: 9,000 (k_commit_level), 1,125 (multi, 5 per workgroup), 141, 18, 3, 1 (wide).
    Each kernel writes its origins at 64-bit offsets."""
    dev = arena.device
    shift = G4
    assert shift % slot == 0
    rng = np.random.default_rng(n)
    lens = rng.choice(choices, size=n)
    b, size, last = sc.pointer_forest(n, lens, fanout, slot=slot, revision=9, first_address=(1 << 33) + 7)
    b["birth_revision"][rng.random(len(b)) < 0.4] = 3
    host = np.zeros(size, dtype=np.uint8)
    host[slot:slot + n * slot] = rng.integers(0, 1 << 63, size=n * slot // 8, dtype=np.int64).view(np.uint8)
    perm = rng.permutation(len(b))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(b))
    bp = b[perm].copy()
    has = bp["parent"] >= 0
    bp["parent"][has] = inv[bp["parent"][has]]
    ref_arena, ref_b = host.copy(), bp.copy()
    want_cs, want_last = o.commit(ref_arena, ref_b, 9, last)

    far = bp.copy()
    root = far["origin_pointer"] == sc.SING_SPACE_POINTER
    assert root.sum() == 1 and not (far["origin_pointer"] == np.uint64(sc.NO_ORIGIN)).any()
    far["data_offset"] += np.uint64(shift)
    far["origin_pointer"][~root] += np.uint64(shift)
    far["origin_type"][~root] += np.uint64(shift)
    assert int(far["data_offset"].min()) >= G4 and int((far["data_offset"] + far["length"]).max()) <= arena.numel()
    assert int(far["origin_pointer"].max()) + 24 <= arena.numel() and int(far["origin_type"].max()) < arena.numel()
    assert int(far["origin_pointer"][~root].min()) >= G4 and shift + size <= arena.numel()
    arena[shift:shift + size] = torch.from_numpy(host).to(dev)
    arena[:slot] = 0
    cs, last2 = sc.commit_device(arena.data_ptr(), far, 9, last)
    assert np.array_equal(cs, want_cs) and last2 == want_last
    assert np.array_equal(far["address"], ref_b["address"]) and np.array_equal(far["birth_revision"], ref_b["birth_revision"])
    window = arena[shift:shift + size].cpu().numpy()
    assert np.array_equal(window[slot:], ref_arena[slot:]) and not window[:slot].any()
    assert np.array_equal(arena[:slot].cpu().numpy(), ref_arena[:slot])


# ---------------------------------------------------------------------------
# scrub
# ---------------------------------------------------------------------------

def test_scrub_tree_at_block_addresses_past_4gib(arena):
    """A tree built on the device at block addresses whose byte offsets are past 2^32: 1,300
    synthetic 32 KiB leaves from address 140,000 (byte 4,587,520,000), their two pointer blocks
    and the root behind them. k_scrub_expand forms address * block_size; the frontiers of 1, 2
    and 1,300 blocks are gathers through k_xxh64_wide and k_xxh64_wide_multi. Intact, then one
    flipped byte in a leaf."""
    n, F, bs, rev, first = 1300, 1200, 32768, 3, 140000
    nodes, root_addr = first + n, first + n + 2
    n_blocks = root_addr + 1
    assert first * bs > G4 and n_blocks * bs <= arena.numel()
    base = arena.data_ptr()
    dev = arena.device
    cs = torch.zeros(n, dtype=torch.int64, device=dev)
    engine.fill_synthetic_device(base + first * bs, bs, n, 0, o.SYNTH_SEED)
    engine.checksum_device(base + first * bs, bs, n, cs.data_ptr(), bs)
    engine.pack_pointer_blocks_device(cs.data_ptr(), n, first, rev, 2, F, base + nodes * bs, bs)
    ws = torch.zeros(engine.merkle_workspace_bytes(n, F) // 8, dtype=torch.int64, device=dev)
    root = torch.zeros(4, dtype=torch.int64, device=dev)
    engine.merkle_root_device(cs.data_ptr(), n, first, nodes, rev, F, ws.data_ptr(), ws.numel() * 8, root.data_ptr(),
                              root.data_ptr() + 24)
    assert ws.numel() == 3
    engine.pack_pointer_blocks_device(ws.data_ptr(), 2, nodes, rev, 1, F, base + root_addr * bs, bs)
    torch.cuda.synchronize()
    r_cs, r_addr, r_rev, r_type = engine.as_tuple(root)
    assert (r_addr, r_rev, r_type) == (root_addr, rev, 1)
    assert r_cs == o.merkle_root(_u64(cs), first, nodes, rev, F)[0]
    lay = scrub.ScrubLayout.production(n_blocks)
    assert lay.image_bytes() <= arena.numel()
    rep = scrub.scrub_tree_device(arena, lay, (r_cs, r_addr, r_rev), r_type, scrub.BLOB, reachable=True)
    assert rep.ok and rep.n_mismatch == 0 and rep.n_structural == 0 and rep.first_error == 0
    assert rep.verified == (2 + 1, 0, 0, n) and rep.levels == 3
    assert rep.bytes_hashed == 3 * 30000 + n * bs
    bitmap = rep.reachable.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")[:n_blocks]
    assert bits[first:n_blocks].all() and int(bits.sum()) - 1 == sum(rep.verified) == n + 3

    victim = first + 1234  # the second pointer block's 35th child
    arena[victim * bs + 20001] ^= 0x10
    damaged = torch.zeros(1, dtype=torch.int64, device=dev)
    engine.checksum_device(base + victim * bs, bs, 1, damaged.data_ptr(), bs)
    rep = scrub.scrub_tree_device(arena, lay, (r_cs, r_addr, r_rev), r_type, scrub.BLOB, reachable=True)
    assert rep.code == _lib.EMISMATCH and rep.n_mismatch == 1 and rep.n_structural == 0
    assert rep.verified == (3, 0, 0, n - 1)
    assert (rep.first_error, rep.first_address, rep.first_level) == (scrub.MISMATCH, victim, 2)
    assert (rep.first_parent, rep.first_slot) == (nodes + 1234 // F, 1234 % F)
    assert rep.first_computed == int(engine.u64(damaged)[0])
    assert rep.first_expected == int(engine.u64(cs)[1234])
