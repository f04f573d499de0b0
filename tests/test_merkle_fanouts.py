"""Merkle pointer levels at fan-outs other than storm's 10 and 1200.

A node is (25*F+7)&~7 bytes: 3*F words of {Checksum, Address, BirthRevision}, F type bytes,
zero padding. The (F, n) list below covers, between its cases:
  * the tail after the last whole 32-byte stripe: 0 (F=5, 65, 4096, 65536), 8 (F=4, 40, 41,
    1311), 16 (F=3, 7, 21, 1310) and 24 bytes (F=2);
  * the 16-stripe prefetch groups of hash_words_quad: none (F=2..7, nodes below 512 B), one
    (F=21, 40: 528 and 1,000 B), two (F=41), three (F=65) and many;
  * both sides of kNodeLds: F=1310 is 32,752 B (k_pointer_level_wide / hash_node_wide up to
    256 nodes), F=1311 is 32,776 B (k_pointer_level even for one node), and nodes far past
    the LDS (F=4096, 65536);
  * levels of at most 256 nodes (k_pointer_level_wide) and of more (k_pointer_level) at
    several fan-outs, three and more levels at small F;
  * a last node with one child, and last nodes whose child count is no multiple of 8 (the
    type word that holds fewer than 8 type bytes).

CPU: the C oracle's merkle_root against a level-by-level restatement from
pack_pointer_block_py + xxh64; that restatement, computed once per case, is also the GPU
tests' reference. Everything is bit-exact.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as o

CASES = [(2, 1), (2, 2), (2, 3), (2, 1025), (3, 28), (4, 4097), (5, 626), (7, 50), (21, 6301), (40, 10280),
         (41, 41 * 257 + 3), (65, 4226), (1310, 1311), (1311, 1312), (1311, 1311 * 257 + 5), (4096, 4097),
         (65536, 65537)]
LEAF_BASE, NODE_BASE, REV = (1 << 40) + 5, (1 << 41) + 9, (1 << 33) + 1
LEAF, POINTER = 2, 1
K_NODE_LDS, K_WIDE_NODES = 32768, 256  # dispatch.h kPlanNodeLds, kWideNodes


def node_size(fanout):
    return (25 * fanout + 7) & ~7


class Level:
    """One level of parents: the children it packs and, per node, bytes and checksum."""

    def __init__(self, child_cs, addr_base, child_type, fanout):
        self.child_cs, self.addr_base, self.child_type, self.fanout = child_cs, addr_base, child_type, fanout
        m = len(child_cs)
        self.pm = (m + fanout - 1) // fanout
        self.nodes = []
        for j in range(self.pm):
            ent = [(int(child_cs[k]), addr_base + k, REV, child_type)
                   for k in range(j * fanout, min(m, (j + 1) * fanout))]
            self.nodes.append(o.pack_pointer_block_py(ent, fanout))
        self.cs = np.array([o.xxh64(b) for b in self.nodes], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def restated(fanout, n):
    """(leaf checksums, levels bottom-up, root tuple) as storm builds the shard tree: node
    addresses sequential from NODE_BASE, level by level."""
    leaf = o.synth_leaf_checksums(n, 0xF00 + fanout)
    leaf.setflags(write=False)
    levels = []
    cs, addr_base, typ, next_addr = leaf, LEAF_BASE, LEAF, NODE_BASE
    while len(cs) > 1:
        lv = Level(cs, addr_base, typ, fanout)
        lv.cs.setflags(write=False)
        levels.append(lv)
        cs, addr_base, next_addr, typ = lv.cs, next_addr, next_addr + lv.pm, POINTER
    return leaf, levels, (int(cs[0]), addr_base, REV, typ)


def test_case_list_covers_what_it_claims():
    sizes = {f: node_size(f) for f, _ in CASES}
    assert {s % 32 for s in sizes.values()} == {0, 8, 16, 24}
    groups = {s // 32 // 16 for s in sizes.values()}
    assert {0, 1, 2} <= groups and max(groups) > 2
    assert sizes[1310] == 32752 <= K_NODE_LDS < sizes[1311] == 32776
    assert sizes[2] == 56 and sizes[4] == 104
    last_counts = {(f, n): (n - 1) % f + 1 for f, n in CASES if n > 1}
    assert 1 in last_counts.values() and any(c % 8 for c in last_counts.values())
    for f in (2, 4, 41, 1311):  # levels on both sides of kWideNodes
        pms = [(n + f - 1) // f for ff, n in CASES if ff == f]
        assert max(pms) > K_WIDE_NODES
    assert any(len(restated(f, n)[1]) >= 3 for f, n in CASES if f <= 7)


@pytest.mark.parametrize("fanout,n", CASES)
def test_oracle_merkle_root_equals_level_by_level_restatement(fanout, n):
    leaf, levels, root = restated(fanout, n)
    assert o.merkle_root(leaf, LEAF_BASE, NODE_BASE, REV, fanout) == root
    m = n
    for lv in levels:  # the shape the restatement walked
        assert lv.pm == (m + fanout - 1) // fanout and all(len(b) == node_size(fanout) for b in lv.nodes)
        m = lv.pm
    assert m == 1


# ---------------------------------------------------------------------------
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _dev_u64(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to(dev)  # a copy: the reference stays read-only


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _odd_stride(size):
    """A row stride that is 8- but not 16-byte aligned and leaves at least 8 bytes of slack."""
    return size + 8 if (size + 8) % 16 == 8 else size + 16


@pytest.mark.gpu
@pytest.mark.parametrize("fanout,n", CASES)
def test_device_levels_equal_the_restatement(dev, fanout, n):
    """Per level: k_pointer_level_wide when the level has at most 256 nodes and the node fits
    kNodeLds (F <= 1310), else the register quad k_pointer_level (no case here has storm's
    fan-out, so never k_pointer_level_pc); k_pack_pointer_blocks for the materialised blocks;
    their checksums through the batch dispatch (k_xxh64_wide up to 128 nodes, wide-multi,
    quad-spread and quad above, rows 8- but not 16-byte aligned)."""
    from storm_amd import engine
    leaf, levels, root = restated(fanout, n)
    d_leaf = _dev_u64(leaf, dev)
    assert d_leaf.numel() == n
    got_root = engine.merkle_root_tensor(d_leaf, LEAF_BASE, NODE_BASE, REV, fanout)
    assert engine.as_tuple(got_root) == root
    size = node_size(fanout)
    stride = _odd_stride(size)
    assert stride % 8 == 0 and stride % 16 == 8 and stride >= size + 8
    for depth, lv in enumerate(levels):
        m = len(lv.child_cs)
        d_child = d_leaf if depth == 0 else _dev_u64(lv.child_cs, dev)
        fused = torch.zeros(lv.pm, dtype=torch.int64, device=dev)
        assert d_child.numel() == m and fused.numel() == (m + fanout - 1) // fanout
        engine.pointer_level_device(d_child.data_ptr(), m, lv.addr_base, REV, lv.child_type, fanout, fused.data_ptr())
        blocks = torch.full((lv.pm, stride), 0xA5, dtype=torch.uint8, device=dev)
        assert blocks.data_ptr() % 16 == 0 and (lv.pm - 1) * stride + size <= blocks.numel()
        engine.pack_pointer_blocks_device(d_child.data_ptr(), m, lv.addr_base, REV, lv.child_type, fanout,
                                          blocks.data_ptr(), stride)
        via_bytes = engine.checksum_tensor(blocks, length=size)
        torch.cuda.synchronize()
        got = _u64(fused)
        bad = np.nonzero(got != lv.cs)[0]
        assert len(bad) == 0, (fanout, n, depth, lv.pm, bad[:8])
        host = blocks.cpu().numpy()
        for j in range(lv.pm):  # 25*F..size are the node's own zero padding: part of lv.nodes[j]
            assert host[j, :size].tobytes() == lv.nodes[j], (fanout, n, depth, j)
        assert bool((host[:, size:] == 0xA5).all()), "bytes past a block's size were written"
        assert np.array_equal(_u64(via_bytes), got), (fanout, n, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [7, 300])
def test_fanout_one_level(dev, m):
    """F=1: 32-byte nodes (one stripe, one type byte in the fourth word). 300 nodes take
    k_pointer_level, 7 take k_pointer_level_wide."""
    from storm_amd import engine
    cs = o.synth_leaf_checksums(m, 0xF1)
    want = np.array([o.xxh64(o.pack_pointer_block_py([(int(cs[k]), LEAF_BASE + k, REV, LEAF)], 1)) for k in range(m)],
                    dtype=np.uint64)
    d_cs = _dev_u64(cs, dev)
    out = torch.zeros(m, dtype=torch.int64, device=dev)
    assert d_cs.numel() == m and out.numel() == m
    engine.pointer_level_device(d_cs.data_ptr(), m, LEAF_BASE, REV, LEAF, 1, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_u64(out), want)


NODE_CASES = [(0, 2), (1, 2), (2, 2), (7, 10), (8, 8), (9, 16), (1200, 1200), (1310, 1310), (5, 1311), (1311, 1311),
              (4097, 65536)]


@pytest.mark.gpu
@pytest.mark.parametrize("count,fanout", NODE_CASES)
def test_pointer_node_mixed_types(dev, count, fanout):
    """k_pointer_node over explicit entries whose type bytes differ per entry (0, 1, 2, 255
    interleaved): EntryWords builds each type word byte by byte. Nodes up to kNodeLds bytes
    (F <= 1310) go through hash_node_wide, larger ones through hash_words_quad in one quad."""
    from storm_amd import engine
    rng = np.random.default_rng(count * 131 + fanout)
    ent = rng.integers(0, 1 << 63, size=(count, 3), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    types = np.array([(0, 1, 2, 255)[(k + k // 5) % 4] for k in range(count)], dtype=np.uint8)
    if count >= 4:
        assert set(types.tolist()) == {0, 1, 2, 255}
    want = o.xxh64(o.pack_pointer_block_py([(int(e[0]), int(e[1]), int(e[2]), int(t)) for e, t in zip(ent, types)],
                                           fanout))
    d_ent = _dev_u64(ent, dev) if count else None
    d_types = torch.from_numpy(types).to(dev) if count else None
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    assert count <= fanout and (count == 0 or (d_ent.numel() == 3 * count and d_types.numel() == count))
    engine.pointer_node_device(d_ent.data_ptr() if count else 0, d_types.data_ptr() if count else 0, count, fanout,
                               out.data_ptr())
    torch.cuda.synchronize()
    assert int(_u64(out)[0]) == want
