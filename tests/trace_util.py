"""TEST INFRASTRUCTURE for the trace tests (tests/test_trace.py, tests/test_trace_gpu.py).

``reference_trace`` is a pure-Python walk of one tag at a time with the C oracle's XXH64: the
rules of include/stormck.h "trace", literally and in their order. It is the reference for
every result field, every report field and the set of distinct references. The images come
from tests/scrub_util.py. ``fuzz_case`` is the seeded damage fuzz of tests/test_trace_fuzz.py and
tests/test_trace_fuzz_gpu.py.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import oracle as o
from storm_amd import trace
from storm_amd.scrub import BLOB, POINTER, ScrubLayout
from storm_amd.trace import ABSENT, BAD, DEPTH, FOUND, MAX_DEPTH, MISMATCH, RANGE, TYPE
from tests import scrub_util as su

RESULT_FIELDS = ("address", "reminder", "parent", "slot", "depth", "status")
U64 = 2 ** 64 - 1


def reference_trace(img, lay: ScrubLayout, root, root_type, leaf_kind, tags, leaf_len=0, verify_leaves=True):
    """(results, report, references, leaf checksums): results[i] = (address, reminder, parent,
    slot, depth, status) of tags[i]; references = the set of (depth, parent, slot) hashed."""
    img = memoryview(np.ascontiguousarray(img).view(np.uint8).reshape(-1))
    lens = su.kind_lens(lay, leaf_kind, leaf_len)
    bs, F = lay.block_size, lay.pointer_fanout
    hashed = {}  # reference -> (kind, computed): the block's bytes do not change during a trace

    def walk(tag):
        expected, address, typ = root[0], root[1], root_type
        parent, slot, depth, reminder = 0, 0, 0, tag
        while True:
            if typ == su.FREE_T:
                return (address if depth else 0, reminder, parent, slot, depth, ABSENT), 0
            if typ > su.LEAF_T:
                return (address, reminder, parent, slot, depth, TYPE), 0
            if address == 0 or address >= lay.n_blocks:
                return (address, reminder, parent, slot, depth, RANGE), 0
            if typ == su.POINTER_T and depth >= MAX_DEPTH:
                return (address, reminder, parent, slot, depth, DEPTH), 0
            kind = POINTER if typ == su.POINTER_T else leaf_kind
            if kind != POINTER and not verify_leaves:
                return (address, reminder, parent, slot, depth, FOUND), expected
            ref = (depth, parent, slot)
            if ref not in hashed:
                hashed[ref] = (kind, o.xxh64(img[address * bs:address * bs + lens[kind]]))
            if hashed[ref][1] != expected:
                return (address, reminder, parent, slot, depth, MISMATCH), 0
            if kind != POINTER:
                return (address, reminder, parent, slot, depth, FOUND), expected
            depth += 1
            slot, reminder, parent = reminder % F, reminder // F, address
            expected, address = struct.unpack_from("<QQ", img, parent * bs + 24 * slot)
            typ = img[parent * bs + 24 * F + slot]

    results, leaf_cs = [], []
    for t in tags:
        res, cs = walk(int(t))
        results.append(res)
        leaf_cs.append(cs)
    n = len(results)
    n_status = [0] * 7
    for r in results:
        n_status[r[5]] += 1
    n_ptr = sum(1 for k, _ in hashed.values() if k == POINTER)
    n_leaf = len(hashed) - n_ptr
    report = dict(n_status=tuple(n_status), blocks_hashed=(n_ptr, n_leaf),
                  bytes_hashed=n_ptr * lens[POINTER] + n_leaf * lens[leaf_kind],
                  first_bad=min((i for i, r in enumerate(results) if r[5] in BAD), default=n),
                  levels=1 + max(d for d, _, _ in hashed) if hashed else 0)
    return results, report, set(hashed), leaf_cs


def as_tuples(records):
    """RESULT_DTYPE records as the reference's tuples."""
    return [tuple(int(rec[f]) for f in RESULT_FIELDS) for rec in records]


def tags_u64(tags) -> np.ndarray:
    return np.array([int(t) for t in tags], dtype=np.uint64)


# ---- the inputs both test files use ------------------------------------------------------------

class Tree:
    """An image and the arguments that trace one tree of it."""

    def __init__(self, img, lay, root, root_type, leaf_kind=BLOB, leaf_len=0):
        self.img, self.lay, self.root, self.root_type = img, lay, tuple(root), root_type
        self.leaf_kind, self.leaf_len = leaf_kind, leaf_len

    def args(self):
        return self.lay, self.root[:2] + (2,), self.root_type, self.leaf_kind

    memo = None  # a dict: the references of this tree are kept, per tag list (by identity) and verify_leaves

    def reference(self, tags, verify_leaves=True):
        if self.memo is not None and (id(tags), verify_leaves) in self.memo:
            return self.memo[id(tags), verify_leaves][1]
        ref = reference_trace(self.img, self.lay, self.root, self.root_type, self.leaf_kind, tags, self.leaf_len,
                              verify_leaves)
        if self.memo is not None:
            self.memo[id(tags), verify_leaves] = (tags, ref)  # holds the list: its id stays its own
        return ref


@functools.lru_cache(maxsize=None)
def shape(name) -> Tree:
    img, lay, root, root_type, leaf_len = su.tree_shape(name)
    return Tree(img, lay, root, root_type, BLOB, leaf_len)


F10_TAGS = list(range(1000)) * 3 + [2 ** 64 - 1, 1000, 12345]
F65_TAGS = [0, 64, 65 ** 2 - 1, 65 ** 3 - 1, 1, 65, 2 ** 64 - 1]


def shape_tags(name):
    """The tag list of an intact-tree case: the issue's lists for f10 and f65, every present
    tag plus absent ones for f64 and f1200."""
    if name == "f10":
        return F10_TAGS
    if name == "f65":
        return F65_TAGS
    present = list(su.TREE_SHAPES[name][1])
    if name == "f64":
        return present + [1, 3, 8191, 8192, 64 ** 3, 2 ** 64 - 1, 2 ** 63]
    return present + [1300, 1199 * 1200 + 1, 1200 ** 2, 2 ** 64 - 1, 2 ** 32]


@functools.lru_cache(maxsize=None)
def mixed_depth_tree() -> Tree:
    """Fan-out 10; leaves at depths 1 and 2 beside pointer blocks, and free slots."""
    b = su.Builder(ScrubLayout(1024, 0, 10, 10, 536, 728))
    deep = b.pointer({0: b.leaf(BLOB), 7: b.leaf(BLOB)})
    mid = b.pointer({1: b.leaf(BLOB), 2: deep, 9: b.leaf(BLOB)})
    root = b.pointer({0: b.leaf(BLOB), 3: mid, 4: b.pointer({4: b.leaf(BLOB)}), 9: b.leaf(BLOB)})
    img, lay = b.finish(None, slack=su.SLACK)
    return Tree(su.frozen(img), lay, root[:2], root[2])


MIXED_TAGS = [0, 10, 9, 19, 3, 13, 23, 123, 223, 723, 1723, 93, 44, 144, 5, 2 ** 64 - 1, 4, 14]


@functools.lru_cache(maxsize=None)
def leaf_root_tree() -> Tree:
    b = su.Builder(ScrubLayout(1024, 0, 10, 10, 536, 728))
    leaf = b.leaf(BLOB)
    img, lay = b.finish(None, slack=su.SLACK)
    return Tree(su.frozen(img), lay, leaf[:2], leaf[2])


def free_root_tree() -> Tree:
    t = leaf_root_tree()
    return Tree(t.img, t.lay, (0x1234, 1), su.FREE_T)


CHAIN_LAYOUT = ScrubLayout(1024, 0, 10, 10, 536, 728)


@functools.lru_cache(maxsize=None)
def chain(k) -> Tree:
    """`k` pointer blocks, each holding only slot 0, over one leaf."""
    b = su.Builder(CHAIN_LAYOUT)
    node = b.leaf(BLOB)
    for _ in range(k):
        node = b.pointer({0: node})
    img, lay = b.finish(None, slack=su.SLACK)
    return Tree(su.frozen(img), lay, node[:2], node[2])


# ---- damage: (image copy, Tree, index of the intact tree) -> what the edit fixes ----------------

def intact_index(name):
    return su.intact_index(name)


def damaged(name, edit, keep_bad=()):
    """A copy of tree `name` after edit(img, lay, index), resealed so that only the blocks in
    keep_bad (chosen by the edit's return value) mismatch. Returns (Tree, what the edit returned)."""
    t, index = shape(name), su.intact_index(name)
    img = t.img.copy()
    out = edit(img, t.lay, index)
    cs = su.reseal(img, t.lay, index, out.get("keep_bad", ()), lens=su.kind_lens(t.lay, BLOB, t.leaf_len))
    return Tree(img, t.lay, (cs, t.root[1]), t.root_type, BLOB, t.leaf_len), out


def flip_mid_level(img, lay, index):
    victim = min(a for a, (_, _, k, lvl) in index.items() if k == POINTER and lvl == 1)  # 100 leaves under it
    img[victim * lay.block_size + 17] ^= 0x40  # entry 0's birth revision: reseal rewrites the checksums only
    return dict(keep_bad={victim}, victim=victim)


def flip_one_leaf(img, lay, index):
    victim = sorted(a for a, (_, _, k, _) in index.items() if k == BLOB)[123]
    img[victim * lay.block_size + 700] ^= 0x01
    return dict(keep_bad={victim}, victim=victim)


def entry_address(address):
    def edit(img, lay, index):
        parent, slot, off, _ = su.pointer_entry(img, lay, index, level=3)
        old = su._u64(img, off + 8)
        su._put_u64(img, off + 8, lay.n_blocks if address is None else address)
        return dict(parent=parent, slot=slot, old=old, address=lay.n_blocks if address is None else address)
    return edit


def entry_type_3(img, lay, index):
    parent, slot, off, toff = su.pointer_entry(img, lay, index, level=3)
    img[toff] = 3
    return dict(parent=parent, slot=slot, old=su._u64(img, off + 8))


# ---- seeded damage fuzz (tests/test_trace_fuzz.py, tests/test_trace_fuzz_gpu.py) -----------------

FUZZ_IMAGES = ("f10", "f64", "f65")
FUZZ_SEEDS = 40
FUZZ_TAG_COUNTS = (65, 257, 1500, 4099)  # a wave and a bit, a workgroup and a bit, several workgroups
FUZZ_STREAM = 100                        # second word of the rng's seed from here on: the scrub's fuzz uses 0..4
fuzz_statuses = {}  # (image, seed) -> the reference's n_status (leaves verified), for the conditions


def fuzz_tags(name, seed, rng):
    """About 60 % present tags drawn with repetition, 20 % random odd 64-bit values and 20 %
    present + k * F**j (j in 1..5, k in 0..2): walks that share the upper path with a present
    tag and part from it deeper, to end ABSENT at a free entry or FOUND with a non-zero reminder."""
    F, present = su.TREE_SHAPES[name][0], np.array(list(su.TREE_SHAPES[name][1]), dtype=np.uint64)
    n = FUZZ_TAG_COUNTS[seed % len(FUZZ_TAG_COUNTS)]
    tags = [int(t) for t in present[rng.integers(0, len(present), n)]]
    what = rng.random(n)
    for i in range(n):
        if what[i] < 0.2:
            tags[i] = (int(rng.integers(0, 2 ** 63, dtype=np.uint64)) * 2 + 1) & U64
        elif what[i] < 0.4:
            tags[i] = (tags[i] + int(rng.integers(3)) * F ** int(rng.integers(1, 6))) & U64
    return tags


def assert_inside(tree, results):
    """What the device cases rely on, asserted on the host before any upload, from the reference's
    `results` (leaves verified) for the tags to be traced: the image has exactly n_blocks + SLACK
    blocks, and every reference a walk ends at names a block of it; a block that is hashed lies
    below n_blocks. (The references a walk passes through are below n_blocks by the RANGE rule. A
    bit flip can leave a larger address in a pointer block; that block then mismatches and no
    walk reads its entries.)"""
    lay = tree.lay
    assert tree.img.dtype == np.uint8 and tree.img.size == (lay.n_blocks + su.SLACK) * lay.block_size
    assert 0 < tree.root[1] < lay.n_blocks
    for address, _, _, _, _, status in results:
        assert address < lay.n_blocks + su.SLACK
        assert 0 < address < lay.n_blocks or status not in (FOUND, MISMATCH)


@functools.lru_cache(maxsize=2)  # the two verify_leaves settings of one case follow one another
def fuzz_case(name, seed):
    """(Tree, tags): tree `name` after su.random_damage with the scrub's edit counts, resealed
    so that only the deliberate damage is wrong, and the tags of fuzz_tags."""
    t, index = shape(name), su.intact_index(name)
    rng = np.random.default_rng([seed, FUZZ_STREAM + FUZZ_IMAGES.index(name)])
    n_edits = su.FUZZ_EDITS[seed % len(su.FUZZ_EDITS)]
    if t.lay.n_blocks < 1000:  # small images: at most an edit per four blocks
        n_edits = max(1, min(n_edits, t.lay.n_blocks // 4))
    img = t.img.copy()
    keep_bad = su.random_damage(img, t.lay, index, rng, n_edits, whole_store=False)
    cs = su.reseal(img, t.lay, index, keep_bad, lens=su.kind_lens(t.lay, BLOB, t.leaf_len))
    tree = Tree(su.frozen(img), t.lay, (cs, t.root[1]), t.root_type, BLOB, t.leaf_len)
    tree.memo = {}
    tags = fuzz_tags(name, seed, rng)
    results, report, _, _ = tree.reference(tags)
    assert_inside(tree, results)
    fuzz_statuses[name, seed] = report["n_status"]
    return tree, tags


def fuzz_n_status(name, seed):
    """The reference's n_status of a fuzz case with the leaves verified, once per process."""
    if (name, seed) not in fuzz_statuses:
        fuzz_case(name, seed)
    return fuzz_statuses[name, seed]


def tags_under(index, address):
    """The f10 tags whose leaf lies under block `address` (build_tree: leaf of tag t at t + 1)."""
    out = []
    for a, (_, _, k, _) in index.items():
        if k != BLOB:
            continue
        p = a
        while p and p != address:
            p = index[p][0]
        if p == address:
            out.append(a - 1)
    return sorted(out)
