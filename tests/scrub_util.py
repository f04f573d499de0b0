"""TEST INFRASTRUCTURE for the scrub tests (tests/test_scrub.py, tests/test_scrub_gpu.py).

* ``reference_scrub``: a short pure-Python breadth-first walk with the C oracle's XXH64,
  the reference for every report field and for the reachable set;
* ``Builder``: whole stores by hand (singularity -> space tree -> spacelist leaves -> key
  and object trees), children first;
* ``flatten``: ``oracle.storm_cache.Store.dev`` as one contiguous image;
* ``rehash_path``: after a deliberate edit, new checksums up the path to the root, so
  that only the edit itself is wrong;
* the stores and tree shapes both test files use, built once per process;
* for tests/test_scrub_damage.py and tests/test_scrub_damage_gpu.py: ``reseal`` after any
  number of edits, the seeded ``random_damage``, the contested-reference constructions, the
  wide store whose blocks hold more than 64 entries, and committed forests as images.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import oracle as o
from oracle.storm_cache import SING_SIZE, Store, build_tree, initialize
from storm_amd.scrub import (BLOB, DUPLICATE, MISMATCH, OBJECTLIST, POINTER, RANGE, SPACELIST, TYPE, ScrubLayout)

FREE_T, POINTER_T, LEAF_T = 0, 1, 2
REPORT_FIELDS = ("verified", "bytes_hashed", "n_mismatch", "n_structural", "levels", "first_error", "first_level",
                 "first_slot", "first_parent", "first_address", "first_computed", "first_expected")


def kind_lens(lay: ScrubLayout, leaf_kind=None, leaf_len=0):
    lens = [(25 * lay.pointer_fanout + 7) & ~7, (72 * lay.spaces_per_block + 2 + 7) & ~7, lay.objectlist_len,
            lay.blob_len]
    if leaf_kind is not None and leaf_len:
        lens[leaf_kind] = leaf_len
    return lens


def _u64(img, off):
    return struct.unpack_from("<Q", img, off)[0]


def pointer_offset(lay: ScrubLayout, parent_kind, slot):
    """Byte offset, in a parent of `parent_kind` (None: the singularity), of the Pointer
    that reference `slot` holds."""
    if parent_kind is None:
        return 32
    return 24 * slot if parent_kind == POINTER else 72 * (slot // 2) + 16 + 24 * (slot & 1)


def _ref(lay, lens, expected, address, typ, leaf):
    """(status, kind): status None = not followed and no error."""
    if typ == FREE_T:
        return None, 0
    if typ > LEAF_T:
        return TYPE, 0
    kind = POINTER if typ == POINTER_T else leaf
    return (RANGE if address == 0 or address >= lay.n_blocks else 0), kind


def _children(lay, lens, blk, kind, leaf):
    """(slot, expected, address, status, kind, leaf) of the entries that are followed or wrong."""
    F, S = lay.pointer_fanout, lay.spaces_per_block
    if kind == POINTER:
        types = np.frombuffer(blk, np.uint8, F, 24 * F)
        for i in np.nonzero(types)[0]:
            i = int(i)
            cs, addr = struct.unpack_from("<QQ", blk, 24 * i)
            st, k = _ref(lay, lens, cs, addr, int(types[i]), leaf)
            yield i, cs, addr, st, k, leaf
    elif kind == SPACELIST:
        for s in range(S):
            sp = 72 * s
            state = blk[sp + 66]
            if state > 2:
                yield 2 * s, 0, 0, TYPE, 0, 0
                continue
            if state != 1:
                continue
            for which, lf in ((0, OBJECTLIST), (1, BLOB)):
                cs, addr = struct.unpack_from("<QQ", blk, sp + 16 + 24 * which)
                st, k = _ref(lay, lens, cs, addr, blk[sp + 64 + which], lf)
                if st is None:
                    continue
                yield 2 * s + which, cs, addr, st, k, lf


def reference_scrub(img, lay: ScrubLayout, root=None, root_type=None, leaf_kind=None, leaf_len=0):
    """The walk include/stormck.h describes, one block at a time. Whole store when `root`
    is None, else one tree from root = (checksum, address). Returns (report dict, bitmap
    words, index) with index[address] = (parent, slot, kind, level) of every block read."""
    img = memoryview(np.ascontiguousarray(img).view(np.uint8).reshape(-1))
    lens = kind_lens(lay, leaf_kind, leaf_len)
    bs = lay.block_size
    rep = {f: 0 for f in REPORT_FIELDS}
    rep["verified"] = [0, 0, 0, 0]
    errors = []  # (level, parent, slot, code, address, computed, expected)
    visited, index, frontier = {0}, {}, []
    if root is None:
        s = bytearray(img[:SING_SIZE])
        expected = _u64(s, 0)
        s[0:8] = bytes(8)
        computed = o.xxh64(bytes(s))
        rep["bytes_hashed"] = SING_SIZE
        if computed != expected:
            rep["n_mismatch"] = 1
            errors.append((0, 0, 0, MISMATCH, 0, computed, expected))
            st = None
        else:
            cs, addr, typ, leaf = _u64(s, 32), _u64(s, 40), s[56], SPACELIST
            st, kind = _ref(lay, lens, cs, addr, typ, leaf)
    else:
        cs, addr, typ, leaf = root[0], root[1], root_type, leaf_kind
        st, kind = _ref(lay, lens, cs, addr, typ, leaf)
    if st:
        rep["n_structural"] = 1
        errors.append((0, 0, 0, st, addr, 0, 0))
    elif st == 0:
        frontier.append((addr, cs, 0, 0, kind, leaf))
        visited.add(addr)
    level = 0
    while frontier:
        nxt = []
        for addr, expected, parent, slot, kind, leaf in sorted(frontier):
            index[addr] = (parent, slot, kind, level)
            blk = img[addr * bs:addr * bs + lens[kind]]
            rep["bytes_hashed"] += lens[kind]
            computed = o.xxh64(blk)
            if computed != expected:
                rep["n_mismatch"] += 1
                errors.append((level, parent, slot, MISMATCH, addr, computed, expected))
                continue
            rep["verified"][kind] += 1
            for e, cs, child, st, k, lf in _children(lay, lens, blk, kind, leaf):
                if st == 0 and child in visited:
                    st = DUPLICATE
                if st:
                    rep["n_structural"] += 1
                    errors.append((level + 1, addr, e, st, child, 0, 0))
                else:
                    visited.add(child)
                    nxt.append((child, cs, addr, e, k, lf))
        frontier = nxt
        level += 1
    rep["levels"] = level
    if errors:
        lvl, parent, slot, code, address, computed, expected = min(errors)
        rep.update(first_error=code, first_level=lvl, first_slot=slot, first_parent=parent, first_address=address,
                   first_computed=computed, first_expected=expected)
    rep["verified"] = tuple(rep["verified"])
    words = np.zeros(lay.bitmap_words(), dtype=np.uint32)
    for a in visited:
        words[a >> 5] |= np.uint32(1 << (a & 31))
    return rep, words, index


def popcount(words) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def flatten(store: Store, n_blocks: int, slack: int = 0) -> np.ndarray:
    """Store.dev as one contiguous (n_blocks + slack) x block_size image."""
    img = np.zeros((n_blocks + slack) * store.block_size, dtype=np.uint8)
    for a, b in store.dev.items():
        assert a < n_blocks
        img[a * store.block_size:(a + 1) * store.block_size] = np.frombuffer(b, np.uint8)
    return img


def rehash_path(img: np.ndarray, lay: ScrubLayout, index, address, lens=None):
    """New checksums from block `address` up to the root after an edit of it. Whole
    stores end at the singularity (rewritten in place); for a tree (index built from an
    explicit root) the new root checksum is returned."""
    lens = lens or kind_lens(lay)
    bs = lay.block_size
    while True:
        parent, slot, kind, _ = index[address]
        cs = o.xxh64(img[address * bs:address * bs + lens[kind]])
        if parent == 0:
            break
        off = parent * bs + pointer_offset(lay, index[parent][2], slot)
        img[off:off + 8] = np.frombuffer(struct.pack("<Q", cs), np.uint8)
        address = parent
    return cs


def seal_singularity(img: np.ndarray, root_cs=None):
    """Store `root_cs` (when given) as the space root's checksum and re-hash the singularity."""
    if root_cs is not None:
        img[32:40] = np.frombuffer(struct.pack("<Q", root_cs), np.uint8)
    img[0:8] = 0
    img[0:8] = np.frombuffer(struct.pack("<Q", o.xxh64(img[:SING_SIZE])), np.uint8)


def rehash_store(img, lay, index, address):
    seal_singularity(img, rehash_path(img, lay, index, address))


class Builder:
    """A whole store by hand, children first. Nodes are (checksum, address, block type)."""

    def __init__(self, lay: ScrubLayout, seed: int = 7):
        self.lay, self.lens = lay, kind_lens(lay)
        self.rng = np.random.default_rng(seed)
        self.blocks = {}
        self.next = 1

    def _put(self, data: bytes, typ: int):
        addr = self.next
        self.next += 1
        self.blocks[addr] = data
        return o.xxh64(data), addr, typ

    def leaf(self, kind: int):
        return self._put(self.rng.integers(0, 256, self.lens[kind], dtype=np.uint8).tobytes(), LEAF_T)

    def pointer(self, kids: dict):
        F = self.lay.pointer_fanout
        b = bytearray(self.lens[POINTER])
        for slot, (cs, addr, typ) in kids.items():
            struct.pack_into("<QQQ", b, 24 * slot, cs, addr, 1)
            b[24 * F + slot] = typ
        return self._put(bytes(b), POINTER_T)

    def spacelist(self, spaces: dict):
        """spaces[k] = (state, key tree node or None, object tree node or None)."""
        b = bytearray(self.lens[SPACELIST])
        for k, (state, key, obj) in spaces.items():
            struct.pack_into("<QQ", b, 72 * k, 0x1000 + k, 1)
            for which, node in ((0, key), (1, obj)):
                if node is not None:
                    struct.pack_into("<QQQ", b, 72 * k + 16 + 24 * which, node[0], node[1], 1)
                    b[72 * k + 64 + which] = node[2]
            b[72 * k + 66] = state
        struct.pack_into("<H", b, 72 * self.lay.spaces_per_block, len(spaces))
        return self._put(bytes(b), LEAF_T)

    def finish(self, root, slack: int = 0):
        """(image, layout with n_blocks = blocks built + 1): the singularity names `root`
        (None: an empty store). `slack` more blocks of zeros follow the image."""
        n = self.next
        lay = ScrubLayout(self.lay.block_size, n, self.lay.pointer_fanout, self.lay.spaces_per_block,
                          self.lay.objectlist_len, self.lay.blob_len)
        img = np.zeros((n + slack) * lay.block_size, dtype=np.uint8)
        for a, b in self.blocks.items():
            img[a * lay.block_size:a * lay.block_size + len(b)] = np.frombuffer(b, np.uint8)
        s = bytearray(SING_SIZE)
        struct.pack_into("<QQQ", s, 8, 0x4200812112C24445, 3, n)
        if root is not None:
            struct.pack_into("<QQQ", s, 32, root[0], root[1], 1)
            s[56] = root[2]
        struct.pack_into("<Q", s, 64, n - 1)
        img[:SING_SIZE] = np.frombuffer(bytes(s), np.uint8)
        seal_singularity(img)
        return img, lay


SLACK = 4  # blocks past n_blocks that the GPU damage cases may point into


def _whole_store(lay0: ScrubLayout, one_spacelist: bool):
    """Spaces that are Free, Defined and Invalid; a space with only a key tree and one with
    only an object tree; a leaf and a pointer block side by side at depth 1; trees whose
    root is directly a leaf."""
    b = Builder(lay0)
    F = lay0.pointer_fanout
    key_deep = b.pointer({0: b.leaf(OBJECTLIST), 3: b.pointer({1: b.leaf(OBJECTLIST), F - 1: b.leaf(OBJECTLIST)})})
    obj_deep = b.pointer({2: b.leaf(BLOB), 5: b.pointer({0: b.leaf(BLOB), 4: b.leaf(BLOB)}), F - 1: b.leaf(BLOB)})
    spaces = {
        0: (1, key_deep, obj_deep),
        1: (0, None, None),                      # Free
        2: (1, b.leaf(OBJECTLIST), None),        # key tree only, its root directly a leaf
        3: (2, b.leaf(OBJECTLIST), b.leaf(BLOB)),  # Invalid: not followed (its blocks stay unreachable)
        4: (1, None, b.pointer({1: b.leaf(BLOB)})),  # object tree only
        lay0.spaces_per_block - 1: (1, b.leaf(OBJECTLIST), b.leaf(BLOB)),
    }
    sl = b.spacelist(spaces)
    if one_spacelist:
        root = sl
    else:
        sl2 = b.spacelist({0: (1, b.pointer({F - 1: b.leaf(OBJECTLIST)}), None), 7: (1, None, b.leaf(BLOB))})
        root = b.pointer({0: sl, 6: b.pointer({2: sl2})})  # a leaf and a pointer block side by side
    img, lay = b.finish(root, slack=SLACK)
    return frozen(img), lay


@functools.lru_cache(maxsize=None)
def tag_store():
    return _whole_store(ScrubLayout.test_tag(0), one_spacelist=False)


@functools.lru_cache(maxsize=None)
def production_store():
    return _whole_store(ScrubLayout.production(0), one_spacelist=True)


@functools.lru_cache(maxsize=None)
def empty_store():
    img, lay = Builder(ScrubLayout.test_tag(0)).finish(None, slack=SLACK)
    return frozen(img), lay


@functools.lru_cache(maxsize=None)
def leaf_root_store():
    b = Builder(ScrubLayout.test_tag(0))
    img, lay = b.finish(b.spacelist({0: (1, b.leaf(OBJECTLIST), b.leaf(BLOB))}), slack=SLACK)
    return frozen(img), lay


# F, tags, leaf length, block size, the level sizes and the pointer blocks / leaves to expect
TREE_SHAPES = {
    "f10": (10, range(1000), 728, 1024, (1, 10, 100, 1000), 111, 1000),
    "f65": (65, (0, 64, 65 ** 2 - 1, 65 ** 3 - 1), 256, 2048, (1, 2, 3, 4), 6, 4),
    "f64": (64, range(0, 8192, 2), 728, 2048, (1, 32, 2048, 4096), 2081, 4096),
    "f1200": (1200, tuple(range(1300)) + (1200 * 1199, 1200 ** 2 - 1), 32768, 32768, (1, 1200, 1302), 1201, 1302),
}


@functools.lru_cache(maxsize=None)
def tree_shape(name: str):
    """(image with SLACK blocks of slack, layout, root (cs, address), root type, leaf length)
    of a committed tree from oracle.storm_cache.build_tree."""
    F, tags, leaf_len, bs, _, n_ptr, n_leaf = TREE_SHAPES[name]
    n = 1 + n_ptr + n_leaf
    store = Store(bs, n)
    initialize(store)
    build_tree(store, F, leaf_len, tags, revision=2, seed=11)
    img = flatten(store, n, SLACK)
    lay = ScrubLayout(bs, n, F, 10, 536, leaf_len)
    return frozen(img), lay, (_u64(img, 32), _u64(img, 40)), int(img[56]), leaf_len


def frozen(img: np.ndarray) -> np.ndarray:
    img.flags.writeable = False  # shared among the tests: edit a copy
    return img


# ---- damage: edits of a whole store. Each takes (image copy, layout, index of the intact
# store) and returns the report fields the edit must produce. --------------------------------

def pointer_entry(img, lay, index, level=None, leaf_child=None):
    """(pointer block address, slot, entry offset, type offset) of a used entry."""
    F, bs = lay.pointer_fanout, lay.block_size
    for a in sorted(index):
        parent, slot, kind, lvl = index[a]
        if parent and index[parent][2] == POINTER and (level is None or lvl == level) and \
                (leaf_child is None or (kind != POINTER) == leaf_child):
            return parent, slot, parent * bs + 24 * slot, parent * bs + 24 * F + slot
    raise AssertionError("no such entry")


def set_address(address):
    def edit(img, lay, index):
        parent, slot, off, _ = pointer_entry(img, lay, index)
        img[off + 8:off + 16] = np.frombuffer(struct.pack("<Q", address), np.uint8)
        rehash_store(img, lay, index, parent)
        return dict(first_error=RANGE, first_parent=parent, first_slot=slot, first_address=address, n_structural=1,
                    n_mismatch=0)
    return edit


def _type_byte(img, lay, index):
    parent, slot, _, toff = pointer_entry(img, lay, index)
    img[toff] = 3
    rehash_store(img, lay, index, parent)
    return dict(first_error=TYPE, first_parent=parent, first_slot=slot, n_structural=1, n_mismatch=0)


def _space_state(img, lay, index):
    sl = min(a for a, (_, _, k, _) in index.items() if k == SPACELIST)
    img[sl * lay.block_size + 72 * 4 + 66] = 7  # space 4 (object tree only): its tree is no longer followed
    rehash_store(img, lay, index, sl)
    return dict(first_error=TYPE, first_parent=sl, first_slot=8, n_structural=1, n_mismatch=0)


def _duplicate_in_one_block(img, lay, index):
    """Two slots of one pointer block name one child: the smaller slot is followed, once."""
    F, bs = lay.pointer_fanout, lay.block_size
    parent, slot, off, toff = pointer_entry(img, lay, index, leaf_child=True)
    types = img[parent * bs + 24 * F:parent * bs + 25 * F]
    free = next(i for i in range(F - 1, -1, -1) if types[i] == 0)
    img[parent * bs + 24 * free:parent * bs + 24 * free + 24] = img[off:off + 24]
    img[parent * bs + 24 * F + free] = img[toff]
    rehash_store(img, lay, index, parent)
    lo, hi = sorted((slot, free))
    return dict(first_error=DUPLICATE, first_parent=parent, first_slot=hi, n_structural=1, n_mismatch=0,
                first_address=int(struct.unpack_from("<Q", img, off + 8)[0]), verified=(8, 2, 6, 7))


def _duplicate_of_a_shallower_block(img, lay, index):
    """A deep pointer entry names a block that a shallower level already reached."""
    parent, slot, off, _ = pointer_entry(img, lay, index, level=max(l for _, _, _, l in index.values()))
    shallow = min(a for a, (_, _, _, lvl) in index.items() if lvl == 1)
    img[off + 8:off + 16] = np.frombuffer(struct.pack("<Q", shallow), np.uint8)
    rehash_store(img, lay, index, parent)
    return dict(first_error=DUPLICATE, first_parent=parent, first_slot=slot, first_address=shallow, n_structural=1)


def flip_leaf(img, lay, index):
    victim = max(a for a, (_, _, k, _) in index.items() if k == BLOB)
    img[victim * lay.block_size + lay.blob_len - 1] ^= 1  # the last hashed byte
    return dict(first_error=MISMATCH, first_address=victim, n_mismatch=1, n_structural=0)


def _flip_singularity(img, lay, index):
    img[20] ^= 0x10
    return dict(first_error=MISMATCH, first_address=0, first_level=0, n_mismatch=1, levels=0, verified=(0, 0, 0, 0),
                bytes_hashed=72)


def _two_mismatches_on_one_level(img, lay, index):
    """Two leaves of the deepest level: the first error is the one with the smaller
    (parent, slot), whichever address is smaller."""
    deepest = max(l for _, _, _, l in index.values())
    rows = sorted((index[a][0], index[a][1], a) for a in index if index[a][3] == deepest)
    assert len(rows) >= 2
    for _, _, a in (rows[0], rows[-1]):
        img[a * lay.block_size + 3] ^= 0xff
    return dict(first_error=MISMATCH, first_parent=rows[0][0], first_slot=rows[0][1], first_address=rows[0][2],
                first_level=deepest, n_mismatch=2)


def _mismatch_and_range_on_one_level(img, lay, index):
    """A RANGE error and a mismatch whose references sit on one level: the smaller
    (parent, slot) of the two is first."""
    parent, slot, off, _ = pointer_entry(img, lay, index, level=2)
    img[off + 8:off + 16] = np.frombuffer(struct.pack("<Q", lay.n_blocks + 1), np.uint8)
    rehash_store(img, lay, index, parent)
    other = max(a for a in index if index[a][3] == 2 and (index[a][0], index[a][1]) != (parent, slot))
    img[other * lay.block_size + 1] ^= 2
    first = min((parent, slot, RANGE), (index[other][0], index[other][1], MISMATCH))
    return dict(first_error=first[2], first_parent=first[0], first_slot=first[1], first_level=2, n_mismatch=1,
                n_structural=1)


DAMAGE = {
    "leaf": flip_leaf,
    "singularity": _flip_singularity,
    "address n_blocks": lambda img, lay, index: set_address(lay.n_blocks)(img, lay, index),
    "address 2**63": set_address(2 ** 63),
    "address 2**64-1": set_address(2 ** 64 - 1),
    "address 0": set_address(0),
    "type byte 3": _type_byte,
    "space state 7": _space_state,
    "duplicate in one block": _duplicate_in_one_block,
    "duplicate of a shallower block": _duplicate_of_a_shallower_block,
    "two mismatches on one level": _two_mismatches_on_one_level,
    "mismatch and range on one level": _mismatch_and_range_on_one_level,
}


# ---- mass damage: any number of edits, then reseal, so that only the deliberate damage is
# wrong (tests/test_scrub_damage.py, tests/test_scrub_damage_gpu.py) -----------------------------

def entry_offsets(lay: ScrubLayout, parent, parent_kind, slot):
    """(offset of the Pointer, offset of the type byte) of entry `slot` of block `parent`."""
    bs = lay.block_size
    if parent_kind == POINTER:
        return parent * bs + 24 * slot, parent * bs + 24 * lay.pointer_fanout + slot
    sp = parent * bs + 72 * (slot // 2)
    return sp + 16 + 24 * (slot & 1), sp + 64 + (slot & 1)


def _put_u64(img, off, value):
    img[off:off + 8] = np.frombuffer(struct.pack("<Q", value), np.uint8)


def write_entry(img, lay, parent, parent_kind, slot, checksum=None, address=None, typ=None):
    off, toff = entry_offsets(lay, parent, parent_kind, slot)
    if checksum is not None:
        _put_u64(img, off, checksum)
    if address is not None:
        _put_u64(img, off + 8, address)
    if typ is not None:
        img[toff] = typ


def reseal(img: np.ndarray, lay: ScrubLayout, index, keep_bad=(), whole_store=False, lens=None):
    """After any number of edits: re-hash every block of the intact store's `index`, deepest
    level first, and store its new checksum in its parent's entry where that entry still
    names the block. Blocks in `keep_bad` are meant to mismatch: the entry that names them
    keeps the checksum it has. Returns the root's checksum (a tree's new root); with
    `whole_store` it is also stored in the singularity, which is sealed."""
    lens = lens or kind_lens(lay)
    bs = lay.block_size
    keep_bad = set(keep_bad)
    root_cs = None
    for a in sorted(index, key=lambda a: -index[a][3]):
        parent, slot, kind, _ = index[a]
        if a in keep_bad:
            continue
        cs = o.xxh64(img[a * bs:a * bs + lens[kind]])
        if parent == 0:
            root_cs = cs
            continue
        off, _ = entry_offsets(lay, parent, index[parent][2], slot)
        if _u64(img, off + 8) == a:
            _put_u64(img, off, cs)
    if whole_store:
        seal_singularity(img, root_cs)
    return root_cs


FUZZ_EDITS = (1, 3, 10, 40, 150)


def random_damage(img, lay, index, rng, n_edits, whole_store):
    """`n_edits` seeded edits of the image (the intact store's `index`): bit flips in hashed
    bytes, entry addresses (0, n_blocks, into the slack, another block, the block itself,
    its parent), type bytes 3..255, entries copied onto other slots and, for whole stores,
    space states and the type bytes of key and object pointers. The root block is spared.
    Every address written is below n_blocks + SLACK. Returns the blocks to keep_bad."""
    lens = kind_lens(lay)
    bs, n = lay.block_size, lay.n_blocks
    blocks = sorted(a for a in index if index[a][0] != 0)
    parents = [a for a in blocks if index[a][2] in (POINTER, SPACELIST)]
    spacelists = [a for a in blocks if index[a][2] == SPACELIST]
    kinds = ["flip", "address", "type", "copy"] + (["state", "space type"] if whole_store and spacelists else [])
    keep_bad = set()

    def entry():
        p = parents[rng.integers(len(parents))]
        kind = index[p][2]
        entries = lay.pointer_fanout if kind == POINTER else 2 * lay.spaces_per_block
        used = [s for s in range(entries) if img[entry_offsets(lay, p, kind, s)[1]] != 0]
        slot = used[rng.integers(len(used))] if used and rng.integers(2) else int(rng.integers(entries))
        return p, kind, entries, slot

    for _ in range(n_edits):
        what = kinds[rng.integers(len(kinds))]
        if what == "flip" or not parents:
            a = blocks[rng.integers(len(blocks))]
            img[a * bs + rng.integers(lens[index[a][2]])] ^= np.uint8(1 << rng.integers(8))
            keep_bad.add(a)
        elif what == "address":
            p, kind, _, slot = entry()
            address = (0, n, n + 1 + int(rng.integers(SLACK - 1)), 1 + int(rng.integers(n - 1)), p,
                       index[p][0])[rng.integers(6)]
            assert address < n + SLACK
            off, toff = entry_offsets(lay, p, kind, slot)
            _put_u64(img, off + 8, address)
            if img[toff] == FREE_T:
                img[toff] = 1 + rng.integers(2)
        elif what == "type":
            p, kind, _, slot = entry()
            img[entry_offsets(lay, p, kind, slot)[1]] = 3 + rng.integers(253)
        elif what == "copy":
            p, kind, entries, slot = entry()
            to = int(rng.integers(entries))
            (src, tsrc), (dst, tdst) = entry_offsets(lay, p, kind, slot), entry_offsets(lay, p, kind, to)
            img[dst:dst + 24] = img[src:src + 24].copy()
            img[tdst] = img[tsrc]
        elif what == "state":
            sl = spacelists[rng.integers(len(spacelists))]
            img[sl * bs + 72 * rng.integers(lay.spaces_per_block) + 66] = (0, 2, 3 + int(rng.integers(253)))[rng.integers(3)]
        else:
            sl = spacelists[rng.integers(len(spacelists))]
            img[sl * bs + 72 * rng.integers(lay.spaces_per_block) + 64 + rng.integers(2)] = rng.integers(256)
    return keep_bad


class Case:
    """One image to scrub: a whole store (tree None) or one tree, tree = ((checksum,
    address, revision), root type, leaf kind, leaf length); `expect`: report fields the
    construction fixes."""

    def __init__(self, img, lay, tree=None, expect=None):
        self.img, self.lay, self.tree, self.expect = img, lay, tree, expect or {}

    def reference(self):
        if self.tree is None:
            return reference_scrub(self.img, self.lay)
        root, root_type, leaf_kind, leaf_len = self.tree
        return reference_scrub(self.img, self.lay, root[:2], root_type, leaf_kind, leaf_len)


def intact_case(name) -> Case:
    """The shared images by name: a tree of TREE_SHAPES, "tag_store" or "wide_store"."""
    if name in TREE_SHAPES:
        img, lay, root, root_type, leaf_len = tree_shape(name)
        return Case(img, lay, (root + (2,), root_type, BLOB, leaf_len))
    img, lay = {"tag_store": tag_store, "wide_store": wide_store}[name]()
    return Case(img, lay)


@functools.lru_cache(maxsize=None)
def intact_index(name):
    return intact_case(name).reference()[2]


def edited(name, edit) -> Case:
    """A copy of the shared image `name` after edit(img, lay, index) -> (keep_bad, expect),
    resealed."""
    c, index = intact_case(name), intact_index(name)
    img = c.img.copy()
    keep_bad, expect = edit(img, c.lay, index)
    cs = reseal(img, c.lay, index, keep_bad, whole_store=c.tree is None)
    tree = c.tree and ((cs,) + c.tree[0][1:],) + c.tree[1:]
    return Case(img, c.lay, tree, expect)


FUZZ_IMAGES = ("f10", "f64", "f65", "tag_store", "wide_store")
FUZZ_SEEDS = 40
fuzz_reports = {}  # (image, seed) -> the reference's report, for the dead-root condition


def fuzz_case(name, seed) -> Case:
    rng = np.random.default_rng([seed, FUZZ_IMAGES.index(name)])
    n_blocks = intact_case(name).lay.n_blocks
    n_edits = FUZZ_EDITS[seed % len(FUZZ_EDITS)]
    if n_blocks < 1000:  # small images: at most an edit per four blocks
        n_edits = max(1, min(n_edits, n_blocks // 4))
    return edited(name, lambda img, lay, index: (random_damage(img, lay, index, rng, n_edits, name.endswith("store")),
                                                 {}))


def check_fuzz_reference(name, seed, rep, index):
    """What the fuzz asserts from the reference's own report: the root block was spared (it
    verified and was expanded); the report is kept for still_alive()."""
    root = min(a for a in index if index[a][0] == 0)
    assert not (rep["first_error"] and rep["first_level"] == 0) and rep["levels"] >= 2 and sum(rep["verified"]) >= 1
    assert index[root][3] == 0
    fuzz_reports[name, seed] = rep


def still_alive(name, make_reference):
    """Of the image's fuzz cases, the share in which the reference still verifies at least
    half of the blocks (make_reference(seed) for the seeds no test has run yet)."""
    n_blocks = intact_case(name).lay.n_blocks
    alive = 0
    for seed in range(FUZZ_SEEDS):
        if (name, seed) not in fuzz_reports:
            make_reference(seed)
        alive += 2 * sum(fuzz_reports[name, seed]["verified"]) >= n_blocks - 1
    return alive / FUZZ_SEEDS


# ---- contested references (tree f64: levels 1 / 32 / 2,048 / 4,096; its level-2 pointer
# blocks hold two leaves each and 62 free slots) ----------------------------------------------

N_PAIRS = 450
WRONG = 0x5A5A5A5A5A5A5A5A  # xor'ed into a checksum that is meant to be wrong


def _level(index, level, kind=None):
    return sorted(a for a, (_, _, k, lvl) in index.items() if lvl == level and (kind is None or k == kind))


def _kids(index, parent):
    return sorted((slot, a) for a, (p, slot, _, _) in index.items() if p == parent)


def _free_slot(img, lay, block, nth=0):
    F, bs = lay.pointer_fanout, lay.block_size
    return [s for s in range(F) if img[block * bs + 24 * F + s] == 0][nth]


def _contested_pairs(img, lay, index):
    """450 disjoint pairs (A, B) of level-2 pointer blocks, every A below every B, in three
    modes (the issue's section 2). The winner of each contest is A, the smaller parent."""
    rng = np.random.default_rng(450)
    bs = lay.block_size
    chosen = np.sort(rng.choice(_level(index, 2), size=2 * N_PAIRS, replace=False))
    As, Bs = rng.permutation(chosen[:N_PAIRS]), rng.permutation(chosen[N_PAIRS:])
    keep_bad = set()
    for i, (A, B) in enumerate(zip(As.tolist(), Bs.tolist())):
        assert A < B
        mode = i % 3
        owner, thief = (B, A) if mode < 2 else (A, B)  # the thief gets a copy of one of the owner's leaf entries
        slot, leaf = _kids(index, owner)[i % 2]
        good = _u64(img, entry_offsets(lay, owner, POINTER, slot)[0])
        assert good == o.xxh64(img[leaf * bs:leaf * bs + lay.blob_len])
        a_cs, b_cs = (good, good ^ WRONG) if mode != 1 else (good ^ WRONG, good)
        write_entry(img, lay, thief, POINTER, _free_slot(img, lay, thief, i % 5), a_cs if thief == A else b_cs, leaf,
                    LEAF_T)
        write_entry(img, lay, owner, POINTER, slot, a_cs if owner == A else b_cs)
        keep_bad.add(leaf)
    return keep_bad, dict(n_structural=N_PAIRS, n_mismatch=N_PAIRS // 3, verified=(2081, 0, 0, 4096 - N_PAIRS // 3),
                          first_error=MISMATCH, first_level=3)


def _across_levels(img, lay, index):
    """Eight level-1 blocks each name, in place of one of their level-2 children, a leaf
    that a level-2 block elsewhere holds. The level-1 entry wins although its key is the
    larger one (level-1 blocks have the larger addresses): it is the shallower. Even i: the
    level-1 entry is right and the level-2 entry wrong; odd i: the other way round."""
    bs = lay.block_size
    level1, keep_bad = _level(index, 1), set()
    lost, n_bad = 0, 0
    for i in range(8):
        P = level1[3 * i]
        slot, _ = _kids(index, P)[5 + i]  # this level-2 block and its two leaves are no longer reached
        D = _kids(index, level1[3 * i + 1])[7][1]
        dslot, leaf = _kids(index, D)[i % 2]
        assert P > D and index[leaf][3] == 3
        good = _u64(img, entry_offsets(lay, D, POINTER, dslot)[0])
        write_entry(img, lay, P, POINTER, slot, good ^ (WRONG if i & 1 else 0), leaf, LEAF_T)
        write_entry(img, lay, D, POINTER, dslot, good ^ (0 if i & 1 else WRONG))
        keep_bad.add(leaf)
        lost += 1
        n_bad += i & 1
    return keep_bad, dict(n_structural=8, n_mismatch=n_bad, verified=(2081 - lost, 0, 0, 4096 - 2 * lost - n_bad),
                          first_error=MISMATCH, first_level=2, levels=4)


def _kind_conflict(img, lay, index):
    """Level-2 blocks A < B contest a leaf of B under different block types; A's type decides
    the hashed length and whether the block is expanded. Even i: A names it as a pointer block
    (the checksum of its first 1,600 bytes; it holds no entries) and B as the leaf it is; odd
    i: A names it as the leaf it is and B as a pointer block."""
    bs, plen = lay.block_size, kind_lens(lay)[POINTER]
    level2, keep_bad = _level(index, 2), set()
    for i in range(6):
        A, B = level2[100 + 7 * i], level2[1500 + 11 * i]
        slot, leaf = _kids(index, B)[i % 2]
        assert not img[leaf * bs + 24 * lay.pointer_fanout:leaf * bs + plen].any()  # as a pointer block: all Free
        good = _u64(img, entry_offsets(lay, B, POINTER, slot)[0])
        if i & 1:
            write_entry(img, lay, A, POINTER, _free_slot(img, lay, A, 3), good, leaf, LEAF_T)
            write_entry(img, lay, B, POINTER, slot, typ=POINTER_T)
        else:
            write_entry(img, lay, A, POINTER, _free_slot(img, lay, A, 3), o.xxh64(img[leaf * bs:leaf * bs + plen]), leaf,
                        POINTER_T)
        keep_bad.add(leaf)
    return keep_bad, dict(n_structural=6, n_mismatch=0, verified=(2081 + 3, 0, 0, 4096 - 3), first_error=DUPLICATE,
                          first_level=3)


def _ancestor_cycles(img, lay, index):
    """A level-2 block names itself, another its grandparent (the root), a third its parent:
    each is a DUPLICATE and the walk ends."""
    level2 = _level(index, 2)
    root = _level(index, 0)[0]
    me, grand, child = level2[10], level2[900], level2[2000]
    write_entry(img, lay, me, POINTER, _free_slot(img, lay, me), 1, me, POINTER_T)
    write_entry(img, lay, grand, POINTER, _free_slot(img, lay, grand, 40), 2, root, POINTER_T)
    write_entry(img, lay, child, POINTER, _free_slot(img, lay, child, 61), 3, index[child][0], POINTER_T)
    return (), dict(n_structural=3, n_mismatch=0, verified=(2081, 0, 0, 4096), first_error=DUPLICATE, first_level=3,
                    first_parent=me, first_address=me, levels=4)


def _forty_leaf_mismatches(img, lay, index):
    """Forty flipped leaves spread over f10's level of 1,000 leaves, which holds nothing to
    expand: the first error is the smallest (parent, slot), which is not the smallest address."""
    leaves = _level(index, 3)
    victims = leaves[7::25]
    for a in victims:
        img[a * lay.block_size + 100 + a % 600] ^= 0x04
    parent, slot, first = min((index[a][0], index[a][1], a) for a in victims)
    assert first != min(victims) and len(victims) == 40
    return set(victims), dict(n_structural=0, n_mismatch=40, verified=(111, 0, 0, 960), first_error=MISMATCH,
                              first_level=3, first_parent=parent, first_slot=slot, first_address=first)


# name -> (image, edit for edited())
CONTESTED = {"450 pairs": ("f64", _contested_pairs), "across levels": ("f64", _across_levels),
             "kind conflict": ("f64", _kind_conflict), "ancestor cycles": ("f64", _ancestor_cycles),
             "forty leaf mismatches": ("f10", _forty_leaf_mismatches)}


# ---- entries past lane 63 -----------------------------------------------------------------

WIDE_SPACES = {31: 1, 32: 0, 63: 1, 69: 0}  # space -> which of its two pointers: entries 63, 64, 127, 138
WIDE_SLOTS = (63, 64, 127, 128, 129)
WIDE_KINDS = ("range", "type", "duplicate", "mismatch")


@functools.lru_cache(maxsize=None)
def wide_store():
    """Small blocks, wide entries: fan-out 130 and 70 spaces (140 entries) per spacelist
    block, so that a wave meets three 64-entry chunks. One pointer block over two spacelist
    blocks with all 70 spaces used (Defined, Free and Invalid); each Defined space has a
    key-tree leaf and a small object tree. Space 32 of the first spacelist block holds the
    130-wide pointer block whose slots 0 and WIDE_SLOTS are leaves."""
    lay0 = ScrubLayout(8192, 0, 130, 70, 536, 728)
    b = Builder(lay0, seed=23)
    F = lay0.pointer_fanout

    def spaces(first):
        out = {}
        for k in range(lay0.spaces_per_block):
            if k in WIDE_SPACES or k % 4 < 2:
                if first and k == 32:
                    obj = b.pointer({s: b.leaf(BLOB) for s in (0,) + WIDE_SLOTS})
                else:
                    obj = b.pointer({k: b.leaf(BLOB), (7 * k + 71) % F: b.leaf(BLOB)})
                out[k] = (1, b.leaf(OBJECTLIST), obj)
            elif k % 4 == 2:
                out[k] = (0, None, None)
            else:
                out[k] = (2, b.leaf(OBJECTLIST), b.leaf(BLOB))
        return out

    first, second = b.spacelist(spaces(True)), b.spacelist(spaces(False))
    img, lay = b.finish(b.pointer({0: first, F - 1: second}), slack=SLACK)
    return frozen(img), lay


def place_damage(parent_of, slot, kind):
    """An edit for edited(): damage `kind` of WIDE_KINDS at entry `slot` of the block
    parent_of(index), which holds a followed reference there."""
    def edit(img, lay, index):
        parent = parent_of(index)
        child = dict(_kids(index, parent))[slot]
        root = _level(index, 0)[0]
        expect = dict(first_parent=parent, first_slot=slot, first_level=index[child][3], n_structural=1, n_mismatch=0)
        if kind == "range":
            write_entry(img, lay, parent, index[parent][2], slot, address=lay.n_blocks)
            expect.update(first_error=RANGE, first_address=lay.n_blocks)
        elif kind == "type":
            write_entry(img, lay, parent, index[parent][2], slot, typ=3)
            expect.update(first_error=TYPE)
        elif kind == "duplicate":
            write_entry(img, lay, parent, index[parent][2], slot, address=root)
            expect.update(first_error=DUPLICATE, first_address=root)
        else:
            img[child * lay.block_size + 9] ^= 0x20
            expect.update(first_error=MISMATCH, first_address=child, n_structural=0, n_mismatch=1)
            return {child}, expect
        return (), expect
    return edit


def wide_first_spacelist(index):
    return min(a for a, (_, slot, k, _) in index.items() if k == SPACELIST and slot == 0)


def wide_pointer_block(index):
    return dict(_kids(index, wide_first_spacelist(index)))[2 * 32 + 1]


WIDE_DAMAGE = {}
for _s, _which in WIDE_SPACES.items():
    for _k in WIDE_KINDS:
        WIDE_DAMAGE["space %d %s" % (_s, _k)] = (wide_first_spacelist, 2 * _s + _which, _k)
for _s in WIDE_SLOTS:
    for _k in WIDE_KINDS:
        WIDE_DAMAGE["slot %d %s" % (_s, _k)] = (wide_pointer_block, _s, _k)


def f1200_first_level1(index):
    return dict(_kids(index, _level(index, 0)[0]))[0]  # tags 0, 1200 and 1200 * 1199: slots 0, 1 and 1199


def _f1200_new_entry(slot, kind):
    """A level-1 block of f1200 gets an entry at the free `slot`: a copy of its slot 0
    (DUPLICATE) or a leaf reference to n_blocks (RANGE)."""
    def edit(img, lay, index):
        parent = f1200_first_level1(index)
        src, tsrc = entry_offsets(lay, parent, POINTER, 0)
        dst, tdst = entry_offsets(lay, parent, POINTER, slot)
        assert img[tdst] == FREE_T
        img[dst:dst + 24] = img[src:src + 24].copy()
        img[tdst] = img[tsrc]
        expect = dict(first_parent=parent, first_slot=slot, first_level=2, n_structural=1, n_mismatch=0,
                      first_error=DUPLICATE, first_address=_u64(img, src + 8))
        if kind == "range":
            _put_u64(img, dst + 8, lay.n_blocks)
            expect.update(first_error=RANGE, first_address=lay.n_blocks)
        return (), expect
    return edit


F1200_DAMAGE = {"slot 63 duplicate": _f1200_new_entry(63, "duplicate"), "slot 64 range": _f1200_new_entry(64, "range"),
                "slot 1199 mismatch": place_damage(f1200_first_level1, 1199, "mismatch")}


# ---- block_size = 8 (mod 16) ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def odd_stride_tree():
    """A tree of 2,056-byte blocks, leaves of the whole block: 300 leaves under 65 + 1
    pointer blocks of fan-out 65. Every second block starts 8 bytes off a 16-byte boundary."""
    F, n_leaf, bs = 65, 300, 2056
    n = 1 + n_leaf + 65 + 1
    store = Store(bs, n)
    initialize(store)
    build_tree(store, F, bs, range(n_leaf), revision=2, seed=5)
    img = flatten(store, n, SLACK)
    lay = ScrubLayout(bs, n, F, 10, 536, bs)
    return frozen(img), lay, (_u64(img, 32), _u64(img, 40), 2), int(img[56]), bs


# ---- commit -> scrub: the bytes the library's own commit wrote ---------------------------------

ROUND_TRIPS = [(1, 10, 1024, 728), (2, 10, 1024, 728), (10, 10, 1024, 728), (11, 10, 1024, 728),
               (5000, 10, 1024, 728), (700, 65, 2056, 2056), (1201, 1200, 32768, 32768), (2500, 1200, 32768, 31808)]


def forest_arena(n, F, slot, L):
    """(blocks, arena, last_allocated, pointer blocks per level bottom-up) of
    commit.pointer_forest with nothing relocated: random leaves, slot 0 and the pointer
    blocks' slots zeroed."""
    from storm_amd import commit
    blocks, arena_bytes, last = commit.pointer_forest(n, L, F, slot)
    rng = np.random.default_rng(n)
    arena = np.zeros(arena_bytes, dtype=np.uint8)
    leaves = arena[slot:(n + 1) * slot].reshape(n, slot)
    leaves[:, :L] = rng.integers(0, 256, (n, L), dtype=np.uint8)
    levels, m = [], n
    while m > 1:
        m = (m + F - 1) // F
        levels.append(m)
    return blocks, arena, last, levels


def committed_tree(arena, n, F, slot, L, levels) -> Case:
    """The committed arena as an image of `slot`-byte blocks, rooted where the commit left
    the root: the singularity's SpacePointer (bytes 32..55) and SpaceBlockType (byte 56)."""
    total = n + sum(levels)
    lay = ScrubLayout(slot, total + 1, F, 10, 536, L)
    root = struct.unpack_from("<QQQ", arena, 32)
    plen = kind_lens(lay)[POINTER]
    return Case(arena, lay, (root, int(arena[56]), BLOB, L),
                dict(verified=(sum(levels), 0, 0, n), levels=len(levels) + 1, n_mismatch=0, n_structural=0,
                     first_error=0, bytes_hashed=sum(levels) * plen + n * L))
