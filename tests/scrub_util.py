"""TEST INFRASTRUCTURE for the scrub tests (tests/test_scrub.py, tests/test_scrub_gpu.py).

* ``reference_scrub``: a short pure-Python breadth-first walk with the C oracle's XXH64,
  the reference for every report field and for the reachable set;
* ``Builder``: whole stores by hand (singularity -> space tree -> spacelist leaves -> key
  and object trees), children first;
* ``flatten``: ``oracle.storm_cache.Store.dev`` as one contiguous image;
* ``rehash_path``: after a deliberate edit, new checksums up the path to the root, so
  that only the edit itself is wrong;
* the stores and tree shapes both test files use, built once per process.
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
