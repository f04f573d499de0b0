"""TEST INFRASTRUCTURE for the lookup tests (tests/test_lookup.py, tests/test_lookup_gpu.py).

* ``probe``: findChunkPointerForKey and verifyKeyInChunks in literal Python, with the bounds of
  include/stormck.h "lookup";
* ``reference_lookup``: tests/trace_util.reference_trace over the keys' tags, then the status
  order of the header and ``probe`` per key: the reference for every result and report field;
* ``Leaf``: an objectlist.Block of C chunks as bytes, with storm's ``setKeyInChunks`` (``insert``)
  and ``plant`` for hand-made items;
* ``KeyTree``: keys placed into the leaves of a tree by their tag digits (no split: a leaf that
  would overflow raises), laid out with scrub_util.Builder;
* ``table``: addressing tables, seeded numpy permutations;
* the designed cases both test files run (``CASES``), built once per process;
* the fuzz of tests/test_lookup_fuzz.py and tests/test_lookup_fuzz_gpu.py: ``damaged_tree_case``
  (the stored tree under scrub_util.random_damage) and ``leaf_fuzz_case`` (leaves whose fields
  are edited at random), whose keys tests/test_lookup_sanitize.py also writes out as a corpus.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import oracle as o
from storm_amd import keystore as ks
from storm_amd.scrub import OBJECTLIST, ScrubLayout
from storm_amd.trace import ABSENT, FOUND, MISMATCH
from tests import scrub_util as su
from tests import trace_util as tu

FREE, DEFINED, INVALID = 0, 1, 2
NO_SLOT, KEY = ks.NO_SLOT, ks.KEY
RESULT_FIELDS = ("object_id", "address", "reminder", "index", "probes", "status")


def table(C: int, seed: int = 0) -> np.ndarray:
    """An addressing table: a seeded permutation of 0..C-1."""
    return np.random.default_rng(1000 + seed).permutation(C).astype(np.uint16)


# ---- the leaf ----------------------------------------------------------------------------------

class Leaf:
    """objectlist.Block with C chunks (blocks/objectlist/block.go:29-40) as its bytes."""

    def __init__(self, C: int):
        self.C = C
        self.b = bytearray(ks.leaf_len(C))

    # field access: (offset of the array, struct code, element size)
    def _at(self, base, code, size, i, value=None):
        off = base * self.C + size * i
        if value is None:
            return struct.unpack_from(code, self.b, off)[0]
        struct.pack_into(code, self.b, off, value)

    def reminder(self, i, v=None): return self._at(32, "<Q", 8, i, v)
    def link(self, i, v=None): return self._at(40, "<Q", 8, i, v)
    def chunk_pointer(self, i, v=None): return self._at(48, "<H", 2, i, v)
    def next_pointer(self, i, v=None): return self._at(50, "<H", 2, i, v)
    def state(self, i, v=None): return self._at(52, "B", 1, i, v)
    def n_used(self, v=None): return self._at(53, "<H", 2, 0, v)
    def free_index(self, v=None): return self._at(53, "<H", 2, 1, v)

    def store_key(self, key: bytes) -> int:
        """setKeyInChunks's chunk part (keystore.go:141-173): the key into chunks taken from the
        free list; returns the first chunk."""
        C = self.C
        if self.n_used() + (len(key) + 31) // 32 > C:
            raise OverflowError("block does not contain enough free chunks to add new key")
        if self.n_used() == 0:
            for i in range(C):  # initFreeChunkList
                self.next_pointer(i, i + 1)
        first, rest, last, copied = self.free_index(), key, 0, 0
        while rest:
            self.n_used(self.n_used() + 1)
            last = self.free_index()
            self.free_index(self.next_pointer(last))
            copied = min(32, len(rest))
            self.b[32 * last:32 * last + copied] = rest[:copied]
            rest = rest[copied:]
        self.next_pointer(last, C + copied)
        return first

    def plant(self, index, stored_key, reminder, object_id, state=DEFINED):
        """A hand-made item in slot `index`: `stored_key` (None: no chunks, chunk pointer 0)
        under `reminder`, whatever the probe sequence would say about the slot."""
        self.state(index, state)
        self.reminder(index, reminder)
        self.link(index, object_id)
        self.chunk_pointer(index, self.store_key(stored_key) if stored_key else 0)

    def insert(self, A, key: bytes, reminder, object_id) -> int:
        """EnsureObjectID's insert without the split: the slot findChunkPointerForKey hands out."""
        _, index, _, found, _ = probe(self.b, self.C, A, key, reminder)
        if found:
            raise KeyError("the key is already there")
        if index == NO_SLOT:
            raise OverflowError("cannot find chunk for key")
        self.plant(index, key, reminder, object_id)
        return index


def plant(leaf: Leaf, index, stored_key, reminder, object_id, state=DEFINED):
    leaf.plant(index, stored_key, reminder, object_id, state)


def sequence(C, A, reminder):
    """The slots a key of that reminder probes, in order."""
    return [(reminder % C + int(A[i])) % C for i in range(C)]


# ---- the probe, literally ------------------------------------------------------------------------

def _chain_equals(b, C, chunk, key):
    """(equal, malformed): verifyKeyInChunks after the reminder test."""
    left = key
    for _ in range(9):
        if chunk >= C:
            break
        nxt = struct.unpack_from("<H", b, 50 * C + 2 * chunk)[0]
        if nxt > C:
            rest = nxt - C
            if rest > 32:
                break
            return bytes(b[32 * chunk:32 * chunk + rest]) == left, False
        if len(left) < 32:
            break
        if bytes(b[32 * chunk:32 * chunk + 32]) != left[:32]:
            return False, False
        left, chunk = left[32:], nxt
    return False, True


def probe(b, C, A, key: bytes, reminder):
    """(object_id, index, probes, found, malformed) of findChunkPointerForKey over leaf bytes b."""
    seed, invalid, malformed = reminder % C, None, False
    for i in range(C):
        index = (seed + int(A[i])) % C
        state = b[52 * C + index]
        if state == DEFINED:
            if struct.unpack_from("<Q", b, 32 * C + 8 * index)[0] == reminder:
                equal, bad = _chain_equals(b, C, struct.unpack_from("<H", b, 48 * C + 2 * index)[0], key)
                malformed |= bad
                if equal:
                    return struct.unpack_from("<Q", b, 40 * C + 8 * index)[0], index, i + 1, True, malformed
        elif state == INVALID:
            if invalid is None:
                invalid = index
        elif state == FREE:
            return 0, index if invalid is None else invalid, i + 1, False, malformed
    return 0, NO_SLOT, C, False, malformed


def key_text(n):
    if n == 0:
        return "key cannot be empty"
    return f"maximum key component length exceeded, maximum: 256, actual: {n}"


def reference_lookup(img, lay: ScrubLayout, root, root_type, C, A, keys, verify_leaves=True):
    """(results, report, message): results[i] = RESULT_FIELDS of keys[i]; message is the KEY
    text when key first_bad ends KEY, "" when no key ends badly, else None (the trace's words:
    compare with the trace's own entry point)."""
    tags = [o.xxh64(k) for k in keys]
    tres, trep, _, _ = tu.reference_trace(img, lay, root, root_type, OBJECTLIST, tags, 0, verify_leaves)
    view = memoryview(np.ascontiguousarray(img).view(np.uint8).reshape(-1))
    results, n_probed, probes, n_malformed = [], 0, 0, 0
    for k, (address, reminder, _, _, _, status) in zip(keys, tres):
        if not 1 <= len(k) <= 256:
            results.append((0, 0, 0, NO_SLOT, 0, KEY))
        elif status != FOUND:
            results.append((0, address, reminder, NO_SLOT, 0, status))
        else:
            leaf = view[address * lay.block_size:address * lay.block_size + ks.leaf_len(C)]
            oid, index, p, found, bad = probe(leaf, C, A, k, reminder)
            results.append((oid, address, reminder, index, p, FOUND if found else ABSENT))
            n_probed, probes, n_malformed = n_probed + 1, probes + p, n_malformed + bad
    n = len(keys)
    n_status = [0] * 8
    for r in results:
        n_status[r[5]] += 1
    first_bad = min((i for i, r in enumerate(results) if r[5] in ks.BAD), default=n)
    report = dict(n_status=tuple(n_status), n_probed=n_probed, probes=probes, n_malformed=n_malformed,
                  first_bad=first_bad, trace=trep)
    message = "" if first_bad == n else key_text(len(keys[first_bad])) if results[first_bad][5] == KEY else None
    return results, report, message


def as_tuples(records):
    return [tuple(int(rec[f]) for f in RESULT_FIELDS) for rec in records]


# ---- trees of keys -------------------------------------------------------------------------------

TEST_LAYOUT = ScrubLayout(1024, 0, 10, 10, 536, 728)        # storm's -tags test sizes, C = 10
PRODUCTION_LAYOUT = ScrubLayout(32768, 0, 1200, 400, 31808, 32768)  # C = 600


class Tree:
    """An image and the arguments that look keys up in one key tree of it."""

    def __init__(self, img, lay, root, root_type, C, A, address_of=None):
        self.img, self.lay, self.root, self.root_type = img, lay, tuple(root), root_type
        self.C, self.A = C, A
        self.params = ks.ObjectListParams(A, C)
        self.address_of = address_of or {}  # path (tuple of slots) -> block address

    def args(self):
        return self.lay, self.root[:2] + (2,), self.root_type, self.params

    def reference(self, keys, verify_leaves=True):
        return reference_lookup(self.img, self.lay, self.root, self.root_type, self.C, self.A, keys, verify_leaves)


class KeyTree:
    """Keys in the objectlist leaves of a tree of `depth` pointer levels, by their tag digits
    (cache/trace.go:38-40): the leaf at path (t % F, t // F % F, ...), reminder t // F^depth."""

    def __init__(self, lay: ScrubLayout, A, depth: int = 1):
        self.lay, self.A, self.C, self.depth = lay, A, len(A), depth
        assert lay.objectlist_len == ks.leaf_len(self.C)
        self.leaves = {}

    def locate(self, key: bytes):
        """(path, reminder) of the key."""
        t, path = o.xxh64(key), []
        for _ in range(self.depth):
            path.append(t % self.lay.pointer_fanout)
            t //= self.lay.pointer_fanout
        return tuple(path), t

    def leaf(self, path) -> Leaf:
        return self.leaves.setdefault(tuple(path), Leaf(self.C))

    def add(self, key: bytes, object_id: int) -> int:
        path, reminder = self.locate(key)
        return self.leaf(path).insert(self.A, key, reminder, object_id)

    def build(self, slack: int = su.SLACK) -> Tree:
        """The image: pointer blocks first (the root at address 1), then the leaves in the order
        of their paths, so that the last leaf is the image's last block."""
        nodes = sorted({p[:k] for p in self.leaves for k in range(self.depth)}, key=lambda p: (len(p), p))
        address = {p: 1 + i for i, p in enumerate(nodes + sorted(self.leaves))}
        b = su.Builder(self.lay)
        below = {}
        for p in address:
            if p:
                below.setdefault(p[:-1], []).append(p)

        def put(path):
            if len(path) == self.depth:
                b.next = address[path]
                return b._put(bytes(self.leaves[path].b), su.LEAF_T)
            kids = {p[-1]: put(p) for p in below[path]}
            b.next = address[path]
            return b.pointer(kids)

        root = put(()) if self.leaves else None
        b.next = 1 + len(address)
        img, lay = b.finish(None, slack=slack)
        if root is None:
            return Tree(su.frozen(img), lay, (0, 0), su.FREE_T, self.C, self.A)
        return Tree(su.frozen(img), lay, root[:2], root[2], self.C, self.A, address)


def key_in(kt: KeyTree, path, rng, length, accept=lambda reminder: True) -> bytes:
    """A random key of `length` bytes that lives in the leaf at `path` (any leaf when None) and
    whose reminder passes `accept`."""
    while True:
        k = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        p, reminder = kt.locate(k)
        if (path is None or p == tuple(path)) and accept(reminder):
            return k


# ---- key addressing --------------------------------------------------------------------------------

def pack(keys, mode="flat"):
    """The keys as the arguments of a lookup: dict(keys=, offsets=, lens=, length=).
    flat: one byte buffer, keys at offsets of both parities with gaps, offsets + lens;
    rows: (n, len) with len == stride; wide: (n, stride) with stride = len + 5 and `length`;
    rows+lens: (n, stride) rows with a lens array."""
    if mode == "flat":
        buf, offsets = bytearray(b"\xaa"), []
        for i, k in enumerate(keys):
            offsets.append(len(buf))
            buf += k + b"\xbb" * (1 + i % 2)
        return dict(keys=np.frombuffer(bytes(buf), np.uint8), offsets=np.array(offsets, np.uint64),
                    lens=np.array([len(k) for k in keys], np.uint32), length=None)
    width = max((len(k) for k in keys), default=1)
    if mode == "rows+lens":
        rows = np.full((len(keys), width + 3), 0xCC, np.uint8)
        for i, k in enumerate(keys):
            rows[i, :len(k)] = np.frombuffer(k, np.uint8)
        return dict(keys=rows, offsets=None, lens=np.array([len(k) for k in keys], np.uint32), length=None)
    assert all(len(k) == width for k in keys)
    rows = np.full((len(keys), width + (5 if mode == "wide" else 0)), 0xDD, np.uint8)
    for i, k in enumerate(keys):
        rows[i, :width] = np.frombuffer(k, np.uint8)
    return dict(keys=rows, offsets=None, lens=None, length=width if mode == "wide" else None)


class Case:
    """A tree, the keys to look up, how they are addressed, and what the case is about:
    check(results as tuples, report dict) asserts the facts the case was designed for."""

    def __init__(self, tree: Tree, keys, check=None, mode="flat", verify_leaves=True):
        self.tree, self.keys, self.check, self.mode, self.verify_leaves = tree, list(keys), check, mode, verify_leaves


def host_lookup(case: Case, **kw):
    return ks.get_object_ids_host(case.tree.img, *case.tree.args(), **pack(case.keys, case.mode),
                                  verify_leaves=case.verify_leaves, **kw)


def host_trace_message(case: Case):
    """The words of the trace's own entry point for these keys' tags."""
    from storm_amd import trace
    t = case.tree
    tags = tu.tags_u64([o.xxh64(k) for k in case.keys])
    _, rep = trace.trace_host(t.img, t.lay, t.root[:2] + (2,), t.root_type, OBJECTLIST, tags, 0, case.verify_leaves)
    return rep.message


def reference_of(case: Case):
    """The case's reference (results, report, message), once per case and process."""
    if not hasattr(case, "_reference"):
        case._reference = case.tree.reference(case.keys, case.verify_leaves)
    return case._reference


def check_against_reference(case: Case, records, report):
    """records and report (of either leg) against the pure-Python reference, then the case's
    own facts."""
    want, want_rep, message = reference_of(case)
    assert as_tuples(records) == want
    assert report.as_dict() == want_rep
    n = len(case.keys)
    assert report.code == (-5 if want_rep["first_bad"] < n else 0)
    assert report.message == (host_trace_message(case) if message is None else message)
    if case.check:
        case.check(want, want_rep)
    return want, want_rep


# ---- the designed cases ----------------------------------------------------------------------------

EDGE_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 255, 256)


def _flip(k: bytes, i: int) -> bytes:
    return k[:i] + bytes([k[i] ^ 0x5A]) + k[i + 1:]


@functools.lru_cache(maxsize=None)
def edge_lengths() -> Case:
    """Keys of every length at the chunk edges, each present, and its near misses."""
    rng = np.random.default_rng(1)
    A = table(10, 1)
    kt = KeyTree(TEST_LAYOUT, A, depth=2)  # 24 chunks of 9 keys over 100 leaves: no leaf overflows
    present = []
    for n in EDGE_LENGTHS:
        while True:  # a leaf must hold the key's chunks: at most one long key per leaf
            k = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            leaf = kt.leaf(kt.locate(k)[0])
            if leaf.n_used() + (n + 31) // 32 <= 10:
                break
        kt.add(k, 0x1000 + n)
        present.append(k)
    keys = []
    for k in present:
        n = len(k)
        keys += [k, _flip(k, n - 1), _flip(k, 0), _flip(k, n // 2)]  # last, first, a byte of the middle chunk
        keys += [k[:32], k + b"\x01"]  # the 32-byte prefix (the key itself up to 32 bytes); one byte more (257: KEY)
    tree = kt.build()

    def check(res, rep):
        for j, k in enumerate(present):
            own = res[6 * j:6 * j + 6]
            assert own[0][5] == FOUND and own[0][0] == 0x1000 + len(k)
            assert [r[5] for r in own[1:4]] == [ABSENT] * 3  # a changed byte: another tag, nowhere to be found
            assert own[4][5] == (FOUND if len(k) <= 32 else ABSENT)
            assert own[5][5] == (KEY if len(k) == 256 else ABSENT)
        assert rep["first_bad"] == 6 * 8 + 5 and rep["n_status"][KEY] == 1
    return Case(tree, keys, check)


def _one_leaf(seed, C=10, lay=TEST_LAYOUT):
    """A tree of one pointer block; returns (KeyTree, rng)."""
    return KeyTree(lay, table(C, seed), depth=1), np.random.default_rng(seed)


C40_LAYOUT = ScrubLayout(4096, 0, 10, 10, ks.leaf_len(40), 4096)  # room for a 256-byte key and its decoys
DECOY_LENGTHS = (40, 65, 256)


@functools.lru_cache(maxsize=None)
def decoys() -> Case:
    """Earlier in the key's sequence sit Defined items with the key's own reminder and a stored
    key that is longer, shorter, equal up to the last chunk (its last byte changed), and changed
    in its first byte and in a middle chunk; the real item is still found, with the right probes.
    A changed key byte alone changes the tag, so only a planted item makes the chain compare say no."""
    kt, rng = _one_leaf(2, 40, C40_LAYOUT)
    keys, want = [], []
    for slot, n in enumerate(DECOY_LENGTHS):
        k = key_in(kt, (slot,), rng, n)
        path, reminder = kt.locate(k)
        leaf, seq = kt.leaf(path), sequence(40, kt.A, reminder)
        stored = [k[:-1], _flip(k, n - 1), _flip(k, 0), _flip(k, n // 2)] + ([k + b"\x07"] if n < 256 else [])
        for j, d in enumerate(stored):
            leaf.plant(seq[j], d, reminder, 90 + j)
        leaf.plant(seq[len(stored)], k, reminder, 900 + n)
        keys.append(k)
        want.append((900 + n, seq[len(stored)], len(stored) + 1, FOUND))
    tree = kt.build()

    def check(res, rep):
        assert [r[:1] + r[3:] for r in res] == want and rep["n_malformed"] == 0
    return Case(tree, keys, check)


@functools.lru_cache(maxsize=None)
def probe_order() -> Case:
    """The key's item at probe position 1, 2 and C (one leaf each), and a seed that wraps."""
    kt, rng = _one_leaf(3)
    A, keys, want = kt.A, [], []
    for slot, position in ((0, 1), (1, 2), (2, 10)):
        k = key_in(kt, (slot,), rng, 20)
        _, reminder = kt.locate(k)
        leaf, seq = kt.leaf((slot,)), sequence(10, A, reminder)
        for j in range(position - 1):
            leaf.plant(seq[j], None, reminder ^ (j + 1), 50 + j)  # Defined, another reminder
        leaf.plant(seq[position - 1], k, reminder, 700 + position)
        keys.append(k)
        want.append((700 + position, seq[position - 1], position))
    # a seed that wraps: the item sits where A is largest, so seed + A[j] >= C for any seed above 0
    j = int(np.argmax(A))
    k = key_in(kt, (4,), rng, 20, accept=lambda r: r % 10 >= 1)
    _, reminder = kt.locate(k)
    seq = sequence(10, A, reminder)
    assert reminder % 10 + int(A[j]) >= 10
    for i in range(j):
        kt.leaf((4,)).plant(seq[i], None, reminder ^ (i + 1), 60 + i, state=DEFINED if i else INVALID)
    kt.leaf((4,)).plant(seq[j], k, reminder, 777)
    keys.append(k)
    want.append((777, seq[j], j + 1))
    tree = kt.build()

    def check(res, rep):
        assert [(r[0], r[3], r[4]) for r in res] == want and all(r[5] == FOUND for r in res)
        assert rep["probes"] == sum(w[2] for w in want)
    return Case(tree, keys, check)


@functools.lru_cache(maxsize=None)
def invalid_and_free() -> Case:
    """Invalid before Free; Free first; no Free and no match; state bytes 3 and 255 skipped."""
    kt, rng = _one_leaf(4)
    A, keys, want = kt.A, [], []

    def absent_key(slot):
        k = key_in(kt, (slot,), rng, 12)
        keys.append(k)
        return kt.leaf((slot,)), sequence(10, A, kt.locate(k)[1]), kt.locate(k)[1]

    leaf, seq, r = absent_key(0)   # Defined (another key), Invalid, Invalid, then Free
    leaf.plant(seq[0], b"other", r, 1)
    leaf.plant(seq[1], None, r, 2, state=INVALID)
    leaf.plant(seq[2], None, r, 3, state=INVALID)
    want.append((0, seq[1], 4, ABSENT))
    leaf, seq, r = absent_key(1)   # Free first (the leaf holds an item elsewhere)
    leaf.plant(seq[5], b"elsewhere", r ^ 1, 4)
    want.append((0, seq[0], 1, ABSENT))
    leaf, seq, r = absent_key(2)   # no Free and no match: Invalid slots passed do not count
    for j in range(10):
        leaf.plant(seq[j], None, r ^ (j + 1), 5, state=INVALID if j in (2, 6) else DEFINED)
    want.append((0, NO_SLOT, 10, ABSENT))
    leaf, seq, r = absent_key(3)   # 3 and 255 are skipped: neither remembered nor an end
    leaf.plant(seq[0], None, r, 6, state=3)
    leaf.plant(seq[1], None, r, 7, state=255)
    want.append((0, seq[2], 3, ABSENT))
    k = key_in(kt, (4,), rng, 12)  # ... and an item behind them is found
    leaf, seq, r = kt.leaf((4,)), sequence(10, A, kt.locate(k)[1]), kt.locate(k)[1]
    leaf.plant(seq[0], k, r, 8, state=3)
    leaf.plant(seq[1], k, r, 9, state=255)
    leaf.plant(seq[2], k, r, 10)
    keys.append(k)
    want.append((10, seq[2], 3, FOUND))
    tree = kt.build()

    def check(res, rep):
        assert [(r[0], r[3], r[4], r[5]) for r in res] == want
    return Case(tree, keys, check)


MALFORMED = ("chunk pointer C", "chunk pointer 65535", "next pointer C", "remaining 33", "remaining 65535-C", "self chain")


@functools.lru_cache(maxsize=None)
def malformed(name) -> Case:
    """One malformed item earlier in the key's sequence than the real one, in a leaf that is the
    last block of an image with no slack: no match, the probe goes on, n_malformed counts it."""
    kt, rng = _one_leaf(5)
    C = 10
    n = 256 if name == "self chain" else 40
    k = key_in(kt, (9,), rng, 32) * 8 if name == "self chain" else key_in(kt, (9,), rng, n)
    if name == "self chain":  # eight times the same 32 bytes: its leaf and reminder are what they are
        kt = KeyTree(TEST_LAYOUT, kt.A, depth=1)
    path, reminder = kt.locate(k)
    leaf, seq = kt.leaf(path), sequence(C, kt.A, reminder)
    if name == "self chain":
        leaf.plant(seq[0], k[:32], reminder, 66)
        chunk = leaf.chunk_pointer(seq[0])
        leaf.next_pointer(chunk, chunk)       # every step matches 32 bytes and comes back
        found = False                          # 9 chunks are not left for the real item: it is absent
    else:
        leaf.plant(seq[0], k, reminder, 66)
        first = leaf.chunk_pointer(seq[0])
        if name.startswith("chunk pointer"):
            leaf.chunk_pointer(seq[0], C if name.endswith(" C") else 65535)
        elif name == "next pointer C":
            leaf.next_pointer(first, C)        # the first 32 bytes match, then chunk C
        elif name == "remaining 33":
            leaf.next_pointer(leaf.next_pointer(first), C + 33)
        else:
            leaf.next_pointer(leaf.next_pointer(first), 65535)  # remaining 65535 - C
        leaf.plant(seq[1], k, reminder, 67)
        found = True
    tree = kt.build(slack=0)
    assert tree.address_of[path] == tree.lay.n_blocks - 1 and tree.img.size == tree.lay.n_blocks * tree.lay.block_size

    def check(res, rep):
        assert rep["n_malformed"] == 1 and rep["n_probed"] == 1
        assert (res[0][0], res[0][5]) == ((67, FOUND) if found else (0, ABSENT))
        assert res[0][4] == 2
    return Case(tree, [k], check)


@functools.lru_cache(maxsize=None)
def _stored(depth=2, n_keys=120, seed=6):
    """A fan-out 10 tree of `depth` pointer levels with keys of 1..64 bytes; (KeyTree, keys)."""
    rng = np.random.default_rng(seed)
    kt = KeyTree(TEST_LAYOUT, table(10, seed), depth=depth)
    keys = []
    while len(keys) < n_keys:
        k = rng.integers(0, 256, int(rng.integers(1, 65)), dtype=np.uint8).tobytes()
        leaf = kt.leaf(kt.locate(k)[0])
        if leaf.n_used() + (len(k) + 31) // 32 > 7 or sum(leaf.state(i) != FREE for i in range(10)) >= 7 or k in keys:
            continue  # storm would have split this leaf (SplitTrigger): the builder does not; no key twice
        kt.add(k, 1 + len(keys))
        keys.append(k)
    return kt, keys


@functools.lru_cache(maxsize=None)
def _stored_tree(depth=2, n_keys=120, seed=6) -> Tree:
    return _stored(depth, n_keys, seed)[0].build()


def _absent_keys(rng, n):
    return [rng.integers(0, 256, 70, dtype=np.uint8).tobytes() for _ in range(n)]  # longer than any stored key


@functools.lru_cache(maxsize=None)
def free_entry_on_the_path() -> Case:
    """Keys whose digits lead to a Free entry of a pointer block: ABSENT, not probed."""
    kt, stored = _stored()
    rng = np.random.default_rng(7)
    keys = []
    while len(keys) < 5:
        k = rng.integers(0, 256, 9, dtype=np.uint8).tobytes()
        if kt.locate(k)[0] not in kt.leaves:
            keys.append(k)

    def check(res, rep):
        assert all(r[5] == ABSENT and r[4] == 0 and r[3] == NO_SLOT for r in res[:5]) and rep["n_probed"] == 3
    return Case(_stored_tree(), keys + stored[:3], check)


def _damaged(tree: Tree, address, byte):
    img = tree.img.copy()
    img[address * tree.lay.block_size + byte] ^= 0x10
    return Tree(su.frozen(img), tree.lay, tree.root, tree.root_type, tree.C, tree.A, tree.address_of)


@functools.lru_cache(maxsize=None)
def flipped_leaf(verify_leaves=True) -> Case:
    """A flipped byte in one leaf's unused tail: MISMATCH for exactly the keys under it; with the
    leaves unverified those keys are probed and found."""
    kt, stored = _stored()
    tree = _stored_tree()
    victim = kt.locate(stored[0])[0]
    under = [i for i, k in enumerate(stored) if kt.locate(k)[0] == victim]
    bad = _damaged(tree, tree.address_of[victim], 534)  # past FreeChunkIndex: no probe reads it

    def check(res, rep):
        st = [r[5] for r in res]
        if verify_leaves:
            assert [i for i, s in enumerate(st) if s == MISMATCH] == under and rep["first_bad"] == 0
            assert all(s == FOUND for i, s in enumerate(st) if i not in under)
        else:
            assert st == [FOUND] * len(stored) and rep["n_probed"] == len(stored)
            assert rep["trace"]["blocks_hashed"][1] == 0
    return Case(bad, stored, check, verify_leaves=verify_leaves)


@functools.lru_cache(maxsize=None)
def flipped_pointer_block() -> Case:
    """A flipped byte in a mid-level pointer block: MISMATCH for every key under it."""
    kt, stored = _stored()
    tree = _stored_tree()
    victim = kt.locate(stored[1])[0][:1]
    under = [i for i, k in enumerate(stored) if kt.locate(k)[0][:1] == victim]
    bad = _damaged(tree, tree.address_of[victim], 17)  # entry 0's birth revision

    def check(res, rep):
        assert [i for i, r in enumerate(res) if r[5] == MISMATCH] == under
        assert all(res[i][1] == tree.address_of[victim] and res[i][4] == 0 for i in under)
    return Case(bad, stored, check, verify_leaves=False)


@functools.lru_cache(maxsize=None)
def one_key_many_times() -> Case:
    _, stored = _stored()

    def check(res, rep):
        assert rep["trace"]["blocks_hashed"] == (2, 1) and rep["n_status"][FOUND] == 10000 and len(set(res)) == 1
    return Case(_stored_tree(), [stored[5]] * 10000, check)


COUNTS = (0, 1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def count(n) -> Case:
    _, stored = _stored()
    rng = np.random.default_rng(n)
    pool = stored + _absent_keys(rng, 12)

    def check(res, rep):
        assert rep["first_bad"] == n == sum(rep["n_status"])
    return Case(_stored_tree(), [pool[int(i)] for i in rng.integers(0, len(pool), n)], check)


ADDRESSING = ("rows", "wide", "flat", "bad lens")


@functools.lru_cache(maxsize=None)
def addressing(mode) -> Case:
    """Uniform stride with len == stride and len < stride; offsets + lens at odd byte offsets;
    lens holding 0 and 257: KEY, first_bad and storm's message."""
    kt, rng = _one_leaf(8)
    if mode in ("rows", "wide"):
        stored = [key_in(kt, None, rng, 24) for _ in range(30)]
    else:
        stored = [key_in(kt, None, rng, int(rng.integers(1, 60))) for _ in range(30)]
    for i, k in enumerate(stored):
        kt.add(k, 300 + i)
    tree = kt.build()
    if mode in ("rows", "wide"):
        keys = stored + [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in range(70)]

        def check_rows(res, rep):
            assert [r[0] for r in res[:30]] == list(range(300, 330))
        return Case(tree, keys, check_rows, mode=mode)
    if mode == "flat":
        return Case(tree, stored + _absent_keys(rng, 10), None, mode="flat")
    keys = stored[:4] + [rng.integers(0, 256, 257, dtype=np.uint8).tobytes(), stored[4], b"", stored[5]]

    def check(res, rep):
        assert res[4] == res[6] == (0, 0, 0, NO_SLOT, 0, KEY) and rep["first_bad"] == 4 and rep["n_status"][KEY] == 2
        assert rep["trace"]["n_status"][FOUND] + rep["trace"]["n_status"][ABSENT] == 8 and rep["n_probed"] == 6
    return Case(tree, keys, check, mode="rows+lens")


@functools.lru_cache(maxsize=None)
def empty_key_first() -> Case:
    """lens holding 0 before 257: the message is the empty key's."""
    c = addressing("bad lens")
    keys = [c.keys[0], b"", c.keys[4]]

    def check(res, rep):
        assert rep["first_bad"] == 1 and [r[5] for r in res[1:]] == [KEY, KEY]
    return Case(c.tree, keys, check, mode="flat")


@functools.lru_cache(maxsize=None)
def volume() -> Case:
    """20,000 lookups drawn with repetition from about 3,000 stored keys of 1..64 bytes in a
    fan-out 10 tree of depth 3, a tenth of them absent keys."""
    _, stored = _stored(3, 3000, 9)
    rng = np.random.default_rng(10)
    absent = _absent_keys(rng, 500)
    keys = [stored[int(i)] for i in rng.integers(0, len(stored), 20000)]
    for j in rng.integers(0, 20000, 2000):
        keys[int(j)] = absent[int(rng.integers(0, len(absent)))]

    def check(res, rep):
        assert rep["n_status"][FOUND] >= 17000 and rep["n_status"][FOUND] + rep["n_status"][ABSENT] == 20000
    return Case(_stored_tree(3, 3000, 9), keys, check)


@functools.lru_cache(maxsize=None)
def production() -> Case:
    """Production sizes: block 32768, fan-out 1200, C = 600, about 2,000 keys of 48 bytes (and 40
    of 64) in 20 leaves under one pointer block: the table's size, C + 32 = 632 as a u16, long
    probe runs."""
    A = table(600, 11)
    kt = KeyTree(PRODUCTION_LAYOUT, A, depth=1)
    rng = np.random.default_rng(11)
    for slot in range(0, 1200, 60):  # 20 leaves, each with 350 items of another reminder in the way: long probe runs
        for index in rng.permutation(600)[:350]:
            kt.leaf((slot,)).plant(int(index), None, 2 ** 64 - 1, 0)
    stored = []
    while len(stored) < 2000:  # about 100 keys and 200 chunks per leaf
        k = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
        if kt.locate(k)[0] in kt.leaves:
            kt.add(k, 1 + len(stored))
            stored.append(k)
    while len(stored) < 2040:  # 64-byte keys: a full last chunk, whose next pointer is C + 32 = 632
        k = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        if kt.locate(k)[0] in kt.leaves:
            kt.add(k, 1 + len(stored))
            stored.append(k)
    absent = []
    while len(absent) < 200:  # absent keys that reach a leaf and are probed there
        k = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
        if kt.locate(k)[0] in kt.leaves:
            absent.append(k)
    tree = kt.build()

    def check(res, rep):
        assert [r[0] for r in res[:2040]] == list(range(1, 2041)) and rep["n_probed"] == 2240
        assert sum(leaf.next_pointer(c) == 632 for leaf in kt.leaves.values() for c in range(600)) == 40
        assert rep["trace"]["blocks_hashed"] == (1, 20) and max(r[4] for r in res) >= 20
    return Case(tree, stored + absent, check, mode="flat")


# ---- fuzz (tests/test_lookup_fuzz.py, tests/test_lookup_fuzz_gpu.py) -------------------------------

DAMAGED_TREE_SEEDS = 30
DAMAGED_TREE_EDITS = (1, 3, 10)
FUZZ_STREAM = 200  # second word of the rngs' seeds: apart from the scrub's (0..4) and the trace's fuzz


@functools.lru_cache(maxsize=None)
def _stored_index():
    t = _stored_tree()
    return su.reference_scrub(t.img, t.lay, t.root, t.root_type, OBJECTLIST, 0)[2]


def assert_inside(tree: Tree, keys):
    """trace_util.assert_inside for the keys' tags in a key tree, on the host before any upload;
    a probe of any block below n_blocks, leaf or not, stays inside that block."""
    as_traced = tu.Tree(tree.img, tree.lay, tree.root, tree.root_type, OBJECTLIST)
    tu.assert_inside(as_traced, as_traced.reference([o.xxh64(k) for k in keys])[0])
    assert ks.leaf_len(tree.C) <= tree.lay.block_size


@functools.lru_cache(maxsize=None)
def _damaged_tree(seed):
    """(Tree, keys, mode): the stored tree of 120 keys under su.random_damage, resealed; its keys
    shuffled among 20 absent ones and, in odd seeds, one key of length 0 or 257."""
    _, stored = _stored()
    t, index = _stored_tree(), _stored_index()
    rng = np.random.default_rng([seed, FUZZ_STREAM])
    img = t.img.copy()
    keep_bad = su.random_damage(img, t.lay, index, rng, DAMAGED_TREE_EDITS[seed % 3], whole_store=False)
    cs = su.reseal(img, t.lay, index, keep_bad)
    tree = Tree(su.frozen(img), t.lay, (cs, t.root[1]), t.root_type, t.C, t.A, t.address_of)
    keys = stored + _absent_keys(rng, 20)
    keys = [keys[int(i)] for i in rng.permutation(len(keys))]
    if seed % 2:
        bad = rng.integers(0, 256, 257 * int(rng.integers(2)), dtype=np.uint8).tobytes()
        keys.insert(int(rng.integers(len(keys) + 1)), bad)
    assert_inside(tree, keys)
    return tree, keys, "rows+lens" if seed % 2 else "flat"


@functools.lru_cache(maxsize=None)
def damaged_tree_case(seed, verify_leaves=True) -> Case:
    """Lookup on a damaged key tree. Unverified, a re-typed or re-addressed entry hands the probe
    a block that is no objectlist leaf, and a flipped leaf is probed as it is."""
    tree, keys, mode = _damaged_tree(seed)
    return Case(tree, keys, None, mode=mode, verify_leaves=verify_leaves)


LEAF_FUZZ = ((10, range(60)), (40, range(60)), (600, range(4)))  # (C, seeds)
LEAF_FUZZ_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 96, 255, 256)  # both sides of 8 and 32: the compare runs in 8-byte words
LEAF_FUZZ_EDITS = ("state", "reminder", "chunk pointer", "next pointer", "chunk bytes", "defined", "no free slot")
_LEAF_FUZZ_LAYOUTS = {10: TEST_LAYOUT, 40: C40_LAYOUT, 600: PRODUCTION_LAYOUT}


def _edit_leaf(leaf: Leaf, rng, pool, reminders):
    """One random field edit of LEAF_FUZZ_EDITS."""
    C = leaf.C
    pick = lambda values: values[int(rng.integers(len(values)))]  # noqa: E731
    below_C = lambda: int(rng.integers(C))  # noqa: E731
    what = pick(LEAF_FUZZ_EDITS)
    if what == "state":
        leaf.state(below_C(), pick((0, 1, 1, 2, 3, 255)))
    elif what == "reminder":
        leaf.reminder(below_C(), pick(reminders))
    elif what == "chunk pointer":
        leaf.chunk_pointer(below_C(), pick((below_C(), C, C + 1, 65535)))
    elif what == "next pointer":
        chunk = below_C()
        leaf.next_pointer(chunk, pick((below_C(), chunk, C, C + int(rng.integers(1, 33)), C + 32, C + 33, 65535)))
    elif what == "chunk bytes":
        key, chunk = pick(pool), below_C()
        piece = key[32 * int(rng.integers((len(key) + 31) // 32)):][:32]
        leaf.b[32 * chunk:32 * chunk + 32] = piece.ljust(32, b"\0")
    elif what == "defined":
        index = below_C()
        leaf.state(index, DEFINED)
        leaf.reminder(index, pick(reminders))
        leaf.chunk_pointer(index, below_C())
    else:  # every Free state byte becomes another: a probe that finds no match sees all C slots
        for index in range(C):
            if leaf.state(index) == FREE:
                leaf.state(index, pick((DEFINED, INVALID, 3, 255)))


def _leaf_pool(kt: KeyTree, slot, rng):
    """Five different keys of LEAF_FUZZ_LENGTHS that locate in the leaf at (slot,)."""
    pool = []
    while len(pool) < 5:
        n = int(LEAF_FUZZ_LENGTHS[rng.integers(len(LEAF_FUZZ_LENGTHS))])
        if n == 1:  # 256 keys in all: one of those that locate here, if any is left (else another length)
            here = [bytes([b]) for b in range(256) if kt.locate(bytes([b]))[0] == (slot,) and bytes([b]) not in pool]
            pool += [here[int(rng.integers(len(here)))]] if here else []
        else:
            pool.append(key_in(kt, (slot,), rng, n))
    return pool


@functools.lru_cache(maxsize=None)
def _leaf_fuzz(C, seed):
    """(Tree, keys, mode): one pointer block over ten leaves (three at C = 600), each with a pool
    of five keys that locate there, about two thirds of them inserted properly while chunks
    last, then 0..8 random field edits. KeyTree.build hashes the leaves after the edits, so the
    leaves verify and every key is probed."""
    kt = KeyTree(_LEAF_FUZZ_LAYOUTS[C], table(C, seed), depth=1)
    rng = np.random.default_rng([seed, FUZZ_STREAM + C])
    keys = []
    for slot in range(3 if C == 600 else 10):
        leaf = kt.leaf((slot,))
        pool = _leaf_pool(kt, slot, rng)
        for j, k in enumerate(pool):
            if rng.random() < 2 / 3:
                try:
                    kt.add(k, 1000 * slot + j + 1)
                except OverflowError:  # the chunks (or the slots) have run out
                    pass
        reminders = [kt.locate(k)[1] for k in pool]
        for _ in range(int(rng.integers(9))):
            _edit_leaf(leaf, rng, pool, reminders)
        keys += pool
    keys = [keys[int(i)] for i in rng.permutation(len(keys))]
    tree = kt.build()
    assert_inside(tree, keys)
    return tree, keys, "rows+lens" if seed % 2 else "flat"


@functools.lru_cache(maxsize=None)
def leaf_fuzz_case(C, seed, verify_leaves=True) -> Case:
    """Lookup in leaves whose every field may be arbitrary: all pool keys, shuffled."""
    tree, keys, mode = _leaf_fuzz(C, seed)
    return Case(tree, keys, None, mode=mode, verify_leaves=verify_leaves)


def leaf_fuzz_ids():
    return [(C, seed) for C, seeds in LEAF_FUZZ for seed in seeds]


CASES = {"edge lengths": edge_lengths, "decoys": decoys, "probe order": probe_order,
         "invalid and free": invalid_and_free, "free entry on the path": free_entry_on_the_path,
         "flipped leaf": flipped_leaf, "flipped leaf, unverified": lambda: flipped_leaf(False),
         "flipped pointer block": flipped_pointer_block, "one key 10000 times": one_key_many_times,
         "empty key first": empty_key_first, "volume": volume, "production sizes": production}
CASES.update({f"malformed: {m}": functools.partial(malformed, m) for m in MALFORMED})
CASES.update({f"n = {n}": functools.partial(count, n) for n in COUNTS})
CASES.update({f"addressing: {m}": functools.partial(addressing, m) for m in ADDRESSING})
