"""TEST INFRASTRUCTURE for the objects tests (tests/test_objects.py, tests/test_objects_gpu.py,
tests/test_objects_fuzz.py, tests/test_objects_fuzz_gpu.py, tests/test_objects_sanitize.py).

* ``find_object``: findObject (objectstore/objectstore.go:92-123) in literal Python;
* ``reference_objects``: tests/trace_util.reference_trace over the IDs with blob leaves, then the
  status order of include/stormck.h "objects" and ``find_object`` per ID: the reference for every
  result field, every row byte and every report field;
* ``Blob``: a blob.Block of N slots of S-byte objects as bytes, with SetObject's slot choice
  without the split (``set``) and ``plant`` for hand-made slots;
* ``ObjectTree``: objects placed into the leaves of a tree by their ID's digits (no split: a leaf
  that is full raises), laid out with scrub_util.Builder;
* the designed cases both legs run (``CASES``), built once per process;
* the fuzz: ``damaged_tree_case`` (the stored tree under scrub_util.random_damage) and
  ``leaf_fuzz_case`` (leaves whose states and reminders are edited at random), whose leaves
  tests/test_objects_sanitize.py also writes out as a corpus, and ``assert_fuzz_reaches``, the
  condition on these inputs;
* for the spaces tests (tests/test_spaces.py, tests/test_spaces_gpu.py): ``find_space``
  (findSpace, spacestore/spacestore.go:92-121, literally), ``reference_spaces``, ``SpaceList`` (a
  spacelist.Block as bytes) and the designed ``SPACE_CASES``;
* for the get tests (tests/test_get.py, tests/test_get_gpu.py): ``Store`` (a whole store on
  scrub_util.Builder: singularity, space tree, spacelist leaf, a KeyTree and an ObjectTree),
  ``reference_get`` (the singularity's check and the three references chained by hand) and the
  designed ``GET_CASES``.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from storm_amd import keystore as ks
from storm_amd import objectstore as obs
from storm_amd.scrub import BLOB, ScrubLayout
from storm_amd.trace import ABSENT, DEPTH, FOUND, MISMATCH, RANGE, TYPE
from tests import scrub_util as su
from tests import trace_util as tu

FREE, DEFINED, INVALID = 0, 1, 2
NO_SLOT = obs.NO_SLOT
RESULT_FIELDS = ("object_id", "address", "reminder", "index", "probes", "status")
FILL = 0xEE  # what the rows hold before a call: the bytes past object_size must still hold it after


def stride_of(S: int) -> int:
    """unsafe.Sizeof(blob.Object[T]): u64 at 0, T at 8, the State byte at 8 + S, rounded up to 8."""
    return (8 + S + 1 + 7) & ~7


# ---- the probe, literally ------------------------------------------------------------------------

def find_object(b, N, S, reminder):
    """(index, probes, found) of findObject over leaf bytes b; index None: findObject's nil."""
    stride = stride_of(S)
    start, invalid = reminder % N, None
    i = start
    for j in range(N):
        state = b[i * stride + 8 + S]
        if state == DEFINED:
            if struct.unpack_from("<Q", b, i * stride)[0] == reminder:
                return i, j + 1, True
        elif state == INVALID:
            if invalid is None:
                invalid = i
        elif state == FREE:
            return (i if invalid is None else invalid), j + 1, False
        i = (i + 1) % N
    return None, N, False


class Blob:
    """blob.Block (blocks/blob/block.go:25-29) of `blob_len` bytes viewed as N slots of
    blob.Object[T] with unsafe.Sizeof(T) == S."""

    def __init__(self, N: int, S: int, blob_len: int):
        assert N * stride_of(S) <= blob_len - 8
        self.N, self.S, self.stride = N, S, stride_of(S)
        self.b = bytearray(blob_len)

    def reminder(self, k, v=None):
        if v is None:
            return struct.unpack_from("<Q", self.b, k * self.stride)[0]
        struct.pack_into("<Q", self.b, k * self.stride, v)

    def state(self, k, v=None):
        if v is None:
            return self.b[k * self.stride + 8 + self.S]
        self.b[k * self.stride + 8 + self.S] = v

    def object(self, k, v=None):
        off = k * self.stride + 8
        if v is None:
            return bytes(self.b[off:off + self.S])
        assert len(v) == self.S
        self.b[off:off + self.S] = v

    def n_used(self, v=None):
        if v is None:
            return struct.unpack_from("<Q", self.b, len(self.b) - 8)[0]
        struct.pack_into("<Q", self.b, len(self.b) - 8, v)

    def plant(self, k, reminder, obj=None, state=DEFINED):
        """A hand-made slot, whatever the probe sequence would say about it."""
        self.reminder(k, reminder)
        self.state(k, state)
        if obj is not None:
            self.object(k, obj)

    def set(self, reminder, obj) -> int:
        """SetObject without the split (objectstore.go:59-85): the slot findObject hands out."""
        k, _, found = find_object(self.b, self.N, self.S, reminder)
        if k is None:
            raise OverflowError("cannot find slot for object ID")
        self.object(k, obj)
        if not found:
            self.n_used(self.n_used() + 1)
            self.reminder(k, reminder)
            self.state(k, DEFINED)
        return k


def sequence(N, reminder):
    """The slots an ID of that reminder probes, in order."""
    return [(reminder % N + j) % N for j in range(N)]


# ---- the reference -------------------------------------------------------------------------------

def reference_objects(img, lay: ScrubLayout, root, root_type, N, S, ids, verify_leaves=True):
    """(results, rows, report, message): results[i] = RESULT_FIELDS of ids[i]; rows[i] = the S
    bytes of its row; message is "" when no ID ends badly, else None (the trace's words: compare
    with the trace's own entry point)."""
    tres, trep, _, _ = tu.reference_trace(img, lay, root, root_type, BLOB, ids, 0, verify_leaves)
    view = memoryview(np.ascontiguousarray(img).view(np.uint8).reshape(-1))
    results, rows, n_probed, probes = [], [], 0, 0
    for oid, (address, reminder, _, _, _, status) in zip(ids, tres):
        row = bytes(S)
        if status != FOUND:
            results.append((oid, address, reminder, NO_SLOT, 0, status))
        else:
            leaf = view[address * lay.block_size:address * lay.block_size + lay.blob_len]
            index, p, found = find_object(leaf, N, S, reminder)
            results.append((oid, address, reminder, NO_SLOT if index is None else index, p, FOUND if found else ABSENT))
            n_probed, probes = n_probed + 1, probes + p
            if found:
                row = bytes(leaf[index * stride_of(S) + 8:index * stride_of(S) + 8 + S])
        rows.append(row)
    n = len(ids)
    n_status = [0] * 8
    for r in results:
        n_status[r[5]] += 1
    first_bad = min((i for i, r in enumerate(results) if r[5] in obs.BAD), default=n)
    report = dict(n_status=tuple(n_status), n_probed=n_probed, probes=probes, first_bad=first_bad, trace=trep)
    return results, rows, report, "" if first_bad == n else None


def as_tuples(records):
    return [tuple(int(rec[f]) for f in RESULT_FIELDS) for rec in records]


# ---- trees of objects ----------------------------------------------------------------------------

TEST_LAYOUT = ScrubLayout(1024, 0, 10, 10, 536, 728)                 # storm's -tags test sizes
MID_LAYOUT = ScrubLayout(4096, 0, 10, 10, 536, 4096)                 # room for objects of 1024 and 4000 bytes
PRODUCTION_LAYOUT = ScrubLayout(32768, 0, 1200, 400, 31808, 32768)


class Tree:
    """An image and the arguments that get objects from one object tree of it."""

    def __init__(self, img, lay, root, root_type, N, S, address_of=None):
        self.img, self.lay, self.root, self.root_type = img, lay, tuple(root), root_type
        self.N, self.S = N, S
        self.params = obs.BlobParams(N, S)
        self.address_of = address_of or {}  # path (tuple of slots) -> block address

    def args(self):
        return self.lay, self.root[:2] + (2,), self.root_type, self.params

    def reference(self, ids, verify_leaves=True):
        return reference_objects(self.img, self.lay, self.root, self.root_type, self.N, self.S, ids, verify_leaves)


def with_blob_len(lay: ScrubLayout, blob_len: int) -> ScrubLayout:
    return ScrubLayout(lay.block_size, lay.n_blocks, lay.pointer_fanout, lay.spaces_per_block, lay.objectlist_len, blob_len)


class ObjectTree:
    """Objects in the blob leaves of a tree of `depth` pointer levels, by their ID's digits
    (cache/trace.go:38-40): the leaf at path (id % F, id // F % F, ...), reminder id // F^depth."""

    def __init__(self, lay: ScrubLayout, N: int, S: int, depth: int = 1):
        self.lay, self.N, self.S, self.depth = lay, N, S, depth
        self.leaves = {}

    def locate(self, oid: int):
        """(path, reminder) of the ID."""
        path = []
        for _ in range(self.depth):
            path.append(oid % self.lay.pointer_fanout)
            oid //= self.lay.pointer_fanout
        return tuple(path), oid

    def id_of(self, path, reminder: int) -> int:
        """The ID that lives in the leaf at `path` with that reminder."""
        F = self.lay.pointer_fanout
        oid = reminder * F ** self.depth + sum(s * F ** k for k, s in enumerate(path))
        assert oid < 2 ** 64 and self.locate(oid) == (tuple(path), reminder)
        return oid

    def leaf(self, path) -> Blob:
        return self.leaves.setdefault(tuple(path), Blob(self.N, self.S, self.lay.blob_len))

    def set(self, oid: int, obj: bytes) -> int:
        path, reminder = self.locate(oid)
        return self.leaf(path).set(reminder, obj)

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
            return Tree(su.frozen(img), lay, (0, 0), su.FREE_T, self.N, self.S)
        return Tree(su.frozen(img), lay, root[:2], root[2], self.N, self.S, address)


def payload(rng, S) -> bytes:
    """An object's bytes: none of them 0 or FILL, so a row that was not written, or was zeroed,
    cannot pass for it."""
    return bytes(int(v) for v in rng.integers(1, FILL, S))


class Case:
    """A tree, the IDs to get, how they are addressed (id_stride 8: a dense u64 array; 32: the
    object_id fields of a lookup result array), the rows' stride (None: object_size;
    want_objects False: no rows at all) and what the case is about: check(results as tuples,
    rows, report dict) asserts the facts the case was designed for."""

    def __init__(self, tree: Tree, ids, check=None, id_stride=8, out_stride=None, want_objects=True, verify_leaves=True):
        self.tree, self.ids, self.check = tree, [int(i) for i in ids], check
        self.id_stride, self.want_objects, self.verify_leaves = id_stride, want_objects, verify_leaves
        self.out_stride = tree.S if out_stride is None else out_stride


def ids_array(case: Case) -> np.ndarray:
    if case.id_stride == 8:
        return np.array(case.ids, dtype=np.uint64)
    assert case.id_stride == 32
    rec = np.zeros(len(case.ids), dtype=ks.RESULT_DTYPE)  # a lookup's results: every other field is in the way
    rec["address"], rec["reminder"], rec["index"], rec["probes"] = 0xA1A1A1A1A1A1A1A1, 0xB2B2B2B2B2B2B2B2, 0xC3C3C3C3, 0xD4D4
    rec["object_id"] = np.array(case.ids, dtype=np.uint64)
    return rec


def dirty_rows(case: Case):
    return np.full((len(case.ids), case.out_stride), FILL, dtype=np.uint8) if case.want_objects else None


def host_objects(case: Case, **kw):
    return obs.get_objects_host(case.tree.img, *case.tree.args(), ids_array(case), verify_leaves=case.verify_leaves,
                                want_objects=case.want_objects, out_stride=case.out_stride, objects=dirty_rows(case), **kw)


def host_trace_message(case: Case):
    """The words of the trace's own entry point for these IDs."""
    from storm_amd import trace
    t = case.tree
    _, rep = trace.trace_host(t.img, t.lay, t.root[:2] + (2,), t.root_type, BLOB, tu.tags_u64(case.ids), 0,
                              case.verify_leaves)
    return rep.message


def reference_of(case: Case):
    """The case's reference (results, rows, report, message), once per case and process."""
    if not hasattr(case, "_reference"):
        case._reference = case.tree.reference(case.ids, case.verify_leaves)
    return case._reference


def expected_rows(case: Case) -> bytes:
    """Every byte of the rows array after the call: the object or zeros, then the untouched gap."""
    gap = bytes([FILL]) * (case.out_stride - case.tree.S)
    return b"".join(row + gap for row in reference_of(case)[1])


def check_against_reference(case: Case, records, objects, report):
    """records, rows and report (of either leg) against the pure-Python reference, then the
    case's own facts."""
    want, rows, want_rep, message = reference_of(case)
    assert as_tuples(records) == want
    assert not records["reserved"].any()
    if case.want_objects:
        assert objects.tobytes() == expected_rows(case)
    else:
        assert objects is None
    assert report.as_dict() == want_rep
    n = len(case.ids)
    assert report.code == (-5 if want_rep["first_bad"] < n else 0)
    assert report.message == (host_trace_message(case) if message is None else message)
    if case.check:
        case.check(want, rows, want_rep)
    return want, want_rep


# ---- the designed cases ----------------------------------------------------------------------------

# (S, layout, blob_len or None: the layout's, N): N * stride reaches blob_len - 8 exactly at
# S = 1, 8, 13, 24 (720 bytes of Data), 1024 and 4000 (a blob_len made for it)
SIZES = {1: (TEST_LAYOUT, None, 45), 7: (TEST_LAYOUT, None, 44), 8: (TEST_LAYOUT, None, 30), 9: (TEST_LAYOUT, None, 29),
         13: (TEST_LAYOUT, None, 30), 16: (TEST_LAYOUT, None, 22), 24: (TEST_LAYOUT, None, 18),
         100: (TEST_LAYOUT, None, 6), 1024: (MID_LAYOUT, 3 * 1040 + 8, 3), 4000: (MID_LAYOUT, 4016 + 8, 1)}


def size_layout(S):
    lay, blob_len, N = SIZES[S]
    return (lay if blob_len is None else with_blob_len(lay, blob_len)), N


@functools.lru_cache(maxsize=None)
def size(S) -> Case:
    """Objects of S bytes in three leaves filled to three quarters, each got back, among IDs that
    are absent from their leaf and IDs whose path ends at a Free entry; rows wider than S."""
    lay, N = size_layout(S)
    exact = N * stride_of(S) == lay.blob_len - 8
    rng = np.random.default_rng(100 + S)
    ot = ObjectTree(lay, N, S, depth=1)
    stored = {}
    for slot in (0, 3, 9):
        for _ in range(max(1, 3 * N // 4)):
            oid = ot.id_of((slot,), int(rng.integers(1, 2 ** 40)))
            stored[oid] = payload(rng, S)
            ot.set(oid, stored[oid])
    absent = [ot.id_of((slot,), int(rng.integers(2 ** 40, 2 ** 41))) for slot in (0, 3, 9, 5, 5)]
    ids = list(stored) + absent
    ids = [ids[int(i)] for i in rng.permutation(len(ids))]
    tree = ot.build()

    def check(res, rows, rep):
        assert exact == (S in (1, 8, 13, 24, 1024, 4000))
        for oid, r, row in zip(ids, res, rows):
            assert (r[5] == FOUND and row == stored[oid]) if oid in stored else (r[5] == ABSENT and row == bytes(S))
        assert rep["n_status"][FOUND] == len(stored) and rep["n_probed"] == len(stored) + 3
    return Case(tree, ids, check, out_stride=S + 3 if S % 2 else S + 8)


def _one_level(seed, N=10, S=8, lay=TEST_LAYOUT):
    return ObjectTree(lay, N, S, depth=1), np.random.default_rng(seed)


@functools.lru_cache(maxsize=None)
def probe_order() -> Case:
    """The ID's slot at probe position 1, 2 and N behind Defined slots of other reminders (one
    leaf each), and a start slot of N - 1, so that the probe wraps."""
    ot, rng = _one_level(3)
    ids, want, objs = [], [], []
    for slot, position, reminder in ((0, 1, 1234567), (1, 2, 98765), (2, 10, 55555), (4, 3, 10 * 777 + 9)):
        seq = sequence(10, reminder)
        leaf = ot.leaf((slot,))
        for j in range(position - 1):
            leaf.plant(seq[j], reminder ^ (j + 1) << 8, payload(rng, 8))  # Defined, another reminder
        objs.append(payload(rng, 8))
        leaf.plant(seq[position - 1], reminder, objs[-1])
        ids.append(ot.id_of((slot,), reminder))
        want.append((seq[position - 1], position, FOUND))
    assert want[3][0] == 1 and sequence(10, 10 * 777 + 9)[0] == 9  # N - 1, 0, 1
    tree = ot.build()

    def check(res, rows, rep):
        assert [r[3:] for r in res] == want and rows == objs and rep["probes"] == 1 + 2 + 10 + 3
    return Case(tree, ids, check)


@functools.lru_cache(maxsize=None)
def invalid_and_free() -> Case:
    """Invalid before Free; Free first; no Free and no match; state bytes 3 and 255 skipped; a
    Defined match behind an Invalid slot; a match whose state byte is Invalid, 3 or Free."""
    ot, rng = _one_level(4)
    ids, want = [], []

    def an_id(slot):
        reminder = int(rng.integers(1, 2 ** 50))
        ids.append(ot.id_of((slot,), reminder))
        return ot.leaf((slot,)), sequence(10, reminder), reminder

    leaf, seq, r = an_id(0)   # Defined (another reminder), Invalid, Invalid, then Free
    leaf.plant(seq[0], r + 10, payload(rng, 8))
    leaf.plant(seq[1], r, payload(rng, 8), state=INVALID)   # its own reminder, but Invalid: no match
    leaf.plant(seq[2], r + 20, payload(rng, 8), state=INVALID)
    want.append((seq[1], 4, ABSENT))
    leaf, seq, r = an_id(1)   # Free first (the leaf holds an object elsewhere)
    leaf.plant(seq[5], r + 10, payload(rng, 8))
    want.append((seq[0], 1, ABSENT))
    leaf, seq, r = an_id(2)   # no Free and no match: the Invalid slots passed do not count
    for j in range(10):
        leaf.plant(seq[j], r + 10 * (j + 1), payload(rng, 8), state=INVALID if j in (2, 6) else DEFINED)
    want.append((NO_SLOT, 10, ABSENT))
    leaf, seq, r = an_id(3)   # 3 and 255 are skipped: neither remembered nor an end
    leaf.plant(seq[0], r, payload(rng, 8), state=3)
    leaf.plant(seq[1], r, payload(rng, 8), state=255)
    want.append((seq[2], 3, ABSENT))
    leaf, seq, r = an_id(4)   # a Defined match behind an Invalid slot and a skipped one
    leaf.plant(seq[0], r, payload(rng, 8), state=INVALID)
    leaf.plant(seq[1], r, payload(rng, 8), state=255)
    behind = payload(rng, 8)
    leaf.plant(seq[2], r, behind)
    want.append((seq[2], 3, FOUND))
    leaf, seq, r = an_id(5)   # a Free slot that holds the reminder and bytes: absent, and its row is zeros
    leaf.plant(seq[0], r, payload(rng, 8), state=FREE)
    want.append((seq[0], 1, ABSENT))
    tree = ot.build()

    def check(res, rows, rep):
        assert [r[3:] for r in res] == want
        assert rows == [bytes(8)] * 4 + [behind] + [bytes(8)]
    return Case(tree, ids, check, out_stride=16)


@functools.lru_cache(maxsize=None)
def _stored(depth=2, n_objects=120, seed=6, N=10, S=13):
    """A fan-out 10 tree of `depth` pointer levels with objects of S bytes; (ObjectTree, {id: object})."""
    rng = np.random.default_rng(seed)
    ot = ObjectTree(TEST_LAYOUT, N, S, depth=depth)
    stored = {}
    while len(stored) < n_objects:
        oid = int(rng.integers(1, 2 ** 63))
        leaf = ot.leaf(ot.locate(oid)[0])
        if leaf.n_used() >= 3 * N // 4 or oid in stored:
            continue  # storm would have split this leaf (objectstore.go:62): the builder does not
        stored[oid] = payload(rng, S)
        ot.set(oid, stored[oid])
    return ot, stored


@functools.lru_cache(maxsize=None)
def _stored_tree(depth=2, n_objects=120, seed=6) -> Tree:
    return _stored(depth, n_objects, seed)[0].build()


def _absent_ids(rng, n):
    return [int(v) for v in rng.integers(2 ** 63, 2 ** 64 - 1, n, dtype=np.uint64)]  # the stored IDs are below 2^63


@functools.lru_cache(maxsize=None)
def free_entry_on_the_path() -> Case:
    """IDs whose digits lead to a Free entry of a pointer block: ABSENT, not probed, rows zeroed."""
    ot, stored = _stored()
    rng = np.random.default_rng(7)
    ids = []
    while len(ids) < 5:
        oid = int(rng.integers(1, 2 ** 63))
        if ot.locate(oid)[0] not in ot.leaves:
            ids.append(oid)

    def check(res, rows, rep):
        assert all(r[5] == ABSENT and r[4] == 0 and r[3] == NO_SLOT for r in res[:5]) and rep["n_probed"] == 3
        assert rows[:5] == [bytes(13)] * 5
    return Case(_stored_tree(), ids + list(stored)[:3], check)


def _damaged(tree: Tree, address, byte):
    img = tree.img.copy()
    img[address * tree.lay.block_size + byte] ^= 0x10
    return Tree(su.frozen(img), tree.lay, tree.root, tree.root_type, tree.N, tree.S, tree.address_of)


@functools.lru_cache(maxsize=None)
def flipped_leaf(verify_leaves=True) -> Case:
    """A flipped byte in one leaf's NUsedSlots: MISMATCH for exactly the IDs under it, rows
    zeroed; with the leaves unverified those IDs are probed and their objects returned."""
    ot, stored = _stored()
    tree = _stored_tree()
    ids = list(stored)
    victim = ot.locate(ids[0])[0]
    under = [i for i, oid in enumerate(ids) if ot.locate(oid)[0] == victim]
    bad = _damaged(tree, tree.address_of[victim], 727)  # NUsedSlots: no probe reads it

    def check(res, rows, rep):
        st = [r[5] for r in res]
        if verify_leaves:
            assert [i for i, s in enumerate(st) if s == MISMATCH] == under and rep["first_bad"] == 0
            assert all(s == FOUND for i, s in enumerate(st) if i not in under)
            assert all(rows[i] == (bytes(13) if i in under else stored[ids[i]]) for i in range(len(ids)))
        else:
            assert st == [FOUND] * len(ids) and rep["n_probed"] == len(ids) and rows == list(stored.values())
            assert rep["trace"]["blocks_hashed"][1] == 0
    return Case(bad, ids, check, verify_leaves=verify_leaves, out_stride=16)


@functools.lru_cache(maxsize=None)
def flipped_pointer_block() -> Case:
    """A flipped byte in a mid-level pointer block: MISMATCH for every ID under it."""
    ot, stored = _stored()
    tree = _stored_tree()
    ids = list(stored)
    victim = ot.locate(ids[1])[0][:1]
    under = [i for i, oid in enumerate(ids) if ot.locate(oid)[0][:1] == victim]
    bad = _damaged(tree, tree.address_of[victim], 17)  # entry 0's birth revision

    def check(res, rows, rep):
        assert [i for i, r in enumerate(res) if r[5] == MISMATCH] == under
        assert all(res[i][1] == tree.address_of[victim] and res[i][4] == 0 and rows[i] == bytes(13) for i in under)
    return Case(bad, ids, check, verify_leaves=False)


@functools.lru_cache(maxsize=None)
def one_id_many_times() -> Case:
    _, stored = _stored()
    oid = list(stored)[5]

    def check(res, rows, rep):
        assert rep["trace"]["blocks_hashed"] == (2, 1) and rep["n_status"][FOUND] == 10000
        assert len(set(res)) == 1 and set(rows) == {stored[oid]}
    return Case(_stored_tree(), [oid] * 10000, check)


COUNTS = (0, 1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def count(n) -> Case:
    _, stored = _stored()
    rng = np.random.default_rng(n)
    pool = list(stored) + _absent_ids(rng, 12)

    def check(res, rows, rep):
        assert rep["first_bad"] == n == sum(rep["n_status"])
    return Case(_stored_tree(), [pool[int(i)] for i in rng.integers(0, len(pool), n)], check, out_stride=13 + n % 4)


@functools.lru_cache(maxsize=None)
def no_rows() -> Case:
    """objects == NULL: only the results are written."""
    c = count(257)
    return Case(c.tree, c.ids, None, want_objects=False)


@functools.lru_cache(maxsize=None)
def lookup_results_in_place() -> Case:
    """id_stride 32: the IDs are the object_id fields of a lookup result array."""
    c = count(257)
    return Case(c.tree, c.ids, None, id_stride=32, out_stride=16)


@functools.lru_cache(maxsize=None)
def last_block() -> Case:
    """The leaf is the last block of an image with no slack, N * stride reaches blob_len - 8 and
    the object sits in slot N - 1: the last Data bytes of the image that a probe may read."""
    ot, rng = _one_level(12, N=30, S=8)
    obj = payload(rng, 8)
    ot.leaf((9,)).plant(29, 30 * 5 + 29, obj)
    tree = ot.build(slack=0)
    assert tree.address_of[(9,)] == tree.lay.n_blocks - 1 and tree.img.size == tree.lay.n_blocks * tree.lay.block_size

    def check(res, rows, rep):
        assert res[0][3:] == (29, 1, FOUND) and rows[0] == obj and res[1][3:] == (0, 2, ABSENT)
    return Case(tree, [ot.id_of((9,), 30 * 5 + 29), ot.id_of((9,), 30 * 7 + 29)], check)


@functools.lru_cache(maxsize=None)
def too_deep() -> Case:
    """65 pointer blocks over one leaf: DEPTH, the one bad status no damage can make."""
    t = tu.chain(65)

    def check(res, rows, rep):
        assert [r[5] for r in res] == [DEPTH] * 3 and rep["first_bad"] == 0 and rows == [bytes(8)] * 3
    return Case(Tree(t.img, t.lay, t.root, t.root_type, 10, 8), [0, 0, 0], check)


@functools.lru_cache(maxsize=None)
def volume() -> Case:
    """20,000 IDs drawn with repetition from about 3,000 stored objects of 13 bytes in a fan-out 10
    tree of depth 3, a tenth of them absent IDs."""
    _, stored = _stored(3, 3000, 9)
    rng = np.random.default_rng(10)
    absent = _absent_ids(rng, 500)
    pool = list(stored)
    ids = [pool[int(i)] for i in rng.integers(0, len(pool), 20000)]
    for j in rng.integers(0, 20000, 2000):
        ids[int(j)] = absent[int(rng.integers(len(absent)))]

    def check(res, rows, rep):
        assert rep["n_status"][FOUND] >= 17000 and rep["n_status"][FOUND] + rep["n_status"][ABSENT] == 20000
    return Case(_stored_tree(3, 3000, 9), ids, check)


PRODUCTION = {"N = 100, S = 8": (100, 8), "N = 31, S = 1024": (31, 1024)}


@functools.lru_cache(maxsize=None)
def production(name) -> Case:
    """Production sizes: block 32768, fan-out 1200, 20 leaves under one pointer block, each filled
    to 70 % with sequential object IDs as storm hands them out, and long runs to probe past."""
    N, S = PRODUCTION[name]
    ot = ObjectTree(PRODUCTION_LAYOUT, N, S, depth=1)
    rng = np.random.default_rng(11 + N)
    stored = {}
    slots = list(range(0, 1200, 60))
    for r in range(7 * N // 10):  # five IDs per start slot, the start slots three apart: runs to probe past
        for slot in slots:
            oid = ot.id_of((slot,), 3 * (r // 5) % N + N * (r + 1))
            stored[oid] = payload(rng, S)
            ot.set(oid, stored[oid])
    absent = [ot.id_of((slot,), N * 10 ** 6 + k) for slot in slots for k in range(5)]
    ids = list(stored) + absent
    tree = ot.build()

    def check(res, rows, rep):
        assert rows[:len(stored)] == list(stored.values()) and rep["n_probed"] == len(ids)
        assert rep["trace"]["blocks_hashed"] == (1, 20) and max(r[4] for r in res) >= 5
    return Case(tree, ids, check)


CASES = {"probe order": probe_order, "invalid and free": invalid_and_free,
         "free entry on the path": free_entry_on_the_path, "flipped leaf": flipped_leaf,
         "flipped leaf, unverified": lambda: flipped_leaf(False), "flipped pointer block": flipped_pointer_block,
         "one ID 10000 times": one_id_many_times, "no rows": no_rows, "id stride 32": lookup_results_in_place,
         "last block": last_block, "too deep": too_deep, "volume": volume}
CASES.update({f"S = {S}": functools.partial(size, S) for S in SIZES})
CASES.update({f"n = {n}": functools.partial(count, n) for n in COUNTS})
CASES.update({f"production: {p}": functools.partial(production, p) for p in PRODUCTION})


# ---- fuzz ------------------------------------------------------------------------------------------

DAMAGED_TREE_SEEDS = 30
DAMAGED_TREE_EDITS = (1, 3, 10)
FUZZ_STREAM = 300  # second word of the rngs' seeds: apart from the scrub's, the trace's and the lookup's fuzz


@functools.lru_cache(maxsize=None)
def _stored_index():
    t = _stored_tree()
    return su.reference_scrub(t.img, t.lay, t.root, t.root_type, BLOB, 0)[2]


def assert_inside(tree: Tree, ids):
    """trace_util.assert_inside for the IDs in an object tree, on the host before any upload; a
    probe of any block below n_blocks, leaf or not, stays inside the first blob_len bytes of it."""
    as_traced = tu.Tree(tree.img, tree.lay, tree.root, tree.root_type, BLOB)
    tu.assert_inside(as_traced, as_traced.reference(ids)[0])
    assert tree.N * stride_of(tree.S) + 8 <= tree.lay.blob_len <= tree.lay.block_size


@functools.lru_cache(maxsize=None)
def _damaged_tree(seed):
    """(Tree, ids): the stored tree of 120 objects under su.random_damage, resealed; its IDs
    shuffled among 20 absent ones."""
    _, stored = _stored()
    t, index = _stored_tree(), _stored_index()
    rng = np.random.default_rng([seed, FUZZ_STREAM])
    img = t.img.copy()
    keep_bad = su.random_damage(img, t.lay, index, rng, DAMAGED_TREE_EDITS[seed % 3], whole_store=False)
    cs = su.reseal(img, t.lay, index, keep_bad)
    tree = Tree(su.frozen(img), t.lay, (cs, t.root[1]), t.root_type, t.N, t.S, t.address_of)
    ids = list(stored) + _absent_ids(rng, 20)
    ids = [ids[int(i)] for i in rng.permutation(len(ids))]
    assert_inside(tree, ids)
    return tree, ids


@functools.lru_cache(maxsize=None)
def damaged_tree_case(seed, verify_leaves=True) -> Case:
    """Objects from a damaged tree. Unverified, a re-typed or re-addressed entry hands the probe
    a block that is no blob leaf, and a flipped leaf is probed and read as it is."""
    tree, ids = _damaged_tree(seed)
    return Case(tree, ids, None, id_stride=32 if seed % 2 else 8, out_stride=13 + seed % 4, verify_leaves=verify_leaves)


LEAF_FUZZ = ((10, 8, range(40)), (30, 13, range(40)), (100, 8, range(4)))  # (N, S, seeds)
LEAF_FUZZ_EDITS = ("state", "reminder", "defined", "no free slot")
LEAF_FUZZ_POOL = 7   # IDs per leaf: 70 per case, more than a wave
_LEAF_FUZZ_LAYOUTS = {10: TEST_LAYOUT, 30: TEST_LAYOUT, 100: PRODUCTION_LAYOUT}


def _edit_leaf(leaf: Blob, rng, reminders):
    """One random edit of LEAF_FUZZ_EDITS."""
    pick = lambda values: values[int(rng.integers(len(values)))]  # noqa: E731
    k = int(rng.integers(leaf.N))
    what = pick(LEAF_FUZZ_EDITS)
    if what == "state":
        leaf.state(k, pick((0, 1, 1, 2, 3, 255)))
    elif what == "reminder":
        leaf.reminder(k, pick(reminders))
    elif what == "defined":
        leaf.plant(k, pick(reminders))
    else:  # every Free state byte becomes another: a probe that finds no match sees all N slots
        for j in range(leaf.N):
            if leaf.state(j) == FREE:
                leaf.state(j, pick((DEFINED, INVALID, 3, 255)))


@functools.lru_cache(maxsize=None)
def _leaf_fuzz(N, S, seed):
    """(Tree, ids): one pointer block over ten leaves (three at N = 100), each with a pool of
    seven IDs that locate there, about two thirds of them set properly, then 0..8 random edits of
    states and reminders. In every eighth seed the IDs asked for are others, of reminders no slot
    holds: a batch of more than a wave in which nothing is found. ObjectTree.build hashes the
    leaves after the edits, so the leaves verify and every ID is probed."""
    ot = ObjectTree(_LEAF_FUZZ_LAYOUTS[N], N, S, depth=1)
    rng = np.random.default_rng([seed, FUZZ_STREAM + N])
    ids = []
    for slot in range(3 if N == 100 else 10):
        leaf = ot.leaf((slot,))
        reminders = [int(rng.integers(0, 2 ** 48)) for _ in range(LEAF_FUZZ_POOL)]
        for r in reminders:
            if rng.random() < 2 / 3 and leaf.n_used() < N:
                try:
                    leaf.set(r, payload(rng, S))
                except OverflowError:  # no slot left to hand out
                    pass
        for _ in range(int(rng.integers(9))):
            _edit_leaf(leaf, rng, reminders)
        if seed % 8 == 7:
            reminders = [r + 2 ** 50 for r in reminders]
        ids += [ot.id_of((slot,), r) for r in reminders]
    ids = [ids[int(i)] for i in rng.permutation(len(ids))]
    tree = ot.build()
    assert_inside(tree, ids)
    return tree, ids


@functools.lru_cache(maxsize=None)
def leaf_fuzz_case(N, S, seed, verify_leaves=True) -> Case:
    """Objects from leaves whose states and reminders may be arbitrary: all pool IDs, shuffled."""
    tree, ids = _leaf_fuzz(N, S, seed)
    return Case(tree, ids, None, id_stride=32 if seed % 2 else 8, out_stride=S + seed % 5, verify_leaves=verify_leaves)


def leaf_fuzz_ids():
    return [(N, S, seed) for N, S, seeds in LEAF_FUZZ for seed in seeds]


def assert_fuzz_reaches():
    """The condition on the fuzz inputs, from the Python reference alone: across the seeds every
    status a damaged tree can end with occurs (DEPTH needs 64 verified pointer blocks on one walk
    and a cycle never verifies: CASES["too deep"] has it), both forms of ABSENT after a probe (a
    slot handed out, and NO_SLOT after N probes), and a batch of at least a wave in which no ID
    is FOUND."""
    seen, handed_out, no_slot, nothing_found = set(), 0, 0, 0
    for seed in range(DAMAGED_TREE_SEEDS):
        for verify in (True, False):
            res, _, rep, _ = reference_of(damaged_tree_case(seed, verify))
            seen |= {r[5] for r in res}
    for N, S, seed in leaf_fuzz_ids():
        res, _, rep, _ = reference_of(leaf_fuzz_case(N, S, seed))
        assert rep["n_probed"] == len(res)  # the leaves verify: every ID is probed
        seen |= {r[5] for r in res}
        handed_out += sum(1 for r in res if r[5] == ABSENT and r[3] != NO_SLOT and r[4] > 0)
        no_slot += sum(1 for r in res if r[5] == ABSENT and r[3] == NO_SLOT and r[4] == N)
        nothing_found += len(res) >= 64 and rep["n_status"][FOUND] == 0
    assert seen == {FOUND, MISMATCH, RANGE, TYPE, ABSENT}, seen
    assert handed_out >= 100 and no_slot >= 10 and nothing_found >= 5, (handed_out, no_slot, nothing_found)


# ---- spaces (tests/test_spaces.py, tests/test_spaces_gpu.py) ---------------------------------------

SPACE_FIELDS = ("key_root", "object_root", "next_object_id", "address", "reminder", "index", "probes", "key_type",
                "object_type", "status")


def space_table(S: int, seed: int = 0) -> np.ndarray:
    """An addressing table for spaces: a seeded permutation of 0..S-1."""
    return np.random.default_rng(2000 + seed).permutation(S).astype(np.uint16)


def find_space(b, S, A, reminder):
    """(index, probes, found) of findSpace (spacestore/spacestore.go:92-121) over leaf bytes b;
    index None: findSpace's nil."""
    seed, invalid = reminder % S, None
    for i in range(S):
        index = (seed + int(A[i])) % S
        state = b[72 * index + 66]
        if state == DEFINED:
            if struct.unpack_from("<Q", b, 72 * index)[0] == reminder:
                return index, i + 1, True
        elif state == INVALID:
            if invalid is None:
                invalid = index
        elif state == FREE:
            return (index if invalid is None else invalid), i + 1, False
    return None, S, False


def space_sequence(S, A, reminder):
    return [(reminder % S + int(A[i])) % S for i in range(S)]


class SpaceList:
    """spacelist.Block of S spaces (blocks/spacelist/block.go:21-36) as its bytes."""

    def __init__(self, S: int):
        self.S = S
        self.b = bytearray((72 * S + 2 + 7) & ~7)

    def plant(self, k, reminder, state=DEFINED, key=(0, 0, 0, 0), obj=(0, 0, 0, 0), next_object_id=0):
        """Space k by hand; key and obj are (checksum, address, birth revision, block type)."""
        struct.pack_into("<QQ", self.b, 72 * k, reminder, next_object_id)
        struct.pack_into("<QQQ", self.b, 72 * k + 16, *key[:3])
        struct.pack_into("<QQQ", self.b, 72 * k + 40, *obj[:3])
        self.b[72 * k + 64], self.b[72 * k + 65], self.b[72 * k + 66] = key[3], obj[3], state


def reference_spaces(img, lay: ScrubLayout, root, root_type, A, ids, verify_leaves=True):
    """(results, report, message): results[i] = SPACE_FIELDS of ids[i], the roots as (checksum,
    address, birth revision); message as in reference_objects."""
    from storm_amd.scrub import SPACELIST
    S = lay.spaces_per_block
    tres, trep, _, _ = tu.reference_trace(img, lay, root, root_type, SPACELIST, ids, 0, verify_leaves)
    view = memoryview(np.ascontiguousarray(img).view(np.uint8).reshape(-1))
    results, n_probed, probes = [], 0, 0
    zero = (0, 0, 0)
    for address, reminder, _, _, _, status in tres:
        if status != FOUND:
            results.append((zero, zero, 0, address, reminder, NO_SLOT, 0, 0, 0, status))
            continue
        leaf = view[address * lay.block_size:address * lay.block_size + ((72 * S + 2 + 7) & ~7)]
        index, p, found = find_space(leaf, S, A, reminder)
        n_probed, probes = n_probed + 1, probes + p
        if not found:
            results.append((zero, zero, 0, address, reminder, NO_SLOT if index is None else index, p, 0, 0, ABSENT))
            continue
        _, next_id = struct.unpack_from("<QQ", leaf, 72 * index)
        results.append((struct.unpack_from("<QQQ", leaf, 72 * index + 16), struct.unpack_from("<QQQ", leaf, 72 * index + 40),
                        next_id, address, reminder, index, p, leaf[72 * index + 64], leaf[72 * index + 65], FOUND))
    n = len(ids)
    n_status = [0] * 8
    for r in results:
        n_status[r[9]] += 1
    first_bad = min((i for i, r in enumerate(results) if r[9] in obs.BAD), default=n)
    report = dict(n_status=tuple(n_status), n_probed=n_probed, probes=probes, first_bad=first_bad, trace=trep)
    return results, report, "" if first_bad == n else None


def space_tuples(records):
    def one(rec, f):
        v = rec[f]
        return tuple(int(v[g]) for g in ("checksum", "address", "birth_revision")) if f.endswith("_root") else int(v)
    return [tuple(one(rec, f) for f in SPACE_FIELDS) for rec in records]


class SpaceCase:
    """An image, the arguments that get spaces from its space tree, the IDs, and what the case is
    about: check(results as tuples, report dict)."""

    def __init__(self, img, lay, root, root_type, A, ids, check=None, verify_leaves=True):
        self.img, self.lay, self.root, self.root_type, self.A = img, lay, tuple(root), root_type, A
        self.ids, self.check, self.verify_leaves = [int(i) for i in ids], check, verify_leaves

    def args(self):
        return self.lay, self.root[:2] + (2,), self.root_type, self.A

    def reference(self):
        if not hasattr(self, "_reference"):
            self._reference = reference_spaces(self.img, self.lay, self.root, self.root_type, self.A, self.ids,
                                               self.verify_leaves)
        return self._reference


def host_spaces(case: SpaceCase, **kw):
    from storm_amd import spacestore as sps
    return sps.get_spaces_host(case.img, *case.args(), np.array(case.ids, dtype=np.uint64),
                               verify_leaves=case.verify_leaves, **kw)


def check_spaces(case: SpaceCase, records, report):
    from storm_amd import trace
    from storm_amd.scrub import SPACELIST
    want, want_rep, message = case.reference()
    assert space_tuples(records) == want
    assert not records["reserved"].any()
    assert report.as_dict() == want_rep
    assert report.code == (-5 if want_rep["first_bad"] < len(case.ids) else 0)
    if message is None:
        _, trep = trace.trace_host(case.img, case.lay, case.root[:2] + (2,), case.root_type, SPACELIST,
                                   tu.tags_u64(case.ids), 0, case.verify_leaves)
        message = trep.message
    assert report.message == message
    if case.check:
        case.check(want, want_rep)


def _space_tree(leaves, depth=1, slack=su.SLACK, lay=TEST_LAYOUT):
    """The image of a space tree: {path: SpaceList} under `depth` pointer levels, built as
    ObjectTree.build builds its own. Returns (img, lay, root, root_type, address_of)."""
    shim = ObjectTree(lay, 1, 1, depth)
    shim.leaves = leaves
    t = shim.build(slack)
    return t.img, t.lay, t.root, t.root_type, t.address_of


def _space_id(lay, path, reminder):
    F = lay.pointer_fanout
    return reminder * F ** len(path) + sum(s * F ** k for k, s in enumerate(path))


KEY_NODE, OBJ_NODE = (0x1111222233334444, 77, 5, su.POINTER_T), (0x5555666677778888, 99, 6, su.LEAF_T)


@functools.lru_cache(maxsize=None)
def space_states() -> SpaceCase:
    """Defined, Free and Invalid spaces; a space with only a key tree; a Defined match behind an
    Invalid slot and skipped state bytes; no Free slot and no match; a seed that wraps."""
    S, A = 10, space_table(10, 1)
    leaves, ids, want = {}, [], []

    def an_id(slot, reminder):
        ids.append(_space_id(TEST_LAYOUT, (slot,), reminder))
        return leaves.setdefault((slot,), SpaceList(S)), space_sequence(S, A, reminder)

    leaf, seq = an_id(0, 1000)       # Defined at the first slot of its sequence, both trees
    leaf.plant(seq[0], 1000, key=KEY_NODE, obj=OBJ_NODE, next_object_id=42)
    want.append((KEY_NODE[:3], OBJ_NODE[:3], 42, seq[0], 1, KEY_NODE[3], OBJ_NODE[3], FOUND))
    leaf, seq = an_id(1, 2001)       # Free first: the space does not exist
    leaf.plant(seq[4], 5555, key=KEY_NODE)
    want.append(((0, 0, 0), (0, 0, 0), 0, seq[0], 1, 0, 0, ABSENT))
    leaf, seq = an_id(2, 3002)       # its own reminder in an Invalid space, then Free: absent, the Invalid slot handed out
    leaf.plant(seq[0], 3002, state=INVALID, key=KEY_NODE, obj=OBJ_NODE, next_object_id=9)
    want.append(((0, 0, 0), (0, 0, 0), 0, seq[0], 2, 0, 0, ABSENT))
    leaf, seq = an_id(3, 4003)       # only a key tree: the object root is Free (type 0) and zeros
    leaf.plant(seq[0], 4003, key=KEY_NODE, next_object_id=1)
    want.append((KEY_NODE[:3], (0, 0, 0), 1, seq[0], 1, KEY_NODE[3], su.FREE_T, FOUND))
    leaf, seq = an_id(4, 5004)       # Invalid, state 3, state 255, another's Defined, then the match
    leaf.plant(seq[0], 5004, state=INVALID)
    leaf.plant(seq[1], 5004, state=3)
    leaf.plant(seq[2], 5004, state=255)
    leaf.plant(seq[3], 6004)
    leaf.plant(seq[4], 5004, key=KEY_NODE, obj=OBJ_NODE, next_object_id=7)
    want.append((KEY_NODE[:3], OBJ_NODE[:3], 7, seq[4], 5, KEY_NODE[3], OBJ_NODE[3], FOUND))
    leaf, seq = an_id(5, 7005)       # no Free slot and no match: S probes, no slot, whatever was Invalid
    for j in range(S):
        leaf.plant(seq[j], 8000 + j, state=INVALID if j in (2, 6) else DEFINED)
    want.append(((0, 0, 0), (0, 0, 0), 0, NO_SLOT, S, 0, 0, ABSENT))
    j = max(i for i in (1, 2, 3) if A[i] >= 1)  # a seed of S - 1 and an offset above 0: seed + A[j] wraps
    leaf, seq = an_id(6, 9009)
    assert 9009 % S + int(A[j]) >= S and seq[j] == int(A[j]) - 1
    for i in range(j):
        leaf.plant(seq[i], 100 + i)
    leaf.plant(seq[j], 9009, obj=OBJ_NODE)
    want.append(((0, 0, 0), OBJ_NODE[:3], 0, seq[j], j + 1, su.FREE_T, OBJ_NODE[3], FOUND))
    ids.append(_space_id(TEST_LAYOUT, (8,), 5))  # a Free entry of the pointer block: absent, not probed
    img, lay, root, root_type, _ = _space_tree(leaves)

    def check(res, rep):
        assert [r[:3] + r[5:] for r in res[:-1]] == want
        assert res[-1][5:] == (NO_SLOT, 0, 0, 0, ABSENT) and rep["n_probed"] == 7 and rep["first_bad"] == 8
    return SpaceCase(img, lay, root, root_type, A, ids, check)


@functools.lru_cache(maxsize=None)
def space_damage(verify_leaves=True) -> SpaceCase:
    """Two pointer levels, a flipped byte in one spacelist leaf's unused tail: MISMATCH for the IDs
    under it and the trace's words; unverified, the leaf is probed as it is. 70 IDs: more than a wave."""
    S, A = 10, space_table(10, 2)
    rng = np.random.default_rng(21)
    leaves, ids = {}, []
    for path in ((0, 0), (3, 1), (9, 9)):
        leaf = leaves.setdefault(path, SpaceList(S))
        for r in range(5):
            reminder = int(rng.integers(1, 2 ** 40))
            index, _, _ = find_space(leaf.b, S, A, reminder)
            leaf.plant(index, reminder, key=KEY_NODE, obj=OBJ_NODE, next_object_id=r)
            ids.append(_space_id(TEST_LAYOUT, path, reminder))
    ids = (ids + [_space_id(TEST_LAYOUT, (3, 1), 2 ** 41 + k) for k in range(20)]) * 2
    img, lay, root, root_type, address_of = _space_tree(leaves, depth=2)
    img = img.copy()
    img[address_of[(3, 1)] * lay.block_size + 725] ^= 0x10  # past NUsedSpaces: no probe reads it
    under = [i for i, s in enumerate(ids) if (s % 10, s // 10 % 10) == (3, 1)]

    def check(res, rep):
        st = [r[9] for r in res]
        if verify_leaves:
            assert [i for i, s in enumerate(st) if s == MISMATCH] == under and rep["first_bad"] == under[0]
        else:
            assert MISMATCH not in st and rep["n_probed"] == len(ids) and rep["trace"]["blocks_hashed"][1] == 0
    return SpaceCase(su.frozen(img), lay, root, root_type, A, ids, check, verify_leaves)


@functools.lru_cache(maxsize=None)
def space_count(n) -> SpaceCase:
    c = space_damage(False)
    return SpaceCase(c.img, c.lay, c.root, c.root_type, c.A, c.ids[:n], None)


@functools.lru_cache(maxsize=None)
def space_production() -> SpaceCase:
    """Production sizes: block 32768, fan-out 1200, S = 400, 250 spaces in one leaf that is the last
    block of an image with no slack; absent IDs probe past long runs."""
    S, A = 400, space_table(400, 3)
    rng = np.random.default_rng(31)
    leaf, ids = SpaceList(S), []
    for r in range(250):
        reminder = int(rng.integers(1, 2 ** 40))
        index, _, found = find_space(leaf.b, S, A, reminder)
        assert not found
        leaf.plant(index, reminder, key=KEY_NODE[:2] + (r, su.POINTER_T), obj=OBJ_NODE, next_object_id=r)
        ids.append(_space_id(PRODUCTION_LAYOUT, (1199,), reminder))
    ids += [_space_id(PRODUCTION_LAYOUT, (1199,), 2 ** 41 + k) for k in range(50)]
    img, lay, root, root_type, address_of = _space_tree({(1199,): leaf}, slack=0, lay=PRODUCTION_LAYOUT)
    assert address_of[(1199,)] == lay.n_blocks - 1 and img.size == lay.n_blocks * lay.block_size

    def check(res, rep):
        assert [r[2] for r in res[:250]] == list(range(250)) and rep["n_status"][FOUND] == 250
        assert rep["n_status"][ABSENT] == 50 and max(r[6] for r in res) >= 5
    return SpaceCase(img, lay, root, root_type, A, ids, check)


SPACE_CASES = {"states": space_states, "damage": space_damage, "damage, unverified": lambda: space_damage(False),
               "production sizes": space_production}
SPACE_CASES.update({f"n = {n}": functools.partial(space_count, n) for n in (0, 1, 63, 64, 65)})


# ---- get (tests/test_get.py, tests/test_get_gpu.py) --------------------------------------------------

GET_FIELDS = ("object_id", "key_address", "object_address", "index", "stage", "status")
GET_N, GET_S = 10, 13  # the object trees of the test stores: ten slots of 13-byte objects


def _put_tree(b, leaves, depth):
    """The tree {path: leaf with .b} under `depth` pointer levels into the Builder b, children
    first; returns its root node (checksum, address, block type), None for no leaves."""
    if not leaves:
        return None

    def put(path):
        if len(path) == depth:
            return b._put(bytes(leaves[path].b), su.LEAF_T)
        below = sorted({q[:len(path) + 1] for q in leaves if q[:len(path)] == path})
        return b.pointer({p[-1]: put(p) for p in below})
    return put(())


class Store:
    """A whole store on scrub_util.Builder: the singularity, a space tree of one pointer block over
    spacelist leaves, and per Defined space a key tree (lookup_util.KeyTree) and an object tree
    (ObjectTree). spaces[space_id] = (state, KeyTree or None, ObjectTree or None)."""

    def __init__(self, spaces, SA, A, lay=TEST_LAYOUT, blob=(GET_N, GET_S)):
        from tests import lookup_util as lu
        self.SA, self.A, self.C = SA, A, len(A)
        S = lay.spaces_per_block
        b = su.Builder(lay)
        self.nodes, lists = {}, {}
        for space_id, (state, kt, ot) in spaces.items():
            key = _put_tree(b, kt.leaves, kt.depth) if kt is not None else None
            obj = _put_tree(b, ot.leaves, ot.depth) if ot is not None else None
            self.nodes[space_id] = (key, obj)
            path, reminder = (space_id % lay.pointer_fanout,), space_id // lay.pointer_fanout
            leaf = lists.setdefault(path, SpaceList(S))
            index, _, found = find_space(leaf.b, S, SA, reminder)
            assert index is not None and not found
            leaf.plant(index, reminder, state, key=(key[0], key[1], 1, key[2]) if key else (0, 0, 0, 0),
                       obj=(obj[0], obj[1], 1, obj[2]) if obj else (0, 0, 0, 0), next_object_id=space_id + 1000)
        self.space_leaves = {}
        kids = {}
        for path, leaf in sorted(lists.items()):
            kids[path[0]] = b._put(bytes(leaf.b), su.LEAF_T)
            self.space_leaves[path] = kids[path[0]][1]
        root = b.pointer(kids)
        img, self.lay = b.finish(root, slack=su.SLACK)
        self.img = su.frozen(img)
        from storm_amd import storm
        self.params = storm.GetParams(SA, lu.ks.ObjectListParams(A, self.C), obs.BlobParams(*blob))

    def damaged(self, address, byte):
        import copy
        other = copy.copy(self)
        img = self.img.copy()
        img[address * self.lay.block_size + byte] ^= 0x10
        other.img = su.frozen(img)
        return other


def reference_get(store: Store, space_id, keys, verify_leaves=True):
    """(results, rows, report, message source): results[i] = GET_FIELDS of keys[i]; the report as
    GetReport.as_dict() without its space; message source: "" (no bad key), a text (the
    singularity's), or "space" / "lookup" / "objects": the words of that stage's own entry point."""
    from tests import lookup_util as lu
    img, lay, n = store.img, store.lay, len(keys)
    no_lookup = dict(n_status=(0,) * 8, n_probed=0, probes=0, n_malformed=0, first_bad=n,
                     trace=dict(n_status=(0,) * 7, blocks_hashed=(0, 0), bytes_hashed=0, first_bad=n, levels=0))
    rep = dict(n_selected=0, n_status=(0,) * 8, blocks_hashed=(0, 0), bytes_hashed=0, probes=0, levels=0, n_found=0,
               first_bad=n, lookup=no_lookup)

    def at_space(status, message):
        rep["first_bad"] = 0 if status in obs.BAD and n else n
        return [(0, 0, 0, NO_SLOT, 0, status)] * n, [bytes(GET_S)] * n, rep, message if rep["first_bad"] < n else "", None

    if n == 0:  # a no-op: nothing is read
        return [], [], rep, "", None
    s = bytearray(img[:72].tobytes())
    expected = struct.unpack_from("<Q", s, 0)[0]
    s[0:8] = bytes(8)
    from oracle import oracle as o
    computed = o.xxh64(bytes(s))
    if computed != expected:
        return at_space(MISMATCH, f"checksum mismatch for block 0, computed: 0x{computed:x}, expected: 0x{expected:x}")
    sroot, stype = struct.unpack_from("<QQ", s, 32), s[56]
    sres, _, _ = reference_spaces(img, lay, sroot, stype, store.SA, [space_id], True)
    space = sres[0]
    if space[9] != FOUND:
        return at_space(space[9], "space")[:4] + (space,)
    lres, lrep, _ = lu.reference_lookup(img, lay, space[0][:2], space[7], store.C, store.A, keys, verify_leaves)
    sel = [i for i, r in enumerate(lres) if r[5] == FOUND]
    ores, orows, orep, _ = reference_objects(img, lay, space[1][:2], space[8], GET_N, GET_S, [lres[i][0] for i in sel],
                                             verify_leaves)
    place = {i: j for j, i in enumerate(sel)}
    results, rows = [], []
    for i, l in enumerate(lres):
        if i in place:
            r = ores[place[i]]
            results.append((l[0], l[1], r[1], r[3], 2, r[5]))
            rows.append(orows[place[i]])
        else:
            results.append((l[0], l[1], 0, l[3], 1, l[5]))
            rows.append(bytes(GET_S))
    object_bad = sel[orep["first_bad"]] if orep["first_bad"] < len(sel) else n
    rep.update(n_selected=len(sel), n_status=orep["n_status"], blocks_hashed=orep["trace"]["blocks_hashed"],
               bytes_hashed=orep["trace"]["bytes_hashed"], probes=orep["probes"], levels=orep["trace"]["levels"],
               n_found=orep["n_status"][FOUND], first_bad=min(lrep["first_bad"], object_bad), lookup=lrep)
    source = "" if rep["first_bad"] == n else "lookup" if rep["first_bad"] == lrep["first_bad"] else "objects"
    return results, rows, rep, source, space


class GetCase:
    def __init__(self, store: Store, space_id, keys, check=None, verify_leaves=True, out_stride=16, want_objects=True):
        self.store, self.space_id, self.keys, self.check = store, space_id, list(keys), check
        self.verify_leaves, self.out_stride, self.want_objects = verify_leaves, out_stride, want_objects

    def reference(self):
        if not hasattr(self, "_reference"):
            self._reference = reference_get(self.store, self.space_id, self.keys, self.verify_leaves)
        return self._reference

    def rows(self):
        return np.full((len(self.keys), self.out_stride), FILL, dtype=np.uint8) if self.want_objects else None


def host_get(case: GetCase, **kw):
    from storm_amd import storm
    from tests import lookup_util as lu
    return storm.get_host(case.store.img, case.store.lay, case.space_id, case.store.params, **lu.pack(case.keys, "flat"),
                          verify_leaves=case.verify_leaves, want_objects=case.want_objects, out_stride=case.out_stride,
                          objects=case.rows(), **kw)


def get_tuples(records):
    return [tuple(int(rec[f]) for f in GET_FIELDS) for rec in records]


def stage_message(case: GetCase, source, space):
    """The words of the stage's own host entry point for the call's bad key."""
    from storm_amd import keystore as ks, spacestore as sps
    from tests import lookup_util as lu
    st = case.store
    s = st.img[:72].tobytes()
    if source == "space":
        root = struct.unpack_from("<QQ", s, 32)
        return sps.get_spaces_host(st.img, st.lay, root + (1,), s[56], st.SA, np.array([case.space_id], np.uint64))[1].message
    if source == "lookup":
        return ks.get_object_ids_host(st.img, st.lay, space[0], space[7], st.params.keys, **lu.pack(case.keys, "flat"),
                                      verify_leaves=case.verify_leaves)[1].message
    lres = reference_get(st, case.space_id, case.keys, case.verify_leaves)[0]
    ids = np.array([r[0] for r in lres if r[4] == 2], dtype=np.uint64)
    return obs.get_objects_host(st.img, st.lay, space[1], space[8], st.params.objects, ids,
                                verify_leaves=case.verify_leaves)[2].message


def check_get(case: GetCase, records, objects, report):
    want, rows, want_rep, source, space = case.reference()
    assert get_tuples(records) == want
    assert not records["reserved"].any()
    if case.want_objects:
        gap = bytes([FILL]) * (case.out_stride - GET_S)
        assert objects.tobytes() == b"".join(r + gap for r in rows)
    else:
        assert objects is None
    got = report.as_dict()
    got.pop("space")
    assert got == want_rep
    if space is None:
        assert space_tuples([report.space]) == [((0, 0, 0), (0, 0, 0), 0, 0, 0, NO_SLOT, 0, 0, 0, 0)]  # no space was looked up
    else:
        assert space_tuples([report.space]) == [space]
    n = len(case.keys)
    assert report.code == (-5 if want_rep["first_bad"] < n else 0)
    message = stage_message(case, source, space) if source in ("space", "lookup", "objects") else source
    assert report.message == message
    if case.check:
        case.check(want, rows, want_rep)


GET_SPACE, GET_INVALID, GET_NO_OBJECTS, GET_ABSENT = 4321, 5322, 6323, 7324


@functools.lru_cache(maxsize=None)
def get_store():
    """(Store, present keys -> object, the key whose object was never set, the KeyTree, the ObjectTree)."""
    from tests import lookup_util as lu
    rng = np.random.default_rng(77)
    A, SA = lu.table(10, 7), space_table(10, 7)
    kt = lu.KeyTree(TEST_LAYOUT, A, depth=2)
    ot = ObjectTree(TEST_LAYOUT, GET_N, GET_S, depth=2)
    present = {}
    while len(present) < 80:
        k = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        leaf = kt.leaf(kt.locate(k)[0])
        oid = 5000 + 37 * len(present)
        if k in present or leaf.n_used() + 2 > 7 or ot.leaf(ot.locate(oid)[0]).n_used() >= 7:
            continue
        kt.add(k, oid)
        present[k] = payload(rng, GET_S)
        ot.set(oid, present[k])
    orphan = rng.integers(0, 256, 21, dtype=np.uint8).tobytes()  # present as a key, its object never set (storm.go:51)
    kt.add(orphan, 5000 + 37 * 3 + 100 * 10 ** 4)  # the leaf of object 5000 + 37 * 3, another reminder: its slot is Free
    kt2 = lu.KeyTree(TEST_LAYOUT, A, depth=1)
    for k in list(present)[:5]:
        kt2.add(k, 9000)
    store = Store({GET_SPACE: (DEFINED, kt, ot), GET_INVALID: (INVALID, None, None), GET_NO_OBJECTS: (DEFINED, kt2, None)},
                  SA, A)
    return store, present, orphan, kt, ot


def _absent_keys(rng, n):
    return [rng.integers(0, 256, 50, dtype=np.uint8).tobytes() for _ in range(n)]  # longer than any stored key


@functools.lru_cache(maxsize=None)
def get_mixed() -> GetCase:
    """Keys present with their object, keys absent, the key whose object slot is Free (ABSENT at
    stage 2), keys of length 0 and 257 (KEY at stage 1)."""
    store, present, orphan, _, _ = get_store()
    rng = np.random.default_rng(78)
    keys = list(present) + _absent_keys(rng, 15) + [orphan]
    keys = [keys[int(i)] for i in rng.permutation(len(keys))]
    keys.insert(40, b"")
    keys.insert(70, bytes(257))

    def check(res, rows, rep):
        for k, r, row in zip(keys, res, rows):
            if k in present:
                assert r[4:] == (2, FOUND) and row == present[k]
            elif k == orphan:
                assert r[4:] == (2, ABSENT) and r[0] == 5000 + 37 * 3 + 100 * 10 ** 4 and row == bytes(GET_S)
            elif len(k) in (0, 257):
                assert r[4:] == (1, ks.KEY)
            else:
                assert r[4:] == (1, ABSENT) and r[0] == 0
        assert rep["first_bad"] == 40 and rep["n_selected"] == 81 and rep["n_found"] == 80
    return GetCase(store, GET_SPACE, keys, check)


@functools.lru_cache(maxsize=None)
def get_space_case(name) -> GetCase:
    """The walk of every key ends at the space: absent, Invalid, or the spacelist leaf or the
    singularity damaged (stage 0 owns first_bad); or at stage 2 under a Free object root."""
    store, present, _, _, _ = get_store()
    keys = list(present)[:70]
    if name == "absent space":
        return GetCase(store, GET_ABSENT, keys, lambda res, rows, rep: res[0] == (0, 0, 0, NO_SLOT, 0, ABSENT) or 1 / 0)
    if name == "invalid space":
        return GetCase(store, GET_INVALID, keys, lambda res, rows, rep: set(res) == {(0, 0, 0, NO_SLOT, 0, ABSENT)} or 1 / 0)
    if name == "free object root":
        def check(res, rows, rep):
            assert [r[4:] for r in res[:5]] == [(2, ABSENT)] * 5 and [r[4:] for r in res[5:]] == [(1, ABSENT)] * 65
            assert rep["n_selected"] == 5 and rep["blocks_hashed"] == (0, 0) and rep["first_bad"] == 70
        return GetCase(store, GET_NO_OBJECTS, keys, check)
    if name == "damaged spacelist leaf":
        bad = store.damaged(store.space_leaves[(GET_SPACE % 10,)], 725)
    else:
        bad = store.damaged(0, 20)  # the singularity's Revision

    def check(res, rows, rep):
        assert set(res) == {(0, 0, 0, NO_SLOT, 0, MISMATCH)} and rep["first_bad"] == 0 and rep["lookup"]["first_bad"] == 70
    return GetCase(bad, GET_SPACE, keys, check)


@functools.lru_cache(maxsize=None)
def get_damaged_tree(which, verify_leaves=True) -> GetCase:
    """A flipped byte in one key leaf (stage 1 owns first_bad) or in one blob leaf (stage 2 does)."""
    store, present, _, kt, ot = get_store()
    keys = list(present)
    img, lay = store.img, store.lay
    sres = reference_get(store, GET_SPACE, keys[:1])[4]
    if which == "key tree":
        tres = tu.reference_trace(img, lay, sres[0][:2], sres[7], 2, [__import__("oracle.oracle", fromlist=["x"]).xxh64(k) for k in keys])[0]
        victim = tres[len(keys) // 2][0]
        bad = store.damaged(victim, 534)  # past FreeChunkIndex: no probe reads it
        under = [i for i, t in enumerate(tres) if t[0] == victim]
        stage = 1
    else:
        oids = [5000 + 37 * i for i in range(len(keys))]
        tres = tu.reference_trace(img, lay, sres[1][:2], sres[8], BLOB, oids)[0]
        victim = tres[len(keys) // 2][0]
        bad = store.damaged(victim, 727)  # NUsedSlots: no probe reads it
        under = [i for i, t in enumerate(tres) if t[0] == victim]
        stage = 2

    def check(res, rows, rep):
        if verify_leaves:
            assert [i for i, r in enumerate(res) if r[5] == MISMATCH] == under and rep["first_bad"] == under[0]
            assert all(res[i][4] == stage and rows[i] == bytes(GET_S) for i in under)
        else:
            assert all(r[4:] == (2, FOUND) for r in res) and rows == list(present.values())
    return GetCase(bad, GET_SPACE, keys, check, verify_leaves)


@functools.lru_cache(maxsize=None)
def get_nothing_found() -> GetCase:
    """No key is FOUND: the object stage runs with zero IDs. More than a wave of keys."""
    store = get_store()[0]

    def check(res, rows, rep):
        assert rep["n_selected"] == 0 and rep["n_status"] == (0,) * 8 and all(r[4:] == (1, ABSENT) for r in res)
    return GetCase(store, GET_SPACE, _absent_keys(np.random.default_rng(79), 70), check)


@functools.lru_cache(maxsize=None)
def get_count(n, want_objects=True) -> GetCase:
    c = get_mixed()
    keys = [k for k in c.keys if 1 <= len(k) <= 256]
    return GetCase(c.store, GET_SPACE, (keys * 4)[:n], None, out_stride=13 + n % 4, want_objects=want_objects)


GET_CASES = {"mixed": get_mixed, "nothing found": get_nothing_found, "no rows": lambda: get_count(65, False)}
GET_CASES.update({n: functools.partial(get_space_case, n) for n in
                  ("absent space", "invalid space", "free object root", "damaged spacelist leaf", "damaged singularity")})
GET_CASES.update({f"damaged {w}": functools.partial(get_damaged_tree, w) for w in ("key tree", "object tree")})
GET_CASES.update({f"damaged {w}, unverified": functools.partial(get_damaged_tree, w, False) for w in ("key tree", "object tree")})
GET_CASES.update({f"n = {n}": functools.partial(get_count, n) for n in (0, 1, 63, 64, 65, 257, 300)})
