"""TEST INFRASTRUCTURE for the update tests (tests/test_update.py, tests/test_update_fuzz.py and
their GPU twins): storm.Set for keys that already have an object (include/stormck.h "update").

* ``roomy``: a store's image (built images are read-only) with room for a new revision inside
  n_blocks and guard blocks of 0xA5 past it;
* ``reference_update``: a pure-Python restatement of rules A to D over ``objects_util.reference_get``;
* ``check_update``: the semantic checks, which do not rest on that restatement: the scrub as an
  independent judge, a get over every key, the singularity, the bytes that must not change, the
  old snapshot, the reachable bitmaps;
* the stores and the designed cases both legs run.
"""
from __future__ import annotations

import copy
import functools
import struct

import numpy as np

from oracle import oracle as o
from storm_amd import scrub, storm
from storm_amd.scrub import BLOB, POINTER, SPACELIST, ScrubLayout
from tests import lookup_util as lu
from tests import objects_util as ou
from tests import scrub_util as su

SLACK = 4       # guard blocks past n_blocks
GUARD = 0xA5
NONE, WRITTEN, SUPERSEDED = 0, 1, 2
UPDATE_FIELDS = ou.GET_FIELDS + ("action",)
OK, EMISMATCH, ENOSPC = 0, -5, -6
ENOSPC_TEXT = "update: the image has no room for the dirty blocks (LastAllocatedBlock + dirty blocks >= n_blocks)"


def blob_shape(store):
    return store.params.objects.objects_per_block, store.params.objects.object_size


def roomy(store, room: int):
    """(writable image, layout): the store's n_blocks blocks, `room` more zeroed blocks inside
    n_blocks, then SLACK guard blocks of 0xA5."""
    lay0, bs = store.lay, store.lay.block_size
    n = lay0.n_blocks
    img = np.full((n + room + SLACK) * bs, GUARD, dtype=np.uint8)
    img[:n * bs] = store.img[:n * bs]
    img[n * bs:(n + room) * bs] = 0
    lay = ScrubLayout(bs, n + room, lay0.pointer_fanout, lay0.spaces_per_block, lay0.objectlist_len, lay0.blob_len)
    return img, lay


def on_image(store, img, lay):
    """The store's tables and parameters over another image."""
    other = copy.copy(store)
    other.img, other.lay = img, lay
    return other


def pack_rows(rows, S, in_stride):
    """The rows in_stride apart, the gaps holding FILL."""
    a = np.full((len(rows), in_stride), ou.FILL, dtype=np.uint8)
    for i, r in enumerate(rows):
        assert len(r) == S
        a[i, :S] = np.frombuffer(r, np.uint8)
    return a


def new_rows(rng, n, S):
    return [ou.payload(rng, S) for _ in range(n)]


def _reference_get(st, space_id, keys):
    """objects_util.reference_get with the store's own blob shape."""
    saved = ou.GET_N, ou.GET_S
    ou.GET_N, ou.GET_S = blob_shape(st)
    try:
        return ou.reference_get(st, space_id, keys)
    finally:
        ou.GET_N, ou.GET_S = saved


def _walk(img, lay, address, typ, parent, slot, tag, leaf_kind):
    """The blocks (address, kind, parent, slot) on the tag's walk from a reference
    (cache/trace.go:21-33: index = reminder % PointersPerBlock, reminder /= PointersPerBlock)."""
    F, bs, out = lay.pointer_fanout, lay.block_size, []
    while True:
        assert typ in (su.POINTER_T, su.LEAF_T) and 0 < address < lay.n_blocks
        if typ == su.LEAF_T:
            out.append((address, leaf_kind, parent, slot))
            return out
        out.append((address, POINTER, parent, slot))
        e, tag = tag % F, tag // F
        base = address * bs
        parent, slot = address, e
        address, typ = struct.unpack_from("<Q", img, base + 24 * e + 8)[0], int(img[base + 24 * F + e])


def reference_update(img, lay, space_id, store, keys, rows):
    """Rules A to D of include/stormck.h "update", one block at a time. Returns (results as
    UPDATE_FIELDS tuples, the new image, the report as UpdateReport.as_dict() without its get's
    space, the return code, the message source: a text, or what reference_get names)."""
    st = on_image(store, img, lay)
    N, S = blob_shape(st)
    n = len(keys)
    res, _, grep, source, space = _reference_get(st, space_id, keys)  # A. locate (storm.go:62-70 find what Get finds)
    rep = dict(n_written=0, n_superseded=0, n_dirty=(0, 0, 0, 0), bytes_copied=0, bytes_hashed=0, revision=0,
               last_allocated=0, first_new=0, heights=0, get=grep)
    if n == 0 or grep["first_bad"] < n:
        return [r + (NONE,) for r in res], img.copy(), rep, (EMISMATCH if n else OK), source, space
    revision, last = struct.unpack_from("<Q", img, 16)[0], struct.unpack_from("<Q", img, 64)[0]
    rep.update(revision=revision, last_allocated=last)
    # B. select: storm's serial loop, the last Set of a slot wins
    winner = {}
    for i, r in enumerate(res):
        if r[4:] == (2, ou.FOUND):
            winner[(r[2], r[3])] = i
    actions = [NONE if r[4:] != (2, ou.FOUND) else WRITTEN if winner[(r[2], r[3])] == i else SUPERSEDED
               for i, r in enumerate(res)]
    results = [r + (a,) for r, a in zip(res, actions)]
    rep.update(n_written=actions.count(WRITTEN), n_superseded=actions.count(SUPERSEDED))
    if not rep["n_written"]:
        return results, img.copy(), rep, OK, "", space
    # C. the dirty forest (cache/cache.go:87-137: every dirty block, children first)
    blocks = {}
    for b in _walk(img, lay, struct.unpack_from("<Q", img, 40)[0], int(img[56]), 0, 0, space_id, SPACELIST):
        blocks.setdefault(b[0], b)
    assert space[3] in blocks
    for i, r in enumerate(results):
        if r[6] == WRITTEN:
            path = _walk(img, lay, space[1][1], space[8], space[3], space[5], r[0], BLOB)
            assert path[-1][0] == r[2]
            for b in path:
                assert blocks.setdefault(b[0], b) == b
    kids = {}
    for a, (_, _, parent, _) in blocks.items():
        kids.setdefault(parent, []).append(a)

    def height(a):
        return 1 + max(height(k) for k in kids[a]) if a in kids else 0
    order = sorted(blocks, key=lambda a: (height(a), a))
    D = len(order)
    if last + D >= lay.n_blocks or last >= lay.n_blocks:
        return results, img.copy(), rep, ENOSPC, ENOSPC_TEXT, space
    new = {a: last + 1 + k for k, a in enumerate(order)}
    # D. write
    out, bs, lens = img.copy(), lay.block_size, su.kind_lens(lay)
    for a in order:
        out[new[a] * bs:(new[a] + 1) * bs] = img[a * bs:(a + 1) * bs]
    for i, r in enumerate(results):
        if r[6] == WRITTEN:  # objectstore.go:53-56: objectSlot.Object = object
            at = new[r[2]] * bs + r[3] * ou.stride_of(S) + 8
            out[at:at + S] = np.frombuffer(rows[i], np.uint8)
    sing = bytearray(out[:72].tobytes())
    n_dirty = [0, 0, 0, 0]
    for a in order:
        _, kind, parent, slot = blocks[a]
        n_dirty[kind] += 1
        cs = o.xxh64(out[new[a] * bs:new[a] * bs + lens[kind]])
        typ = su.POINTER_T if kind == POINTER else su.LEAF_T
        if parent == 0:
            struct.pack_into("<QQQ", sing, 32, cs, new[a], revision + 1)
            sing[56] = typ
            continue
        pkind, pat = blocks[parent][1], new[parent] * bs
        at, tat = (pat + 24 * slot, pat + 24 * lay.pointer_fanout + slot) if pkind == POINTER else \
            (pat + 72 * slot + 40, pat + 72 * slot + 65)
        out[at:at + 24] = np.frombuffer(struct.pack("<QQQ", cs, new[a], revision + 1), np.uint8)
        out[tat] = typ
    struct.pack_into("<Q", sing, 16, revision + 1)
    struct.pack_into("<Q", sing, 64, last + D)
    sing[0:8] = bytes(8)
    sing[0:8] = struct.pack("<Q", o.xxh64(bytes(sing)))
    out[:72] = np.frombuffer(bytes(sing), np.uint8)
    rep.update(n_dirty=tuple(n_dirty), bytes_copied=D * bs, bytes_hashed=72 + sum(lens[blocks[a][1]] for a in order),
               revision=revision + 1, last_allocated=last + D, first_new=last + 1, heights=1 + height(order[-1]))
    return results, out, rep, OK, "", space


def update_tuples(records):
    return [tuple(int(rec[f]) for f in UPDATE_FIELDS) for rec in records]


def host_update(img, lay, store, space_id, keys, rows, in_stride=None, **kw):
    """stormck_update_host on `img`, in place: (records, report)."""
    S = blob_shape(store)[1]
    p = lu.pack(keys, "flat")
    return storm.update_host(img, lay, space_id, store.params, p["keys"], pack_rows(rows, S, in_stride or S + 3),
                             offsets=p["offsets"], lens=p["lens"], **kw)


def _get(img, lay, store, space_id, keys):
    return storm.get_host(img, lay, space_id, store.params, **lu.pack(keys, "flat"),
                          out_stride=blob_shape(store)[1])


def _blocks(img, lay, lo, hi):
    return img[lo * lay.block_size:hi * lay.block_size].tobytes()


def check_update(store, old, lay, space_id, keys, rows, records, new, report, all_keys):
    """The semantic checks of one update that returned OK: `old` and `new` are the image before
    and after, `records` / `report` the call's, `all_keys` every key of the store's space."""
    bs, n = lay.block_size, lay.n_blocks
    assert new.size == old.size and report.code == OK
    old_sing = old[:72].tobytes()
    old_rev, L = struct.unpack_from("<Q", old_sing, 16)[0], struct.unpack_from("<Q", old_sing, 64)[0]
    D = sum(report.n_dirty)
    if report.n_written == 0:  # a batch that changes nothing makes no revision
        assert new.tobytes() == old.tobytes() and D == 0 and report.first_new == 0
        assert (report.revision, report.last_allocated) == ((old_rev, L) if len(keys) else (0, 0))  # n == 0 reads nothing
        return
    # scrub: the new image is clean and holds as many blocks of every kind
    s_old, s_new = scrub.scrub_host(old, lay, reachable=True), scrub.scrub_host(new, lay, reachable=True)
    assert s_old.ok and s_new.ok and s_new.verified == s_old.verified
    # get: the new row of every WRITTEN key's slot, the old row of every other key
    g_old, r_old, rep_old = _get(old, lay, store, space_id, all_keys)
    g_new, r_new, rep_new = _get(new, lay, store, space_id, all_keys)
    assert rep_old.ok and rep_new.ok
    written = {(int(r["object_address"]), int(r["index"])): rows[i] for i, r in enumerate(records) if r["action"] == WRITTEN}
    assert len(written) == report.n_written == sum(r["action"] == WRITTEN for r in records)
    seen = set()
    for j in range(len(all_keys)):
        slot = (int(g_old[j]["object_address"]), int(g_old[j]["index"]))
        found = (g_old[j]["stage"], g_old[j]["status"]) == (2, ou.FOUND)
        want = written[slot] if found and slot in written else r_old[j].tobytes()
        seen.add(slot if found and slot in written else None)
        assert r_new[j].tobytes() == want
        for f in ("object_id", "key_address", "index", "stage", "status"):
            assert g_new[j][f] == g_old[j][f]
    assert seen - {None} == set(written)  # all_keys reach every written slot
    # the singularity
    new_rev, new_last = struct.unpack_from("<Q", new, 16)[0], struct.unpack_from("<Q", new, 64)[0]
    assert (new_rev, new_last) == (old_rev + 1, L + D) == (report.revision, report.last_allocated)
    assert report.first_new == L + 1 and report.bytes_copied == D * bs
    # the bytes that do not change
    assert _blocks(new, lay, 1, L + 1) == _blocks(old, lay, 1, L + 1)
    assert new[(L + D + 1) * bs:].tobytes() == old[(L + D + 1) * bs:].tobytes()  # up to n_blocks, and the guards
    assert new[n * bs:].tobytes() == bytes([GUARD]) * (new.size - n * bs)
    assert new[72:bs].tobytes() == old[72:bs].tobytes()
    # the old snapshot
    back = new.copy()
    back[:72] = old[:72]
    assert _blocks(back, lay, 0, L + 1) == _blocks(old, lay, 0, L + 1)
    s_back = scrub.scrub_host(back, lay, reachable=True)
    assert s_back.ok and s_back.verified == s_old.verified
    g_back, r_back, _ = _get(back, lay, store, space_id, all_keys)
    assert g_back.tobytes() == g_old.tobytes() and r_back.tobytes() == r_old.tobytes()
    # reachable: the new revision shares everything but the D dirty blocks, which it replaces by L + 1 .. L + D
    bits = lambda words: set(np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))[0].tolist())  # noqa: E731
    b_old, b_new = bits(s_old.reachable), bits(s_new.reachable)
    assert b_new - b_old == set(range(L + 1, L + D + 1))
    dirty = b_old - b_new
    assert len(dirty) == D and b_old & b_new == b_old - dirty
    assert {int(r["object_address"]) for r in records if r["action"] == WRITTEN} <= dirty
    assert int(report.get.space["address"]) in dirty and max(b_old) <= L


# ---- stores ---------------------------------------------------------------------------------------

def _keys_and_objects(rng, kt, ot, n_keys, per_leaf):
    present, tries = {}, 0
    while len(present) < n_keys:
        tries += 1
        assert tries < 100 * n_keys, "the trees have no room for that many keys"
        k = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        oid = 5000 + 37 * tries
        if k in present or kt.leaf(kt.locate(k)[0]).n_used() + 2 > 7 or ot.leaf(ot.locate(oid)[0]).n_used() >= per_leaf:
            continue
        kt.add(k, oid)
        present[k] = ou.payload(rng, ot.S)
        ot.set(oid, present[k])
    return present


@functools.lru_cache(maxsize=None)
def depth_store(depth):
    return _depth_store(depth)


def _depth_store(depth, lay=None, N=ou.GET_N, S=ou.GET_S, seed=0):
    """(Store, present keys -> object): one Defined space whose object tree has `depth` pointer
    levels; depth 0: the root is a leaf and the space's record is its origin."""
    lay = lay or ou.TEST_LAYOUT
    rng = np.random.default_rng(500 + 10 * depth + seed)
    A, SA = lu.table(10, 7), ou.space_table(10, 7)
    kt, ot = lu.KeyTree(lay, A, depth=1), ou.ObjectTree(lay, N, S, depth=depth)
    per_leaf = max(1, min(7, N - 1))
    present = _keys_and_objects(rng, kt, ot, min(N, 6) if depth == 0 else min(40, 6 * per_leaf), per_leaf)
    return ou.Store({ou.GET_SPACE: (ou.DEFINED, kt, ot)}, SA, A, lay=lay, blob=(N, S)), present


@functools.lru_cache(maxsize=None)
def size_store(S):
    """Objects of S bytes (objects_util.SIZES, its layout and N), for the store's row forms."""
    lay, N = ou.size_layout(S)
    return _depth_store(1, lay, N, S)


@functools.lru_cache(maxsize=None)
def two_space_store(same_leaf: bool):
    """Two Defined spaces, in one spacelist leaf or in two: (Store, {space: present})."""
    rng = np.random.default_rng(600 + same_leaf)
    A, SA = lu.table(10, 7), ou.space_table(10, 7)
    other = ou.GET_SPACE + (10 if same_leaf else 1)  # the space tree's slot is space_id % 10
    spaces, present = {}, {}
    for sid in (ou.GET_SPACE, other):
        kt, ot = lu.KeyTree(ou.TEST_LAYOUT, A, depth=1), ou.ObjectTree(ou.TEST_LAYOUT, ou.GET_N, ou.GET_S, depth=1)
        present[sid] = _keys_and_objects(rng, kt, ot, 30, 7)
        spaces[sid] = (ou.DEFINED, kt, ot)
    store = ou.Store(spaces, SA, A)
    assert (len(store.space_leaves) == 1) == same_leaf
    return store, present, other


@functools.lru_cache(maxsize=None)
def irregular_store():
    """An object tree built by hand: under the root pointer block a leaf directly (slot 2) beside
    a pointer block (slot 5) with leaves under it (slots 0 and 4), so that the root has dirty
    children of heights 0 and 1. (Store, present keys -> object, keys per leaf path)."""
    lay0 = ou.TEST_LAYOUT
    F, N, S = lay0.pointer_fanout, ou.GET_N, ou.GET_S
    rng = np.random.default_rng(700)
    A, SA = lu.table(10, 7), ou.space_table(10, 7)
    kt = lu.KeyTree(lay0, A, depth=1)
    leaves = {(2,): ou.Blob(N, S, lay0.blob_len), (5, 0): ou.Blob(N, S, lay0.blob_len), (5, 4): ou.Blob(N, S, lay0.blob_len)}
    present, under = {}, {p: [] for p in leaves}
    for path in leaves:
        while len(under[path]) < 5:
            k = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            if k in present or kt.leaf(kt.locate(k)[0]).n_used() + 2 > 7:
                continue
            reminder = int(rng.integers(1, 2 ** 30))
            oid = reminder * F ** len(path) + sum(s * F ** d for d, s in enumerate(path))
            kt.add(k, oid)
            present[k] = ou.payload(rng, S)
            leaves[path].set(reminder, present[k])
            under[path].append(k)
    b = su.Builder(lay0)
    key = ou._put_tree(b, kt.leaves, kt.depth)
    low = b.pointer({0: b._put(bytes(leaves[(5, 0)].b), su.LEAF_T), 4: b._put(bytes(leaves[(5, 4)].b), su.LEAF_T)})
    obj = b.pointer({2: b._put(bytes(leaves[(2,)].b), su.LEAF_T), 5: low})
    path, reminder = (ou.GET_SPACE % F,), ou.GET_SPACE // F
    sl = ou.SpaceList(lay0.spaces_per_block)
    index, _, found = ou.find_space(sl.b, lay0.spaces_per_block, SA, reminder)
    assert index is not None and not found
    sl.plant(index, reminder, ou.DEFINED, key=(key[0], key[1], 1, key[2]), obj=(obj[0], obj[1], 1, obj[2]),
             next_object_id=1)
    leaf = b._put(bytes(sl.b), su.LEAF_T)
    img, lay = b.finish(b.pointer({path[0]: leaf}), slack=su.SLACK)
    store = object.__new__(ou.Store)
    store.SA, store.A, store.C = SA, A, len(A)
    store.img, store.lay = su.frozen(img), lay
    store.space_leaves = {path: leaf[1]}
    store.params = storm.GetParams(SA, lu.ks.ObjectListParams(A, store.C), ou.obs.BlobParams(N, S))
    return store, present, under


# ---- running a case on the host leg ------------------------------------------------------------------

def same_as_reference(store, space_id, keys, rows, all_keys, room=120, img=None, lay=None, in_stride=None, run=None):
    """The leg `run` (default: the host leg) against reference_update on the same image: image
    bytes, result bytes, report, code and message; then check_update. Returns (new image, layout,
    records, report)."""
    if img is None:
        img, lay = roomy(store, room)
    old = img.copy()
    want, want_img, want_rep, want_code, source, space = reference_update(old, lay, space_id, store, keys, rows)
    records, report = (run or host_update)(img, lay, store, space_id, keys, rows, in_stride)
    assert update_tuples(records) == want and not records["reserved"].any()
    assert img.tobytes() == want_img.tobytes()
    got = report.as_dict()
    got["get"].pop("space")
    assert got == want_rep
    assert report.code == want_code
    if source in ("space", "lookup", "objects"):
        case = ou.GetCase(on_image(store, old, lay), space_id, keys)
        saved = ou.GET_N, ou.GET_S
        ou.GET_N, ou.GET_S = blob_shape(store)
        try:
            source = ou.stage_message(case, source, space)
        finally:
            ou.GET_N, ou.GET_S = saved
    assert report.message == source
    if want_code == OK:
        check_update(store, old, lay, space_id, keys, rows, records, img, report, all_keys)
    else:
        assert img.tobytes() == old.tobytes() and (want_code == ENOSPC or not records["action"].any())
    return img, lay, records, report


# ---- the designed cases: each runs on the leg `run` (default: the host leg) ------------------------

def _rng(name):
    return np.random.default_rng([800, sum(name.encode())])


def case_one_key(run=None):
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    _, _, records, report = same_as_reference(store, ou.GET_SPACE, keys[7:8], new_rows(_rng("one"), 1, ou.GET_S), keys, run=run)
    assert report.n_written == 1 and report.n_dirty == (3, 1, 0, 1) and report.heights == 5


def case_whole_store(run=None):
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, keys, new_rows(_rng("all"), 80, ou.GET_S), keys, run=run)
    assert report.n_written == 80 and report.n_dirty[BLOB] == 80


def case_mixed_with_malformed_keys(run=None):
    """get_mixed's keys: the KEY error makes the get fail, so the store is untouched."""
    c = ou.get_mixed()
    _, _, records, report = same_as_reference(c.store, c.space_id, c.keys, new_rows(_rng("mixed"), len(c.keys), ou.GET_S),
                                              list(ou.get_store()[1]), run=run)
    assert report.code == EMISMATCH and report.get.first_bad == 40 and report.revision == 0


def case_mixed(run=None):
    """The same without the two malformed keys: absent keys and the orphan are NONE, the rest WRITTEN."""
    c = ou.get_mixed()
    store, present, orphan, _, _ = ou.get_store()
    keys = [k for k in c.keys if 1 <= len(k) <= 256]
    _, _, records, report = same_as_reference(store, c.space_id, keys, new_rows(_rng("mixed"), len(keys), ou.GET_S),
                                              list(present) + [orphan], run=run)
    assert [int(r["action"]) for r in records] == [WRITTEN if k in present else NONE for k in keys]
    assert report.n_written == 80 and orphan in keys


def case_duplicates(run=None):
    store, present, _, _, _ = ou.get_store()
    all_keys = list(present)
    keys = all_keys[:5] + [all_keys[9]] + all_keys[20:23] + [all_keys[9]] + all_keys[30:31] + [all_keys[9]] + all_keys[40:42]
    rows = new_rows(_rng("dup"), len(keys), ou.GET_S)
    img, lay, records, report = same_as_reference(store, ou.GET_SPACE, keys, rows, all_keys, run=run)
    assert [int(records[i]["action"]) for i in (5, 9, 11)] == [SUPERSEDED, SUPERSEDED, WRITTEN]
    assert (report.n_written, report.n_superseded) == (len(keys) - 2, 2)
    assert _get(img, lay, store, ou.GET_SPACE, [all_keys[9]])[1][0].tobytes() == rows[11]


def case_depth(depth, run=None):
    store, present = depth_store(depth)
    keys = list(present)
    pick = keys[::2]
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, pick, new_rows(_rng("depth"), len(pick), ou.GET_S), keys, run=run)
    assert report.n_dirty[POINTER] >= 1 + depth and report.heights == 3 + depth  # leaf .. the space tree's root
    if depth == 0:
        assert report.n_dirty == (1, 1, 0, 1)


def case_irregular(run=None):
    store, present, under = irregular_store()
    keys = [under[(2,)][0], under[(5, 4)][1], under[(5, 0)][2], under[(2,)][3]]
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, keys, new_rows(_rng("irr"), 4, ou.GET_S), list(present), run=run)
    assert report.n_dirty == (3, 1, 0, 3) and report.heights == 5  # the root block: children of heights 0 and 1


def case_two_spaces(same_leaf, run=None):
    store, present, other = two_space_store(same_leaf)
    keys = list(present[ou.GET_SPACE])
    pick = keys[1::3]
    old, lay = roomy(store, 120)
    before = _get(old, lay, store, other, list(present[other]))
    img, lay, _, report = same_as_reference(store, ou.GET_SPACE, pick, new_rows(_rng("two"), len(pick), ou.GET_S), keys,
                                            img=old, lay=lay, run=run)
    after = _get(img, lay, store, other, list(present[other]))
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert report.n_dirty[SPACELIST] == 1 and report.n_dirty[POINTER] == 2  # the space tree's root, the object tree's


def case_two_in_a_row(run=None):
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    rng = _rng("row")
    img0, lay = roomy(store, 120)
    first = img0.copy()
    same_as_reference(store, ou.GET_SPACE, keys[:30], new_rows(rng, 30, ou.GET_S), keys, img=first, lay=lay, run=run)
    second = first.copy()
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, keys[20:50], new_rows(rng, 30, ou.GET_S), keys, img=second,
                                        lay=lay, run=run)
    assert report.revision == 5
    for earlier in (img0, first):  # the old snapshots, against both earlier singularities
        back = second.copy()
        back[:72] = earlier[:72]
        L = struct.unpack_from("<Q", earlier, 64)[0]
        assert _blocks(back, lay, 0, L + 1) == _blocks(earlier, lay, 0, L + 1)
        assert scrub.scrub_host(back, lay).ok
        want, got = _get(earlier, lay, store, ou.GET_SPACE, keys), _get(back, lay, store, ou.GET_SPACE, keys)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def case_room(run=None):
    """Exactly D free blocks: OK. One fewer: STORMCK_ENOSPC, the image untouched."""
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    pick, rows = keys[:12], new_rows(_rng("room"), 12, ou.GET_S)
    img, lay = roomy(store, 120)
    D = sum(same_as_reference(store, ou.GET_SPACE, pick, rows, keys, img=img, lay=lay, run=run)[3].n_dirty)
    img, lay = roomy(store, D)
    assert same_as_reference(store, ou.GET_SPACE, pick, rows, keys, img=img, lay=lay, run=run)[3].code == OK
    img, lay = roomy(store, D - 1)
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, pick, rows, keys, img=img, lay=lay, run=run)
    assert (report.code, report.message) == (ENOSPC, ENOSPC_TEXT)


def case_damage(where, run=None):
    """A flipped byte: EMISMATCH with the get's text, the image untouched byte for byte."""
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    img, lay = roomy(store, 120)
    res = _get(img, lay, store, ou.GET_SPACE, keys[:1])[0][0]
    index = su.reference_scrub(img, lay)[2]
    leaf = int(res["object_address"])
    address, byte = {"blob leaf": (leaf, 727), "object pointer block": (index[leaf][0], 3),
                     "spacelist leaf": (store.space_leaves[(ou.GET_SPACE % 10,)], 725), "singularity": (0, 20)}[where]
    img[address * lay.block_size + byte] ^= 0x10
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, keys, new_rows(_rng("dmg"), 80, ou.GET_S), keys, img=img, lay=lay,
                                        run=run)
    assert report.code == EMISMATCH and report.message and report.n_written == 0


def case_nothing_to_write(name, run=None):
    c = ou.get_nothing_found() if name == "nothing found" else ou.get_space_case(name)
    _, _, records, report = same_as_reference(c.store, c.space_id, c.keys, new_rows(_rng("none"), len(c.keys), ou.GET_S),
                                              list(ou.get_store()[1]), run=run)
    assert report.code == OK and report.n_written == 0 and report.revision == 3 and not records["action"].any()


def case_count(n, run=None):
    """Keys repeated to reach n: duplicates across waves and workgroups."""
    c = ou.get_count(n)
    store, present, orphan, _, _ = ou.get_store()
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, c.keys, new_rows(_rng("count"), n, ou.GET_S),
                                        list(present) + [orphan], in_stride=13 + n % 4, run=run)
    assert report.n_written + report.n_superseded == sum(k in present for k in c.keys)
    assert (report.n_superseded > 0) == (n > 96)


def case_size(S, gap, run=None):
    """Objects of S bytes (both forms of the store), rows in_stride = S + gap apart."""
    store, present = size_store(S)
    keys = list(present)
    _, _, _, report = same_as_reference(store, ou.GET_SPACE, keys, new_rows(_rng("size"), len(keys), S), keys,
                                        in_stride=S + gap, run=run)
    assert report.n_written == len(keys)


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 300)
GAPS = (0, 1, 3)
CASES = {"one key": case_one_key, "whole store": case_whole_store, "mixed, malformed keys": case_mixed_with_malformed_keys,
         "mixed": case_mixed, "duplicates": case_duplicates, "irregular": case_irregular,
         "two in a row": case_two_in_a_row, "room": case_room}
CASES.update({f"depth {d}": functools.partial(case_depth, d) for d in (0, 1, 2)})
CASES.update({f"two spaces, {'one leaf' if s else 'two leaves'}": functools.partial(case_two_spaces, s) for s in (True, False)})
CASES.update({f"damaged {w}": functools.partial(case_damage, w)
              for w in ("blob leaf", "object pointer block", "spacelist leaf", "singularity")})
CASES.update({n: functools.partial(case_nothing_to_write, n)
              for n in ("absent space", "invalid space", "free object root", "nothing found")})
CASES.update({f"n = {n}": functools.partial(case_count, n) for n in COUNTS})
CASES.update({f"S = {S}, in_stride = S + {g}": functools.partial(case_size, S, g) for S in ou.SIZES for g in GAPS})


# ---- the seeded fuzz -----------------------------------------------------------------------------------

FUZZ_SEEDS = 44
FUZZ_STREAM = 400  # second word of the rngs' seeds: apart from the other fuzzes


def fuzz_case(seed):
    """(store, keys, rows, all_keys): a random subset of the keys with repeats, absent keys mixed
    in and random rows, over get_store() (even seeds) or a depth-1 store (odd seeds). Every fourth
    seed takes every key, so that every leaf of the tree is dirty."""
    rng = np.random.default_rng([seed, FUZZ_STREAM])
    if seed % 2 == 0:
        store, present = ou.get_store()[:2]
    else:
        store, present = depth_store(1)
    pool = list(present)
    if seed % 4 == 3:
        keys = [pool[int(i)] for i in rng.permutation(len(pool))] + [pool[int(i)] for i in rng.integers(0, len(pool), 5)]
    else:
        keys = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(1, 60)))]
    if seed % 3 == 0:
        for k in ou._absent_keys(rng, int(rng.integers(1, 8))):
            keys.insert(int(rng.integers(0, len(keys) + 1)), k)
    return store, keys, new_rows(rng, len(keys), ou.GET_S), pool


def run_fuzz(seed, run=None):
    store, keys, rows, pool = fuzz_case(seed)
    return same_as_reference(store, ou.GET_SPACE, keys, rows, pool, in_stride=13 + seed % 4, run=run)
