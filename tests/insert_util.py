"""TEST INFRASTRUCTURE for the insert tests (tests/test_insert.py, tests/test_insert_fuzz.py and
their GPU twins): storm.Set for new keys whose leaves have room (include/stormck.h "insert").

* ``reference_insert``: a pure-Python serial restatement of rules A to H on ``lookup_util.Leaf``
  (``Leaf.insert`` / ``store_key``) and ``objects_util.Blob`` (``Blob.set``);
* ``check_insert``: the semantic checks, which do not rest on that restatement: the scrub and the
  get as judges, the bytes that must not change, the old snapshot, NextObjectID, and a second
  call that finds every inserted key and hands it to the update;
* the stores and the designed cases both legs run.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import oracle as o
from storm_amd import objectstore as obs
from storm_amd import scrub, storm
from storm_amd.scrub import BLOB, OBJECTLIST, POINTER, SPACELIST
from tests import lookup_util as lu
from tests import objects_util as ou
from tests import scrub_util as su
from tests import update_util as uu

NONE, INSERTED, REPEATED = 0, 1, 2
R_NONE, R_SPACE, R_EXISTS, R_NO_LEAF, R_KEY_SPLIT, R_NO_SLOT, R_KEY_FULL, R_MALFORMED, R_CROWDED, R_CUT = range(10)
MAX_PER_LEAF = 2048
INSERT_FIELDS = ("object_id", "key_address", "object_address", "key_index", "object_index", "stage", "status", "action",
                 "reason", "wrote")
OK, EMISMATCH, ENOSPC = 0, -5, -6
ENOSPC_TEXT = "insert: the image has no room for the dirty blocks (LastAllocatedBlock + dirty blocks >= n_blocks)"
FOUND, ABSENT, NO_SLOT = ou.FOUND, ou.ABSENT, ou.NO_SLOT
SPACE = ou.GET_SPACE
KEY_ORIGIN = 1 << 31  # update_plan.h kUpdateKeyOrigin


# ---- the reference ---------------------------------------------------------------------------------

def _located(l, failed=False):
    """A key's result as the locate leaves it, from its lookup result (lookup_util.RESULT_FIELDS)."""
    oid, address, _, index, probes, status = l
    reason = R_EXISTS if status == FOUND else R_NO_LEAF if status == ABSENT and probes == 0 else R_NONE
    return dict(object_id=oid if status == FOUND else 0, key_address=address, object_address=0, key_index=index,
                object_index=NO_SLOT, stage=1, status=status, action=NONE, reason=R_NONE if failed else reason, wrote=0)


def _leaf_at(img, lay, address, C):
    leaf = lu.Leaf(C)
    leaf.b[:] = img[address * lay.block_size:address * lay.block_size + len(leaf.b)].tobytes()
    return leaf


def _blob_at(img, lay, address, N, S):
    blob = ou.Blob(N, S, lay.blob_len)
    blob.b[:] = img[address * lay.block_size:address * lay.block_size + lay.blob_len].tobytes()
    return blob


def _judge_key(leaf, A, key, reminder, link):
    """Rule B for one key on a lookup_util.Leaf: (verdict, index, link). INSERTED changes the leaf."""
    C = leaf.C
    oid, index, _, found, _ = lu.probe(leaf.b, C, A, key, reminder)
    if found:
        return REPEATED, index, oid
    if leaf.n_used() >= C * 3 // 4:
        return R_KEY_SPLIT, None, None
    if index == lu.NO_SLOT:
        return R_NO_SLOT, None, None
    need = (len(key) + 31) // 32
    if leaf.n_used() + need > C:
        return R_KEY_FULL, None, None
    f = leaf.free_index()
    for _ in range(need):  # the free list, before anything changes
        if f >= C:
            return R_MALFORMED, None, None
        f = f + 1 if leaf.n_used() == 0 else leaf.next_pointer(f)
    leaf.plant(index, key, reminder, link)  # setKeyInChunks (Leaf.store_key) and ObjectLinks
    return INSERTED, index, link


def _tuple(r):
    return tuple(r[f] for f in INSERT_FIELDS)


def reference_insert(img, lay, space_id, store, keys, rows):
    """Rules A to H of include/stormck.h "insert", one key at a time. Returns (results as
    INSERT_FIELDS tuples, the new image, the report as InsertReport.as_dict() without its space,
    the return code, the message source: a text, or "space" / "lookup" / "objects", the space's
    reference result, the new IDs)."""
    st = uu.on_image(store, img, lay)
    N, S = uu.blob_shape(st)
    C, A, n = store.C, store.A, len(keys)
    no_lookup = dict(n_status=(0,) * 8, n_probed=0, probes=0, n_malformed=0, first_bad=n,
                     trace=dict(n_status=(0,) * 7, blocks_hashed=(0, 0), bytes_hashed=0, first_bad=n, levels=0))
    rep = dict(n_inserted=0, n_repeated=0, n_none=[0] * 10, first_id=0, next_object_id=0, cut=0, limit=n,
               n_dirty=(0, 0, 0, 0), bytes_copied=0, bytes_hashed=0, revision=0, last_allocated=0, first_new=0, heights=0,
               lookup=no_lookup)

    def done(results, out, code, source, space=None, ids=()):
        for r in results:
            if r["action"] == INSERTED:
                rep["n_inserted"] += 1
            elif r["action"] == REPEATED:
                rep["n_repeated"] += 1
            else:
                rep["n_none"][r["reason"]] += 1
        rep["n_none"] = tuple(rep["n_none"])
        return [_tuple(r) for r in results], out, rep, code, source, space, list(ids)

    if n == 0:
        return done([], img.copy(), OK, "")
    # A. locate
    s = bytearray(img[:72].tobytes())
    expected = struct.unpack_from("<Q", s, 0)[0]
    s[0:8] = bytes(8)
    computed = o.xxh64(bytes(s))
    at_space = dict(object_id=0, key_address=0, object_address=0, key_index=NO_SLOT, object_index=NO_SLOT, stage=0,
                    action=NONE, wrote=0)
    if computed != expected:
        text = f"checksum mismatch for block 0, computed: 0x{computed:x}, expected: 0x{expected:x}"
        return done([dict(at_space, status=ou.MISMATCH, reason=R_NONE) for _ in keys], img.copy(), EMISMATCH, text)
    sres, _, _ = ou.reference_spaces(img, lay, struct.unpack_from("<QQ", s, 32), s[56], store.SA, [space_id], True)
    space = sres[0]
    if space[9] != FOUND:
        bad = space[9] in obs.BAD
        return done([dict(at_space, status=space[9], reason=R_NONE if bad else R_SPACE) for _ in keys], img.copy(),
                    EMISMATCH if bad else OK, "space" if bad else "", space)
    lres, lrep, _ = lu.reference_lookup(img, lay, space[0][:2], space[7], C, A, keys, True)
    rep["lookup"] = lrep
    failed = lrep["first_bad"] < n
    results = [_located(l, failed) for l in lres]
    if failed:
        return done(results, img.copy(), EMISMATCH, "lookup", space)
    revision, last = struct.unpack_from("<Q", img, 16)[0], struct.unpack_from("<Q", img, 64)[0]
    first_id = space[2]
    rep.update(revision=revision, last_allocated=last, first_id=first_id, next_object_id=first_id)
    # B. the key stage: storm's loop inside each leaf
    groups = {}
    for i, l in enumerate(lres):
        if l[5] == ABSENT and l[4] != 0:
            groups.setdefault(l[1], []).append(i)
    for address, g in groups.items():
        if len(g) > MAX_PER_LEAF:
            for i in g:
                results[i]["reason"] = R_CROWDED
            continue
        leaf = _leaf_at(img, lay, address, C)
        for i in g:
            verdict, index, link = _judge_key(leaf, A, keys[i], lres[i][2], i)
            if verdict in (INSERTED, REPEATED):
                results[i].update(action=verdict, key_index=index, object_id=link)
            else:
                results[i]["reason"] = verdict
    # C. the IDs
    key_of = [i for i, r in enumerate(results) if r["action"] == INSERTED]
    rank_of = {i: r for r, i in enumerate(key_of)}
    ids = [first_id + r for r in range(len(key_of))]
    for r in results:
        if r["action"] != NONE:
            r["object_id"] = first_id + rank_of[r["object_id"]]
    # D. the object stage
    ores, _, orep, _ = ou.reference_objects(img, lay, space[1][:2], space[8], N, S, ids, True)
    if orep["first_bad"] < len(ids):
        return done([_located(l, True) for l in lres], img.copy(), EMISMATCH, "objects", space, ids)
    cut, blobs = len(ids), {}
    for r, res in enumerate(ores):
        if res[5] == ABSENT and res[4] == 0:
            cut = min(cut, r)  # a Free reference: storm allocates
        else:
            blobs.setdefault(res[1], []).append(r)
    for address, g in blobs.items():
        if len(g) > MAX_PER_LEAF:
            cut = min(cut, g[0])
            continue
        blob = _blob_at(img, lay, address, N, S)
        for r in g:
            k, _, found = ou.find_object(blob.b, N, S, ores[r][2])
            if (k is None or not found) and blob.n_used() >= N * 3 // 4 or k is None:
                cut = min(cut, r)
                break
            blob.set(ores[r][2], bytes(S))
            results[key_of[r]].update(object_address=address, object_index=k, stage=2, status=FOUND if found else ABSENT)
    # E. the cut
    limit = key_of[cut] if cut < len(ids) else n
    for i in range(limit, n):
        results[i] = dict(_located(lres[i]), reason=R_CUT)
    rep.update(cut=cut, limit=limit)
    if cut == 0:
        return done(results, img.copy(), OK, "", space, ids)
    # G. the dirty forest
    blocks = {}
    for b in uu._walk(img, lay, struct.unpack_from("<Q", img, 40)[0], int(img[56]), 0, 0, space_id, SPACELIST):
        blocks.setdefault(b[0], b)
    for r in range(cut):
        i = key_of[r]
        kpath = uu._walk(img, lay, space[0][1], space[7], space[3], space[5] | KEY_ORIGIN, o.xxh64(keys[i]), OBJECTLIST)
        opath = uu._walk(img, lay, space[1][1], space[8], space[3], space[5], ids[r], BLOB)
        assert kpath[-1][0] == lres[i][1] and opath[-1][0] == ores[r][1]
        for b in kpath + opath:
            assert blocks.setdefault(b[0], b) == b
    kids = {}
    for a, (_, _, parent, _) in blocks.items():
        kids.setdefault(parent, []).append(a)

    def height(a):
        return 1 + max(height(k) for k in kids[a]) if a in kids else 0
    order = sorted(blocks, key=lambda a: (height(a), a))
    D = len(order)
    if last + D >= lay.n_blocks or last >= lay.n_blocks:
        return done(results, img.copy(), ENOSPC, ENOSPC_TEXT, space, ids)
    new = {a: last + 1 + k for k, a in enumerate(order)}
    # F. the rows: storm's last Set wins (wrote says what a slot received: nothing without room)
    winner = {}
    for i in range(limit):
        if results[i]["action"] != NONE:
            winner[results[i]["object_id"]] = i
    for i in winner.values():
        results[i]["wrote"] = 1
    # H. write
    out, bs, lens = img.copy(), lay.block_size, su.kind_lens(lay)
    for a in order:
        out[new[a] * bs:(new[a] + 1) * bs] = img[a * bs:(a + 1) * bs]
    for address, g in groups.items():
        if address not in new:
            continue
        leaf = _leaf_at(img, lay, address, C)
        for i in g:
            if i < limit and results[i]["action"] == INSERTED:  # storm's loop over the accepted keys
                assert leaf.insert(A, keys[i], lres[i][2], results[i]["object_id"]) == results[i]["key_index"]
        out[new[address] * bs:new[address] * bs + len(leaf.b)] = np.frombuffer(bytes(leaf.b), np.uint8)
    for address, g in blobs.items():
        if address not in new:
            continue
        blob = _blob_at(img, lay, address, N, S)
        for r in g:
            if r < cut:
                assert blob.set(ores[r][2], rows[winner[ids[r]]]) == results[key_of[r]]["object_index"]
        out[new[address] * bs:new[address] * bs + lay.blob_len] = np.frombuffer(bytes(blob.b), np.uint8)
    at = new[space[3]] * bs + 72 * space[5] + 8
    out[at:at + 8] = np.frombuffer(struct.pack("<Q", first_id + cut), np.uint8)
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
        if pkind == POINTER:
            at, tat = pat + 24 * slot, pat + 24 * lay.pointer_fanout + slot
        elif slot & KEY_ORIGIN:
            k = slot & ~KEY_ORIGIN
            at, tat = pat + 72 * k + 16, pat + 72 * k + 64
        else:
            at, tat = pat + 72 * slot + 40, pat + 72 * slot + 65
        out[at:at + 24] = np.frombuffer(struct.pack("<QQQ", cs, new[a], revision + 1), np.uint8)
        out[tat] = typ
    struct.pack_into("<Q", sing, 16, revision + 1)
    struct.pack_into("<Q", sing, 64, last + D)
    sing[0:8] = bytes(8)
    sing[0:8] = struct.pack("<Q", o.xxh64(bytes(sing)))
    out[:72] = np.frombuffer(bytes(sing), np.uint8)
    rep.update(n_dirty=tuple(n_dirty), bytes_copied=D * bs, bytes_hashed=72 + sum(lens[blocks[a][1]] for a in order),
               revision=revision + 1, last_allocated=last + D, first_new=last + 1, heights=1 + height(order[-1]),
               next_object_id=first_id + cut)
    return done(results, out, OK, "", space, ids)


# ---- running a case ---------------------------------------------------------------------------------

def insert_tuples(records):
    return [tuple(int(rec[f]) for f in INSERT_FIELDS) for rec in records]


def host_insert(img, lay, store, space_id, keys, rows, in_stride=None, **kw):
    """stormck_insert_host on `img`, in place: (records, report)."""
    S = uu.blob_shape(store)[1]
    p = lu.pack(keys, "flat")
    return storm.insert_host(img, lay, space_id, store.params, p["keys"], uu.pack_rows(rows, S, in_stride or S + 3),
                             offsets=p["offsets"], lens=p["lens"], **kw)


def _get(img, lay, store, space_id, keys):
    return storm.get_host(img, lay, space_id, store.params, **lu.pack(keys, "flat"), out_stride=uu.blob_shape(store)[1])


def _message(store, old, lay, space_id, keys, source, space, ids):
    """The words of the failing stage's own host entry point."""
    if source not in ("space", "lookup", "objects"):
        return source
    st = uu.on_image(store, old, lay)
    if source == "objects":
        return obs.get_objects_host(old, lay, space[1], space[8], st.params.objects, np.array(ids, np.uint64))[2].message
    case = ou.GetCase(st, space_id, keys)
    return ou.stage_message(case, source, space)


def check_insert(store, old, lay, space_id, keys, rows, records, new, report, existing):
    """The semantic checks of one insert that returned OK: `old` and `new` are the image before and
    after, `existing` every key the space held before."""
    bs, n = lay.block_size, lay.n_blocks
    S = uu.blob_shape(store)[1]
    assert new.size == old.size and report.code == OK
    L = struct.unpack_from("<Q", old, 64)[0]
    old_rev = struct.unpack_from("<Q", old, 16)[0]
    D = sum(report.n_dirty)
    actions = [int(r["action"]) for r in records]
    if report.cut == 0:  # a batch that changes nothing makes no revision
        assert new.tobytes() == old.tobytes() and D == 0 and report.first_new == 0 and INSERTED not in actions
        assert report.next_object_id == report.first_id
        return
    assert report.cut == report.n_inserted == actions.count(INSERTED)
    # the scrub: the new image is clean, and so is the old one
    s_old, s_new = scrub.scrub_host(old, lay, reachable=True), scrub.scrub_host(new, lay, reachable=True)
    assert s_old.ok and s_new.ok
    # the bytes that do not change, the singularity, the guards
    assert uu._blocks(new, lay, 1, L + 1) == uu._blocks(old, lay, 1, L + 1)
    assert new[(L + D + 1) * bs:].tobytes() == old[(L + D + 1) * bs:].tobytes()
    assert new[n * bs:].tobytes() == bytes([uu.GUARD]) * (new.size - n * bs)
    assert new[72:bs].tobytes() == old[72:bs].tobytes()
    assert (struct.unpack_from("<Q", new, 16)[0], struct.unpack_from("<Q", new, 64)[0]) == (old_rev + 1, L + D)
    assert (report.revision, report.last_allocated, report.first_new) == (old_rev + 1, L + D, L + 1)
    # the old snapshot
    back = new.copy()
    back[:72] = old[:72]
    assert uu._blocks(back, lay, 0, L + 1) == uu._blocks(old, lay, 0, L + 1)
    assert scrub.scrub_host(back, lay).ok
    g_old, r_old, _ = _get(old, lay, store, space_id, existing)
    g_back, r_back, _ = _get(back, lay, store, space_id, existing)
    assert g_back.tobytes() == g_old.tobytes() and r_back.tobytes() == r_old.tobytes()
    # the get: the winning row of every INSERTED key, the old object of every key that existed
    g_new, r_new, rep_new = _get(new, lay, store, space_id, existing)
    assert rep_new.ok and r_new.tobytes() == r_old.tobytes()
    for f in ("object_id", "stage", "status"):
        assert (g_new[f] == g_old[f]).all()
    last_row = {}
    for i, r in enumerate(records):
        if r["action"] != NONE:
            last_row[int(r["object_id"])] = i
    inserted = [i for i, a in enumerate(actions) if a == INSERTED]
    assert sorted(last_row) == list(range(report.first_id, report.first_id + report.cut))
    assert sorted(int(records[i]["object_id"]) for i in inserted) == sorted(last_row)
    assert {i for i, r in enumerate(records) if r["wrote"]} == set(last_row.values())
    if inserted:
        g_ins, r_ins, rep_ins = _get(new, lay, store, space_id, [keys[i] for i in inserted])
        assert rep_ins.ok
        for j, i in enumerate(inserted):
            assert (g_ins[j]["stage"], g_ins[j]["status"]) == (2, FOUND) and g_ins[j]["object_id"] == records[i]["object_id"]
            assert r_ins[j].tobytes() == rows[last_row[int(records[i]["object_id"])]]
        g_was = _get(old, lay, store, space_id, [keys[i] for i in inserted])[0]
        assert not (g_was["status"] == FOUND).any()
    # NextObjectID
    space_new = _get(new, lay, store, space_id, keys[:1])[2].space
    assert int(space_new["next_object_id"]) == report.first_id + report.cut == report.next_object_id
    # a second call finds them, and the update rewrites them
    again = new.copy()
    pick = [keys[i] for i in inserted]
    rec2, rep2 = host_insert(again, lay, store, space_id, pick, [rows[i] for i in inserted])
    assert rep2.code == OK and again.tobytes() == new.tobytes()
    assert all((r["action"], r["reason"]) == (NONE, R_EXISTS) for r in rec2)
    if L + 2 * D + 2 < n:
        fresh = uu.new_rows(np.random.default_rng(9), len(pick), S)
        rec3, rep3 = uu.host_update(again, lay, store, space_id, pick, fresh)
        assert rep3.code == OK and rep3.n_written == len(pick)
        assert [x.tobytes() for x in _get(again, lay, store, space_id, pick)[1]] == fresh


def same_as_reference(store, space_id, keys, rows, existing, room=160, img=None, lay=None, in_stride=None, run=None):
    """The leg `run` (default: the host leg) against reference_insert on the same image: image
    bytes, results, report, code and message; then check_insert. Returns (new image, layout,
    records, report)."""
    if img is None:
        img, lay = uu.roomy(store, room)
    old = img.copy()
    want, want_img, want_rep, want_code, source, space, ids = reference_insert(old, lay, space_id, store, keys, rows)
    records, report = (run or host_insert)(img, lay, store, space_id, keys, rows, in_stride)
    assert insert_tuples(records) == want and not records["reserved"].any()
    assert img.tobytes() == want_img.tobytes()
    got = report.as_dict()
    got.pop("space")
    assert got == want_rep
    assert report.code == want_code
    assert report.message == _message(store, old, lay, space_id, keys, source, space, ids)
    if want_code == OK:
        check_insert(store, old, lay, space_id, keys, rows, records, img, report, existing)
    else:
        assert img.tobytes() == old.tobytes()
        assert want_code == ENOSPC or not records["action"].any() and not records["reason"].any()
    return img, lay, records, report


# ---- stores ------------------------------------------------------------------------------------------

def _fresh_keys(rng, n, length=lambda rng: int(rng.integers(1, 60))):
    return [rng.integers(0, 256, length(rng), dtype=np.uint8).tobytes() for _ in range(n)]


def build_store(key_depth, object_depth, n_keys, seed=0, N=ou.GET_N, S=ou.GET_S, lay=None, fill=5, per_blob=4,
                all_key_leaves=None, edit=None, next_above=True, ensure_blobs=30, C=10):
    """(Store, existing keys -> object, KeyTree, ObjectTree): one Defined space (NextObjectID 5321)
    whose stored IDs lie just below NextObjectID (above it with next_above False), so that the new
    IDs meet the existing blob leaves. fill: a key leaf takes keys while NUsedChunks + 2 <= fill;
    per_blob: slots used per blob leaf. edit(kt, ot) changes the trees before they are signed."""
    lay = lay or ou.TEST_LAYOUT
    rng = np.random.default_rng([900, seed])
    A, SA = lu.table(C, 7), ou.space_table(10, 7)
    kt, ot = lu.KeyTree(lay, A, depth=key_depth), ou.ObjectTree(lay, N, S, depth=object_depth)
    if all_key_leaves or all_key_leaves is None and key_depth <= 1:
        for t in range(lay.pointer_fanout ** key_depth):
            kt.leaf(_digits(t, lay.pointer_fanout, key_depth))
    F = lay.pointer_fanout  # at most what the trees hold at these fill levels
    n_keys = min(n_keys, F ** key_depth * max(1, (fill - 1) // 2), F ** object_depth * per_blob)
    first, present, t, tries = SPACE + 1000, {}, 0, 0
    while len(present) < n_keys:
        tries += 1
        assert tries < 200 * n_keys + 200, "the key tree has no room for that many keys"
        k = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        if k in present or kt.leaf(kt.locate(k)[0]).n_used() + 2 > fill:
            continue
        while True:
            assert t < 5000, "the object tree has no room for that many objects"
            oid = first - 1 - t if next_above else first + 3 + 7 * t
            t += 1
            if ot.leaf(ot.locate(oid)[0]).n_used() < per_blob:
                break
        kt.add(k, oid)
        present[k] = ou.payload(rng, S)
        ot.set(oid, present[k])
    for r in range(ensure_blobs):  # the leaves the first new IDs meet, empty when no stored ID lives there
        ot.leaf(ot.locate(first + r)[0])
    if edit:
        edit(kt, ot)
    store = ou.Store({SPACE: (ou.DEFINED, kt, ot)}, SA, A, lay=lay, blob=(N, S))
    return store, present, kt, ot


def _digits(t, F, depth):
    path = []
    for _ in range(depth):
        path.append(t % F)
        t //= F
    return tuple(path)


@functools.lru_cache(maxsize=None)
def plain_store(key_depth=1, object_depth=1, n_keys=24, seed=0, ensure_blobs=30):
    return build_store(key_depth, object_depth, n_keys, seed, ensure_blobs=ensure_blobs)


def keys_for_leaf(kt, path, rng, lengths, taken=()):
    """Fresh keys of the given lengths that live in the key leaf at `path`."""
    out = []
    for length in lengths:
        while True:
            k = lu.key_in(kt, path, rng, length)
            if k not in taken and k not in out:
                out.append(k)
                break
    return out


# ---- the designed cases: each runs on the leg `run` (default: the host leg) --------------------------

def _rng(name):
    return np.random.default_rng([901, sum(name.encode())])


def _run(store, present, keys, name, run=None, S=ou.GET_S, **kw):
    return same_as_reference(store, SPACE, keys, uu.new_rows(_rng(name), len(keys), S), list(present), run=run, **kw)


def _reasons(records):
    return [(int(r["action"]), int(r["reason"])) for r in records]


def case_one_key(run=None):
    store, present, kt, _ = plain_store()
    _, _, rec, rep = _run(store, present, _fresh_keys(_rng("one"), 1), "one", run)
    assert _reasons(rec) == [(INSERTED, R_NONE)] and rep.cut == 1 and rep.n_dirty == (3, 1, 1, 1)
    assert int(rec[0]["object_id"]) == SPACE + 1000 and rec[0]["wrote"] == 1


def _some_leaf(kt, used_at_most=3):
    return next(p for p, leaf in sorted(kt.leaves.items()) if leaf.n_used() <= used_at_most)


def case_lengths_into_one_leaf(run=None):
    """Lengths 1, 32 and 33 fit one leaf (4 chunks); 256 needs 8 chunks and meets KEY_FULL or the trigger."""
    store, present, kt, _ = build_store(1, 1, 12, seed=1, fill=3)
    path = _some_leaf(kt, 1)
    keys = keys_for_leaf(kt, path, _rng("len"), (1, 32, 33, 256))
    _, _, rec, rep = _run(store, present, keys, "len", run)
    assert [a for a, _ in _reasons(rec)][:3] == [INSERTED] * 3 and _reasons(rec)[3][0] == NONE


def case_long_key(run=None):
    """A 256-byte key into a leaf that is empty: 8 of 10 chunks."""
    store, present, kt, _ = build_store(1, 1, 12, seed=2, all_key_leaves=True)
    path = next(p for p, leaf in sorted(kt.leaves.items()) if leaf.n_used() == 0)
    keys = keys_for_leaf(kt, path, _rng("long"), (256, 1))
    _, _, rec, rep = _run(store, present, keys, "long", run)
    assert _reasons(rec) == [(INSERTED, R_NONE), (NONE, R_KEY_SPLIT)]


def case_trigger_mid_batch(run=None):
    store, present, kt, _ = plain_store()
    path = _some_leaf(kt, 4)
    keys = keys_for_leaf(kt, path, _rng("trig"), (20,) * 8)
    _, _, rec, rep = _run(store, present, keys, "trig", run)
    got = _reasons(rec)
    assert (INSERTED, R_NONE) in got and got[-1] == (NONE, R_KEY_SPLIT)
    assert got == sorted(got, key=lambda x: x[0] != INSERTED)  # accepted first, then the trigger


def case_full_then_shorter(run=None):
    """NUsedChunks 4 of 10: a 256-byte key (8 chunks) is KEY_FULL, the 10-byte key after it goes in."""
    store, present, kt, _ = build_store(1, 1, 20, seed=3, fill=4)
    path = next(p for p, leaf in sorted(kt.leaves.items()) if leaf.n_used() in (3, 4))
    keys = keys_for_leaf(kt, path, _rng("full"), (256, 10))
    _, _, rec, rep = _run(store, present, keys, "full", run)
    assert _reasons(rec) == [(NONE, R_KEY_FULL), (INSERTED, R_NONE)] and rep.limit == 2


def case_empty_leaf(run=None):
    store, present, kt, _ = build_store(1, 1, 12, seed=2, all_key_leaves=True)
    path = next(p for p, leaf in sorted(kt.leaves.items()) if leaf.n_used() == 0)
    keys = keys_for_leaf(kt, path, _rng("empty"), (40, 5))
    _, _, rec, rep = _run(store, present, keys, "empty", run)
    assert _reasons(rec) == [(INSERTED, R_NONE)] * 2


def _edited(seed, edit, **kw):
    return build_store(1, 1, 16, seed=seed, edit=edit, **kw)


def case_invalid_slot_reused(run=None):
    """Every slot of one leaf that holds no key is Invalid but one: the first Invalid slot on the
    key's probe sequence is the one it receives."""
    def edit(kt, ot):
        leaf = kt.leaves[_some_leaf(kt, 2)]
        free = [i for i in range(leaf.C) if leaf.state(i) == lu.FREE]
        for i in free[:-1]:
            leaf.state(i, lu.INVALID)
    store, present, kt, _ = _edited(4, edit)
    path = next(p for p, leaf in sorted(kt.leaves.items()) if any(leaf.state(i) == lu.INVALID for i in range(10)))
    keys = keys_for_leaf(kt, path, _rng("inv"), (9, 9))
    _, _, rec, rep = _run(store, present, keys, "inv", run)
    assert _reasons(rec) == [(INSERTED, R_NONE)] * 2
    assert all(kt.leaves[path].state(int(r["key_index"])) == lu.INVALID for r in rec)


def case_no_slot(run=None):
    def edit(kt, ot):
        leaf = kt.leaves[_some_leaf(kt, 2)]
        for i in range(leaf.C):
            if leaf.state(i) == lu.FREE:
                leaf.state(i, 7)  # no state storm knows: skipped by the probe
    store, present, kt, _ = _edited(5, edit)
    path = next(p for p, leaf in sorted(kt.leaves.items()) if any(leaf.state(i) == 7 for i in range(10)))
    keys = keys_for_leaf(kt, path, _rng("noslot"), (9,))
    _, _, rec, rep = _run(store, present, keys, "noslot", run)
    assert _reasons(rec) == [(NONE, R_NO_SLOT)] and rep.cut == 0


def case_malformed_free_list(run=None):
    """FreeChunkIndex's chain leaves the leaf after one chunk: a 40-byte key (2 chunks) is MALFORMED
    and leaves no trace; a 5-byte key after it takes the one chunk."""
    def edit(kt, ot):
        leaf = next(leaf for _, leaf in sorted(kt.leaves.items()) if 1 <= leaf.n_used() <= 3)
        leaf.next_pointer(leaf.free_index(), 60000)
    store, present, kt, _ = _edited(6, edit)
    path = next(p for p, leaf in sorted(kt.leaves.items())
                if leaf.n_used() and leaf.free_index() < 10 and leaf.next_pointer(leaf.free_index()) == 60000)
    keys = keys_for_leaf(kt, path, _rng("mal"), (40, 5, 5))
    _, _, rec, rep = _run(store, present, keys, "mal", run)
    assert _reasons(rec) == [(NONE, R_MALFORMED), (INSERTED, R_NONE), (NONE, R_MALFORMED)]


def case_repeats(run=None):
    """A new key three times with three rows, between other keys: one ID, the last row, ranks by
    first occurrence."""
    store, present, kt, _ = plain_store()
    a, b, c, d = _fresh_keys(_rng("rep"), 4)
    keys = [a, b, c, b, d, b]
    _, _, rec, rep = _run(store, present, keys, "rep", run)
    assert [int(r["action"]) for r in rec] == [INSERTED, INSERTED, INSERTED, REPEATED, INSERTED, REPEATED]
    first = SPACE + 1000
    assert [int(r["object_id"]) for r in rec] == [first, first + 1, first + 2, first + 1, first + 3, first + 1]
    assert [int(r["wrote"]) for r in rec] == [1, 0, 1, 0, 1, 1]


def case_mixed_with_existing_and_no_leaf(run=None):
    """EXISTS and NO_LEAF keys between new ones consume no IDs (a key tree of depth 2 with few leaves)."""
    store, present, kt, _ = plain_store(2, 1, 30, 1)
    rng = _rng("mix")
    fresh = _fresh_keys(rng, 200)
    with_leaf = [k for k in fresh if kt.locate(k)[0] in kt.leaves and kt.leaves[kt.locate(k)[0]].n_used() <= 3][:6]
    no_leaf = [k for k in fresh if kt.locate(k)[0] not in kt.leaves][:3]
    old = list(present)
    keys = [old[0], with_leaf[0], no_leaf[0], with_leaf[1], old[5], no_leaf[1], with_leaf[2], with_leaf[3]]
    _, _, rec, rep = _run(store, present, keys, "mix", run)
    got = _reasons(rec)
    assert got[0] == got[4] == (NONE, R_EXISTS) and got[2] == got[5] == (NONE, R_NO_LEAF)
    ins = [int(r["object_id"]) for r in rec if r["action"] == INSERTED]
    assert ins == list(range(SPACE + 1000, SPACE + 1000 + len(ins))) and len(ins) >= 3


def case_bad_key_lengths(run=None):
    store, present, kt, _ = plain_store()
    keys = _fresh_keys(_rng("bad"), 3)
    for bad in (b"", bytes(257)):
        _, _, rec, rep = _run(store, present, keys[:2] + [bad] + keys[2:], "bad", run)
        assert rep.code == EMISMATCH and rep.lookup.first_bad == 2


def case_object_leaf_full(run=None):
    """The blob leaves hold 6 of 10 slots: the second ID that meets one leaf finds NUsedSlots at
    N * 3 / 4 and fails; it and every later key, of whatever key leaf, are CUT."""
    store, present, kt, _ = build_store(2, 0, 6, seed=7, per_blob=6, all_key_leaves=True)
    keys = _fresh_keys(_rng("ofull"), 5, lambda rng: 12)
    _, _, rec, rep = _run(store, present, keys, "ofull", run)
    assert rep.cut == 1 and rep.limit == 1
    assert _reasons(rec) == [(INSERTED, R_NONE)] + [(NONE, R_CUT)] * 4


def case_free_object_reference(run=None):
    """An object tree of depth 2 without the leaf of the third new ID's digits: cut 2."""
    first = SPACE + 1000

    def edit(kt, ot):
        del ot.leaves[_digits(first + 2, 10, 2)]
    store, present, kt, ot = build_store(1, 2, 24, seed=8, edit=edit)
    keys = _fresh_keys(_rng("free"), 6, lambda rng: 12)
    img, lay = uu.roomy(store, 160)
    g = _get(img, lay, store, SPACE, list(present))[0]
    existing = [k for k, r in zip(present, g) if r["status"] == FOUND]  # without the keys of the deleted leaf
    _, _, rec, rep = same_as_reference(store, SPACE, keys, uu.new_rows(_rng("free"), 6, ou.GET_S), existing, img=img, lay=lay,
                                       run=run)
    assert rep.cut == 2 and _reasons(rec)[2:] == [(NONE, R_CUT)] * 4


def case_lagging_next_object_id(run=None):
    """NextObjectID lags: the stored IDs are NextObjectID + 3 + 7 t, so the fourth new ID's slot is
    already Defined with its reminder: it is overwritten without counting, as storm does (and the
    key that owned the ID now reads the new object, which check_insert would not accept)."""
    store, present, kt, ot = build_store(1, 1, 24, seed=9, next_above=False)
    keys = _fresh_keys(_rng("lag"), 6, lambda rng: 9)
    rows = uu.new_rows(_rng("lag"), 6, ou.GET_S)
    img, lay = uu.roomy(store, 160)
    want = reference_insert(img.copy(), lay, SPACE, store, keys, rows)
    rec, rep = (run or host_insert)(img, lay, store, SPACE, keys, rows, None)
    assert insert_tuples(rec) == want[0] and img.tobytes() == want[1].tobytes() and rep.code == want[3] == OK
    got = rep.as_dict()
    got.pop("space")
    assert got == want[2] and rep.cut >= 4
    assert (rec[3]["action"], rec[3]["stage"], rec[3]["status"]) == (INSERTED, 2, FOUND) and scrub.scrub_host(img, lay).ok


def case_cut_zero(run=None):
    """The first new ID fails: the store is untouched, no revision."""
    store, present, kt, _ = build_store(1, 0, 7, seed=10, per_blob=8)
    keys = _fresh_keys(_rng("cut0"), 3, lambda rng: 9)
    _, _, rec, rep = _run(store, present, keys, "cut0", run)
    assert rep.cut == 0 and rep.limit == 0 and _reasons(rec) == [(NONE, R_CUT)] * 3 and rep.revision == 3


def case_space(name, run=None):
    c = ou.get_space_case(name)
    keys = _fresh_keys(_rng("space"), 5)
    img, lay = uu.roomy(c.store, 60)
    _, _, rec, rep = same_as_reference(c.store, c.space_id, keys, uu.new_rows(_rng("space"), 5, ou.GET_S), [], img=img, lay=lay,
                                       run=run)
    assert rep.code == OK and _reasons(rec) == [(NONE, R_SPACE)] * 5 and rep.revision == 0


def case_damage(where, run=None):
    """A flipped byte: EMISMATCH with the stage's text, the image untouched byte for byte."""
    store, present, kt, _ = plain_store()
    keys = _fresh_keys(_rng("dmg"), 12)
    img, lay = uu.roomy(store, 160)
    want = reference_insert(img.copy(), lay, SPACE, store, keys, uu.new_rows(_rng("dmg"), 12, ou.GET_S))
    first_ins = next(i for i, r in enumerate(want[0]) if r[7] == INSERTED)
    index = su.reference_scrub(img, lay)[2]
    key_leaf, blob_leaf = want[0][first_ins][1], want[0][first_ins][2]
    address, byte = {"key leaf": (key_leaf, 534), "key pointer block": (index[key_leaf][0], 3), "blob leaf": (blob_leaf, 727),
                     "spacelist leaf": (store.space_leaves[(SPACE % 10,)], 725), "singularity": (0, 20)}[where]
    img[address * lay.block_size + byte] ^= 0x10
    _, _, rec, rep = same_as_reference(store, SPACE, keys, uu.new_rows(_rng("dmg"), 12, ou.GET_S), list(present), img=img,
                                       lay=lay, run=run)
    assert rep.code == EMISMATCH and rep.message and rep.n_inserted == 0


def case_room(run=None):
    """Exactly D free blocks: OK. One fewer: STORMCK_ENOSPC, the image untouched."""
    store, present, kt, _ = plain_store()
    keys = _fresh_keys(_rng("room"), 10)
    rows = uu.new_rows(_rng("room"), 10, ou.GET_S)
    D = sum(same_as_reference(store, SPACE, keys, rows, list(present), run=run)[3].n_dirty)
    img, lay = uu.roomy(store, D)
    assert same_as_reference(store, SPACE, keys, rows, list(present), img=img, lay=lay, run=run)[3].code == OK
    img, lay = uu.roomy(store, D - 1)
    _, _, _, rep = same_as_reference(store, SPACE, keys, rows, list(present), img=img, lay=lay, run=run)
    assert (rep.code, rep.message) == (ENOSPC, ENOSPC_TEXT)


def case_depths(key_depth, object_depth, run=None):
    store, present, kt, _ = plain_store(key_depth, object_depth, min((2, 24, 60)[key_depth], (4, 30, 60)[object_depth]),
                                        key_depth + 3 * object_depth)
    fresh = _fresh_keys(_rng("depth"), 400)
    keys = [k for k in fresh if kt.locate(k)[0] in kt.leaves][:14]
    _, _, rec, rep = _run(store, present, keys, "depth", run)
    assert rep.cut >= 1 and rep.n_dirty[OBJECTLIST] >= 1 and rep.n_dirty[BLOB] >= 1
    assert rep.n_dirty[POINTER] >= 1 + min(key_depth, 1) + min(object_depth, 1)


def case_irregular(run=None):
    """update_util's irregular object tree (a leaf beside a pointer block under the root); its
    NextObjectID is 1, so the new IDs 1, 2, ... meet the leaf at slot 2 and Free references."""
    store, present, under = uu.irregular_store()
    keys = _fresh_keys(_rng("irr"), 8)
    _, _, rec, rep = same_as_reference(store, SPACE, keys, uu.new_rows(_rng("irr"), 8, ou.GET_S), list(present), run=run)
    assert rep.first_id == 1 and rep.cut < 8


def case_two_spaces(run=None):
    """Two spaces in one spacelist leaf: the other space's keys and objects are as they were."""
    store, present, other = uu.two_space_store(True)
    keys = _fresh_keys(_rng("two"), 6)
    old, lay = uu.roomy(store, 160)
    before = _get(old, lay, store, other, list(present[other]))
    img, lay, rec, rep = same_as_reference(store, SPACE, keys, uu.new_rows(_rng("two"), 6, ou.GET_S), [], img=old, lay=lay,
                                           run=run)
    after = _get(img, lay, store, other, list(present[other]))
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()


def case_crowded(count, run=None):
    """`count` candidates for the one leaf of a key tree of depth 0: 2048 are judged, 2049 are CROWDED."""
    store, present, kt, _ = plain_store(0, 1, 2, 11)
    rng = _rng("crowd")
    keys = [struct.pack("<I", i) + bytes(rng.integers(0, 256, 3, dtype=np.uint8)) for i in range(count)]
    _, _, rec, rep = _run(store, present, keys, "crowd", run)
    if count > MAX_PER_LEAF:
        assert _reasons(rec) == [(NONE, R_CROWDED)] * count and rep.cut == 0
    else:
        assert rep.n_inserted >= 1 and rep.n_none[R_KEY_SPLIT] >= count - 8


@functools.lru_cache(maxsize=None)
def wide_store():
    """Ten key leaves of C = 400 chunks (the trigger at 300) over one blob leaf of N = 3000 one-byte
    objects (room while NUsedSlots < 2250): more than 2048 keys can be INSERTED, and all their IDs
    meet the one blob leaf."""
    C, N, S = 400, 3000, 1
    lay = su.ScrubLayout(49152, 0, 10, 10, lu.ks.leaf_len(C), 16 * N + 8)
    return build_store(1, 0, 1, seed=30, N=N, S=S, lay=lay, per_blob=1, C=C)


def case_crowded_ids(count, run=None):
    """`count` IDs for the one leaf of an object tree of depth 0: 2048 are placed; 2049 fail at the
    smallest rank, so the cut is 0 and the store is untouched."""
    store, present, kt, _ = wide_store()
    keys = [struct.pack("<Q", 0x9E3779B97F4A7C15 * (i + 1) & (2 ** 64 - 1)) for i in range(count)]
    _, _, rec, rep = _run(store, present, keys, "ids", run, S=1, room=40)
    if count > MAX_PER_LEAF:
        assert _reasons(rec) == [(NONE, R_CUT)] * count and rep.cut == 0
    else:
        assert _reasons(rec) == [(INSERTED, R_NONE)] * count and rep.cut == count and rep.n_dirty == (2, 1, 10, 1)


def case_count(n, run=None):
    store, present, kt, _ = plain_store(2, 2, 60, 2, ensure_blobs=320)
    pool = [k for k in _fresh_keys(_rng("count"), 900) if kt.locate(k)[0] in kt.leaves]
    keys = (pool[:max(1, n * 2 // 3)] * 3)[:n]
    _, _, rec, rep = _run(store, present, keys, "count", run, in_stride=13 + n % 4, room=400)
    assert rep.cut >= min(n, 1) and (n < 64 or rep.n_repeated > 0)


@functools.lru_cache(maxsize=None)
def size_store(S):
    lay, N = ou.size_layout(S)
    return build_store(1, 1, 8, seed=20 + S % 7, N=N, S=S, lay=lay, per_blob=max(1, min(4, N // 3)))


def case_size(S, gap, run=None):
    """Objects of S bytes (both forms of the row store), rows in_stride = S + gap apart."""
    store, present, kt, _ = size_store(S)
    keys = _fresh_keys(_rng("size"), 8)
    _, _, rec, rep = _run(store, present, keys, "size", run, S=S, in_stride=S + gap)
    assert rep.cut >= 1 or S == 4000  # one slot a leaf: N * 3 / 4 == 0, storm always splits


COUNTS = (0, 1, 63, 64, 65, 257, 300)
CASES = {"one key": case_one_key, "lengths into one leaf": case_lengths_into_one_leaf, "long key": case_long_key,
         "trigger mid-batch": case_trigger_mid_batch, "KEY_FULL, then a shorter key": case_full_then_shorter,
         "empty leaf": case_empty_leaf, "Invalid slot reused": case_invalid_slot_reused, "NO_SLOT": case_no_slot,
         "malformed free list": case_malformed_free_list, "repeats": case_repeats,
         "EXISTS and NO_LEAF mixed in": case_mixed_with_existing_and_no_leaf, "key lengths 0 and 257": case_bad_key_lengths,
         "object leaf full": case_object_leaf_full, "Free object reference": case_free_object_reference,
         "lagging NextObjectID": case_lagging_next_object_id, "cut 0": case_cut_zero, "room": case_room,
         "irregular": case_irregular, "two spaces, one leaf": case_two_spaces}
CASES.update({n: functools.partial(case_space, n) for n in ("absent space", "invalid space")})
CASES.update({f"damaged {w}": functools.partial(case_damage, w)
              for w in ("singularity", "spacelist leaf", "key pointer block", "key leaf", "blob leaf")})
CASES.update({f"depths {k}, {d}": functools.partial(case_depths, k, d) for k in (0, 1, 2) for d in (0, 1, 2)})
CASES.update({f"{c} candidates for one leaf": functools.partial(case_crowded, c) for c in (2048, 2049)})
CASES.update({f"{c} IDs for one blob leaf": functools.partial(case_crowded_ids, c) for c in (2048, 2049)})
CASES.update({f"n = {n}": functools.partial(case_count, n) for n in COUNTS})
CASES.update({f"S = {S}, in_stride = S + {g}": functools.partial(case_size, S, g) for S in ou.SIZES for g in (0, 3)})


# ---- the seeded fuzz -----------------------------------------------------------------------------------

FUZZ_SEEDS = 40
FUZZ_STREAM = 500  # second word of the rngs' seeds: apart from the other fuzzes


def _fuzz_edit(rng):
    def edit(kt, ot):
        leaves = sorted(kt.leaves.items())
        for path, leaf in leaves:
            roll = rng.integers(0, 12)
            if roll == 0 and leaf.n_used():
                leaf.next_pointer(leaf.free_index(), 60000)  # MALFORMED for keys of two chunks
            elif roll == 1:
                for i in range(leaf.C):
                    if leaf.state(i) == lu.FREE:
                        leaf.state(i, 7 if rng.integers(0, 2) else lu.INVALID)  # NO_SLOT
            elif roll == 2:
                for i in range(leaf.C):
                    if leaf.state(i) == lu.FREE and rng.integers(0, 2):
                        leaf.state(i, lu.INVALID)
    return edit


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """(store, keys, rows, existing keys, space ID): a random store (depths, fill levels, damaged free lists,
    Invalid and unknown slot states) and a random batch: fresh keys of random lengths with
    repeats, existing keys, keys without a leaf."""
    rng = np.random.default_rng([seed, FUZZ_STREAM])
    key_depth, object_depth = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    if seed % 4 == 1:
        key_depth, object_depth = 2, 1
    n_keys = {0: 2, 1: 22, 2: 60}[key_depth]
    if object_depth == 0:
        n_keys = min(n_keys, 5)
    store, present, kt, ot = build_store(key_depth, object_depth, n_keys, seed=100 + seed, fill=int(rng.integers(3, 8)),
                                         per_blob=int(rng.integers(2, 8)), edit=_fuzz_edit(rng),
                                         ensure_blobs=int(rng.choice((2, 5, 12, 30))))
    n = int(rng.integers(1, 50))
    lengths = (1, 9, 20, 31, 32, 33, 64, 65, 100, 200, 256)
    fresh = _fresh_keys(rng, n, lambda r: int(r.choice(lengths)))
    if key_depth == 2 and seed % 4 != 1:
        fresh = [k for k in _fresh_keys(rng, 40 * n, lambda r: int(r.choice(lengths))) if kt.locate(k)[0] in kt.leaves][:n] + fresh[:3]
    keys = list(fresh)
    for _ in range(int(rng.integers(0, 6))):
        keys.insert(int(rng.integers(0, len(keys) + 1)), keys[int(rng.integers(0, len(keys)))])
    old = list(present)
    for _ in range(int(rng.integers(0, 4))):
        keys.insert(int(rng.integers(0, len(keys) + 1)), old[int(rng.integers(0, len(old)))])
    space_id = ou.GET_ABSENT if seed % 13 == 5 else SPACE  # a space the store does not hold: every key is SPACE
    return store, keys, uu.new_rows(rng, len(keys), ou.GET_S), old, space_id


def run_fuzz(seed, run=None):
    store, keys, rows, old, space_id = fuzz_case(seed)
    return same_as_reference(store, space_id, keys, rows, old, in_stride=13 + seed % 4, run=run)
