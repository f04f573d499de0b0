"""Scrub, host leg and ABI (CPU): stormck_scrub_host / stormck_scrub_tree_host walk a whole
snapshot from its root, and for every case the report and the reachable bitmap equal the
pure-Python breadth-first reference (tests/scrub_util.py) exactly."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from storm_amd import _lib, scrub
from storm_amd.scrub import BLOB, DUPLICATE, MISMATCH, OBJECTLIST, POINTER, RANGE, SPACELIST, TYPE
from tests import scrub_util as su
from tests.conftest import ROOT


def same(rep, bitmap, want, want_bitmap):
    assert rep.as_dict() == want
    assert np.array_equal(bitmap, want_bitmap)
    if not (want["first_error"] == MISMATCH and want["first_address"] == 0):  # a failed singularity is bit 0 itself
        assert su.popcount(bitmap) == 1 + sum(rep.verified) + rep.n_mismatch
    assert rep.ok == (rep.code == _lib.OK) == (rep.n_mismatch + rep.n_structural == 0)


def host_store(img, lay, threads=0):
    want, want_bitmap, index = su.reference_scrub(img, lay)
    rep = scrub.scrub_host(img, lay, threads=threads, reachable=True)
    same(rep, rep.reachable, want, want_bitmap)
    return rep, index


def host_tree(img, lay, root, root_type, leaf_kind, leaf_len, threads=0):
    want, want_bitmap, index = su.reference_scrub(img, lay, root, root_type, leaf_kind, leaf_len)
    rep = scrub.scrub_tree_host(img, lay, root, root_type, leaf_kind, leaf_len, threads=threads, reachable=True)
    same(rep, rep.reachable, want, want_bitmap)
    return rep, index


# ---- tree shapes -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(su.TREE_SHAPES))
def test_tree_shapes(name):
    img, lay, root, root_type, leaf_len = su.tree_shape(name)
    _, _, _, _, levels, n_ptr, n_leaf = su.TREE_SHAPES[name]
    rep, index = host_tree(img, lay, root + (2,), root_type, BLOB, leaf_len)
    assert rep.ok and rep.first_error == 0 and rep.message == ""
    assert rep.verified == (n_ptr, 0, 0, n_leaf) and rep.levels == len(levels)
    assert rep.bytes_hashed == n_ptr * su.kind_lens(lay)[POINTER] + n_leaf * leaf_len
    sizes = [0] * len(levels)
    for _, _, _, lvl in index.values():
        sizes[lvl] += 1
    assert tuple(sizes) == levels
    assert su.popcount(rep.reachable) == lay.n_blocks  # every block of the image, and bit 0


def test_tree_with_objectlist_leaves_and_one_thread():
    img, lay, root, root_type, leaf_len = su.tree_shape("f65")
    rep, _ = host_tree(img, lay, root + (2,), root_type, OBJECTLIST, leaf_len, threads=1)
    assert rep.verified == (6, 0, 4, 0)


def test_tree_free_root_and_leaf_root():
    img, lay, root, root_type, leaf_len = su.tree_shape("f10")
    rep, _ = host_tree(img, lay, (0, 0, 0), 0, BLOB, leaf_len)
    assert rep.ok and rep.levels == 0 and sum(rep.verified) == 0 and list(rep.reachable[:1]) == [1]
    bs = lay.block_size
    leaf = (su.o.xxh64(img[bs:bs + leaf_len]), 1, 2)  # build_tree puts the leaves first
    rep, _ = host_tree(img, lay, leaf, 2, BLOB, leaf_len)
    assert rep.ok and rep.levels == 1 and rep.verified == (0, 0, 0, 1)


def test_tree_mid_level_damage_drops_its_subtree():
    """One flipped byte in a level-1 pointer block: it mismatches, and its 10 + 100 blocks
    below are not counted (a block that mismatches is never expanded)."""
    img, lay, root, root_type, leaf_len = su.tree_shape("f10")
    _, _, index = su.reference_scrub(img, lay, root, root_type, BLOB, leaf_len)
    victim = min(a for a, (_, _, k, lvl) in index.items() if k == POINTER and lvl == 1)
    img = img.copy()
    img[victim * lay.block_size + 5] ^= 0x40
    rep, _ = host_tree(img, lay, root + (2,), root_type, BLOB, leaf_len)
    assert rep.code == _lib.EMISMATCH and rep.n_mismatch == 1 and rep.n_structural == 0
    assert rep.verified == (111 - 11, 0, 0, 1000 - 100)
    assert (rep.first_error, rep.first_address, rep.first_level) == (MISMATCH, victim, 1)
    assert rep.message == "checksum mismatch for block %d, computed: 0x%x, expected: 0x%x" % (
        victim, rep.first_computed, rep.first_expected)


# ---- whole stores ------------------------------------------------------------------------

def test_whole_store_test_tag():
    img, lay = su.tag_store()
    rep, index = host_store(img, lay)
    assert rep.ok and rep.verified == (8, 2, 6, 7) and rep.levels == 5
    # the Invalid space's two leaves are the only blocks nobody reaches
    assert su.popcount(rep.reachable) == lay.n_blocks - 2
    kinds_at_1 = sorted(k for _, _, k, lvl in index.values() if lvl == 1)
    assert kinds_at_1 == [POINTER, SPACELIST]  # a leaf and a pointer block side by side


def test_whole_store_production_constants():
    img, lay = su.production_store()
    assert (lay.pointer_fanout, lay.spaces_per_block, lay.objectlist_len, lay.blob_len) == (1200, 400, 31808, 32768)
    rep, _ = host_store(img, lay)
    assert rep.ok and rep.verified == (5, 1, 5, 6) and rep.levels == 4


def test_empty_store_and_root_that_is_a_leaf():
    img, lay = su.empty_store()
    rep, _ = host_store(img, lay)
    assert rep.ok and rep.levels == 0 and sum(rep.verified) == 0 and rep.bytes_hashed == 72
    img, lay = su.leaf_root_store()
    rep, _ = host_store(img, lay)
    assert rep.ok and rep.levels == 2 and rep.verified == (0, 1, 1, 1)


def test_threads_do_not_change_the_report():
    img, lay = su.tag_store()
    a = scrub.scrub_host(img, lay, threads=1, reachable=True)
    b = scrub.scrub_host(img, lay, threads=5, reachable=True)
    assert a.as_dict() == b.as_dict() and np.array_equal(a.reachable, b.reachable)


# ---- damage (the edits: tests/scrub_util.py DAMAGE) ------------------------------------------

@pytest.mark.parametrize("name", list(su.DAMAGE))
def test_damage(name):
    img, lay = su.tag_store()
    _, _, index = su.reference_scrub(img, lay)
    img = img.copy()
    expect = su.DAMAGE[name](img, lay, index)
    rep, _ = host_store(img, lay)
    assert rep.code == _lib.EMISMATCH and rep.message
    for field, value in expect.items():
        assert getattr(rep, field) == value, field


def test_messages_are_storm_format():
    img, lay = su.tag_store()
    _, _, index = su.reference_scrub(img, lay)
    bad = img.copy()
    su.flip_leaf(bad, lay, index)
    rep = scrub.scrub_host(bad, lay)
    assert rep.message == "checksum mismatch for block %d, computed: 0x%x, expected: 0x%x" % (
        rep.first_address, rep.first_computed, rep.first_expected)  # blocks/checksum.go:25-26
    bad = img.copy()
    su.set_address(2 ** 63)(bad, lay, index)
    rep = scrub.scrub_host(bad, lay)
    assert rep.message.startswith("block %d does not exist" % 2 ** 63)  # cache/cache.go:146


# ---- ABI ---------------------------------------------------------------------------------

NEW = ("stormck_scrub_workspace_bytes", "stormck_scrub_device", "stormck_scrub_tree_device", "stormck_scrub_host",
       "stormck_scrub_tree_host")


def test_header_and_bindings_declare_the_scrub():
    text = open(os.path.join(ROOT, "include", "stormck.h")).read()
    assert re.search(r"#define STORMCK_HAS_SCRUB 1\b", text)
    assert re.search(r"#define STORMCK_ABI_VERSION 7\b", text)  # purely additive
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.ScrubLayoutStruct) == 32 and ctypes.sizeof(_lib.ScrubReportStruct) == 104
    mirror = open(os.path.join(ROOT, "include", "storm_blocks.hpp")).read()
    assert "Scrub(" in mirror and "ScrubTree(" in mirror


def test_workspace_bytes_is_host_logic_and_monotonic():
    sizes = [scrub.workspace_bytes(n) for n in (1, 2, 31, 32, 33, 1000, 2504, 12301, 1 << 20, (1 << 20) + 1)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    n = 1 << 20
    assert scrub.workspace_bytes(n) == 256 + 57 * n + n // 8  # DESIGN.md "Scrub"


def test_argument_errors():
    img, lay = su.leaf_root_store()
    img = img.copy()
    L = _lib.lib
    rep = _lib.ScrubReportStruct()
    root = _lib.PointerStruct(1, 1, 1)
    ws = scrub.workspace_bytes(lay.n_blocks)
    p = img.ctypes.data

    def layout(**kw):
        fields = dict(block_size=lay.block_size, n_blocks=lay.n_blocks, pointer_fanout=lay.pointer_fanout,
                      spaces_per_block=lay.spaces_per_block, objectlist_len=lay.objectlist_len, blob_len=lay.blob_len)
        fields.update(kw)
        return ctypes.byref(scrub.ScrubLayout(**fields))

    cases = [
        ("null store", lambda: L.stormck_scrub_host(None, layout(), None, ctypes.byref(rep), 0)),
        ("null layout", lambda: L.stormck_scrub_host(p, None, None, ctypes.byref(rep), 0)),
        ("null report", lambda: L.stormck_scrub_host(p, layout(), None, None, 0)),
        ("zero fanout", lambda: L.stormck_scrub_host(p, layout(pointer_fanout=0), None, ctypes.byref(rep), 0)),
        ("zero spaces", lambda: L.stormck_scrub_host(p, layout(spaces_per_block=0), None, ctypes.byref(rep), 0)),
        ("zero blocks", lambda: L.stormck_scrub_host(p, layout(n_blocks=0), None, ctypes.byref(rep), 0)),
        ("zero block size", lambda: L.stormck_scrub_host(p, layout(block_size=0), None, ctypes.byref(rep), 0)),
        ("image wraps", lambda: L.stormck_scrub_host(p, layout(n_blocks=1 << 36, block_size=1 << 40), None,
                                                     ctypes.byref(rep), 0)),
        ("blob longer than a block", lambda: L.stormck_scrub_host(p, layout(blob_len=lay.block_size + 8), None,
                                                                  ctypes.byref(rep), 0)),
        ("objectlist longer than a block", lambda: L.stormck_scrub_host(p, layout(objectlist_len=lay.block_size + 1),
                                                                        None, ctypes.byref(rep), 0)),
        ("pointer block longer than a block", lambda: L.stormck_scrub_host(p, layout(pointer_fanout=1400), None,
                                                                           ctypes.byref(rep), 0)),
        ("tree null root", lambda: L.stormck_scrub_tree_host(p, layout(), None, 2, BLOB, 0, None, ctypes.byref(rep), 0)),
        ("tree leaf kind pointer", lambda: L.stormck_scrub_tree_host(p, layout(), ctypes.byref(root), 2, POINTER, 0,
                                                                     None, ctypes.byref(rep), 0)),
        ("tree leaf kind 4", lambda: L.stormck_scrub_tree_host(p, layout(), ctypes.byref(root), 2, 4, 0, None,
                                                               ctypes.byref(rep), 0)),
        ("tree leaf_len longer than a block", lambda: L.stormck_scrub_tree_host(
            p, layout(), ctypes.byref(root), 2, BLOB, lay.block_size + 8, None, ctypes.byref(rep), 0)),
        ("device null workspace", lambda: L.stormck_scrub_device(p, layout(), None, ws, None, ctypes.byref(rep), None)),
        ("device small workspace", lambda: L.stormck_scrub_device(p, layout(), 1 << 20, ws - 1, None,
                                                                  ctypes.byref(rep), None)),
        ("device null store", lambda: L.stormck_scrub_device(None, layout(), 1 << 20, ws, None, ctypes.byref(rep),
                                                             None)),
        ("device zero fanout", lambda: L.stormck_scrub_tree_device(1 << 21, layout(pointer_fanout=0),
                                                                   ctypes.byref(root), 2, BLOB, 0, 1 << 20, ws, None,
                                                                   ctypes.byref(rep), None)),
        ("device tree null root", lambda: L.stormck_scrub_tree_device(1 << 21, layout(), None, 2, BLOB, 0, 1 << 20,
                                                                      ws, None, ctypes.byref(rep), None)),
        ("device misaligned store", lambda: L.stormck_scrub_device((1 << 21) + 4, layout(), 1 << 20, ws, None,
                                                                   ctypes.byref(rep), None)),
    ]
    for name, fn in cases:
        assert fn() == _lib.EINVAL, name
        assert _lib.last_error(), name
    with pytest.raises(ValueError):
        scrub.scrub_host(img[:100], lay)


def _has_gpu():
    return _lib.device_count() > 0


@pytest.mark.skipif("_has_gpu()")
def test_device_entries_need_a_device():
    img, lay = su.leaf_root_store()
    rep = _lib.ScrubReportStruct()
    root = _lib.PointerStruct(1, 1, 1)
    ws = scrub.workspace_bytes(lay.n_blocks)
    L = _lib.lib
    assert L.stormck_scrub_device(1 << 21, ctypes.byref(lay), 1 << 20, ws, None, ctypes.byref(rep), None) == _lib.ENODEV
    assert "no HIP device" in _lib.last_error() or "gfx950" in _lib.last_error()
    assert L.stormck_scrub_tree_device(1 << 21, ctypes.byref(lay), ctypes.byref(root), 2, BLOB, 0, 1 << 20, ws, None,
                                       ctypes.byref(rep), None) == _lib.ENODEV
    # the host entries need none
    assert scrub.scrub_host(img, lay).ok
