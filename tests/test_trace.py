"""Trace, the host leg (CPU): stormck_trace_host gives, in every result field and every
report field, what the pure-Python reference of tests/trace_util.py gives on the same images,
hashes each distinct reference once, and reports damage as statuses. The device engine is held
against both in tests/test_trace_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
from storm_amd import _lib, trace
from storm_amd.scrub import BLOB, POINTER, ScrubLayout
from storm_amd.trace import ABSENT, DEPTH, FOUND, MISMATCH, RANGE, TYPE
from tests import scrub_util as su
from tests import trace_util as tu
from tests.conftest import ROOT


def same_as_reference(tree, tags, verify_leaves=True, threads=0):
    want, want_rep, refs, want_cs = tree.reference(tags, verify_leaves)
    res, rep = trace.trace_host(tree.img, *tree.args(), tu.tags_u64(tags), tree.leaf_len, verify_leaves, threads,
                                leaf_checksums=True)
    assert tu.as_tuples(res) == want
    assert rep.as_dict() == want_rep
    assert sum(rep.blocks_hashed) == len(refs)
    assert [int(c) for c in rep.leaf_checksums] == want_cs
    assert not res["reserved"].any()
    assert rep.code == (_lib.EMISMATCH if rep.first_bad < len(tags) else _lib.OK) and bool(rep.message) == (not rep.ok)
    return res, rep


# ---- intact trees ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(su.TREE_SHAPES))
def test_tree_shapes(name):
    tags = tu.shape_tags(name)
    res, rep = same_as_reference(tu.shape(name), tags)
    present = set(su.TREE_SHAPES[name][1])
    for t, r in zip(tags, res):
        if t in present:
            assert r["status"] == FOUND
    assert rep.ok and rep.first_bad == len(tags)


def test_f10_facts():
    """What a reference run on the CPU found for this input (the issue's figures)."""
    res, rep = same_as_reference(tu.shape("f10"), tu.F10_TAGS)
    assert rep.n_status[FOUND] == 3003 and rep.blocks_hashed == (111, 1000) and rep.levels == 4
    rows = tu.as_tuples(res)
    assert (rows[3000][0], rows[3000][1], rows[3000][4]) == (616, 18446744073709551, 3)
    assert rows[3001][:2] == (1, 1) and rows[3002][:2] == (346, 12)
    assert rows[:1000] == rows[1000:2000] == rows[2000:3000]


def test_f65_facts():
    res, rep = same_as_reference(tu.shape("f65"), tu.F65_TAGS)
    assert [int(s) for s in res["status"]] == [FOUND] * 4 + [ABSENT] * 3
    assert [int(d) for d in res["depth"][4:]] == [1, 2, 1]
    assert 64 in [int(s) for s in res["slot"][:4]]  # past lane 63
    assert sum(rep.blocks_hashed) == 10


def test_leaves_at_three_depths():
    res, rep = same_as_reference(tu.mixed_depth_tree(), tu.MIXED_TAGS)
    found_depths = {int(r["depth"]) for r in res if r["status"] == FOUND}
    assert found_depths == {1, 2, 3} and rep.n_status[ABSENT] > 0


def test_leaves_beside_pointer_blocks_in_the_root():
    """The root's own slots hold leaves and pointer blocks side by side."""
    t = tu.mixed_depth_tree()
    res, _ = same_as_reference(t, [0, 9, 3, 4])
    assert [int(s) for s in res["status"]] == [FOUND, FOUND, ABSENT, ABSENT]
    assert [int(d) for d in res["depth"]] == [1, 1, 2, 2]


def test_free_root():
    tags = [0, 1, 77, 2 ** 64 - 1]
    res, rep = same_as_reference(tu.free_root_tree(), tags)
    assert tu.as_tuples(res) == [(0, t, 0, 0, 0, ABSENT) for t in tags]
    assert rep.ok and rep.blocks_hashed == (0, 0) and rep.levels == 0


def test_leaf_root():
    t = tu.leaf_root_tree()
    tags = [0, 5, 2 ** 64 - 1]
    res, rep = same_as_reference(t, tags)
    assert tu.as_tuples(res) == [(t.root[1], tag, 0, 0, 0, FOUND) for tag in tags]
    assert rep.blocks_hashed == (0, 1) and rep.levels == 1
    res, rep = same_as_reference(t, tags, verify_leaves=False)
    assert rep.blocks_hashed == (0, 0) and [int(c) for c in rep.leaf_checksums] == [t.root[0]] * 3


# ---- tag-list shapes -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_tag_counts(n):
    rng = np.random.default_rng(n)
    tags = [int(t) for t in rng.integers(0, 1100, n)]
    _, rep = same_as_reference(tu.shape("f10"), tags)
    assert sum(rep.n_status) == n and rep.first_bad == n


def test_one_tag_ten_thousand_times():
    res, rep = same_as_reference(tu.shape("f10"), [437] * 10000)
    assert sum(rep.blocks_hashed) == 4 and rep.blocks_hashed == (3, 1)  # the depth of one path
    assert rep.n_status[FOUND] == 10000 and len(set(tu.as_tuples(res))) == 1


@pytest.mark.parametrize("threads", [1, 2, 16])
def test_thread_counts_agree(threads):
    same_as_reference(tu.shape("f64"), tu.shape_tags("f64"), threads=threads)


# ---- chains: the depth cap ----------------------------------------------------------------------

def test_chain_of_64_is_found():
    res, rep = same_as_reference(tu.chain(64), [0, 1])
    assert (int(res["status"][0]), int(res["depth"][0])) == (FOUND, 64) and sum(rep.blocks_hashed) == 65
    assert (int(res["status"][1]), int(res["depth"][1])) == (ABSENT, 1) and rep.ok


def test_chain_of_65_ends_at_the_cap():
    t = tu.chain(65)
    res, rep = same_as_reference(t, [0, 1])
    first_block = t.root[1] - 64  # the 65th pointer block on the way down is the one built first
    assert tu.as_tuples(res)[0] == (first_block, 0, first_block + 1, 0, 64, DEPTH)
    assert (int(res["status"][1]), int(res["depth"][1])) == (ABSENT, 1)
    assert sum(rep.blocks_hashed) == 64 and rep.first_bad == 0 and rep.code == _lib.EMISMATCH
    assert rep.message == "more than 64 pointer blocks on the way to block %d (block %d, slot 0)" % (first_block,
                                                                                                   first_block + 1)


# ---- damage ------------------------------------------------------------------------------------

def test_mid_level_pointer_block():
    t, what = tu.damaged("f10", tu.flip_mid_level)
    victim = what["victim"]
    under = set(tu.tags_under(tu.intact_index("f10"), victim))
    assert len(under) == 100
    tags = list(range(1000))
    res, rep = same_as_reference(t, tags)
    for tag, r in zip(tags, res):
        if tag in under:
            assert (int(r["status"]), int(r["address"]), int(r["depth"])) == (MISMATCH, victim, 1)
        else:
            assert r["status"] == FOUND
    assert rep.n_status[MISMATCH] == 100 and rep.n_status[FOUND] == 900 and rep.first_bad == min(under)
    computed = o.xxh64(t.img[victim * t.lay.block_size:victim * t.lay.block_size + 256])
    assert rep.code == _lib.EMISMATCH
    assert re.fullmatch(r"checksum mismatch for block %d, computed: 0x%x, expected: 0x[0-9a-f]+" % (victim, computed),
                        rep.message)


def test_flipped_leaf():
    t, what = tu.damaged("f10", tu.flip_one_leaf)
    victim = what["victim"]
    tags = [victim - 1, 5, victim - 1, 999]
    res, rep = same_as_reference(t, tags)
    assert [int(s) for s in res["status"]] == [MISMATCH, FOUND, MISMATCH, FOUND]
    assert rep.first_bad == 0 and rep.message.startswith("checksum mismatch for block %d, computed: 0x" % victim)
    # the same leaf unverified: FOUND, unhashed, with the checksum its parent holds
    res, rep = same_as_reference(t, tags, verify_leaves=False)
    assert [int(s) for s in res["status"]] == [FOUND] * 4 and rep.blocks_hashed[1] == 0 and rep.ok
    index = tu.intact_index("f10")
    off, _ = su.entry_offsets(t.lay, index[victim][0], POINTER, index[victim][1])
    assert int(rep.leaf_checksums[0]) == su._u64(t.img, off) != o.xxh64(
        t.img[victim * t.lay.block_size:victim * t.lay.block_size + t.leaf_len])


@pytest.mark.parametrize("address", [None, 0, 2 ** 63, 2 ** 64 - 1], ids=["n_blocks", "0", "2**63", "2**64-1"])
def test_entry_address_out_of_range(address):
    t, what = tu.damaged("f10", tu.entry_address(address))
    tag = what["old"] - 1
    tags = [3, tag, tag]
    res, rep = same_as_reference(t, tags)
    assert tu.as_tuples(res)[1] == (what["address"], 0, what["parent"], what["slot"], 3, RANGE)
    assert rep.first_bad == 1 and rep.n_status[RANGE] == 2 and rep.code == _lib.EMISMATCH
    assert rep.message == "block %d does not exist (block %d, slot %d)" % (what["address"], what["parent"], what["slot"])


def test_type_byte_3():
    t, what = tu.damaged("f10", tu.entry_type_3)
    tag = what["old"] - 1
    res, rep = same_as_reference(t, [tag, 3])
    assert tu.as_tuples(res)[0] == (what["old"], 0, what["parent"], what["slot"], 3, TYPE)
    assert rep.first_bad == 0 and rep.code == _lib.EMISMATCH
    assert rep.message == "invalid block type or space state in block %d, slot %d" % (what["parent"], what["slot"])
    # the same entry with leaves unverified: the TYPE rule comes first
    res, rep = same_as_reference(t, [tag, 3], verify_leaves=False)
    assert int(res["status"][0]) == TYPE


def test_bad_root_reference():
    t = tu.shape("f10")
    for root, root_type, status in (((t.root[0], t.lay.n_blocks), 1, RANGE), ((t.root[0], 0), 2, RANGE),
                                    (t.root, 7, TYPE)):
        bad = tu.Tree(t.img, t.lay, root, root_type, BLOB, t.leaf_len)
        res, rep = same_as_reference(bad, [4, 5])
        assert tu.as_tuples(res) == [(root[1], tag, 0, 0, 0, status) for tag in (4, 5)]
        assert rep.first_bad == 0 and rep.code == _lib.EMISMATCH and rep.levels == 0


def test_first_bad_is_the_smallest_index_not_the_shallowest_error():
    """A leaf mismatch (depth 3) at index 1 precedes a mid-level mismatch (depth 1) at index 2."""
    def both(img, lay, index):
        a = tu.flip_mid_level(img, lay, index)
        leaf = 1000  # tag 999: not under the first level-1 block
        img[leaf * lay.block_size + 9] ^= 2
        return dict(keep_bad=a["keep_bad"] | {leaf}, victim=a["victim"])
    t, what = tu.damaged("f10", both)
    under = tu.tags_under(tu.intact_index("f10"), what["victim"])
    res, rep = same_as_reference(t, [500, 999, under[0]])
    assert [int(s) for s in res["status"]] in ([FOUND, MISMATCH, MISMATCH], [MISMATCH, MISMATCH, MISMATCH])
    assert rep.first_bad == (1 if res["status"][0] == FOUND else 0)
    assert "block %d," % int(res["address"][rep.first_bad]) in rep.message


# ---- arguments ---------------------------------------------------------------------------------

def test_argument_errors_precede_the_device_check():
    L = _lib.lib
    t = tu.shape("f10")
    lay, root = t.lay, _lib.PointerStruct(t.root[0], t.root[1], 2)
    tags = tu.tags_u64([1, 2, 3])
    res = np.zeros(3, dtype=trace.RESULT_DTYPE)
    raw = _lib.TraceReportStruct()
    img = t.img.ctypes.data
    big = ScrubLayout(lay.block_size, lay.n_blocks, lay.pointer_fanout, 10, 536, lay.block_size + 8)
    zero_fanout = ScrubLayout(lay.block_size, lay.n_blocks, 0, 10, 536, 728)

    def device(store=img, layout=lay, rootp=ctypes.byref(root), leaf_kind=BLOB, tagp=tags.ctypes.data, n=3, flags=0,
               resp=res.ctypes.data, ws=8, ws_bytes=1 << 30, report=ctypes.byref(raw)):
        return L.stormck_trace_device(store, ctypes.byref(layout), rootp, 1, leaf_kind, 0, tagp, n, flags, resp, None, ws,
                                      ws_bytes, report, None)

    def host(store=img, layout=lay, rootp=ctypes.byref(root), leaf_kind=BLOB, tagp=tags.ctypes.data, n=3, flags=0,
             resp=res.ctypes.data, report=ctypes.byref(raw)):
        return L.stormck_trace_host(store, ctypes.byref(layout), rootp, 1, leaf_kind, 0, tagp, n, flags, resp, None,
                                    report, 0)

    for call in (device, host):
        for kwargs, text in ((dict(store=None), "null"), (dict(rootp=None), "null"), (dict(report=None), "null"),
                             (dict(tagp=None), "null"), (dict(resp=None), "null"), (dict(leaf_kind=0), "leaf_kind"),
                             (dict(leaf_kind=4), "leaf_kind"), (dict(layout=big), "block_size"),
                             (dict(layout=zero_fanout), "fanout"), (dict(flags=2), "flag"),
                             (dict(n=2 ** 31 + 1), "2^31")):
            assert call(**kwargs) == _lib.EINVAL, kwargs
            assert text in _lib.last_error(), (kwargs, _lib.last_error())
    assert device(ws_bytes=trace.workspace_bytes(3) - 1) == _lib.EINVAL and "workspace" in _lib.last_error()
    assert device(ws=None) == _lib.EINVAL and "workspace" in _lib.last_error()
    for kwargs in (dict(store=img + 4), dict(tagp=tags.ctypes.data + 4), dict(resp=res.ctypes.data + 2), dict(ws=12)):
        assert device(**kwargs) == _lib.EINVAL and "aligned" in _lib.last_error(), kwargs
    assert host(n=0) == _lib.OK and raw.first_bad == 0 and raw.levels == 0 and sum(raw.n_status) == 0


def test_workspace_bytes_is_host_logic_of_the_tag_count_alone():
    w = trace.workspace_bytes
    assert w(0) == 256 + 12 * 64
    assert w(1) == 256 + 12 * 64 + 118 * 8
    assert w(32) == 256 + 12 * 64 + 118 * 32 and w(33) == 256 + 12 * 128 + 118 * 40
    assert w(1 << 20) == 256 + 12 * (1 << 21) + 118 * (1 << 20)
    for n in (1, 1000, 12345, 1 << 20, (1 << 20) + 1, 1 << 31):
        assert w(n) % 8 == 0 and w(n) <= 256 + 12 * 64 + 166 * ((n + 7) & ~7)
    # 1M tags of a 32 GiB image: a few hundred bytes per tag, not 57 bytes per block of the image
    assert w(1 << 20) < 160 << 20


def test_cpp_mirror_traces_on_the_host_leg():
    """TraceTags of include/storm_blocks.hpp compiles with -Wall -Wextra and traces a small
    tree it builds itself (tests/cpp/trace_test.cpp)."""
    import subprocess
    from storm_amd import build as b
    out = os.path.join(ROOT, "tests", "cpp", "build", "trace_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    libdir = os.path.dirname(b.LIB)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "trace_test.cpp"), "-o", out, "-L", libdir, "-lstormck",
                    f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_header_announces_the_trace():
    text = open(os.path.join(ROOT, "include", "stormck.h")).read()
    assert re.search(r"^#define STORMCK_HAS_TRACE 1$", text, re.M)
    assert re.search(r"^#define STORMCK_ABI_VERSION 7$", text, re.M)
    assert ctypes.sizeof(_lib.TraceResultStruct) == 32 and ctypes.sizeof(_lib.TraceReportStruct) == 7 * 8 + 16 + 24
