"""Trace on the device (MI355X): stormck_trace_device gives the results and the report of the
host leg and of the pure-Python reference (tests/trace_util.py) on the same images. Every
wrong address used here points inside the tensor the test allocated (the images carry slack
blocks past n_blocks); the huge-address cases stay on the host leg (tests/test_trace.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as o  # noqa: E402
from oracle.storm_cache import Store, build_tree, initialize  # noqa: E402
from storm_amd import _lib, commit, engine, trace  # noqa: E402
from storm_amd.scrub import BLOB, OBJECTLIST, ScrubLayout  # noqa: E402
from storm_amd.trace import ABSENT, DEPTH, FOUND, MISMATCH, RANGE, TYPE  # noqa: E402
from tests import scrub_util as su  # noqa: E402
from tests import trace_util as tu  # noqa: E402

_device_images = {}


def on_device(key, img):
    """The image as a device tensor, uploaded once per tree."""
    if key not in _device_images:
        _device_images[key] = torch.from_numpy(np.array(img)).cuda()
    return _device_images[key]


def device_tags(tags):
    return torch.from_numpy(tu.tags_u64(tags).view(np.int64)).cuda()


def same_everywhere(tree, tags, image, verify_leaves=True, stream=0, workspace=None):
    """Device == host leg == reference: results, report, leaf checksums, code and message.
    `workspace`: a device tensor the device call uses as it is (tests/test_trace_fuzz_gpu.py)."""
    want, want_rep, refs, want_cs = tree.reference(tags, verify_leaves)
    hres, hrep = trace.trace_host(tree.img, *tree.args(), tu.tags_u64(tags), tree.leaf_len, verify_leaves,
                                  leaf_checksums=True)
    dres, drep = trace.trace_device(image, *tree.args(), device_tags(tags), tree.leaf_len, verify_leaves, stream,
                                    workspace, leaf_checksums=True)
    res = trace.results_numpy(dres)
    assert res.tobytes() == hres.tobytes()
    assert tu.as_tuples(res) == want
    assert drep.as_dict() == want_rep == hrep.as_dict()
    assert sum(drep.blocks_hashed) == len(refs)
    cs = drep.leaf_checksums.cpu().numpy().view(np.uint64)
    assert np.array_equal(cs, hrep.leaf_checksums) and [int(c) for c in cs] == want_cs
    assert (drep.code, drep.message) == (hrep.code, hrep.message)
    assert drep.code == (_lib.EMISMATCH if drep.first_bad < len(tags) else _lib.OK)
    return res, drep


# ---- intact trees ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(su.TREE_SHAPES))
def test_tree_shapes(name):
    t = tu.shape(name)
    _, rep = same_everywhere(t, tu.shape_tags(name), on_device(name, t.img))
    assert rep.ok


def test_f10_facts():
    t = tu.shape("f10")
    res, rep = same_everywhere(t, tu.F10_TAGS, on_device("f10", t.img))
    assert rep.n_status[FOUND] == 3003 and rep.blocks_hashed == (111, 1000)
    assert (int(res["address"][3000]), int(res["reminder"][3000]), int(res["depth"][3000])) == (616, 18446744073709551, 3)


@pytest.mark.parametrize("name", ["mixed", "free root", "leaf root", "leaf root unverified"])
def test_small_trees(name):
    t = {"mixed": tu.mixed_depth_tree, "free root": tu.free_root_tree}.get(name, tu.leaf_root_tree)()
    tags = tu.MIXED_TAGS if name == "mixed" else [0, 5, 2 ** 64 - 1]
    res, rep = same_everywhere(t, tags, on_device(name.split(" unverified")[0], t.img), verify_leaves="unverified" not in name)
    assert rep.ok
    if name == "free root":
        assert tu.as_tuples(res) == [(0, tag, 0, 0, 0, ABSENT) for tag in tags]


@pytest.mark.parametrize("name, n", [("f10", 100_000), ("f64", 100_000), ("f65", 20_000)])
def test_many_tags_per_reference(name, n):
    """Tags drawn with repetition from the tree's own and from absent ones: many lanes per
    reference, the table under contention."""
    t = tu.shape(name)
    rng = np.random.default_rng(n)
    present = np.array(list(su.TREE_SHAPES[name][1]), dtype=np.uint64)
    tags = present[rng.integers(0, len(present), n)]
    absent = rng.integers(0, 2 ** 63, n // 10, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    tags[rng.integers(0, n, n // 10)] = absent
    _, rep = same_everywhere(t, tags.tolist(), on_device(name, t.img))
    assert rep.ok and rep.n_status[FOUND] >= n * 8 // 10


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_tag_counts(n):
    t = tu.shape("f10")
    tags = [int(x) for x in np.random.default_rng(n).integers(0, 1100, n)]
    _, rep = same_everywhere(t, tags, on_device("f10", t.img))
    assert sum(rep.n_status) == n and rep.first_bad == n


def test_one_tag_ten_thousand_times():
    t = tu.shape("f10")
    _, rep = same_everywhere(t, [437] * 10000, on_device("f10", t.img))
    assert rep.blocks_hashed == (3, 1)


# ---- damage ------------------------------------------------------------------------------------

def test_mid_level_pointer_block():
    t, what = tu.damaged("f10", tu.flip_mid_level)
    under = set(tu.tags_under(tu.intact_index("f10"), what["victim"]))
    tags = list(range(1000))
    res, rep = same_everywhere(t, tags, torch.from_numpy(t.img).cuda())
    bad = {tag for tag, r in zip(tags, res) if r["status"] == MISMATCH}
    assert bad == under and len(under) == 100 and rep.n_status[FOUND] == 900 and rep.first_bad == min(under)
    assert {int(a) for a in res["address"][sorted(under)]} == {what["victim"]}


@pytest.mark.parametrize("verify_leaves", [True, False])
def test_flipped_leaf(verify_leaves):
    t, what = tu.damaged("f10", tu.flip_one_leaf)
    tags = [what["victim"] - 1, 5, what["victim"] - 1, 999]
    res, rep = same_everywhere(t, tags, torch.from_numpy(t.img).cuda(), verify_leaves=verify_leaves)
    if verify_leaves:
        assert [int(s) for s in res["status"]] == [MISMATCH, FOUND, MISMATCH, FOUND] and rep.first_bad == 0
    else:
        assert [int(s) for s in res["status"]] == [FOUND] * 4 and rep.blocks_hashed[1] == 0 and rep.ok


def test_entry_address_n_blocks():
    t, what = tu.damaged("f10", tu.entry_address(None))
    assert what["address"] == t.lay.n_blocks < t.lay.n_blocks + su.SLACK  # inside the tensor
    tag = what["old"] - 1
    res, rep = same_everywhere(t, [3, tag, tag], torch.from_numpy(t.img).cuda())
    assert tu.as_tuples(res)[1] == (what["address"], 0, what["parent"], what["slot"], 3, RANGE) and rep.first_bad == 1


def test_type_byte_3():
    t, what = tu.damaged("f10", tu.entry_type_3)
    res, rep = same_everywhere(t, [what["old"] - 1, 3], torch.from_numpy(t.img).cuda())
    assert int(res["status"][0]) == TYPE and rep.first_bad == 0 and "invalid block type" in rep.message


# ---- dispatch boundaries, chains -----------------------------------------------------------------

def test_committed_forest_leaves_the_small_batch_kernels():
    """A forest the library's own commit wrote: 5,000 leaves under 500 + 50 + 5 + 1 pointer
    blocks of fan-out 10, traced for all its leaves, so one level holds 5,000 distinct short
    blocks. The leaf with index i = d3 d2 d1 d0 (decimal) is reached by the tag d0 d1 d2 d3."""
    n, F, slot, L = 5000, 10, 1024, 728
    blocks, arena, last, levels = su.forest_arena(n, F, slot, L)
    commit.commit_host(arena, blocks, 1, last)
    case = su.committed_tree(arena, n, F, slot, L, levels)
    root, root_type, _, _ = case.tree
    t = tu.Tree(arena, case.lay, root[:2], root_type, BLOB, L)
    tags = [int(("%04d" % i)[::-1]) for i in range(n)]
    res, rep = same_everywhere(t, tags, torch.from_numpy(arena).cuda())
    assert rep.ok and rep.blocks_hashed == (556, 5000) and rep.levels == 5
    assert [int(a) for a in res["address"]] == list(range(1, n + 1)) and not res["reminder"].any()


@pytest.mark.parametrize("k", [64, 65])
def test_chain(k):
    t = tu.chain(k)
    res, rep = same_everywhere(t, [0, 1], on_device("chain %d" % k, t.img))
    assert (int(res["status"][1]), int(res["depth"][1])) == (ABSENT, 1)
    if k == 64:
        assert (int(res["status"][0]), int(res["depth"][0])) == (FOUND, 64) and sum(rep.blocks_hashed) == 65
    else:
        assert (int(res["status"][0]), int(res["depth"][0])) == (DEPTH, 64) and sum(rep.blocks_hashed) == 64
        assert int(res["address"][0]) == t.root[1] - 64 and rep.first_bad == 0 and "more than 64" in rep.message


# ---- streams -----------------------------------------------------------------------------------

def test_trace_on_a_side_stream_sees_the_write_queued_before_it():
    """The last leaf is wrong until a copy queued on a non-default stream, behind a kernel that
    keeps that stream busy, repairs it. A trace given that stream runs behind the copy."""
    t = tu.shape("f10")
    bs, last_leaf = t.lay.block_size, 1000  # build_tree puts the leaves at addresses 1..1000
    image = torch.from_numpy(np.array(t.img)).cuda()
    good = image[last_leaf * bs:last_leaf * bs + t.leaf_len].clone()
    image[last_leaf * bs:last_leaf * bs + t.leaf_len] = 0
    tags = device_tags([999, 0])
    torch.cuda.synchronize()
    res, before = trace.trace_device(image, *t.args(), tags, t.leaf_len)
    assert before.first_bad == 0 and before.n_status[MISMATCH] == 1
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)  # a few milliseconds in which the stream has not reached the copy
        image[last_leaf * bs:last_leaf * bs + t.leaf_len].copy_(good, non_blocking=True)
        assert not side.query()
        res, rep = trace.trace_device(image, *t.args(), tags, t.leaf_len, stream=side.cuda_stream)
    assert side.query()  # synchronous: nothing of the trace is still queued
    assert rep.ok and rep.n_status[FOUND] == 2
    engine.stream_forget(side.cuda_stream)


def test_capturing_stream_is_rejected():
    t = tu.leaf_root_tree()
    image = on_device("leaf root", t.img)
    tags = device_tags([1, 2])
    ws = torch.empty(trace.workspace_bytes(2) // 8 + 1, dtype=torch.int64, device="cuda")
    results = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    scratch = torch.zeros(8, dtype=torch.int64, device="cuda")
    raw = _lib.TraceReportStruct()
    root = _lib.PointerStruct(t.root[0], t.root[1], 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1)  # the capture holds one node of its own
        rc = _lib.lib.stormck_trace_device(image.data_ptr(), ctypes.byref(t.lay), ctypes.byref(root), t.root_type, BLOB, 0,
                                           tags.data_ptr(), 2, 0, results.data_ptr(), None, ws.data_ptr(),
                                           ws.numel() * 8, ctypes.byref(raw), torch.cuda.current_stream().cuda_stream)
        message = _lib.last_error()
    assert rc == _lib.EINVAL and "captured" in message
    graph.replay()
    torch.cuda.synchronize()
    assert int(scratch[0]) == 1 and not results.any()  # the capture holds nothing of the trace


# ---- keys --------------------------------------------------------------------------------------

def test_trace_keys_device():
    """keystore's lookup: 200 keys of 48 bytes, their tree at fan-out 10 over the oracle's
    XXH64 tags (20 digits deep), and 50 keys that were never stored."""
    rng = np.random.default_rng(48)
    keys = rng.integers(0, 256, (250, 48), dtype=np.uint8)
    tags = [o.xxh64(k.tobytes()) for k in keys]
    bs, leaf_len = 1024, 536
    store = Store(bs, 1)
    initialize(store)
    build_tree(store, 10, leaf_len, tags[:200], revision=2, seed=3)
    n_blocks = max(store.dev) + 1
    img = su.flatten(store, n_blocks, su.SLACK)
    lay = ScrubLayout(bs, n_blocks, 10, 10, leaf_len, 728)
    t = tu.Tree(img, lay, (su._u64(img, 32), su._u64(img, 40)), int(img[56]), OBJECTLIST)
    image = torch.from_numpy(img).cuda()
    dres, drep, dtags = trace.trace_keys_device(image, lay, t.root + (2,), t.root_type, torch.from_numpy(keys).cuda())
    assert [int(x) for x in engine.u64(dtags)] == tags
    res = trace.results_numpy(dres)
    hres, hrep = trace.trace_host(img, *t.args(), tu.tags_u64(tags))
    assert res.tobytes() == hres.tobytes() and drep.as_dict() == hrep.as_dict() and drep.ok
    assert tu.as_tuples(res) == t.reference(tags)[0]
    leaf_of = {tag: 1 + i for i, tag in enumerate(sorted(tags[:200]))}  # build_tree: leaves in tag order from address 1
    for tag, r in zip(tags[:200], res[:200]):
        assert (int(r["status"]), int(r["address"]), int(r["depth"])) == (FOUND, leaf_of[tag], 20)
    for tag, r in zip(tags[200:], res[200:]):
        assert r["status"] == ABSENT or (r["status"] == FOUND and int(r["address"]) != leaf_of.get(tag))
