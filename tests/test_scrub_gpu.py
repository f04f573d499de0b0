"""Scrub on the device (MI355X): stormck_scrub_device / stormck_scrub_tree_device give the
reports and reachable bitmaps of the host leg and of the pure-Python reference
(tests/scrub_util.py) on the same images. Every wrong address used here points inside the
tensor the test allocated (the images carry slack blocks past n_blocks); the huge-address
cases stay on the host leg (tests/test_scrub.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, engine, scrub  # noqa: E402
from storm_amd.scrub import BLOB, MISMATCH  # noqa: E402
from tests import scrub_util as su  # noqa: E402

_device_images = {}


def on_device(key, img):
    """The image as a device tensor, uploaded once per store."""
    if key not in _device_images:
        _device_images[key] = torch.from_numpy(np.array(img)).cuda()
    return _device_images[key]


def same_as_host_and_reference(dev, host, want, want_bitmap):
    bitmap = dev.reachable.cpu().numpy().view(np.uint32)
    assert dev.as_dict() == want
    assert dev.as_dict() == host.as_dict() and dev.code == host.code and dev.message == host.message
    assert np.array_equal(bitmap, want_bitmap) and np.array_equal(bitmap, host.reachable)


@pytest.mark.parametrize("name", list(su.TREE_SHAPES))
def test_tree_shapes(name):
    img, lay, root, root_type, leaf_len = su.tree_shape(name)
    _, _, _, _, levels, n_ptr, n_leaf = su.TREE_SHAPES[name]
    want, want_bitmap, _ = su.reference_scrub(img, lay, root, root_type, BLOB, leaf_len)
    host = scrub.scrub_tree_host(img, lay, root + (2,), root_type, BLOB, leaf_len, reachable=True)
    dev = scrub.scrub_tree_device(on_device(name, img), lay, root + (2,), root_type, BLOB, leaf_len, reachable=True)
    same_as_host_and_reference(dev, host, want, want_bitmap)
    assert dev.ok and dev.verified == (n_ptr, 0, 0, n_leaf) and dev.levels == len(levels)


STORES = {"test tag": su.tag_store, "production": su.production_store, "empty": su.empty_store,
          "leaf root": su.leaf_root_store}


@pytest.mark.parametrize("name", list(STORES))
def test_whole_stores(name):
    img, lay = STORES[name]()
    want, want_bitmap, _ = su.reference_scrub(img, lay)
    host = scrub.scrub_host(img, lay, reachable=True)
    dev = scrub.scrub_device(on_device(name, img), lay, reachable=True)
    same_as_host_and_reference(dev, host, want, want_bitmap)
    assert dev.ok


IN_ALLOCATION = [n for n in su.DAMAGE if n not in ("address 2**63", "address 2**64-1")]


@pytest.mark.parametrize("name", IN_ALLOCATION)
def test_damage(name):
    img, lay = su.tag_store()
    _, _, index = su.reference_scrub(img, lay)
    img = img.copy()
    expect = su.DAMAGE[name](img, lay, index)
    assert expect.get("first_address", 0) < lay.n_blocks + su.SLACK  # inside the tensor
    want, want_bitmap, _ = su.reference_scrub(img, lay)
    host = scrub.scrub_host(img, lay, reachable=True)
    dev = scrub.scrub_device(torch.from_numpy(img).cuda(), lay, reachable=True)
    same_as_host_and_reference(dev, host, want, want_bitmap)
    assert dev.code == _lib.EMISMATCH
    for field, value in expect.items():
        assert getattr(dev, field) == value, field


def test_tree_mid_level_damage_drops_its_subtree():
    img, lay, root, root_type, leaf_len = su.tree_shape("f10")
    _, _, index = su.reference_scrub(img, lay, root, root_type, BLOB, leaf_len)
    victim = min(a for a, (_, _, k, lvl) in index.items() if k == scrub.POINTER and lvl == 1)
    img = img.copy()
    img[victim * lay.block_size + 5] ^= 0x40
    want, want_bitmap, _ = su.reference_scrub(img, lay, root, root_type, BLOB, leaf_len)
    host = scrub.scrub_tree_host(img, lay, root + (2,), root_type, BLOB, leaf_len, reachable=True)
    dev = scrub.scrub_tree_device(torch.from_numpy(img).cuda(), lay, root + (2,), root_type, BLOB, leaf_len,
                                  reachable=True)
    same_as_host_and_reference(dev, host, want, want_bitmap)
    assert dev.verified == (100, 0, 0, 900) and (dev.first_error, dev.first_address) == (MISMATCH, victim)


def test_device_built_tree_crosses_the_dispatch_boundaries():
    """A tree built entirely on the device by existing entry points: 12,288 synthetic
    32 KiB leaves at addresses 1..n, their pointer blocks packed at n+1.. (11 + 1). Its
    levels of 1, 11 and 12,288 rows take three different kernels of the batch dispatch."""
    n, F, bs, rev = 12288, 1200, 32768, 3
    n_blocks = n + 1 + 11 + 1
    image = torch.zeros((n_blocks + 1, bs), dtype=torch.uint8, device="cuda")
    base = image.data_ptr()
    cs = torch.empty(n, dtype=torch.int64, device="cuda")
    engine.fill_synthetic_device(base + bs, bs, n, 0, su.o.SYNTH_SEED)
    engine.checksum_device(base + bs, bs, n, cs.data_ptr(), bs)
    engine.pack_pointer_blocks_device(cs.data_ptr(), n, 1, rev, 2, F, base + (n + 1) * bs, bs)
    ws = torch.zeros(engine.merkle_workspace_bytes(n, F) // 8, dtype=torch.int64, device="cuda")
    root = torch.zeros(4, dtype=torch.int64, device="cuda")
    engine.merkle_root_device(cs.data_ptr(), n, 1, n + 1, rev, F, ws.data_ptr(), ws.numel() * 8, root.data_ptr(),
                              root.data_ptr() + 24)
    engine.pack_pointer_blocks_device(ws.data_ptr(), 11, n + 1, rev, 1, F, base + (n + 12) * bs, bs)
    torch.cuda.synchronize()
    r_cs, r_addr, r_rev, r_type = engine.as_tuple(root)
    assert (r_addr, r_rev, r_type) == (n + 12, rev, 1)
    lay = scrub.ScrubLayout.production(n_blocks)
    rep = scrub.scrub_tree_device(image, lay, (r_cs, r_addr, r_rev), r_type, BLOB, reachable=True)
    assert rep.ok and rep.n_mismatch == 0 and rep.n_structural == 0 and rep.first_error == 0
    assert rep.verified == (11 + 1, 0, 0, n) and rep.levels == 3
    assert rep.bytes_hashed == 12 * 30000 + n * bs
    bitmap = rep.reachable.cpu().numpy().view(np.uint32)
    assert su.popcount(bitmap) - 1 == sum(rep.verified) == n_blocks - 1

    image[7000, 12345] ^= 0x80  # one byte of leaf 7,000
    damaged = torch.empty(1, dtype=torch.int64, device="cuda")
    engine.checksum_device(base + 7000 * bs, bs, 1, damaged.data_ptr(), bs)
    rep = scrub.scrub_tree_device(image, lay, (r_cs, r_addr, r_rev), r_type, BLOB, reachable=True)
    assert rep.code == _lib.EMISMATCH and rep.n_mismatch == 1 and rep.n_structural == 0
    assert rep.verified == (12, 0, 0, n - 1)
    assert (rep.first_error, rep.first_address, rep.first_level) == (MISMATCH, 7000, 2)
    assert (rep.first_parent, rep.first_slot) == (n + 1 + (7000 - 1) // F, (7000 - 1) % F)
    assert rep.first_computed == int(engine.u64(damaged)[0])
    assert rep.first_expected == int(engine.u64(cs)[7000 - 1])
    assert su.popcount(rep.reachable.cpu().numpy().view(np.uint32)) == n_blocks  # a mismatching block was still read


def test_scrub_on_a_side_stream_sees_the_write_queued_before_it():
    """The image's last leaf is wrong until a copy queued on a non-default stream, behind a
    kernel that keeps that stream busy, repairs it. A scrub given that stream runs behind
    the copy and finds the store intact; it returns only when the walk has finished."""
    img, lay, root, root_type, leaf_len = su.tree_shape("f10")
    bs = lay.block_size
    last_leaf = 1000  # build_tree puts the leaves at addresses 1..1000
    image = torch.from_numpy(np.array(img)).cuda()
    good = image[last_leaf * bs:last_leaf * bs + leaf_len].clone()
    image[last_leaf * bs:last_leaf * bs + leaf_len] = 0
    torch.cuda.synchronize()
    before = scrub.scrub_tree_device(image, lay, root + (2,), root_type, BLOB, leaf_len)
    assert before.n_mismatch == 1 and before.first_address == last_leaf
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)  # a few milliseconds in which the stream has not reached the copy
        image[last_leaf * bs:last_leaf * bs + leaf_len].copy_(good, non_blocking=True)
        assert not side.query()
        rep = scrub.scrub_tree_device(image, lay, root + (2,), root_type, BLOB, leaf_len, stream=side.cuda_stream)
    assert side.query()  # synchronous: nothing of the walk is still queued
    assert rep.ok and rep.verified == (111, 0, 0, 1000)
    engine.stream_forget(side.cuda_stream)


def test_capturing_stream_is_rejected():
    """A scrub synchronises its stream every level, so it cannot be captured into a graph:
    STORMCK_EINVAL before anything is queued."""
    img, lay = su.leaf_root_store()
    image = on_device("leaf root", img)
    ws = torch.empty(scrub.workspace_bytes(lay.n_blocks) // 8 + 1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(8, dtype=torch.int64, device="cuda")
    raw = _lib.ScrubReportStruct()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1)  # the capture holds one node of its own
        rc = _lib.lib.stormck_scrub_device(image.data_ptr(), ctypes.byref(lay), ws.data_ptr(), ws.numel() * 8, None,
                                           ctypes.byref(raw), torch.cuda.current_stream().cuda_stream)
        message = _lib.last_error()
    assert rc == _lib.EINVAL and "captured" in message
