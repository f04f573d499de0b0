"""The routed calls take the leg their plan entry points report (GPU).

stormck_checksum_batch / stormck_commit and stormck_route_plan_batch / _plan_commit ask one
decision (storm_amd/csrc/route_plan.h route_batch, route_commit); tests/test_route.py checks
the plan entry points without a device, and this file that the call itself runs the leg they
name, with checksums exact against the C oracle. Rates are injected and frozen and one device
is used, so the decision is deterministic; the shapes stay small (storm's smallest calls, and
64 x 32 KiB) and the rates move instead, so that the host, the device and the split each win.
Every call here is alone in its process's pool, which is what the plan entry points price.
"""
import numpy as np
import pytest

from oracle import oracle as o
from storm_amd import _lib, blocks, engine
from storm_amd import commit as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STRIDE = 32768
BASE = dict(host_thread=40000.0, host_memory=180000.0, host_cached=180000.0, link_pinned=55000.0,
            link_pageable=50000.0, link_inplace=52000.0, device_latency=120.0)
# 2 MiB (64 x 32 KiB; 70 leaves): the pool at 300 GB/s against a link of 0.1 GB/s
HOST_WINS = dict(host_thread=40000.0, host_memory=300000.0, host_cached=300000.0, link_pinned=100.0,
                 link_pageable=100.0, link_inplace=100.0, device_latency=150.0)
# a host of 0.4 GB/s, and a start latency that prices the split out
DEVICE_WINS = dict(host_thread=100.0, host_memory=400.0, host_cached=400.0, link_pinned=55000.0,
                   link_pageable=50000.0, link_inplace=50000.0, device_latency=1e6)
# a host of 20 GB/s beside an in-place link of 50 GB/s, no start latency, a slow pipeline
SPLIT_WINS = dict(host_thread=20000.0, host_memory=20000.0, host_cached=20000.0, link_pinned=20000.0,
                  link_pageable=20000.0, link_inplace=50000.0, device_latency=1.0)
# (rates, the leg from registered memory, the leg from pageable memory, which never splits:
# the host's 115 us there against 179 us through the staging copy)
RATE_SETS = {"host": (HOST_WINS, _lib.LEG_HOST, _lib.LEG_HOST),
             "device": (DEVICE_WINS, _lib.LEG_DEVICE, _lib.LEG_DEVICE),
             "split": (SPLIT_WINS, _lib.LEG_SPLIT, _lib.LEG_HOST)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()
    engine.init(0)
    blocks.RouteDevices(None)
    yield
    blocks.SetRouteRates(None)


class Registered:
    """A page-aligned host buffer registered with the library (the Go binding's cache.data)."""

    def __init__(self, nbytes):
        self.raw = np.zeros(nbytes + 4096, dtype=np.uint8)
        off = (-self.raw.ctypes.data) % 4096
        self.a = self.raw[off:off + nbytes]
        blocks.RegisterHostMemory(self.a)

    def close(self):
        blocks.UnregisterHostMemory(self.a)


def _batch_agrees(n, stride, length=None, lens=None, want_leg=None, want_pageable=None, seed=0):
    """The routed batch from registered and from pageable memory: the plan's leg, exact."""
    reg = Registered(n * stride)
    try:
        reg.a[:] = np.random.default_rng(seed).integers(0, 256, size=n * stride, dtype=np.uint8)
        pageable = reg.a.copy()
        want = o.checksum_batch(reg.a, n, stride, length or 0, lens=lens)
        for buf, pinned, leg_wanted in ((reg.a, True, want_leg), (pageable, False, want_pageable)):
            plan, us = blocks.PlanBatch(n, stride, length, lens=lens, pinned=pinned, n_devices=1)
            got, leg = blocks.ChecksumBatchLeg(buf, n, stride, length, lens=lens)
            assert leg == plan, (pinned, leg, plan, us)
            assert leg_wanted is None or leg == leg_wanted, (pinned, leg, us)
            assert np.array_equal(got, want), (pinned, leg)
    finally:
        reg.close()


def test_three_blocks_stay_on_the_calling_thread():
    blocks.SetRouteRates(BASE, freeze=True)
    leg, us = blocks.PlanBatch(3, STRIDE, STRIDE, pinned=True, n_devices=1)
    assert np.isinf(us[1])  # host-only: not planned
    _batch_agrees(3, STRIDE, STRIDE, want_leg=_lib.LEG_HOST, want_pageable=_lib.LEG_HOST, seed=1)


def test_test_tag_lengths():
    """100 blocks of storm's `-tags test` sizes, per-block lengths: host-only at the usual
    rates, planned (and still the host's) once one thread needs 50 us for them."""
    lens = np.array([536, 728] * 50, dtype=np.uint32)
    blocks.SetRouteRates(BASE, freeze=True)
    _batch_agrees(100, 1024, lens=lens, want_leg=_lib.LEG_HOST, want_pageable=_lib.LEG_HOST, seed=2)
    blocks.SetRouteRates(dict(BASE, host_thread=float(lens.sum()) / 50.0), freeze=True)
    leg, us = blocks.PlanBatch(100, 1024, lens=lens, pinned=True, n_devices=1)
    assert np.isfinite(us[1])  # planned
    _batch_agrees(100, 1024, lens=lens, seed=2)


@pytest.mark.parametrize("winner", list(RATE_SETS))
def test_batch_of_64_blocks(winner):
    rates, leg_registered, leg_pageable = RATE_SETS[winner]
    blocks.SetRouteRates(rates, freeze=True)
    _batch_agrees(64, STRIDE, STRIDE, want_leg=leg_registered, want_pageable=leg_pageable, seed=3)


def _commit_agrees(n_leaves, leaf_len, rates, want_leg, seed):
    """The routed commit on a registered arena: the plan's leg, exact against storm's loop."""
    slot = 32768
    rng = np.random.default_rng(seed)
    b, size, last = sc.pointer_forest(n_leaves, leaf_len, 1200, slot=slot, revision=9, first_address=100)
    b["birth_revision"][rng.random(len(b)) < 0.4] = 3  # relocations
    reg = Registered(size)
    try:
        reg.a[slot:slot + n_leaves * slot] = rng.integers(0, 256, size=n_leaves * slot, dtype=np.uint8)
        ref_arena, ref_b = reg.a.copy(), b.copy()
        ref_cs, ref_last = o.commit(ref_arena, ref_b, 9, last)
        blocks.SetRouteRates(rates, freeze=True)
        plan, us = sc.plan_commit(b, registered=True, n_devices=1)
        cs, last2, leg = sc.commit(reg.a.ctypes.data, b, 9, last)
        assert leg == plan, (leg, plan, us)
        assert leg == want_leg, (leg, us)
        assert np.array_equal(cs, ref_cs) and last2 == ref_last and np.array_equal(b, ref_b)
        assert np.array_equal(reg.a, ref_arena)
    finally:
        reg.close()


def test_three_block_forest():
    _commit_agrees(2, 31808, BASE, _lib.LEG_HOST, 4)


@pytest.mark.parametrize("winner", list(RATE_SETS))
def test_forest_of_70_leaves(winner):
    rates, leg_registered, _ = RATE_SETS[winner]
    _commit_agrees(70, 32768, rates, leg_registered, 5)


def test_forest_on_an_unregistered_arena_is_the_hosts():
    """Pageable arena: the plan has no device leg, and the call takes the host leg."""
    b, size, last = sc.pointer_forest(70, 32768, 1200, slot=32768, revision=9, first_address=100)
    arena = np.random.default_rng(6).integers(0, 256, size=size, dtype=np.uint8)
    ref_arena, ref_b = arena.copy(), b.copy()
    ref_cs, ref_last = o.commit(ref_arena, ref_b, 9, last)
    blocks.SetRouteRates(DEVICE_WINS, freeze=True)
    plan, us = sc.plan_commit(b, registered=False, n_devices=1)
    cs, last2, leg = sc.commit(arena.ctypes.data, b, 9, last)
    assert leg == plan == _lib.LEG_HOST and np.isinf(us[1])
    assert np.array_equal(cs, ref_cs) and last2 == ref_last and np.array_equal(b, ref_b)
    assert np.array_equal(arena, ref_arena)
