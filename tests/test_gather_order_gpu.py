"""The locality order of large gathers (kernels.h k_order_count / k_order_scan_buckets /
k_order_place / k_order_sort, k_order_scatter, k_order_rank) on designed inputs
(tests/order_cases.py, whose populations tests/test_order_cases.py checks on the CPU).

* The order pass alone, through tests/hip/liborderpass.so (launch_checksum's own
  order_pass helper on the test's buffers; no offset is dereferenced, so no arena): the
  permutation, the carried offsets and lengths, the bucket bounds, the order inside every
  bucket the sort takes, and poisoned slack after every output. Placement order and the
  order among equal keys depend on atomics and are not asserted.
* End to end through stormck_checksum_gather_device on a 1,088 MiB arena, 2^20 + 37 blocks
  that repeat and overlap: per-block lengths and one length, each in the non-persistent and
  in the persistent form (tests/cpp/dispatch_plan_test.cpp pins the four plans), and the
  probe build's variants of the order, each in a child process. Every checksum against
  the C oracle, `out` poisoned before each call.
"""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as o
from tests import order_cases as oc
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLACK = 64
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
B = oc.BUCKETS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from storm_amd import build as sb
    assert os.path.exists(sb.ORDER_PASS), "tests/hip/liborderpass.so missing: storm_amd.build.build_order_pass()"
    h = ctypes.CDLL(sb.ORDER_PASS)
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    h.orderpass_run.argtypes, h.orderpass_run.restype = [p, p, u64, p, p, p, p, p, ctypes.c_int, p], ctypes.c_int
    h.orderpass_scatter.argtypes, h.orderpass_scatter.restype = [p, p, p, u64, p], ctypes.c_int
    h.orderpass_rank.argtypes, h.orderpass_rank.restype = [p, p, p, u64, u64, p], ctypes.c_int
    return h


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = oc.ORDER_CASES[name]()
    return _cases[name]


def _poison32(words, dev):
    return torch.from_numpy(np.full(words, P32, dtype=np.uint32).view(np.int32)).to(dev)


def _poison64(words, dev):
    return torch.from_numpy(np.full(words, P64, dtype=np.uint64).view(np.int64)).to(dev)


def _h32(t):
    return t.cpu().numpy().view(np.uint32)


def _h64(t):
    return t.cpu().numpy().view(np.uint64)


def _run_order(lib, dev, offs, lens, idx):
    """One order pass on poisoned buffers with SLACK words after each; the host copies."""
    n = offs.size
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = None if lens is None else torch.from_numpy(lens.view(np.int32)).to(dev)
    bounds, cursor = _poison32(2 * B + SLACK, dev), _poison32(B + SLACK, dev)
    order, s_offs, s_lens = _poison32(n + SLACK, dev), _poison64(n + SLACK, dev), _poison32(n + SLACK, dev)
    rc = lib.orderpass_run(d_offs.data_ptr(), d_lens.data_ptr() if d_lens is not None else None, n, bounds.data_ptr(),
                           cursor.data_ptr(), order.data_ptr(), s_offs.data_ptr(), s_lens.data_ptr(), int(idx), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return dict(bounds=bounds, cursor=cursor, order=order, s_offs=s_offs, s_lens=s_lens)


def _check_order(offs, lens, bufs):
    n = offs.size
    bounds, cursor = _h32(bufs["bounds"]), _h32(bufs["cursor"])
    order, s_offs, s_lens = _h32(bufs["order"]), _h64(bufs["s_offs"]), _h32(bufs["s_lens"])
    # the slack words are unchanged
    assert (bounds[2 * B:] == P32).all() and (cursor[B:] == P32).all() and (order[n:] == P32).all()
    assert (s_offs[n:] == P64).all() and (s_lens[n:] == P32).all()
    order, s_offs = order[:n], s_offs[:n]
    # a permutation of 0..n-1 (no entry dropped or duplicated)
    assert order.max() < n and np.array_equal(np.bincount(order, minlength=n), np.ones(n, dtype=np.int64))
    # the offsets and lengths in that order
    assert np.array_equal(s_offs, offs[order])
    if lens is None:
        assert (s_lens == P32).all(), "s_lens is untouched without lens"
    else:
        assert np.array_equal(s_lens[:n], lens[order])
    # the bounds: exclusive prefix sums and ends of the bucket histogram
    hist = np.bincount(oc.bucket_of(offs), minlength=B)
    ends = np.cumsum(hist)
    assert np.array_equal(bounds[:B], ends - hist) and np.array_equal(bounds[B:2 * B], ends)
    assert np.array_equal(cursor[:B], ends), "every reservation made, none twice"
    # every entry in [first, end) of a bucket belongs to it
    at = np.repeat(np.arange(B), hist)
    assert np.array_equal(oc.bucket_of(s_offs), at)
    # buckets of at most 2,048 entries: the offset inside the region is non-decreasing
    key = (s_offs & np.uint64(oc.REGION - 1)).astype(np.int64)
    inside = (at[1:] == at[:-1]) & (hist[at[1:]] <= oc.SORT_MAX)
    down = np.nonzero(inside & (np.diff(key) < 0))[0]
    assert down.size == 0, (down.size, at[down[:4]], hist[at[down[:4]]])
    return order


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "nolens"])
@pytest.mark.parametrize("idx", [False, True], ids=["offsets", "idx"])
@pytest.mark.parametrize("name", sorted(oc.ORDER_CASES))
def test_order_pass(lib, dev, name, idx, with_lens):
    """Every branch of k_order_sort and the boundaries between them (the case's claims), with
    offsets placed beside the indices or gathered through them (IDX)."""
    case = _case(name)
    lens = case.lens if with_lens else None
    _check_order(case.offs, lens, _run_order(lib, dev, case.offs, lens, idx))


@pytest.mark.parametrize("name", ["small", "big"])
def test_order_scatter(lib, dev, name):
    """k_order_scatter: out[order[k]] = s_out[k], nothing else written."""
    case = _case(name)
    n = case.n
    bufs = _run_order(lib, dev, case.offs, None, False)
    order = _check_order(case.offs, None, bufs)
    s_out = np.random.default_rng(n).integers(0, 1 << 64, size=n, dtype=np.uint64)
    s_out[s_out == P64] = 0
    d_s_out = torch.from_numpy(s_out.view(np.int64)).to(dev)
    out = _poison64(n + SLACK, dev)
    rc = lib.orderpass_scatter(bufs["order"].data_ptr(), d_s_out.data_ptr(), out.data_ptr(), n, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    got = _h64(out)
    assert (got[n:] == P64).all()
    assert np.array_equal(got[:n][order], s_out)
    assert (_h32(bufs["order"])[n:] == P32).all() and np.array_equal(_h64(d_s_out), s_out)


def test_order_rank(lib, dev):
    """k_order_rank on 2^20 + 37 entries: each full group of 128 keeps its (index, offset,
    length) triples, and inside group g, with k = (g / G) & 7, wave ((r >> 4) + 8 - k) & 7
    holds the 16 entries of length ranks 16 (r >> 4) .. + 15 in rank order, ties by the
    position before; the partial last group is left as it is."""
    case = _case("big")
    n, G = case.n, 256
    lens = np.array([31808, 30000, 32768, 28808], dtype=np.uint32)[np.random.default_rng(9).integers(0, 4, size=n)]
    bufs = _run_order(lib, dev, case.offs, lens, False)
    _check_order(case.offs, lens, bufs)
    before = [_h32(bufs["order"]).copy(), _h64(bufs["s_offs"]).copy(), _h32(bufs["s_lens"]).copy()]
    rc = lib.orderpass_rank(bufs["order"].data_ptr(), bufs["s_offs"].data_ptr(), bufs["s_lens"].data_ptr(), n, G, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    after = [_h32(bufs["order"]), _h64(bufs["s_offs"]), _h32(bufs["s_lens"])]
    full = n // 128 * 128
    for b, a in zip(before, after):
        assert np.array_equal(a[full:], b[full:]), "the partial group and the slack stay"
    groups = full // 128
    ln = before[2][:full].reshape(groups, 128).astype(np.int64)
    # rank = entries of the group that are shorter, or as long and earlier (a stable sort's place)
    by_rank = np.argsort(ln, axis=1, kind="stable")  # by_rank[g, r] = position before of rank r
    k = (np.arange(groups) // G) & 7
    r = np.arange(128)
    to = (((r[None, :] >> 4) + 8 - k[:, None]) & 7) * 16 + (r[None, :] & 15)  # rank r's row in group g
    assert sorted(np.unique(k).tolist()) == list(range(8))  # every rotation occurs
    rows = np.arange(groups)[:, None]
    for b, a in zip(before, after):
        b2, a2 = b[:full].reshape(groups, 128), a[:full].reshape(groups, 128)
        want = np.empty_like(b2)
        want[rows, to] = b2[rows, by_rank]
        assert np.array_equal(a2, want)
    # the same set of triples per group (implied by the rule; stated on its own)
    def triples(x):
        t = np.stack([x[0][:full].astype(np.uint64), x[1][:full], x[2][:full].astype(np.uint64)], axis=1).reshape(groups, 128, 3)
        idx = np.argsort(t[:, :, 0], axis=1, kind="stable")  # the indices are distinct
        return np.take_along_axis(t, idx[:, :, None], axis=1)
    assert np.array_equal(triples(before), triples(after))


# ---- end to end through the product ABI -------------------------------------------------------

SLOT = 32768
ARENA_FIRST = 3  # logical index of the arena's first synthetic block


def _fill_arena(dev):
    from storm_amd import engine
    arena = torch.empty(oc.ARENA_BYTES, dtype=torch.uint8, device=dev)
    engine.fill_synthetic_device(arena.data_ptr(), SLOT, oc.ARENA_BYTES // SLOT, ARENA_FIRST, o.SYNTH_SEED)
    torch.cuda.synchronize()
    return arena


@pytest.fixture(scope="module")
def arena(dev):
    d = _fill_arena(dev)
    return d, d.cpu().numpy()


def _oracle(host, offs, lens, length=0):
    """The oracle over the unique (offset, length) pairs, expanded."""
    if lens is None:
        uniq, inv = np.unique(offs, return_inverse=True)
        return o.checksum_gather(host, uniq, length=length, threads=16)[inv]
    pair = (offs << np.uint64(13)) | lens.astype(np.uint64)  # lengths below 2^13, offsets below 2^31
    assert int(lens.max()) < 1 << 13 and int(offs.max()) < 1 << 31
    uniq, inv = np.unique(pair, return_inverse=True)
    return o.checksum_gather(host, uniq >> np.uint64(13), lens=(uniq & np.uint64(8191)).astype(np.uint32), threads=16)[inv]


@pytest.fixture(scope="module")
def lens_case(arena):
    case = oc.arena_lens()
    return case, _oracle(arena[1], case.offs, case.lens)


def _compare(got, want, n, what):
    assert (got[n:] == P64).all(), (what, "slack after out[n] written")
    got = got[:n]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, f"{bad.size} of {n} differ, {int((got == P64).sum())} never written", bad[:8])


def _gather(dev, d_arena, case, bound, with_lens):
    from storm_amd import engine
    n = case.n
    d_offs = torch.from_numpy(case.offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(case.lens.view(np.int32)).to(dev) if with_lens else None
    out = _poison64(n + SLACK, dev)
    engine.checksum_gather_device(d_arena.data_ptr(), d_offs.data_ptr(), n, out.data_ptr(), bound,
                                  d_lens.data_ptr() if with_lens else 0)
    torch.cuda.synchronize()
    return _h64(out)


@pytest.mark.parametrize("bound", [0, 65536], ids=["bound0-grid8193", "bound65536-persistent"])
def test_ordered_gather_per_block_lengths(dev, arena, lens_case, bound):
    """Per-block lengths of 0..4,200 B, 3 % of the filler's starts off 16 bytes, every designed
    bucket: the non-persistent form (no bound: planned as 32 KiB) and the persistent skewed
    one (bound 65,536)."""
    case, want = lens_case
    _compare(_gather(dev, arena[0], case, bound, True), want, case.n, ("lens", bound))


@pytest.mark.parametrize("length", [4112, 60000], ids=["4112-grid8193", "60000-persistent"])
def test_ordered_gather_one_length(dev, arena, length):
    """One length and no lens (k_xxh64_glds_var<LENS=false, OFFS=true, ORD=true>): 4,112 B in
    the non-persistent form, 60,000 B in the persistent one."""
    case = oc.arena_uniform(length)
    want = _oracle(arena[1], case.offs, None, length)
    _compare(_gather(dev, arena[0], case, length, False), want, case.n, ("uniform", length))


_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from storm_amd import engine
from tests import order_cases as oc
from tests import test_gather_order_gpu as t
assert engine.build_id().endswith("+probes"), engine.build_id()
dev = torch.device("cuda:0")
arena = t._fill_arena(dev)
got = t._gather(dev, arena, oc.arena_lens(), 65536, True)
np.save(sys.stdout.buffer, got)
"""


@pytest.mark.parametrize("knobs", [{"STORMCK_ORDER_IDX": "1"}, {"STORMCK_GATHER_DEFER": "1"}, {"STORMCK_GATHER_RANK": "1"},
                                   {"STORMCK_GATHER_CONTIG": "1"},
                                   {"STORMCK_GATHER_DEFER": "1", "STORMCK_GATHER_CONTIG": "1"},
                                   {"STORMCK_GATHER_ORDER": "0"}],
                         ids=lambda k: "+".join(f"{a[8:]}={b}" for a, b in k.items()))
def test_ordered_gather_probe_variants(dev, lens_case, knobs):
    """The order's variants behind probe knobs, which only the probe build has; each runs in
    a child that loads it (STORMCK_LIBRARY) on the per-block-length case at bound 65,536
    (the rank deal and the contiguous runs need the persistent form). Every checksum equal
    to the oracle's, poison and slack as above."""
    from storm_amd import build as sb
    assert os.path.exists(sb.PROBES_LIB), "probe build missing: storm_amd.build.build_probes_lib()"
    case, want = lens_case
    env = dict(os.environ, STORMCK_LIBRARY=sb.PROBES_LIB, **knobs)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], cwd=ROOT, capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _compare(np.load(io.BytesIO(r.stdout)), want, case.n, knobs)
