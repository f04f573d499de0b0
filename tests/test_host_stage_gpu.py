"""The staged device legs of a host-memory batch on the GPU: the two-stage pipeline of
stormck_checksum_host / _verify_host and the device part of a split, which drive the same
per-device stages (stream, staging and result buffers).

  * stage reuse: 11 blocks at a 64 MiB stride are three pipeline chunks (4, 4, 3), so the
    third chunk reuses the first stage; checksums against the C oracle (blocks.Checksum =
    XXH64 seed 0), verify with mismatches in the first chunk, in the reused stage and in
    the last block, from pageable and from registered memory, with per-block and uniform
    lengths;
  * the same batch through a split's device part: in-place strided chunks of 4 over three
    claims, and mismatches on both sides of the boundary;
  * the argument-error table of every host-memory batch entry point
    (tests/host_batch_cases.py).
"""
import contextlib

import numpy as np
import pytest

from oracle import oracle as o
from storm_amd import blocks, engine
from tests import host_batch_cases as hc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, STRIDE, ROW = 11, 64 << 20, 32768


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()
    engine.init(0)
    yield
    blocks.SetRouteRates(None)
    blocks.RouteDevices(None)


def _aligned_zeros(nbytes):
    raw = np.zeros(nbytes + 4096, dtype=np.uint8)
    off = (-raw.ctypes.data) % 4096
    return raw[off:off + nbytes]


class Batch:
    """11 rows 64 MiB apart, only the first 32 KiB of each filled; the oracle's checksums
    for per-block lengths (with a 0 and a full row) and for uniform full rows."""

    def __init__(self):
        self.buf = _aligned_zeros((N - 1) * STRIDE + ROW)
        rng = np.random.default_rng(2024)
        for i in range(N):
            self.buf[i * STRIDE:i * STRIDE + ROW] = rng.integers(0, 256, size=ROW, dtype=np.uint8)
        lens = rng.integers(0, ROW + 1, size=N).astype(np.uint32)
        lens[3], lens[6] = 0, ROW
        self.shapes = {"lens": dict(lens=lens), "uniform": dict(length=ROW)}
        self.want = {k: o.checksum_batch(self.buf, N, STRIDE, **kw) for k, kw in self.shapes.items()}


@pytest.fixture(scope="module")
def batch():
    return Batch()


@contextlib.contextmanager
def _registered(buf):
    blocks.RegisterHostMemory(buf)
    try:
        yield buf
    finally:
        blocks.UnregisterHostMemory(buf)


def _flipped(want, idx):
    bad = want.copy()
    bad[list(idx)] ^= 1
    return bad


def _pipeline_checks(batch, shape):
    kw, want = batch.shapes[shape], batch.want[shape]
    assert np.array_equal(blocks.ChecksumBatchGPU(batch.buf, N, STRIDE, **kw), want)
    assert blocks.VerifyChecksumBatchGPU(batch.buf, N, STRIDE, want, **kw) == (N, 0)
    # one mismatch in the first chunk, one in the reused stage, one in the last block
    assert blocks.VerifyChecksumBatchGPU(batch.buf, N, STRIDE, _flipped(want, (1, 8, 10)), **kw) == (1, 3)
    assert blocks.VerifyChecksumBatchGPU(batch.buf, N, STRIDE, _flipped(want, (9,)), **kw) == (9, 1)


@pytest.mark.parametrize("shape", ["lens", "uniform"])
def test_pipeline_reuses_a_stage(batch, shape):
    _pipeline_checks(batch, shape)  # pageable: through the pinned staging
    with _registered(batch.buf):    # registered: DMA from where the rows are
        _pipeline_checks(batch, shape)


@pytest.mark.parametrize("shape", ["lens", "uniform"])
def test_split_device_part_over_three_claims(batch, shape):
    kw, want = batch.shapes[shape], batch.want[shape]
    with _registered(batch.buf):
        for d in (0, 5, N):
            got, done = blocks.ChecksumBatchSplit(batch.buf, N, STRIDE, devices=[0], device_blocks=d, **kw)
            assert done == d and np.array_equal(got, want), d
        # the devices own blocks 6..10: mismatches on both sides of the boundary
        assert blocks.VerifyChecksumBatchSplit(batch.buf, N, STRIDE, _flipped(want, (1, 8, 10)), devices=[0],
                                               device_blocks=5, **kw) == (1, 3, 5)


# ---- the argument-error table ------------------------------------------------------------
@pytest.fixture(scope="module")
def table_buffers():
    page = _aligned_zeros(hc.buffer_bytes())
    reg = _aligned_zeros(hc.buffer_bytes())
    blocks.RegisterHostMemory(reg)
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    yield page, reg, dev
    blocks.UnregisterHostMemory(reg)


@pytest.mark.parametrize("entry", list(hc.ENTRIES))
def test_error_table(table_buffers, entry):
    page, reg, dev = table_buffers
    buf = reg if hc.ENTRIES[entry][2] else page  # the split entries take pinned or registered memory only
    for case in hc.cases_of(entry):
        if entry in hc.HOST_LEG and case != "device_base":
            continue  # tests/test_host_batch.py, without a device
        got = hc.run_case(entry, case, buf, dev.data_ptr())
        print(entry, case, got)
        assert got == hc.EXPECTED[entry, case], (entry, case)
