"""Runs the designed cases of tests/stream_cases.py through tests/hip/libstreamkernels*.so and
compares with the C oracle. Shared by tests/test_stream_kernels_gpu.py (in process, the plain
build) and its child process (`python -m tests.stream_run <library>`: the -DSTORMCK_DEBUG_QUAD
build, every case, then the partial-quad count).

Per case and form, on torch's current stream and with one sync at the end: a checksum launch
into `out` (sentinels before, between and after), a verify launch with the oracle's checksums
(result [n, 0]) and verify launches with planted mismatches (result [first, count]). Before
any launch every block is shown to lie inside the buffer."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

from oracle import oracle as o
from tests import stream_cases as sc
from tests.conftest import ROOT

SENTINEL = 0xA5A5A5A55A5A5A5A
PAD = 64  # sentinel words before and after out[0, n)


PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "plan_query.cpp")
PLAN_BIN = os.path.join(ROOT, "tests", "cpp", "build", "plan_query")
BIG_W = 131072  # dispatch.h kBigW


def build_plan_query():
    """tests/cpp/plan_query.cpp: dispatch.h's plan for a uniform batch under the caller's
    environment (HIP-free, -DSTORMCK_PROBES: the probe build's knobs)."""
    os.makedirs(os.path.dirname(PLAN_BIN), exist_ok=True)
    tmp = PLAN_BIN + ".%d.tmp" % os.getpid()
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-DSTORMCK_PROBES", PLAN_SRC, "-o", tmp],
                   check=True)
    os.replace(tmp, PLAN_BIN)
    return PLAN_BIN


def library_cases(cu):
    """(n, len, stride) of the library-level test on `cu` CUs: exactly `cu` groups with a lone
    last block, `cu` full groups, and a batch past kBigW that is no multiple of 128; lengths
    512, 1,000 and 4,136 wherever the batch stays at or below 256 MiB."""
    sizes = [128 * (cu - 1) + 1, 128 * cu, max(BIG_W, 128 * cu) + 77]
    cases = [(n, ln, (ln + 15) // 16 * 16) for n in sizes for ln in (512, 1000, 4136)]
    return [c for c in cases if c[0] * c[2] <= 256 << 20]


class Harness:
    def __init__(self, path):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        h = ctypes.CDLL(path)
        p, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        h.streamk_skew.argtypes, h.streamk_skew.restype = [p, u64, u32, u64, p, p, p, u32, p], i
        h.streamk_var.argtypes, h.streamk_var.restype = [p, u64, p, u32, p, p, u64, p, p, p, i, i, u32, p], i
        h.streamk_last_error.argtypes, h.streamk_last_error.restype = [], i
        self.h = h
        self.blocks = {}  # (kernel, form) -> [cases, blocks compared with the oracle]

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def to_dev(self, a):
        view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
        return self.torch.from_numpy(a.view(view) if view else a).to(self.dev)

    def partial_quads(self, reset=1):
        f = self.h.streamk_debug_partial_quads
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
        c = ctypes.c_uint64(0)
        rc = f(ctypes.byref(c), reset)
        assert rc == 0, rc
        return c.value

    def tally(self, key, n):
        t = self.blocks.setdefault(key, [0, 0])
        t[0] += 1
        t[1] += n


def plant_sets(n):
    """1 to 5 planted mismatches: the last block alone; two blocks of one wave; block 0, block
    n - 1, two blocks of one wave and one more."""
    m = (n // 2) // 16 * 16  # m and m + 1 share a wave where both exist
    pair = sorted({m, min(m + 1, n - 1)})
    return [[n - 1], pair, sorted({0, n - 1, *pair, n // 3})]


def _inside(c, nbytes, n=None):
    first, end = c.extents()
    first, end = first[:n], end[:n]
    assert first.min() >= 0 and end.max() + sc.SLACK <= nbytes, (c.name, int(end.max()), nbytes)


def _launch_set(H, launch, n, want, want_out):
    """launch(out_ptr, expected_ptr, result_ptr) -> rc, for the checksum launch and the verify
    launches; then one sync and every comparison. want: the oracle's checksum of block i;
    want_out: what out[0, n) must hold."""
    torch = H.torch
    out = H.to_dev(np.full(n + 2 * PAD, SENTINEL, dtype=np.uint64))
    rcs = [launch(out.data_ptr() + 8 * PAD, None, None)]
    plants = plant_sets(n)
    exps, results = [], []
    for bad in [[]] + plants:
        e = want.copy()
        e[bad] ^= np.uint64(1) << np.uint64(17)
        exps.append(H.to_dev(e))
        results.append(H.to_dev(np.full(2 + PAD, SENTINEL, dtype=np.uint64)))
        rcs.append(launch(None, exps[-1].data_ptr(), results[-1].data_ptr()))
    err = H.h.streamk_last_error()
    torch.cuda.current_stream().synchronize()
    assert rcs == [0] * len(rcs) and err == 0 and H.h.streamk_last_error() == 0, (rcs, err)
    got = out.cpu().numpy().view(np.uint64)
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + n:] == SENTINEL).all(), "a word outside out[0, n) was written"
    got = got[PAD:PAD + n]
    wrong = np.flatnonzero(got != want_out)
    assert wrong.size == 0, "%d of %d checksums differ from the oracle, first at %d (unwritten: %d)" % (
        wrong.size, n, wrong[0], int((got == SENTINEL).sum()))
    for bad, r in zip([[]] + plants, results):
        r = r.cpu().numpy().view(np.uint64)
        assert (r[2:] == SENTINEL).all()
        assert r[:2].tolist() == ([bad[0], len(bad)] if bad else [n, 0]), (bad, r[:2].tolist())


def run_skew(H, c):
    buf = c.buffer()
    assert buf.size == c.nbytes
    _inside(c, buf.size)
    want = o.checksum_batch(buf[c.base_off:], c.n, c.stride, c.len)
    d = H.to_dev(buf)
    assert d.data_ptr() % 512 == 0
    base = d.data_ptr() + c.base_off

    def launch(out, expected, result):
        return H.h.streamk_skew(base, c.stride, c.len, c.n, out, expected, result, c.grid, H.stream())
    _launch_set(H, launch, c.n, want, want)
    H.tally(("skew", "p"), c.n)


class VarRun:
    """A var case on the device: its buffer, arrays and the oracle's checksums, made once."""

    def __init__(self, H, c):
        self.c = c
        buf = c.buffer()
        assert buf.size == c.nbytes
        _inside(c, buf.size)
        if c.offs is None:
            self.want = o.checksum_batch(buf[c.base_off:], c.n, c.stride, 0, lens=c.lens)
        else:
            self.want = o.checksum_gather(buf[c.base_off:], c.offs, c.len, c.lens)
        self.d = H.to_dev(buf)
        assert self.d.data_ptr() % 512 == 0
        self.lens = None if c.lens is None else H.to_dev(c.lens)
        self.offs = None if c.offs is None else H.to_dev(c.offs)
        self.order = None if c.order is None else H.to_dev(c.order)


def run_var(H, run, f):
    c = run.c
    n = f.n or c.n
    base = run.d.data_ptr() + c.base_off
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    want = run.want[:n]

    def call(order, out, expected, result):
        return H.h.streamk_var(base, c.stride, ptr(run.lens), c.len, ptr(run.offs), order, n, out, expected, result,
                               f.waves, int(f.persistent), f.grid, H.stream())
    if c.order is None:
        _launch_set(H, lambda out, e, r: call(None, out, e, r), n, want, want)
    else:
        # the ordered instances do not verify: the checksum launch alone, every slot written
        assert n == c.n
        want_out = np.empty(n, dtype=np.uint64)
        want_out[c.order] = want
        out = H.to_dev(np.full(n + 2 * PAD, SENTINEL, dtype=np.uint64))
        rc = call(run.order.data_ptr(), out.data_ptr() + 8 * PAD, None, None)
        err = H.h.streamk_last_error()
        H.torch.cuda.current_stream().synchronize()
        assert rc == 0 and err == 0 and H.h.streamk_last_error() == 0, (rc, err)
        got = out.cpu().numpy().view(np.uint64)
        assert (got[:PAD] == SENTINEL).all() and (got[PAD + n:] == SENTINEL).all()
        assert np.array_equal(got[PAD:PAD + n], want_out), int((got[PAD:PAD + n] != want_out).sum())
    H.tally(("var", f.tag), n)


def run_all(H):
    for c in sc.SKEW_CASES:
        run_skew(H, c)
    for c in sc.VAR_CASES:
        run = VarRun(H, c)
        for f in c.forms:
            run_var(H, run, f)


if __name__ == "__main__":  # the debug build's child process
    H = Harness(sys.argv[1])
    res = {"lib": sys.argv[1], "before": H.partial_quads()}
    run_all(H)
    res["partial"] = H.partial_quads()
    res["blocks"] = {"%s %s" % k: v for k, v in H.blocks.items()}
    print("RESULT " + json.dumps(res))
