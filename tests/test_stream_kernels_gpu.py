"""The two persistent streaming kernels at small shapes, by direct launch.

k_xxh64_glds_skew (the kernel behind the headline number) and the persistent form of
k_xxh64_glds_var are reached by the shipped dispatch only from batches of tens of GB
(plan_checksum, storm_amd/csrc/dispatch.h), so the library-level tests see them at two or
three shapes. tests/hip/libstreamkernels.so launches the same source's kernels, in the
template instances launch_checksum ships, on grids of 1 to 7 workgroups; the designed cases
of tests/stream_cases.py (whose coverage tests/test_stream_cases.py checks on the CPU) then
put blocks of 1 to 130 tiles, streams shorter than the start-up ramp, unequal and idle
workgroups, empty groups, unstaged blocks and dead waves within a few MiB. These are
separately compiled instances of the same source, not the kernels inside libstormck.so.

* every case and form: checksums, untouched sentinels around `out`, verify with the oracle's
  checksums and with planted mismatches (tests/stream_run.py), against the C oracle;
* every case again through the -DSTORMCK_DEBUG_QUAD build in a child process: no quad merge
  with a partially active quad (tests/test_quad_debug.py proves that such a counter counts);
* the arguments the kernels do not support are refused without a launch;
* the shipped launch code of k_xxh64_glds_skew (grid = CU count, argument order) through the
  probe build with STORMCK_SKEW_MIN_STEPS=1, the plan shown by tests/cpp/plan_query.cpp. This
  covers the shipped launch code only through the probe build's threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stream_cases as sc
from tests import stream_run as sr
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from storm_amd import build as sb
    assert os.path.exists(sb.STREAM_KERNELS), "tests/hip/libstreamkernels.so missing: storm_amd.build.build_stream_kernels()"
    return sr.Harness(sb.STREAM_KERNELS)


@pytest.mark.parametrize("c", sc.SKEW_CASES, ids=lambda c: c.name)
def test_skew_kernel(H, c):
    sr.run_skew(H, c)


_var_runs = {}


@pytest.mark.parametrize("c,f", [(c, f) for c in sc.VAR_CASES for f in c.forms],
                         ids=lambda v: v.name if isinstance(v, sc.VarCase) else
                         "%s-g%d-n%d" % (v.tag, v.grid, v.n))
def test_var_kernel(H, c, f):
    if c.name not in _var_runs:  # the buffer and the oracle's checksums once per case
        _var_runs.clear()
        _var_runs[c.name] = sr.VarRun(H, c)
    sr.run_var(H, _var_runs[c.name], f)


def test_unsupported_arguments_are_refused(H):
    """A negative return and no launch: nothing is written, no error is left behind."""
    h = H.h
    buf = H.to_dev(np.zeros(1 << 16, dtype=np.uint8))
    out = H.to_dev(np.full(256, sr.SENTINEL, dtype=np.uint64))
    res = H.to_dev(np.full(2, sr.SENTINEL, dtype=np.uint64))
    lens = H.to_dev(np.full(64, 100, dtype=np.uint32))
    offs = H.to_dev(np.arange(64, dtype=np.uint64) * np.uint64(512))
    order = H.to_dev(np.arange(64, dtype=np.uint32))
    b, o_, r_, l_, f_, d_ = (t.data_ptr() for t in (buf, out, res, lens, offs, order))
    st = H.stream()
    skew = [  # base, stride, len, n, out, expected, result, grid
        (b, 512, 512, 0, o_, None, None, 1), (b, 512, 512, 64, o_, None, None, 0), (b, 512, 512, 64, None, None, None, 1),
        (b, 512, 511, 64, o_, None, None, 1), (b, 512, 1024, 64, o_, None, None, 1), (b + 8, 512, 512, 64, o_, None, None, 1),
        (b, 520, 512, 64, o_, None, None, 1), (b, 512, 512, 64, None, o_, None, 1),
    ]
    for a in skew:
        assert h.streamk_skew(*a, st) < 0, a
    var = [  # base, stride, lens, len, offs, order, n, out, expected, result, waves, persistent, grid
        (b, 512, l_, 0, None, None, 0, o_, None, None, 8, 1, 1), (b, 512, l_, 0, None, None, 64, o_, None, None, 8, 1, 0),
        (b, 512, l_, 0, None, None, 64, None, None, None, 8, 1, 1), (b, 512, None, 100, None, None, 64, o_, None, None, 8, 1, 1),
        (b, 512, l_, 0, None, None, 64, o_, None, None, 2, 0, 1), (b, 512, l_, 0, None, None, 64, o_, None, None, 4, 0, 1),
        (b, 512, l_, 0, None, None, 64, o_, None, None, 3, 1, 1), (b, 512, l_, 0, None, None, 64, o_, None, None, 1, 1, 1),
        (b, 512, l_, 0, None, d_, 64, o_, None, None, 8, 1, 1), (b, 0, l_, 0, f_, d_, 64, None, o_, r_, 8, 1, 1),
        (b, 0, l_, 0, f_, d_, 64, o_, None, None, 3, 0, 1),
        (b + 8, 512, l_, 0, None, None, 64, o_, None, None, 8, 1, 1), (b, 520, l_, 0, None, None, 64, o_, None, None, 8, 1, 1),
        (b, 512, l_, 0, None, None, 64, None, o_, None, 8, 1, 1),
    ]
    for a in var:
        assert h.streamk_var(*a, st) < 0, a
    # the same shapes, supported: accepted (and correct: zeros hash alike)
    assert h.streamk_skew(b, 512, 512, 64, o_, None, None, 1, st) == 0
    assert h.streamk_var(b + 8, 0, l_, 0, f_, None, 64, o_ + 8 * 64, None, None, 3, 0, 1, st) == 0
    torch.cuda.current_stream().synchronize()
    assert h.streamk_last_error() == 0
    got = out.cpu().numpy().view(np.uint64)
    assert (got[128:] == sr.SENTINEL).all() and (res.cpu().numpy().view(np.uint64) == sr.SENTINEL).all()
    from oracle import oracle as o
    assert (got[:64] == o.xxh64(np.zeros(512, dtype=np.uint8))).all()
    assert (got[64:128] == o.xxh64(np.zeros(100, dtype=np.uint8))).all()


@pytest.mark.timeout(280)
def test_every_case_merges_full_quads():
    """Every case and form again through the -DSTORMCK_DEBUG_QUAD build of the harness, in a
    child process: oracle-equal results (the child asserts them) and no quad merge with part
    of its quad inactive. Both persistent kernels merge under per-wave conditions."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from storm_amd import build as sb
    assert os.path.exists(sb.STREAM_KERNELS_DEBUG), "tests/hip/libstreamkernels_debug.so missing"
    p = subprocess.run([sys.executable, "-m", "tests.stream_run", sb.STREAM_KERNELS_DEBUG], cwd=ROOT, capture_output=True,
                       text=True, timeout=250)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:]
    r = json.loads(line[0][len("RESULT "):])
    print(r)
    assert r["lib"].endswith("libstreamkernels_debug.so"), r
    assert r["partial"] == 0 and r["before"] == 0, r
    forms = {"skew p", "var p", "var w1", "var w3", "var w8"}
    assert set(r["blocks"]) == forms and all(v[1] > 0 for v in r["blocks"].values()), r


# ---- the shipped launch code, through the probe build's threshold ------------------------
LIB_CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from oracle import oracle as o
from storm_amd import _lib, engine
cases = json.loads(sys.argv[2])
dev = torch.device("cuda", 0)
engine.init(0)
res = {"lib": _lib.LIB_PATH, "cu": engine._cu_count(), "bad": [], "blocks": 0}
nbytes = max(n * stride for n, ln, stride in cases)
host = np.random.default_rng(77).integers(0, 256, size=nbytes, dtype=np.uint8)
d = torch.from_numpy(host).to(dev)
res["base_low4"] = d.data_ptr() % 16
for n, ln, stride in cases:
    want = o.checksum_batch(host, n, stride, ln, threads=8)
    out = torch.from_numpy(np.full(n + 64, 0xA5A5A5A55A5A5A5A, dtype=np.uint64).view(np.int64)).to(dev)
    engine.checksum_device(d.data_ptr(), stride, n, out.data_ptr(), ln)
    got = out.cpu().numpy().view(np.uint64)
    if not np.array_equal(got[:n], want) or not (got[n:] == 0xA5A5A5A55A5A5A5A).all():
        res["bad"].append(["checksum", n, ln, int((got[:n] != want).sum())])
    for plant in ([], [n - 1], [0, n // 2, n // 2 + 1, n - 1]):
        e = want.copy()
        e[plant] ^= np.uint64(1 << 40)
        exp = torch.from_numpy(e.view(np.int64)).to(dev)
        r = torch.zeros(2, dtype=torch.int64, device=dev)
        engine.verify_device(d.data_ptr(), stride, n, exp.data_ptr(), r.data_ptr(), ln)
        if r.cpu().tolist() != ([plant[0], len(plant)] if plant else [n, 0]):
            res["bad"].append(["verify", n, ln, plant, r.cpu().tolist()])
    res["blocks"] += n
print("RESULT " + json.dumps(res))
"""


@pytest.mark.timeout(280)
def test_library_launches_the_skew_kernel_on_every_cu():
    """stormck_checksum_device / stormck_verify_device of the probe build with
    STORMCK_SKEW_MIN_STEPS=1: launch_checksum's own launch of k_xxh64_glds_skew (one
    workgroup per CU, its argument order) at batches of a few tiles per block. The plan is
    asked of dispatch.h under the child's environment, not assumed."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from storm_amd import build as sb, engine
    assert os.path.exists(sb.PROBES_LIB), "probe build missing: storm_amd.build.build_probes_lib()"
    env = dict(os.environ, STORMCK_LIBRARY=sb.PROBES_LIB, STORMCK_SKEW_MIN_STEPS="1")
    cu = engine._cu_count()
    cases = sr.library_cases(cu)
    assert {c[1] for c in cases} == {512, 1000, 4136} and len({c[0] for c in cases}) == 3
    query = sr.build_plan_query()
    for n, ln, stride in cases:
        for verify in (0, 1):
            q = subprocess.run([query, str(n), str(ln), str(stride), "0", str(cu), str(verify)], env=env,
                               capture_output=True, text=True, timeout=60)
            assert q.returncode == 0 and q.stdout.split() == ["glds-skew", str(cu), "512"], (n, ln, q.stdout, q.stderr)
    p = subprocess.run([sys.executable, "-c", LIB_CHILD, ROOT, json.dumps(cases)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=250)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = [ln_ for ln_ in p.stdout.splitlines() if ln_.startswith("RESULT ")]
    assert line, p.stdout[-2000:]
    r = json.loads(line[0][len("RESULT "):])
    print(r)
    assert r["lib"].endswith("libstormck_probes.so") and r["cu"] == cu and r["base_low4"] == 0, r
    assert r["bad"] == [] and r["blocks"] == sum(c[0] for c in cases), r
