"""The routing model, without a GPU and without the library (CPU checks).

storm_amd/csrc/route_plan.h holds the cost model of host-memory work (the constants, the
predicted times of the host, device and split legs of a batch and of a commit, the margins
that pick a leg), the host-only bound, the busy-pool rule, the decision of a routed call
(route_batch, route_commit: what the call and its stormck_route_plan_* entry point both ask),
the queue a split's host threads and devices share, and the rates the calls learn.
tests/cpp/route_plan_test.cpp includes that header alone and holds it against a model
written out in the test: times to 1e-9 relative over pinned and pageable memory, 1 to 16
threads, 0 to 8 devices, sizes either side of 64 MiB and three pool / CPU pairs; the margins
just inside and outside; totals one byte either side of the host-only bound; the split
queue's claims by hand and from 8 host and 3 device threads at once; every branch of the
learners. It runs as built, under ASan + UBSan and under TSan."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "route_plan_test.cpp")
HEADER = os.path.join(ROOT, "storm_amd", "csrc", "route_plan.h")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "route_plan_test")

BUILDS = {
    "plain": ["-O2"],
    "asan-ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
}


def build(kind):
    out = OUT + ("" if kind == "plain" else "_" + kind.split("-")[0])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *BUILDS[kind], SRC, "-o", out],
                   check=True)
    return out


@pytest.mark.parametrize("kind", list(BUILDS))
def test_route_plan_matches_the_model(kind):
    r = subprocess.run([build(kind)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    for word in ("runtime error:", "AddressSanitizer", "ThreadSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]


def test_route_plan_header_is_plain_host_code():
    """The model stays code a plain compiler builds and a test can own an instance of: no
    HIP, no thread pool of the library's, no error state."""
    text = open(HEADER).read()
    for word in ("#include <hip", "hipLaunchKernelGGL", "__global__", "ForkJoin", "fail(", "std::function"):
        assert word not in text, word
