"""The commit's forest planning, without a GPU and without the library (CPU checks).

storm_amd/csrc/commit_plan.h validates a dirty forest and computes its heights, the shape the
router prices, the commit order, the relocation in that order and the level-0 chunk schedule,
once for the device, host and split legs; stormck.hip plans, then runs the plan.
tests/cpp/commit_plan_test.cpp includes that header alone and compares the planner, on a
serial executor and on 1, 2, 5 and 16 threads, with a reference model written in the test
(children first, upper-shuffled, shuffled and ragged forests, chains, several roots,
zero-length records, all / none / a third relocating), checks every error and the error
precedence, and the chunk schedule against a hand-written table. It runs as built, under
ASan + UBSan and under TSan (there with a largest forest of 20,000 blocks, not 300,000)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "commit_plan_test.cpp")
HEADER = os.path.join(ROOT, "storm_amd", "csrc", "commit_plan.h")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "commit_plan_test")

BUILDS = {
    "plain": (["-O2"], []),
    "asan-ubsan": (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []),
    "tsan": (["-O1", "-g", "-fsanitize=thread"], ["20000"]),
}


def build(kind):
    out = OUT + ("" if kind == "plain" else "_" + kind.split("-")[0])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *BUILDS[kind][0], SRC, "-o", out],
                   check=True)
    return out


@pytest.mark.parametrize("kind", list(BUILDS))
def test_commit_planner_matches_the_model(kind):
    r = subprocess.run([build(kind), *BUILDS[kind][1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    for word in ("runtime error:", "AddressSanitizer", "ThreadSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]


def test_commit_plan_header_is_plain_host_code():
    """The planner stays code a plain compiler builds and a test can run on any executor:
    no HIP, no thread pool of the library's, no error state."""
    text = open(HEADER).read()
    for word in ("#include <hip", "hipLaunchKernelGGL", "__global__", "ForkJoin", "fail(", "std::function"):
        assert word not in text, word
