"""The device dispatch's decisions, without a GPU (CPU checks).

storm_amd/csrc/dispatch.h decides which kernel runs, in which workgroup shape and on which
grid; stormck.hip only launches the plan. tests/cpp/dispatch_plan_test.cpp includes that
header alone and compares the planners with a hand-written table for 256 CUs and the shipped
knobs (the thresholds between two kernels, the busiest-CU ties, an unknown CU count). It
links no library; it runs once as built and once under ASan + UBSan."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "dispatch_plan_test.cpp")
HEADER = os.path.join(ROOT, "storm_amd", "csrc", "dispatch.h")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "dispatch_plan_test")


def build(sanitize):
    out = OUT + ("_asan" if sanitize else "")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out], check=True)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_dispatch_plans_match_the_table(sanitize):
    r = subprocess.run([build(sanitize)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok: 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error:" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_dispatch_header_has_no_hip():
    """The planners stay host code a plain compiler builds: no HIP include, no launch."""
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipLaunchKernelGGL" not in text and "__global__" not in text
