"""The update's planning, without a GPU and without the library (CPU checks).

storm_amd/csrc/update_plan.h computes, from the distinct dirty blocks of an update, their heights,
the order, the new addresses, the room check, the records of the commit engine and the new
singularity, once for both legs. tests/cpp/update_plan_test.cpp includes that header alone and
checks it on hand-made forests (the irregular one, a depth-0 tree, a wide one, every error). It is
a stand-alone program with its own main: it runs as built and under ASan + UBSan. Nothing is
loaded into Python and nothing is preloaded."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "update_plan_test.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "update_plan_test")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out, flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


def _run(out):
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_planner_program_plain():
    r = _build(OUT, ["-O2"])
    assert r.returncode == 0, r.stderr
    _run(OUT)


def test_planner_program_under_asan_ubsan():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    r = _build(OUT + "_asan", SANITIZE)
    assert r.returncode == 0, r.stderr
    _run(OUT + "_asan")
