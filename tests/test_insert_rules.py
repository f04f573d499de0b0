"""The insert's rules, without a GPU and without the library (CPU checks).

storm_amd/csrc/objlist_insert.h and blob_insert.h hold rule B's steps and rule D's slot step of
include/stormck.h "insert", once for the kernels and the host leg; update_plan.h places the two
origins of a spacelist leaf. tests/cpp/insert_rules_test.cpp includes the three headers alone and
runs the designed leaf cases on heap leaves of exactly their size. It is a stand-alone program
with its own main: it runs as built and under ASan + UBSan. Nothing is loaded into Python and
nothing is preloaded."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "insert_rules_test.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "insert_rules_test")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out, flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


def _run(out):
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_rules_program_plain():
    r = _build(OUT, ["-O2"])
    assert r.returncode == 0, r.stderr
    _run(OUT)


def test_rules_program_under_asan_ubsan():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    r = _build(OUT + "_asan", SANITIZE)
    assert r.returncode == 0, r.stderr
    _run(OUT + "_asan")
