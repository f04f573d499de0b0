"""The probe rules alone under ASan + UBSan (CPU only): tests/lookup_probe_main.cpp is a
stand-alone program that includes storm_amd/csrc/objlist_probe.h, the function the device
kernel and the host leg share, and runs the malformed-chain and probe-order cases on leaves,
keys and tables in heap allocations of exactly their size."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lookup_probe_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "lookup_probe")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out, flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


def _run(out):
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_probe_program_plain():
    r = _build(OUT, ["-O2"])
    assert r.returncode == 0, r.stderr
    _run(OUT)


def test_probe_program_under_asan_ubsan():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    r = _build(OUT + "_asan", SANITIZE)
    assert r.returncode == 0, r.stderr
    _run(OUT + "_asan")
