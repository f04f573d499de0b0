"""The blob probe's rules alone under ASan + UBSan (CPU only): tests/blob_probe_main.cpp is a
stand-alone program that includes storm_amd/csrc/blob_probe.h, the function the device kernel
and the host leg share, and runs the designed probe cases on leaves in heap allocations of
exactly their size, and the designed cases of storm_amd/csrc/space_probe.h (findSpace) on
spacelist leaves and tables of exactly theirs. Given a corpus file it runs that too: every ID of the random leaves of
tests/objects_util.py ``leaf_fuzz_case`` against the answer of the Python probe. No library is
loaded into Python and nothing is preloaded: the program is run as a program.

The corpus: records one after another with no padding, every number little-endian. A record is
a 32-byte head

    u32 N | u32 S | u64 reminder | u64 leaf_len | u32 index | u16 probes | u8 found | u8 zero

(index, probes, found: ``objects_util.find_object``'s answer, index 2^32 - 1 for its nil), then
the leaf (leaf_len bytes)."""
import os
import struct
import subprocess

import pytest

from tests import objects_util as ou
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "blob_probe_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "blob_probe")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out, flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


def _run(out, corpus=None):
    r = subprocess.run([out] + ([corpus[0]] if corpus else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == ("ok %d" % corpus[1] if corpus else "ok"), r.stdout + r.stderr


def corpus_records():
    """One record per ID of every leaf_fuzz_case (the leaves verify: every ID is probed)."""
    for N, S, seed in ou.leaf_fuzz_ids():
        case = ou.leaf_fuzz_case(N, S, seed)
        t = case.tree
        results = ou.reference_of(case)[0]
        for _, address, reminder, index, probes, status in results:
            leaf = t.img[address * t.lay.block_size:address * t.lay.block_size + t.lay.blob_len].tobytes()
            answer = ou.find_object(leaf, N, S, reminder)
            assert (ou.NO_SLOT if answer[0] is None else answer[0], answer[1], answer[2]) == (index, probes, status == ou.FOUND)
            yield struct.pack("<IIQQIHBB", N, S, reminder, len(leaf), index, probes, answer[2], 0) + leaf


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(path, number of records)"""
    path = tmp_path_factory.mktemp("blob_probe") / "corpus.bin"
    n = 0
    with open(path, "wb") as f:
        for record in corpus_records():
            f.write(record)
            n += 1
    assert n == sum(len(ou.leaf_fuzz_case(N, S, seed).ids) for N, S, seed in ou.leaf_fuzz_ids()) >= 5000
    return str(path), n


def test_probe_program_plain(corpus, tmp_path):
    r = _build(OUT, ["-O2"])
    assert r.returncode == 0, r.stderr
    _run(OUT)
    _run(OUT, corpus)
    # the count it prints is of whole records: a cut file is an error, not fewer records
    with open(corpus[0], "rb") as f:
        head = f.read(1000)
    cut = tmp_path / "cut.bin"
    cut.write_bytes(head)
    r = subprocess.run([OUT, str(cut)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not a corpus" in r.stdout


def test_probe_program_under_asan_ubsan(corpus):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    r = _build(OUT + "_asan", SANITIZE)
    assert r.returncode == 0, r.stderr
    _run(OUT + "_asan")
    _run(OUT + "_asan", corpus)
