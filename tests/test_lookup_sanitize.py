"""The probe rules alone under ASan + UBSan (CPU only): tests/lookup_probe_main.cpp is a
stand-alone program that includes storm_amd/csrc/objlist_probe.h, the function the device
kernel and the host leg share, and runs the malformed-chain and probe-order cases on leaves,
keys and tables in heap allocations of exactly their size. Given a corpus file it runs that too:
every key of the random leaves of tests/lookup_util.py ``leaf_fuzz_case`` against the answer of
the Python probe.

The corpus: records one after another with no padding, every number little-endian. A record is
a 32-byte head

    u32 C | u32 key_len | u64 reminder | u64 object_id | u32 index | u16 probes | u8 found | u8 malformed

(the last five: ``lookup_util.probe``'s answer), then the table (C u16), the leaf
(``keystore.leaf_len(C)`` bytes) and the key (key_len bytes)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from storm_amd import keystore as ks
from tests import lookup_util as lu
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lookup_probe_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "lookup_probe")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out, flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


def _run(out, corpus=None):
    r = subprocess.run([out] + ([corpus[0]] if corpus else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == ("ok %d" % corpus[1] if corpus else "ok"), r.stdout + r.stderr


def corpus_records():
    """One record per key of every leaf_fuzz_case (the leaves verify: every key is probed)."""
    for C, seed in lu.leaf_fuzz_ids():
        case = lu.leaf_fuzz_case(C, seed)
        t = case.tree
        table = np.ascontiguousarray(t.A, dtype="<u2").tobytes()
        results, _, _ = lu.reference_of(case)
        for key, (object_id, address, reminder, index, probes, status) in zip(case.keys, results):
            leaf = t.img[address * t.lay.block_size:address * t.lay.block_size + ks.leaf_len(C)].tobytes()
            answer = lu.probe(leaf, C, t.A, key, reminder)
            assert answer[:4] == (object_id, index, probes, status == lu.FOUND)  # what the reference took from it
            yield struct.pack("<IIQQIHBB", C, len(key), reminder, *answer) + table + leaf + key


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(path, number of records)"""
    path = tmp_path_factory.mktemp("lookup_probe") / "corpus.bin"
    n = 0
    with open(path, "wb") as f:
        for record in corpus_records():
            f.write(record)
            n += 1
    assert n == sum(len(lu.leaf_fuzz_case(C, seed).keys) for C, seed in lu.leaf_fuzz_ids()) >= 6000
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
