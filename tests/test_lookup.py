"""Lookup on the host leg (no device): stormck_lookup_host gives the results, the report, the
return code and the message of the pure-Python reference (tests/lookup_util.py) on the designed
cases, and every argument error of both entry points is refused before any work."""
import ctypes
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, keystore as ks
from storm_amd._lib import LookupReportStruct, ObjectListParamsStruct, lib
from storm_amd.scrub import ScrubLayout, _root
from tests import lookup_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(lu.CASES))
def test_case(name):
    case = lu.CASES[name]()
    records, report = lu.host_lookup(case)
    lu.check_against_reference(case, records, report)


def test_threads_and_optional_outputs():
    """One thread and the pool give the same bytes; the trace results and the tags the caller asks
    for are the trace's own."""
    case = lu.volume()
    one, rep1 = lu.host_lookup(case, threads=1)
    many, rep = lu.host_lookup(case, want_trace=True)
    assert one.tobytes() == many.tobytes() and rep1.as_dict() == rep.as_dict()
    from oracle import oracle as o
    assert [int(t) for t in rep.tags[:50]] == [o.xxh64(k) for k in case.keys[:50]]
    assert np.array_equal(rep.trace_results["address"], many["address"])
    assert np.array_equal(rep.trace_results["reminder"], many["reminder"])


def test_key_messages():
    _, rep = lu.host_lookup(lu.addressing("bad lens"))
    assert rep.code == _lib.EMISMATCH
    assert rep.message == "maximum key component length exceeded, maximum: 256, actual: 257"
    _, rep = lu.host_lookup(lu.empty_key_first())
    assert rep.code == _lib.EMISMATCH and rep.message == "key cannot be empty"


def test_probe_reference_on_a_known_leaf():
    """The Python probe itself, on a leaf small enough to check by hand: C = 4, A = 2, 0, 3, 1."""
    A = np.array([2, 0, 3, 1], np.uint16)
    leaf = lu.Leaf(4)
    assert lu.probe(leaf.b, 4, A, b"k", 5) == (0, 3, 1, False, False)   # seed 1: slot (1 + 2) % 4, Free
    assert leaf.insert(A, b"k", 5, 77) == 3
    assert lu.probe(leaf.b, 4, A, b"k", 5) == (77, 3, 1, True, False)
    assert lu.probe(leaf.b, 4, A, b"j", 5) == (0, 1, 2, False, False)   # passes the item, ends at slot 1
    assert leaf.next_pointer(0) == 4 + 1 and leaf.n_used() == 1 and leaf.free_index() == 1
    assert len(leaf.b) == 216 and ks.leaf_len(600) == 31808 and ks.leaf_len(10) == 536


# ---- arguments -------------------------------------------------------------------------------------

def _call(which="host", **over):
    """stormck_lookup_host / _device on the small stored tree with one argument changed; device
    calls are given host pointers: every error here is found before the device is touched."""
    case = lu.count(65)
    t = case.tree
    p = lu.pack(case.keys, "flat")
    n = len(case.keys)
    a = dict(store=t.img.ctypes.data, layout=t.lay, root=_root(t.root[:2] + (2,)), root_type=t.root_type,
             params=t.params.raw, keys=p["keys"].ctypes.data, stride=0, offsets=p["offsets"].ctypes.data,
             lens=p["lens"].ctypes.data, len=0, n=n, flags=0, results=np.zeros(n, ks.RESULT_DTYPE).ctypes.data,
             workspace=np.zeros(ks.workspace_bytes(n, t.C) // 8 + 1, np.uint64).ctypes.data,
             workspace_bytes=ks.workspace_bytes(n, t.C))
    a.update(over)
    raw = LookupReportStruct()
    ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
    head = (a["store"], ref(a["layout"]), ref(a["root"]), a["root_type"], ref(a["params"]), a["keys"], a["stride"],
            a["offsets"], a["lens"], a["len"], a["n"], a["flags"], a["results"], None, None)
    report = over.get("report", ctypes.byref(raw))
    if which == "host":
        rc = lib.stormck_lookup_host(*head, report, 0)
    else:
        rc = lib.stormck_lookup_device(*head, a["workspace"], a["workspace_bytes"], report, None)
    return rc, _lib.last_error()


def _layout(t, **over):
    f = {n: getattr(t.lay, n) for n, _ in t.lay._fields_}
    f.update(over)
    return ScrubLayout(*(f[n] for n, _ in t.lay._fields_))


def _params(table, C):
    table = None if table is None else np.ascontiguousarray(table, np.uint16)
    p = ObjectListParamsStruct(None if table is None else table.ctypes.data, C, 0)
    p._keep = table
    return p


EINVAL_CASES = {
    "null store": lambda t: dict(store=None),
    "null layout": lambda t: dict(layout=None),
    "null root": lambda t: dict(root=None),
    "null params": lambda t: dict(params=None),
    "null keys": lambda t: dict(keys=None),
    "null results": lambda t: dict(results=None),
    "null report": lambda t: dict(report=None),
    "unknown flag": lambda t: dict(flags=2),
    "block size not a multiple of 8": lambda t: dict(layout=_layout(t, block_size=1020)),
    "no blocks": lambda t: dict(layout=_layout(t, n_blocks=0)),
    "fanout 0": lambda t: dict(layout=_layout(t, pointer_fanout=0)),
    "leaf longer than a block": lambda t: dict(layout=_layout(t, objectlist_len=ks.leaf_len(20)),
                                                params=_params(lu.table(20), 20)),
    "too many keys": lambda t: dict(n=2 ** 31 + 1),
    "leaf length of another C": lambda t: dict(layout=_layout(t, objectlist_len=528)),
    "C = 0": lambda t: dict(params=_params(t.A, 0)),
    "C = 4097": lambda t: dict(params=_params(lu.table(4097), 4097), layout=_layout(t, objectlist_len=ks.leaf_len(4097))),
    "null table": lambda t: dict(params=_params(None, 10)),
    "table with a repeat": lambda t: dict(params=_params([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], 10)),
    "table entry = C": lambda t: dict(params=_params([0, 1, 2, 3, 4, 5, 6, 7, 8, 10], 10)),
    "uniform len 0": lambda t: dict(offsets=None, lens=None, stride=16, len=0),
    "uniform len 257": lambda t: dict(offsets=None, lens=None, stride=300, len=257),
}


@pytest.mark.parametrize("which", ["host", "device"])
@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_einval(name, which):
    rc, msg = _call(which, **EINVAL_CASES[name](lu.count(65).tree))
    assert rc == _lib.EINVAL and msg


def test_uniform_len_messages():
    assert _call(offsets=None, lens=None, stride=16, len=0)[1] == "lookup: key cannot be empty"
    assert _call(offsets=None, lens=None, stride=300, len=300)[1].endswith("maximum: 256, actual: 300")


def test_workspace():
    t = lu.count(65).tree
    need = ks.workspace_bytes(65, t.C)
    rc, msg = _call("device", workspace_bytes=need - 1)
    assert rc == _lib.EINVAL and "workspace" in msg
    assert _call("device", workspace=None)[0] == _lib.EINVAL
    from storm_amd import trace
    for n, C in ((0, 10), (1, 10), (65, 10), (10 ** 6, 600), (7, 4096)):
        m = (n + 7) & ~7
        assert ks.workspace_bytes(n, C) == trace.workspace_bytes(n) + 40 * m + ((2 * C + 7) & ~7) + 256


def test_misaligned_pointers():
    t = lu.count(65).tree
    assert _call("device", store=t.img.ctypes.data + 4)[0] == _lib.EINVAL
    buf = np.zeros(65 * 4 + 1, np.uint64)
    assert _call("device", results=buf.ctypes.data + 4)[0] == _lib.EINVAL


def test_n_zero_is_a_noop_with_a_zero_report():
    rc, _ = _call(n=0, keys=None, results=None, offsets=None, lens=None, len=8)
    assert rc == _lib.OK
    case = lu.count(0)
    _, rep = lu.host_lookup(case)
    assert rep.as_dict() == dict(n_status=(0,) * 8, n_probed=0, probes=0, n_malformed=0, first_bad=0,
                                 trace=dict(n_status=(0,) * 7, blocks_hashed=(0, 0), bytes_hashed=0, first_bad=0, levels=0))


def test_header():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        text = f.read()
    assert re.search(r"^#define STORMCK_HAS_LOOKUP 1$", text, re.M)
    assert re.search(r"^#define STORMCK_ABI_VERSION 7$", text, re.M)
    assert re.search(r"^#define STORMCK_LOOKUP_KEY 7\b", text, re.M)
    assert lib.stormck_abi_version() == 7
    assert ctypes.sizeof(_lib.LookupResultStruct) == 32 and ctypes.sizeof(LookupReportStruct) == 96 + 64 + 32


def test_cpp_mirror_looks_keys_up_on_the_host_leg():
    """GetObjectIDs of include/storm_blocks.hpp compiles with -Wall -Wextra and finds a key in a
    leaf it builds itself with ObjectListBlock<10> (tests/cpp/lookup_test.cpp)."""
    import subprocess
    from storm_amd import build as b
    out = os.path.join(ROOT, "tests", "cpp", "build", "lookup_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    libdir = os.path.dirname(b.LIB)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lookup_test.cpp"), "-o", out, "-L", libdir, "-lstormck",
                    f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
