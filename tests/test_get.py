"""Get on the host leg (no device): stormck_get_host gives the results, the rows, the report, the
return code and the message of the pure-Python reference (tests/objects_util.py ``reference_get``:
the singularity's check, ``reference_spaces``, lookup_util's ``reference_lookup`` and
``reference_objects`` chained by hand) on the designed cases, and argument errors are refused
before any work."""
import ctypes
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, keystore as ks, objectstore as obs, spacestore as sps, storm
from storm_amd._lib import GetParamsStruct, GetReportStruct, lib
from tests import lookup_util as lu
from tests import objects_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ou.GET_CASES))
def test_case(name):
    case = ou.GET_CASES[name]()
    records, objects, report = ou.host_get(case)
    ou.check_get(case, records, objects, report)


def test_threads():
    case = ou.get_mixed()
    one, rows1, rep1 = ou.host_get(case, threads=1)
    many, rows, rep = ou.host_get(case)
    assert one.tobytes() == many.tobytes() and rows1.tobytes() == rows.tobytes() and rep1.as_dict() == rep.as_dict()


def test_each_stage_owns_first_bad_once():
    sources = {name: ou.GET_CASES[name]().reference()[3] for name in
               ("damaged spacelist leaf", "damaged key tree", "damaged object tree", "mixed")}
    assert sources == {"damaged spacelist leaf": "space", "damaged key tree": "lookup", "damaged object tree": "objects",
                       "mixed": "lookup"}
    assert ou.GET_CASES["damaged singularity"]().reference()[3].startswith("checksum mismatch for block 0")


def test_get_is_the_three_calls_chained():
    """The one call against spacestore, keystore and objectstore called one after the other."""
    case = ou.get_mixed()
    st = case.store
    records, rows, report = ou.host_get(case)
    s = st.img[:72].tobytes()
    import struct
    spaces, _ = sps.get_spaces_host(st.img, st.lay, struct.unpack_from("<QQ", s, 32) + (1,), s[56], st.SA,
                                    np.array([case.space_id], np.uint64))
    assert spaces[0].tobytes() == report.space.tobytes()
    (key_root, key_type), (object_root, object_type) = sps.roots(spaces[0])
    looked_up, lrep = ks.get_object_ids_host(st.img, st.lay, key_root, key_type, st.params.keys, **lu.pack(case.keys, "flat"))
    assert lrep.as_dict() == report.lookup.as_dict()
    found = looked_up[looked_up["status"] == ks.FOUND]
    ores, orows, orep = obs.get_objects_host(st.img, st.lay, object_root, object_type, st.params.objects, found)
    sel = np.flatnonzero(looked_up["status"] == ks.FOUND)
    assert np.array_equal(records["status"][sel], ores["status"]) and np.array_equal(records["object_address"][sel], ores["address"])
    assert rows[sel, :ou.GET_S].tobytes() == orows.tobytes() and report.n_status == orep.n_status


# ---- arguments -------------------------------------------------------------------------------------

def _call(which="host", **over):
    case = ou.get_count(65)
    st = case.store
    p = lu.pack(case.keys, "flat")
    n = len(case.keys)
    results, objects = np.zeros(n, storm.RESULT_DTYPE), np.zeros((n, 16), np.uint8)  # alive until the call returns
    need = storm.workspace_bytes(n, st.C)
    workspace = np.zeros(need // 8 + 1, np.uint64)
    a = dict(store=st.img.ctypes.data, layout=st.lay, space_id=case.space_id, params=st.params.raw,
             keys=p["keys"].ctypes.data, stride=0, offsets=p["offsets"].ctypes.data, lens=p["lens"].ctypes.data, len=0, n=n,
             flags=0, results=results.ctypes.data, objects=objects.ctypes.data, out_stride=16,
             workspace=workspace.ctypes.data, workspace_bytes=need)
    a.update(over)
    raw = GetReportStruct()
    ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
    head = (a["store"], ref(a["layout"]), a["space_id"], ref(a["params"]), a["keys"], a["stride"], a["offsets"], a["lens"],
            a["len"], a["n"], a["flags"], a["results"], a["objects"], a["out_stride"])
    report = over.get("report", ctypes.byref(raw))
    if which == "host":
        rc = lib.stormck_get_host(*head, report, 0)
    else:
        rc = lib.stormck_get_device(*head, a["workspace"], a["workspace_bytes"], report, None)
    return rc, _lib.last_error()


def _params(st, space=True, keys=None, objects=None):
    table = np.ascontiguousarray(st.SA if space is True else space, np.uint16) if space is not None else None
    p = GetParamsStruct(None if table is None else table.ctypes.data, keys or st.params.keys.raw, objects or st.params.objects.raw)
    p._keep = table
    return p


EINVAL_CASES = {
    "null store": lambda st: dict(store=None),
    "null layout": lambda st: dict(layout=None),
    "null params": lambda st: dict(params=None),
    "null keys": lambda st: dict(keys=None),
    "null results": lambda st: dict(results=None),
    "null report": lambda st: dict(report=None),
    "unknown flag": lambda st: dict(flags=2),
    "too many keys": lambda st: dict(n=2 ** 31 + 1),
    "null space table": lambda st: dict(params=_params(st, space=None)),
    "space table not a permutation": lambda st: dict(params=_params(st, space=[0, 1, 2, 3, 4, 5, 6, 7, 8, 8])),
    "key table not a permutation": lambda st: dict(params=_params(st, keys=ks.ObjectListParams([0, 1, 2, 3, 4, 5, 6, 7, 8, 8]).raw)),
    "objects do not fit": lambda st: dict(params=_params(st, objects=obs.BlobParams(31, 13).raw)),
    "object size 0": lambda st: dict(params=_params(st, objects=obs.BlobParams(10, 0).raw)),
    "out_stride below S": lambda st: dict(out_stride=12),
    "uniform len 257": lambda st: dict(offsets=None, lens=None, stride=300, len=257),
}


@pytest.mark.parametrize("which", ["host", "device"])
@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_einval(name, which):
    rc, msg = _call(which, **EINVAL_CASES[name](ou.get_count(65).store))
    assert rc == _lib.EINVAL and msg


def test_workspace_and_alignment():
    need = storm.workspace_bytes(65, 10)
    rc, msg = _call("device", workspace_bytes=need - 1)
    assert rc == _lib.EINVAL and "workspace" in msg
    assert _call("device", workspace=None)[0] == _lib.EINVAL
    for n, C in ((0, 10), (1, 10), (65, 10), (10 ** 6, 600)):
        m = (n + 7) & ~7
        assert storm.workspace_bytes(n, C) == (max(ks.workspace_bytes(n, C), sps.workspace_bytes(1, 32768)) + 80 * m +
                                               8 * (n // 256 + 2) + 128)
    buf = np.zeros(65 * 4 + 1, np.uint64)
    assert _call("device", results=buf.ctypes.data + 4)[0] == _lib.EINVAL
    assert _call()[0] == _lib.OK and _call(objects=None, out_stride=0)[0] == _lib.OK


def test_n_zero_is_a_noop_with_a_zero_report():
    assert _call(n=0, keys=None, results=None, objects=None, offsets=None, lens=None, len=8)[0] == _lib.OK
    _, _, rep = ou.host_get(ou.get_count(0))
    assert rep.first_bad == 0 and rep.n_selected == 0 and rep.lookup.as_dict()["first_bad"] == 0 and rep.ok


def test_header():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        text = f.read()
    assert re.search(r"^#define STORMCK_HAS_GET 1$", text, re.M) and re.search(r"^#define STORMCK_ABI_VERSION 7$", text, re.M)
    assert ctypes.sizeof(_lib.GetResultStruct) == 32 and ctypes.sizeof(GetReportStruct) == 88 + 192 + 8 + 64 + 16 + 8 + 8 + 8 + 16
    assert ctypes.sizeof(GetParamsStruct) == 8 + 16 + 8
