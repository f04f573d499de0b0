"""Spaces on the host leg (no device): stormck_spaces_host gives the results, the report, the
return code and the message of the pure-Python reference (tests/objects_util.py ``find_space``,
``reference_spaces``) on the designed cases, and every argument error of both entry points is
refused before any work."""
import ctypes
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, spacestore as sps, trace
from storm_amd._lib import SpacesReportStruct, lib
from storm_amd.scrub import ScrubLayout, _root
from tests import objects_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ou.SPACE_CASES))
def test_case(name):
    case = ou.SPACE_CASES[name]()
    records, report = ou.host_spaces(case)
    ou.check_spaces(case, records, report)


def test_roots_feed_the_other_stores():
    case = ou.space_states()
    records, _ = ou.host_spaces(case)
    (key_root, key_type), (object_root, object_type) = sps.roots(records[0])
    assert key_root == ou.KEY_NODE[:3] and key_type == ou.KEY_NODE[3]
    assert object_root == ou.OBJ_NODE[:3] and object_type == ou.OBJ_NODE[3]
    with pytest.raises(ValueError):
        sps.roots(records[1])


def test_find_space_reference_on_a_known_leaf():
    """The Python probe itself, by hand: S = 4, A = 2, 0, 3, 1."""
    A = np.array([2, 0, 3, 1], np.uint16)
    leaf = ou.SpaceList(4)
    assert len(leaf.b) == 296
    assert ou.find_space(leaf.b, 4, A, 5) == (3, 1, False)    # seed 1: slot (1 + 2) % 4, Free
    leaf.plant(3, 5)
    assert ou.find_space(leaf.b, 4, A, 5) == (3, 1, True)
    assert ou.find_space(leaf.b, 4, A, 9) == (1, 2, False)    # passes the space, ends at slot 1
    leaf.plant(3, 5, state=ou.INVALID)
    assert ou.find_space(leaf.b, 4, A, 5) == (3, 2, False)    # the Invalid slot is handed out at the Free one
    for k in (0, 1, 2):
        leaf.plant(k, 100 + k)
    assert ou.find_space(leaf.b, 4, A, 5) == (None, 4, False)


# ---- arguments -------------------------------------------------------------------------------------

def _call(which="host", **over):
    case = ou.space_count(65)
    n = len(case.ids)
    ids, results = np.array(case.ids, np.uint64), np.zeros(n, sps.RESULT_DTYPE)  # alive until the call returns
    table = over.pop("table", case.A)
    table = None if table is None else np.ascontiguousarray(table, np.uint16)
    workspace = np.zeros(sps.workspace_bytes(n, 10) // 8 + 1, np.uint64)
    a = dict(store=case.img.ctypes.data, layout=case.lay, root=_root(case.root[:2] + (2,)), root_type=case.root_type,
             table=None if table is None else table.ctypes.data, ids=ids.ctypes.data, n=n, flags=0,
             results=results.ctypes.data, workspace=workspace.ctypes.data, workspace_bytes=sps.workspace_bytes(n, 10))
    a.update(over)
    raw = SpacesReportStruct()
    ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
    head = (a["store"], ref(a["layout"]), ref(a["root"]), a["root_type"], a["table"], a["ids"], a["n"], a["flags"],
            a["results"])
    report = over.get("report", ctypes.byref(raw))
    if which == "host":
        rc = lib.stormck_spaces_host(*head, report, 0)
    else:
        rc = lib.stormck_spaces_device(*head, a["workspace"], a["workspace_bytes"], report, None)
    return rc, _lib.last_error()


def _layout(lay, **over):
    f = {n: getattr(lay, n) for n, _ in lay._fields_}
    f.update(over)
    return ScrubLayout(*(f[n] for n, _ in lay._fields_))


EINVAL_CASES = {
    "null store": lambda lay: dict(store=None),
    "null layout": lambda lay: dict(layout=None),
    "null root": lambda lay: dict(root=None),
    "null ids": lambda lay: dict(ids=None),
    "null results": lambda lay: dict(results=None),
    "null report": lambda lay: dict(report=None),
    "null table": lambda lay: dict(table=None),
    "unknown flag": lambda lay: dict(flags=2),
    "no blocks": lambda lay: dict(layout=_layout(lay, n_blocks=0)),
    "fanout 0": lambda lay: dict(layout=_layout(lay, pointer_fanout=0)),
    "no spaces": lambda lay: dict(layout=_layout(lay, spaces_per_block=0)),
    "leaf longer than a block": lambda lay: dict(layout=_layout(lay, spaces_per_block=15), table=ou.space_table(15)),
    "too many IDs": lambda lay: dict(n=2 ** 31 + 1),
    "table with a repeat": lambda lay: dict(table=[0, 1, 2, 3, 4, 5, 6, 7, 8, 8]),
    "table entry = S": lambda lay: dict(table=[0, 1, 2, 3, 4, 5, 6, 7, 8, 10]),
}


@pytest.mark.parametrize("which", ["host", "device"])
@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_einval(name, which):
    rc, msg = _call(which, **EINVAL_CASES[name](ou.space_count(65).lay))
    assert rc == _lib.EINVAL and msg


def test_the_table_must_be_a_permutation():
    assert "permutation" in _call(table=[0, 1, 2, 3, 4, 5, 6, 7, 8, 8])[1]
    assert _call()[0] in (_lib.OK, _lib.EMISMATCH)


def test_workspace_and_alignment():
    need = sps.workspace_bytes(65, 10)
    rc, msg = _call("device", workspace_bytes=need - 1)
    assert rc == _lib.EINVAL and "workspace" in msg
    assert _call("device", workspace=None)[0] == _lib.EINVAL
    for n, S in ((0, 10), (1, 10), (65, 400), (10 ** 6, 32768)):
        assert sps.workspace_bytes(n, S) == trace.workspace_bytes(n) + 32 * ((n + 7) & ~7) + ((2 * S + 7) & ~7) + 256
    buf = np.zeros(65 * 11 + 1, np.uint64)
    assert _call("device", results=buf.ctypes.data + 4)[0] == _lib.EINVAL
    assert _call("device", ids=buf.ctypes.data + 4)[0] == _lib.EINVAL


def test_n_zero_is_a_noop_with_a_zero_report():
    assert _call(n=0, ids=None, results=None)[0] == _lib.OK
    _, rep = ou.host_spaces(ou.space_count(0))
    assert rep.as_dict() == dict(n_status=(0,) * 8, n_probed=0, probes=0, first_bad=0,
                                 trace=dict(n_status=(0,) * 7, blocks_hashed=(0, 0), bytes_hashed=0, first_bad=0, levels=0))


def test_header():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        text = f.read()
    assert re.search(r"^#define STORMCK_HAS_SPACES 1$", text, re.M)
    assert re.search(r"^#define STORMCK_ABI_VERSION 7$", text, re.M)
    assert ctypes.sizeof(_lib.SpaceResultStruct) == 88 and ctypes.sizeof(SpacesReportStruct) == 96 + 64 + 24
