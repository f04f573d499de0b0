"""Objects on the host leg (no device): stormck_objects_host gives the results, the rows, the
report, the return code and the message of the pure-Python reference (tests/objects_util.py) on
the designed cases, and every argument error of both entry points is refused before any work."""
import ctypes
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, objectstore as obs, trace
from storm_amd._lib import BlobParamsStruct, ObjectsReportStruct, lib
from storm_amd.scrub import ScrubLayout, _root
from tests import objects_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ou.CASES))
def test_case(name):
    case = ou.CASES[name]()
    records, objects, report = ou.host_objects(case)
    ou.check_against_reference(case, records, objects, report)


def test_threads():
    """One thread and the pool give the same bytes."""
    case = ou.volume()
    one, rows1, rep1 = ou.host_objects(case, threads=1)
    many, rows, rep = ou.host_objects(case)
    assert one.tobytes() == many.tobytes() and rows1.tobytes() == rows.tobytes() and rep1.as_dict() == rep.as_dict()


def test_message_is_the_traces():
    _, _, rep = ou.host_objects(ou.flipped_leaf())
    assert rep.code == _lib.EMISMATCH and rep.message == ou.host_trace_message(ou.flipped_leaf()) and "checksum" in rep.message
    _, _, rep = ou.host_objects(ou.too_deep())
    assert rep.code == _lib.EMISMATCH and rep.message.startswith("more than 64 pointer blocks")


def test_ids_of_a_lookup_are_read_in_place():
    """Object IDs straight out of keystore.get_object_ids_host's results, at stride 32."""
    from storm_amd import keystore as ks
    from tests import lookup_util as lu
    lcase = lu.count(65)
    looked_up, _ = lu.host_lookup(lcase)
    assert looked_up.dtype == ks.RESULT_DTYPE and looked_up["object_id"].any()
    c = ou.count(1)
    records, _, _ = obs.get_objects_host(c.tree.img, *c.tree.args(), looked_up)
    assert np.array_equal(records["object_id"], looked_up["object_id"])
    dense, _, _ = obs.get_objects_host(c.tree.img, *c.tree.args(), looked_up["object_id"].copy())
    assert dense.tobytes() == records.tobytes()


def test_find_object_reference_on_a_known_leaf():
    """The Python probe itself, on a leaf small enough to check by hand: N = 4, S = 3."""
    leaf = ou.Blob(4, 3, 72)
    assert ou.stride_of(3) == 16 and ou.stride_of(8) == 24 and ou.stride_of(7) == 16 and ou.stride_of(1024) == 1040
    assert ou.find_object(leaf.b, 4, 3, 6) == (2, 1, False)           # start 6 % 4, Free
    assert leaf.set(6, b"abc") == 2 and leaf.n_used() == 1
    assert ou.find_object(leaf.b, 4, 3, 6) == (2, 1, True)
    assert ou.find_object(leaf.b, 4, 3, 10) == (3, 2, False)          # passes the object, ends at slot 3
    assert leaf.set(10, b"def") == 3 and leaf.set(14, b"ghi") == 0    # ... and wraps
    assert bytes(leaf.b[2 * 16:2 * 16 + 12]) == b"\x06" + bytes(7) + b"abc\x01"
    leaf.state(2, ou.INVALID)
    assert ou.find_object(leaf.b, 4, 3, 6) == (2, 4, False)           # Invalid remembered, Free at slot 1
    leaf.state(1, 7)
    assert ou.find_object(leaf.b, 4, 3, 6) == (None, 4, False)        # no Free slot: nil, whatever was Invalid


# ---- arguments -------------------------------------------------------------------------------------

def _call(which="host", **over):
    """stormck_objects_host / _device on the small stored tree with one argument changed; device
    calls are given host pointers: every error here is found before the device is touched."""
    case = ou.count(65)
    t = case.tree
    n = len(case.ids)
    ids = ou.ids_array(case)  # the arrays live until the call has returned: the calls that pass write into them
    results, objects = np.zeros(n, obs.RESULT_DTYPE), np.zeros((n, 16), np.uint8)
    workspace = np.zeros(obs.workspace_bytes(n) // 8 + 1, np.uint64)
    a = dict(store=t.img.ctypes.data, layout=t.lay, root=_root(t.root[:2] + (2,)), root_type=t.root_type,
             params=t.params.raw, ids=ids.ctypes.data, id_stride=8, n=n, flags=0, results=results.ctypes.data,
             objects=objects.ctypes.data, out_stride=16, workspace=workspace.ctypes.data,
             workspace_bytes=obs.workspace_bytes(n))
    a.update(over)
    raw = ObjectsReportStruct()
    ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
    head = (a["store"], ref(a["layout"]), ref(a["root"]), a["root_type"], ref(a["params"]), a["ids"], a["id_stride"],
            a["n"], a["flags"], a["results"], a["objects"], a["out_stride"])
    report = over.get("report", ctypes.byref(raw))
    if which == "host":
        rc = lib.stormck_objects_host(*head, report, 0)
    else:
        rc = lib.stormck_objects_device(*head, a["workspace"], a["workspace_bytes"], report, None)
    return rc, _lib.last_error()


def _layout(t, **over):
    f = {n: getattr(t.lay, n) for n, _ in t.lay._fields_}
    f.update(over)
    return ScrubLayout(*(f[n] for n, _ in t.lay._fields_))


EINVAL_CASES = {
    "null store": lambda t: dict(store=None),
    "null layout": lambda t: dict(layout=None),
    "null root": lambda t: dict(root=None),
    "null params": lambda t: dict(params=None),
    "null ids": lambda t: dict(ids=None),
    "null results": lambda t: dict(results=None),
    "null report": lambda t: dict(report=None),
    "unknown flag": lambda t: dict(flags=2),
    "block size not a multiple of 8": lambda t: dict(layout=_layout(t, block_size=1020)),
    "no blocks": lambda t: dict(layout=_layout(t, n_blocks=0)),
    "fanout 0": lambda t: dict(layout=_layout(t, pointer_fanout=0)),
    "leaf longer than a block": lambda t: dict(layout=_layout(t, blob_len=1032)),
    "too many IDs": lambda t: dict(n=2 ** 31 + 1),
    "N = 0": lambda t: dict(params=BlobParamsStruct(0, 13)),
    "N = 4096": lambda t: dict(params=BlobParamsStruct(4096, 1), layout=_layout(t, block_size=2 ** 17, blob_len=2 ** 17)),
    "S = 0": lambda t: dict(params=BlobParamsStruct(10, 0)),
    "one slot too many": lambda t: dict(params=BlobParamsStruct(31, 13)),       # 31 * 24 = 744 > 720
    "one byte too many": lambda t: dict(params=BlobParamsStruct(30, 16)),       # 30 * 32 > 720
    "blob_len one word short": lambda t: dict(params=BlobParamsStruct(30, 13), layout=_layout(t, blob_len=720)),
    "blob_len below 8": lambda t: dict(layout=_layout(t, blob_len=0)),
    "S = 2^32 - 1": lambda t: dict(params=BlobParamsStruct(1, 2 ** 32 - 1)),
    "out_stride below S": lambda t: dict(out_stride=12),
    "id_stride 0": lambda t: dict(id_stride=0),
    "id_stride 4": lambda t: dict(id_stride=4),
    "id_stride 12": lambda t: dict(id_stride=12),
}


@pytest.mark.parametrize("which", ["host", "device"])
@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_einval(name, which):
    rc, msg = _call(which, **EINVAL_CASES[name](ou.count(65).tree))
    assert rc == _lib.EINVAL and msg


def test_the_largest_arguments_that_pass():
    """N * stride == blob_len - 8 exactly, N = 4095, out_stride == S, and out_stride below S when
    there are no rows: none is an error."""
    t = ou.count(65).tree
    assert _call(params=BlobParamsStruct(30, 13))[0] == _lib.OK                          # 30 * 24 == 720
    assert _call(params=BlobParamsStruct(4095, 1), n=0,
                 layout=_layout(t, block_size=2 ** 16, blob_len=4095 * 16 + 8))[0] == _lib.OK
    assert _call(out_stride=13)[0] == _lib.OK
    assert _call(objects=None, out_stride=0)[0] == _lib.OK


def test_workspace():
    need = obs.workspace_bytes(65)
    rc, msg = _call("device", workspace_bytes=need - 1)
    assert rc == _lib.EINVAL and "workspace" in msg
    assert _call("device", workspace=None)[0] == _lib.EINVAL
    for n in (0, 1, 65, 10 ** 6):
        assert obs.workspace_bytes(n) == trace.workspace_bytes(n) + 32 * ((n + 7) & ~7) + 256


def test_misaligned_pointers():
    t = ou.count(65).tree
    assert _call("device", store=t.img.ctypes.data + 4)[0] == _lib.EINVAL
    buf = np.zeros(65 * 4 + 1, np.uint64)
    assert _call("device", results=buf.ctypes.data + 4)[0] == _lib.EINVAL
    assert _call("device", ids=buf.ctypes.data + 4)[0] == _lib.EINVAL


def test_n_zero_is_a_noop_with_a_zero_report():
    rc, _ = _call(n=0, ids=None, results=None, objects=None)
    assert rc == _lib.OK
    _, _, rep = ou.host_objects(ou.count(0))
    assert rep.as_dict() == dict(n_status=(0,) * 8, n_probed=0, probes=0, first_bad=0,
                                 trace=dict(n_status=(0,) * 7, blocks_hashed=(0, 0), bytes_hashed=0, first_bad=0, levels=0))


def test_header():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        text = f.read()
    assert re.search(r"^#define STORMCK_HAS_OBJECTS 1$", text, re.M)
    assert re.search(r"^#define STORMCK_ABI_VERSION 7$", text, re.M)
    assert lib.stormck_abi_version() == 7
    assert ctypes.sizeof(_lib.ObjectResultStruct) == 32 and ctypes.sizeof(ObjectsReportStruct) == 96 + 64 + 24
    assert ctypes.sizeof(BlobParamsStruct) == 8
