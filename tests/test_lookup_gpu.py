"""Lookup on the device (MI355X): stormck_lookup_device gives the result bytes, the report, the
return code and the message of the host leg and of the pure-Python reference
(tests/lookup_util.py) on the designed cases of tests/test_lookup.py. Every image is uploaded
at exactly its size; the malformed leaves are the last block of an image with no slack."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, keystore as ks, trace  # noqa: E402
from storm_amd.scrub import OBJECTLIST  # noqa: E402
from tests import lookup_util as lu  # noqa: E402

_device_images = {}


def on_device(tree):
    """The image as a device tensor, uploaded once per tree."""
    if id(tree) not in _device_images:
        _device_images[id(tree)] = (tree, torch.from_numpy(np.array(tree.img)).cuda())
    return _device_images[id(tree)][1]


def device_lookup(case, **kw):
    p = lu.pack(case.keys, case.mode)
    keys = torch.from_numpy(np.array(p["keys"])).cuda()
    offsets = None if p["offsets"] is None else torch.from_numpy(p["offsets"].view(np.int64)).cuda()
    lens = None if p["lens"] is None else torch.from_numpy(p["lens"].view(np.int32)).cuda()
    return ks.get_object_ids_device(on_device(case.tree), *case.tree.args(), keys, offsets, lens, p["length"],
                                    verify_leaves=case.verify_leaves, **kw)


def same_everywhere(case, **kw):
    """Device == host leg == reference: result bytes, report, code and message."""
    dres, drep = device_lookup(case, **kw)
    hres, hrep = lu.host_lookup(case)
    res = ks.results_numpy(dres)
    assert res.tobytes() == hres.tobytes()
    assert drep.as_dict() == hrep.as_dict()
    assert (drep.code, drep.message) == (hrep.code, hrep.message)
    lu.check_against_reference(case, res, drep)
    return res, drep


@pytest.mark.parametrize("name", list(lu.CASES))
def test_case(name):
    same_everywhere(lu.CASES[name]())


def test_key_messages():
    _, rep = device_lookup(lu.addressing("bad lens"))
    assert rep.code == _lib.EMISMATCH
    assert rep.message == "maximum key component length exceeded, maximum: 256, actual: 257"
    _, rep = device_lookup(lu.empty_key_first())
    assert rep.code == _lib.EMISMATCH and rep.message == "key cannot be empty"


def test_stream_workspace_and_optional_outputs():
    """On a stream of the caller's with a workspace that is reused; the trace results and the
    tags the call hands back are those of trace_keys_device over the same keys."""
    case = lu.addressing("rows")
    t = case.tree
    stream = torch.cuda.Stream()
    n = len(case.keys)
    ws = torch.empty((ks.workspace_bytes(n, t.C) + 7) // 8, dtype=torch.int64, device="cuda")
    for _ in range(2):
        with torch.cuda.stream(stream):
            _, rep = same_everywhere(case, stream=stream.cuda_stream, workspace=ws, want_trace=True)
    keys = torch.from_numpy(np.array(lu.pack(case.keys, "rows")["keys"])).cuda()
    tres, trep, tags = trace.trace_keys_device(on_device(t), t.lay, t.root[:2] + (2,), t.root_type, keys, OBJECTLIST)
    assert torch.equal(tags, rep.tags) and torch.equal(tres, rep.trace_results)
    assert trep.as_dict() == rep.trace.as_dict()


def test_device_refuses_a_small_workspace():
    case = lu.count(65)
    ws = torch.empty(ks.workspace_bytes(65, 10) // 8 - 1, dtype=torch.int64, device="cuda")
    p = lu.pack(case.keys, case.mode)
    import ctypes
    from storm_amd._lib import LookupReportStruct, lib
    from storm_amd.scrub import _root
    t = case.tree
    keys = torch.from_numpy(np.array(p["keys"])).cuda()
    offsets = torch.from_numpy(p["offsets"].view(np.int64)).cuda()
    lens = torch.from_numpy(p["lens"].view(np.int32)).cuda()
    results = torch.empty((65, 4), dtype=torch.int64, device="cuda")
    raw, r = LookupReportStruct(), _root(t.root[:2] + (2,))
    rc = lib.stormck_lookup_device(on_device(t).data_ptr(), ctypes.byref(t.lay), ctypes.byref(r), t.root_type,
                                   ctypes.byref(t.params.raw), keys.data_ptr(), 0, offsets.data_ptr(), lens.data_ptr(),
                                   0, 65, 0, results.data_ptr(), None, None, ws.data_ptr(), ws.numel() * 8,
                                   ctypes.byref(raw), None)
    assert rc == _lib.EINVAL and "workspace" in _lib.last_error()
