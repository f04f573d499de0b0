"""Objects on the device (MI355X): stormck_objects_device gives the result bytes, the row bytes
(the untouched gaps included), the report, the return code and the message of the host leg and
of the pure-Python reference (tests/objects_util.py) on the designed cases of
tests/test_objects.py. Every image is uploaded at exactly its size; "last block" probes the last
block of an image with no slack.

Every device call of this module and of tests/test_objects_fuzz_gpu.py is given the same
workspace tensor: sized for the largest case, filled with 0xFF bytes once and never cleared, so
the trace's table, rows and counters and the call's trace results and counters of one case are
what the next case finds.

Both forms of k_object_fetch's move run every case, whatever rule ships: once more in a child
process on the probe build, with STORMCK_FETCH_COPY forcing the lane form and the wave form."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, objectstore as obs  # noqa: E402
from tests import objects_util as ou  # noqa: E402
from tests.conftest import ROOT  # noqa: E402

MAX_IDS = 20000
_device_images = {}
_workspace = []


def on_device(tree):
    """The image as a device tensor, uploaded once per tree."""
    if id(tree) not in _device_images:
        _device_images[id(tree)] = (tree, torch.from_numpy(np.array(tree.img)).cuda())
    return _device_images[id(tree)][1]


def dirty_workspace(case):
    if not _workspace:
        _workspace.append(torch.full((obs.workspace_bytes(MAX_IDS),), 0xFF, dtype=torch.uint8, device="cuda"))
    ws = _workspace[0]
    assert len(case.ids) <= MAX_IDS and ws.numel() >= obs.workspace_bytes(len(case.ids))
    return ws  # large enough: the call uses it and allocates none of its own


def device_objects(case, **kw):
    ids = ou.ids_array(case)
    ids = torch.from_numpy(ids.view(np.int64).reshape(len(case.ids), -1) if case.id_stride == 32 else ids.view(np.int64)).cuda()
    rows = ou.dirty_rows(case)
    kw.setdefault("workspace", dirty_workspace(case))
    return obs.get_objects_device(on_device(case.tree), *case.tree.args(), ids, verify_leaves=case.verify_leaves,
                                  want_objects=case.want_objects, out_stride=case.out_stride,
                                  objects=None if rows is None else torch.from_numpy(rows).cuda(), **kw)


def same_everywhere(case, **kw):
    """Device == host leg == reference: result bytes, row bytes, report, code and message."""
    dres, drows, drep = device_objects(case, **kw)
    hres, hrows, hrep = ou.host_objects(case)
    res = obs.results_numpy(dres)
    rows = None if drows is None else drows.cpu().numpy()
    assert res.tobytes() == hres.tobytes()
    assert (rows is None and hrows is None) or rows.tobytes() == hrows.tobytes()
    assert drep.as_dict() == hrep.as_dict()
    assert (drep.code, drep.message) == (hrep.code, hrep.message)
    ou.check_against_reference(case, res, rows, drep)
    return res, drep


@pytest.mark.parametrize("name", list(ou.CASES))
def test_case(name):
    same_everywhere(ou.CASES[name]())


def test_stream_and_a_workspace_of_the_calls_own():
    """On a stream of the caller's, twice; and with no workspace given the call allocates one."""
    case = ou.size(24)
    stream = torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(stream):
            same_everywhere(case, stream=stream.cuda_stream)
    same_everywhere(case, workspace=None)


def test_rows_at_an_odd_address():
    """The rows array at an address that is no multiple of 8, rows of S = 24 bytes 27 apart: every
    row is moved by bytes, and the bytes around the array are untouched."""
    case = ou.size(24)
    n = len(case.ids)
    assert case.out_stride == 32
    wide = ou.Case(case.tree, case.ids, None, out_stride=27)
    buf = torch.full((n * 27 + 16,), ou.FILL, dtype=torch.uint8, device="cuda")
    rows = buf[3:3 + n * 27].view(n, 27)
    assert rows.data_ptr() % 8 == 3
    ids = torch.from_numpy(ou.ids_array(wide).view(np.int64)).cuda()
    _, _, rep = obs.get_objects_device(on_device(wide.tree), *wide.tree.args(), ids, out_stride=27, objects=rows,
                                       workspace=dirty_workspace(wide))
    assert rep.ok
    got = buf.cpu().numpy().tobytes()
    assert got[3:3 + n * 27] == ou.expected_rows(wide) and set(got[:3] + got[3 + n * 27:]) == {ou.FILL}


def test_device_refuses_a_small_workspace():
    case = ou.count(65)
    ws = torch.empty(obs.workspace_bytes(65) // 8 - 1, dtype=torch.int64, device="cuda")
    import ctypes
    from storm_amd._lib import ObjectsReportStruct, lib
    from storm_amd.scrub import _root
    t = case.tree
    ids = torch.from_numpy(ou.ids_array(case).view(np.int64)).cuda()
    results = torch.empty((65, 4), dtype=torch.int64, device="cuda")
    raw, r = ObjectsReportStruct(), _root(t.root[:2] + (2,))
    rc = lib.stormck_objects_device(on_device(t).data_ptr(), ctypes.byref(t.lay), ctypes.byref(r), t.root_type,
                                    ctypes.byref(t.params.raw), ids.data_ptr(), 8, 65, 0, results.data_ptr(), None, 0,
                                    ws.data_ptr(), ws.numel() * 8, ctypes.byref(raw), None)
    assert rc == _lib.EINVAL and "workspace" in _lib.last_error()


COPY_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from storm_amd import _lib, build as sb
assert _lib.LIB_PATH == sb.PROBES_LIB
from tests import objects_util as ou
from tests.test_objects_gpu import same_everywhere
for name in ou.CASES:
    same_everywhere(ou.CASES[name]())
print("every leg agrees on", len(ou.CASES), "cases")
"""


@pytest.mark.parametrize("form", ["0", "1"], ids=["lane", "wave"])
def test_both_copy_forms_on_the_probe_build(form):
    """Every designed case, at every object size, through the lane form and through the wave form
    of the move (STORMCK_FETCH_COPY, which only the probe build reads), each in a child process
    that loads the probe build."""
    from storm_amd import build as sb
    assert os.path.exists(sb.PROBES_LIB), "probe build missing: storm_amd.build.build_probes_lib()"
    env = dict(os.environ, STORMCK_LIBRARY=sb.PROBES_LIB, STORMCK_FETCH_COPY=form)
    r = subprocess.run([sys.executable, "-c", COPY_CHILD, ROOT], cwd=ROOT, capture_output=True, text=True, env=env,
                       timeout=250)
    assert r.returncode == 0 and "every leg agrees on %d cases" % len(ou.CASES) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
