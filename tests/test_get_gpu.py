"""Get on the device (MI355X): stormck_get_device gives the result bytes, the row bytes (the
untouched gaps included), the report, the return code and the message of the host leg and of the
pure-Python reference (tests/objects_util.py ``reference_get``) on the designed cases of
tests/test_get.py. Every store is uploaded at exactly its size, and every call is given one
workspace tensor, filled with 0xFF bytes once and never cleared. The designed cases run once
more in a child process on the probe build with STORMCK_FETCH_COPY forcing each form of the move
(k_get_scatter moves the objects as k_object_fetch does)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import storm  # noqa: E402
from tests import lookup_util as lu  # noqa: E402
from tests import objects_util as ou  # noqa: E402
from tests.conftest import ROOT  # noqa: E402

MAX_KEYS = 300
_device_images = {}
_workspace = []


def on_device(store):
    if id(store.img) not in _device_images:
        _device_images[id(store.img)] = (store.img, torch.from_numpy(np.array(store.img)).cuda())
    return _device_images[id(store.img)][1]


def dirty_workspace(case):
    if not _workspace:
        _workspace.append(torch.full((storm.workspace_bytes(MAX_KEYS, 10),), 0xFF, dtype=torch.uint8, device="cuda"))
    assert len(case.keys) <= MAX_KEYS and case.store.C == 10
    return _workspace[0]


def device_get(case, **kw):
    p = lu.pack(case.keys, "flat")
    keys = torch.from_numpy(np.array(p["keys"])).cuda()
    offsets = torch.from_numpy(p["offsets"].view(np.int64)).cuda()
    lens = torch.from_numpy(p["lens"].view(np.int32)).cuda()
    rows = case.rows()
    kw.setdefault("workspace", dirty_workspace(case))
    return storm.get_device(on_device(case.store), case.store.lay, case.space_id, case.store.params, keys, offsets, lens,
                            verify_leaves=case.verify_leaves, want_objects=case.want_objects, out_stride=case.out_stride,
                            objects=None if rows is None else torch.from_numpy(rows).cuda(), **kw)


def same_everywhere(case, **kw):
    """Device == host leg == reference: result bytes, row bytes, report, code and message."""
    dres, drows, drep = device_get(case, **kw)
    hres, hrows, hrep = ou.host_get(case)
    res = storm.results_numpy(dres)
    rows = None if drows is None else drows.cpu().numpy()
    assert res.tobytes() == hres.tobytes()
    assert (rows is None and hrows is None) or rows.tobytes() == hrows.tobytes()
    assert drep.as_dict() == hrep.as_dict()
    assert (drep.code, drep.message) == (hrep.code, hrep.message)
    ou.check_get(case, res, rows, drep)


@pytest.mark.parametrize("name", list(ou.GET_CASES))
def test_case(name):
    same_everywhere(ou.GET_CASES[name]())


def test_stream_and_a_workspace_of_the_calls_own():
    case = ou.get_mixed()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        same_everywhere(case, stream=stream.cuda_stream)
    same_everywhere(case, workspace=None)


COPY_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from storm_amd import _lib, build as sb
assert _lib.LIB_PATH == sb.PROBES_LIB
from tests import objects_util as ou
from tests.test_get_gpu import same_everywhere
for name in ou.GET_CASES:
    same_everywhere(ou.GET_CASES[name]())
print("every leg agrees on", len(ou.GET_CASES), "cases")
"""


@pytest.mark.parametrize("form", ["0", "1"], ids=["lane", "wave"])
def test_both_copy_forms_on_the_probe_build(form):
    from storm_amd import build as sb
    assert os.path.exists(sb.PROBES_LIB), "probe build missing: storm_amd.build.build_probes_lib()"
    env = dict(os.environ, STORMCK_LIBRARY=sb.PROBES_LIB, STORMCK_FETCH_COPY=form)
    r = subprocess.run([sys.executable, "-c", COPY_CHILD, ROOT], cwd=ROOT, capture_output=True, text=True, env=env,
                       timeout=250)
    assert r.returncode == 0 and "every leg agrees on %d cases" % len(ou.GET_CASES) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
