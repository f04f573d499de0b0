"""Spaces on the device (MI355X): stormck_spaces_device gives the result bytes, the report, the
return code and the message of the host leg and of the pure-Python reference
(tests/objects_util.py) on the designed cases of tests/test_spaces.py. Every image is uploaded at
exactly its size ("production sizes" probes the last block of an image with no slack), and every
call is given the dirty workspace of tests/test_objects_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import spacestore as sps  # noqa: E402
from tests import objects_util as ou  # noqa: E402
from tests.test_objects_gpu import _workspace, dirty_workspace  # noqa: E402,F401

_device_images = {}


def on_device(case):
    if id(case.img) not in _device_images:
        _device_images[id(case.img)] = (case.img, torch.from_numpy(np.array(case.img)).cuda())
    return _device_images[id(case.img)][1]


def same_everywhere(case, **kw):
    """Device == host leg == reference: result bytes, report, code and message."""
    ws = dirty_workspace(case)
    assert ws.numel() >= sps.workspace_bytes(len(case.ids), case.lay.spaces_per_block)
    ids = torch.from_numpy(np.array(case.ids, dtype=np.uint64).view(np.int64)).cuda()
    kw.setdefault("workspace", ws)
    dres, drep = sps.get_spaces_device(on_device(case), *case.args(), ids, verify_leaves=case.verify_leaves, **kw)
    hres, hrep = ou.host_spaces(case)
    res = sps.results_numpy(dres)
    assert res.tobytes() == hres.tobytes()
    assert drep.as_dict() == hrep.as_dict() and (drep.code, drep.message) == (hrep.code, hrep.message)
    ou.check_spaces(case, res, drep)


@pytest.mark.parametrize("name", list(ou.SPACE_CASES))
def test_case(name):
    same_everywhere(ou.SPACE_CASES[name]())


def test_stream_and_a_workspace_of_the_calls_own():
    case = ou.space_states()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        same_everywhere(case, stream=stream.cuda_stream)
    same_everywhere(case, workspace=None)
