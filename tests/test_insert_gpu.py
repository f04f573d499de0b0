"""Insert on the device (MI355X): stormck_insert_device leaves the image bytes (downloaded whole,
guard blocks included), the result bytes, the report, the return code and the message of the host
leg and of the pure-Python reference on the designed cases of tests/test_insert.py
(tests/insert_util.py ``CASES``), and ``check_insert`` runs on the downloaded image. Every store is
uploaded at exactly its size plus guards, and every call is given one workspace tensor, filled
with 0xFF bytes once and never cleared. The object sizes of the cases lie on both sides of the
size at which the row store changes its form."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, storm  # noqa: E402
from tests import insert_util as iu  # noqa: E402
from tests import lookup_util as lu  # noqa: E402
from tests import objects_util as ou  # noqa: E402
from tests import update_util as uu  # noqa: E402

MAX_KEYS = 2049
_workspace = []


def dirty_workspace():
    if not _workspace:
        _workspace.append(torch.full((storm.insert_workspace_bytes(MAX_KEYS, 400),), 0xFF, dtype=torch.uint8, device="cuda"))
    return _workspace[0]


def device_insert(img, lay, store, space_id, keys, rows, in_stride=None, workspace="dirty", stream=0):
    """stormck_insert_device on an upload of `img`, which then receives the device's bytes; the
    host leg runs on a copy and must leave the same bytes, results, report, code and message."""
    S = uu.blob_shape(store)[1]
    host = img.copy()
    hres, hrep = iu.host_insert(host, lay, store, space_id, keys, rows, in_stride)
    p = lu.pack(keys, "flat")
    assert len(keys) <= MAX_KEYS and store.C <= 400  # the workspace's size grows with both
    d_img = torch.from_numpy(img).cuda()
    dres, drep = storm.insert_device(d_img, lay, space_id, store.params, torch.from_numpy(np.array(p["keys"])).cuda(),
                                     torch.from_numpy(uu.pack_rows(rows, S, in_stride or S + 3)).cuda(),
                                     offsets=torch.from_numpy(p["offsets"].view(np.int64)).cuda(),
                                     lens=torch.from_numpy(p["lens"].view(np.int32)).cuda(),
                                     workspace=dirty_workspace() if workspace == "dirty" else workspace, stream=stream)
    torch.cuda.synchronize()
    img[:] = d_img.cpu().numpy()
    res = storm.insert_results_numpy(dres)
    assert res.tobytes() == hres.tobytes()
    assert img.tobytes() == host.tobytes()
    assert drep.as_dict() == hrep.as_dict()
    assert (drep.code, drep.message) == (hrep.code, hrep.message)
    return res, drep


@pytest.mark.parametrize("name", list(iu.CASES))
def test_case(name):
    iu.CASES[name](run=device_insert)


def test_stream_and_a_workspace_of_the_calls_own():
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        iu.case_repeats(run=lambda *a: device_insert(*a, stream=stream.cuda_stream))
    iu.case_trigger_mid_batch(run=lambda *a: device_insert(*a, workspace=None))


def test_argument_errors_change_nothing():
    store, present, kt, _ = iu.plain_store()
    img, lay = uu.roomy(store, 160)
    keys = iu._fresh_keys(np.random.default_rng(6), 4)
    p = lu.pack(keys, "flat")
    d_img = torch.from_numpy(img).cuda()
    rows = torch.from_numpy(uu.pack_rows(uu.new_rows(np.random.default_rng(6), 4, ou.GET_S), ou.GET_S, 16)).cuda()
    args = dict(offsets=torch.from_numpy(p["offsets"].view(np.int64)).cuda(), lens=torch.from_numpy(p["lens"].view(np.int32)).cuda())
    d_keys = torch.from_numpy(np.array(p["keys"])).cuda()
    with pytest.raises(_lib.StormckError, match="flags must be 0"):
        storm.insert_device(d_img, lay, iu.SPACE, store.params, d_keys, rows, flags=1, **args)
    with pytest.raises(_lib.StormckError, match="in_stride is below object_size"):
        storm.insert_device(d_img, lay, iu.SPACE, store.params, d_keys, rows[:, :12].contiguous(), **args)
    with pytest.raises(_lib.StormckError, match="8-byte aligned"):
        storm.insert_device(d_img.data_ptr() + 4, lay, iu.SPACE, store.params, d_keys, rows, **args)
    raw = _lib.InsertReportStruct()
    results = torch.empty((4, 5), dtype=torch.int64, device="cuda")
    small = torch.empty(storm.insert_workspace_bytes(4, 10) - 8, dtype=torch.uint8, device="cuda")
    rc = _lib.lib.stormck_insert_device(d_img.data_ptr(), ctypes.byref(lay), iu.SPACE, ctypes.byref(store.params.raw),
                                        d_keys.data_ptr(), 0, args["offsets"].data_ptr(), args["lens"].data_ptr(), 0, 4,
                                        rows.data_ptr(), 16, 0, results.data_ptr(), small.data_ptr(), small.numel(),
                                        ctypes.byref(raw), None)
    assert rc == _lib.EINVAL and "workspace too small" in _lib.last_error()
    torch.cuda.synchronize()
    assert d_img.cpu().numpy().tobytes() == img.tobytes()
