"""Update on the host leg (CPU only): stormck_update_host, storm.Set for keys that already have
an object as a new revision (include/stormck.h "update"), against the pure-Python restatement of
its rules (tests/update_util.py ``reference_update``): image bytes, result bytes, report, return
code and message; then the semantic checks of ``check_update``, which do not rest on that
restatement. The designed cases are tests/update_util.py ``CASES``; tests/test_update_gpu.py runs
the same ones on the device."""
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, storm
from tests import lookup_util as lu
from tests import objects_util as ou
from tests import update_util as uu
from tests.conftest import ROOT


@pytest.mark.parametrize("name", list(uu.CASES))
def test_case(name):
    uu.CASES[name]()


def test_threads_do_not_change_the_bytes():
    store, present, _, _, _ = ou.get_store()
    keys = list(present)
    rows = uu.new_rows(np.random.default_rng(5), len(keys), ou.GET_S)
    images = []
    for threads in (1, 3, 0):
        img, lay = uu.roomy(store, 120)
        uu.host_update(img, lay, store, ou.GET_SPACE, keys, rows, threads=threads)
        images.append(img.tobytes())
    assert images[0] == images[1] == images[2]


def _args():
    store, present, _, _, _ = ou.get_store()
    img, lay = uu.roomy(store, 120)
    keys = list(present)[:4]
    return store, img, lay, lu.pack(keys, "flat"), uu.pack_rows(uu.new_rows(np.random.default_rng(6), 4, ou.GET_S), ou.GET_S, 16)


def test_argument_errors_change_nothing():
    store, img, lay, p, rows = _args()
    old = img.tobytes()

    def call(params=None, objects=rows, **kw):
        return storm.update_host(img, lay, ou.GET_SPACE, params or store.params, p["keys"], objects, offsets=p["offsets"],
                                 lens=p["lens"], **kw)
    with pytest.raises(_lib.StormckError, match="flags must be 0"):
        call(flags=1)  # STORMCK_TRACE_LEAVES_UNVERIFIED
    with pytest.raises(_lib.StormckError, match="in_stride is below object_size"):
        call(objects=np.ascontiguousarray(rows[:, :12]))
    with pytest.raises(_lib.StormckError, match="object_size is 0"):  # an argument error of the get
        call(params=storm.GetParams(store.SA, store.params.keys, ou.obs.BlobParams(10, 0)))
    with pytest.raises(_lib.StormckError, match="do not fit"):
        call(params=storm.GetParams(store.SA, store.params.keys, ou.obs.BlobParams(60, 13)),
             objects=uu.pack_rows([bytes(13)] * 4, 13, 13))
    raw = _lib.UpdateReportStruct()
    results = np.zeros(4, storm.UPDATE_RESULT_DTYPE)
    import ctypes
    rc = _lib.lib.stormck_update_host(img.ctypes.data, ctypes.byref(lay), ou.GET_SPACE, ctypes.byref(store.params.raw),
                                      p["keys"].ctypes.data, 0, p["offsets"].ctypes.data, p["lens"].ctypes.data, 0, 4, None,
                                      16, 0, results.ctypes.data, ctypes.byref(raw), 0)
    assert rc == _lib.EINVAL and "null argument" in _lib.last_error()  # a null objects array with n > 0
    rc = _lib.lib.stormck_update_host(img.ctypes.data, ctypes.byref(lay), ou.GET_SPACE, ctypes.byref(store.params.raw),
                                      p["keys"].ctypes.data, 0, p["offsets"].ctypes.data, p["lens"].ctypes.data, 0, 4,
                                      rows.ctypes.data, 16, 0, None, ctypes.byref(raw), 0)
    assert rc == _lib.EINVAL  # null results
    assert img.tobytes() == old


def test_a_read_only_buffer_is_refused():
    store, img, lay, p, rows = _args()
    with pytest.raises(ValueError, match="read-only"):
        storm.update_host(store.img, store.lay, ou.GET_SPACE, store.params, p["keys"], rows, offsets=p["offsets"], lens=p["lens"])
    with pytest.raises(ValueError, match="smaller than"):
        storm.update_host(img[:1024], lay, ou.GET_SPACE, store.params, p["keys"], rows, offsets=p["offsets"], lens=p["lens"])


def test_the_header_and_the_binding():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        h = f.read()
    assert re.search(r"^#define STORMCK_HAS_UPDATE 1$", h, re.M) and re.search(r"^#define STORMCK_ABI_VERSION 7$", h, re.M)
    assert re.search(r"^#define STORMCK_ENOSPC \(-6\)", h, re.M) and _lib.ENOSPC == -6
    assert _lib.lib.stormck_abi_version() == 7
    import ctypes
    assert ctypes.sizeof(_lib.UpdateResultStruct) == 32 and storm.UPDATE_RESULT_DTYPE.itemsize == 32
    assert ctypes.sizeof(_lib.UpdateReportStruct) == ctypes.sizeof(_lib.GetReportStruct) + 96


def test_the_workspace_is_linear_in_the_keys():
    w = [storm.update_workspace_bytes(n, 600) for n in (1 << 10, 1 << 11, 1 << 20, 1 << 21)]
    assert w[1] < 2.1 * w[0] and w[3] < 2.1 * w[2]
    assert all(storm.update_workspace_bytes(n, 10) > storm.workspace_bytes(n, 10) for n in (0, 1, 300))
