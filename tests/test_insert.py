"""Insert on the host leg (CPU only): stormck_insert_host, storm.Set for new keys whose leaves have
room as a new revision (include/stormck.h "insert"), against the pure-Python restatement of its
rules (tests/insert_util.py ``reference_insert``): image bytes, result bytes, report, return code
and message; then the semantic checks of ``check_insert``, which do not rest on that restatement.
The designed cases are tests/insert_util.py ``CASES``; tests/test_insert_gpu.py runs the same ones
on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

from storm_amd import _lib, storm
from tests import insert_util as iu
from tests import lookup_util as lu
from tests import objects_util as ou
from tests import update_util as uu
from tests.conftest import ROOT


@pytest.mark.parametrize("name", list(iu.CASES))
def test_case(name):
    iu.CASES[name]()


def test_threads_do_not_change_the_bytes():
    store, present, kt, _ = iu.plain_store()
    keys = iu._fresh_keys(np.random.default_rng(5), 30)
    rows = uu.new_rows(np.random.default_rng(5), len(keys), ou.GET_S)
    images = []
    for threads in (1, 3, 0):
        img, lay = uu.roomy(store, 160)
        iu.host_insert(img, lay, store, iu.SPACE, keys, rows, threads=threads)
        images.append(img.tobytes())
    assert images[0] == images[1] == images[2] != uu.roomy(store, 160)[0].tobytes()


def _args():
    store, present, kt, _ = iu.plain_store()
    img, lay = uu.roomy(store, 160)
    keys = iu._fresh_keys(np.random.default_rng(6), 4)
    return store, img, lay, lu.pack(keys, "flat"), uu.pack_rows(uu.new_rows(np.random.default_rng(6), 4, ou.GET_S), ou.GET_S, 16)


def test_argument_errors_change_nothing():
    store, img, lay, p, rows = _args()
    old = img.tobytes()

    def call(params=None, objects=rows, **kw):
        return storm.insert_host(img, lay, iu.SPACE, params or store.params, p["keys"], objects, offsets=p["offsets"],
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
    with pytest.raises(_lib.StormckError, match="not a permutation"):
        call(params=storm.GetParams(store.SA, lu.ks.ObjectListParams(np.zeros(10, np.uint16), 10), store.params.objects))
    raw = _lib.InsertReportStruct()
    results = np.zeros(4, storm.INSERT_RESULT_DTYPE)
    rc = _lib.lib.stormck_insert_host(img.ctypes.data, ctypes.byref(lay), iu.SPACE, ctypes.byref(store.params.raw),
                                      p["keys"].ctypes.data, 0, p["offsets"].ctypes.data, p["lens"].ctypes.data, 0, 4, None,
                                      16, 0, results.ctypes.data, ctypes.byref(raw), 0)
    assert rc == _lib.EINVAL and "null argument" in _lib.last_error()  # a null objects array with n > 0
    rc = _lib.lib.stormck_insert_host(img.ctypes.data, ctypes.byref(lay), iu.SPACE, ctypes.byref(store.params.raw),
                                      p["keys"].ctypes.data, 0, p["offsets"].ctypes.data, p["lens"].ctypes.data, 0, 4,
                                      rows.ctypes.data, 16, 0, None, ctypes.byref(raw), 0)
    assert rc == _lib.EINVAL  # null results
    rc = _lib.lib.stormck_insert_host(img.ctypes.data, ctypes.byref(lay), iu.SPACE, ctypes.byref(store.params.raw),
                                      p["keys"].ctypes.data, 0, p["offsets"].ctypes.data, p["lens"].ctypes.data, 0, 4,
                                      rows.ctypes.data, 16, 0, results.ctypes.data, None, 0)
    assert rc == _lib.EINVAL  # null report
    assert img.tobytes() == old


def test_more_chunks_than_the_leaf_worker_holds():
    """chunks_per_block above STORMCK_INSERT_MAX_CHUNKS is an argument error, before any work."""
    C = storm.INSERT_MAX_CHUNKS + 1
    lay = ou.ScrubLayout(65536, 4, 10, 10, (53 * C + 11) & ~7, 728)
    img = np.zeros(4 * 65536, np.uint8)
    params = storm.GetParams(ou.space_table(10, 7), lu.ks.ObjectListParams(np.arange(C, dtype=np.uint16), C),
                             ou.obs.BlobParams(10, 13))
    with pytest.raises(_lib.StormckError, match="STORMCK_INSERT_MAX_CHUNKS"):
        storm.insert_host(img, lay, 1, params, np.zeros((1, 4), np.uint8), np.zeros((1, 13), np.uint8))
    assert not img.any()


def test_a_read_only_buffer_is_refused():
    store, img, lay, p, rows = _args()
    with pytest.raises(ValueError, match="read-only"):
        storm.insert_host(store.img, store.lay, iu.SPACE, store.params, p["keys"], rows, offsets=p["offsets"], lens=p["lens"])
    with pytest.raises(ValueError, match="smaller than"):
        storm.insert_host(img[:1024], lay, iu.SPACE, store.params, p["keys"], rows, offsets=p["offsets"], lens=p["lens"])


def test_the_header_and_the_binding():
    with open(os.path.join(ROOT, "include", "stormck.h")) as f:
        h = f.read()
    assert re.search(r"^#define STORMCK_HAS_INSERT 1$", h, re.M)
    assert re.search(r"^#define STORMCK_INSERT_MAX_CHUNKS 1024$", h, re.M) and storm.INSERT_MAX_CHUNKS == 1024
    assert re.search(r"^#define STORMCK_INSERT_MAX_PER_LEAF 2048$", h, re.M) and storm.INSERT_MAX_PER_LEAF == iu.MAX_PER_LEAF
    assert ctypes.sizeof(_lib.InsertResultStruct) == 40 and storm.INSERT_RESULT_DTYPE.itemsize == 40
    assert ctypes.sizeof(_lib.InsertReportStruct) == ctypes.sizeof(_lib.SpaceResultStruct) + ctypes.sizeof(_lib.LookupReportStruct) + 8 * 26
    assert (storm.R_CUT, storm.R_CROWDED, storm.INSERT_REPEATED) == (iu.R_CUT, iu.R_CROWDED, iu.REPEATED) == (9, 8, 2)


def test_the_workspace_is_linear_in_the_keys():
    w = [storm.insert_workspace_bytes(n, 600) for n in (1 << 10, 1 << 11, 1 << 20, 1 << 21)]
    assert w[1] < 2.1 * w[0] and w[3] < 2.1 * w[2]
    assert all(storm.insert_workspace_bytes(n, 10) > storm.workspace_bytes(n, 10) for n in (0, 1, 300))
