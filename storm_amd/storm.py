"""Get: storm.Get for many keys of one space (include/stormck.h "get", DESIGN.md "Get").

storm.Get is spacestore.GetSpace, keystore.GetObjectID and objectstore.GetObject, one after the
other. ``get_device`` does the three stages for a batch of keys of one space in one call on a
store that lives in HBM, from its singularity block: the singularity's check, the space, the
lookup, an order-preserving compaction of the keys that were found, the objects call over their
IDs, and the way back to key order. ``get_host`` is the same over a store in host memory and
needs no device.

Keys are addressed as in ``keystore``. Every call returns ``(results, objects, report)``: one
``RESULT_DTYPE`` record per key (a numpy structured array from the host leg; from the device an
int64 tensor of shape (n, 4) that ``results_numpy`` views as the same records), the rows as a
(n, out_stride) uint8 array or tensor (None when ``want_objects`` is False) and a
:class:`GetReport`. ``stage`` says where a key's walk ended: 0 the space, 1 the key, 2 the object.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, keystore, spacestore, trace
from ._lib import (GetParamsStruct, GetReportStruct, GetResultStruct, InsertReportStruct, InsertResultStruct,
                   UpdateReportStruct, UpdateResultStruct, lib)
from .keystore import _addressing
from .objectstore import BlobParams
from .scrub import ScrubLayout
from .trace import ABSENT, DEPTH, FOUND, LEAVES_UNVERIFIED, MISMATCH, RANGE, TYPE  # noqa: F401  (for callers)

KEY = keystore.KEY
NO_SLOT = keystore.NO_SLOT
BAD = keystore.BAD
STAGE_SPACE, STAGE_KEY, STAGE_OBJECT = 0, 1, 2

RESULT_DTYPE = np.dtype([("object_id", "<u8"), ("key_address", "<u8"), ("object_address", "<u8"), ("index", "<u4"),
                         ("stage", "u1"), ("status", "u1"), ("reserved", "<u2")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(GetResultStruct) == 32


class GetParams:
    """stormck_get_params: spacelist.AddressingOffsets, the lookup's ObjectListParams and the
    objects call's BlobParams."""

    def __init__(self, space_offsets, keys: keystore.ObjectListParams, objects: BlobParams):
        self.space_table = np.ascontiguousarray(space_offsets, dtype=np.uint16).reshape(-1)
        self.keys, self.objects = keys, objects
        self.raw = GetParamsStruct(self.space_table.ctypes.data, keys.raw, objects.raw)


class GetReport:
    """stormck_get_report: ``space`` is the space's record (spacestore.RESULT_DTYPE), ``lookup``
    the lookup's report as a dict."""

    FIELDS = ("n_selected", "n_status", "blocks_hashed", "bytes_hashed", "probes", "levels", "n_found", "first_bad")

    def __init__(self, raw: GetReportStruct, code: int, message: str):
        self.space = np.frombuffer(bytes(raw.space), dtype=spacestore.RESULT_DTYPE)[0]
        self.lookup = keystore.LookupReport(raw.lookup, _lib.OK, "")
        self.n_selected = int(raw.n_selected)
        self.n_status = tuple(int(v) for v in raw.n_status)
        self.blocks_hashed = tuple(int(v) for v in raw.blocks_hashed)
        self.bytes_hashed, self.probes, self.levels = int(raw.bytes_hashed), int(raw.probes), int(raw.levels)
        self.n_found, self.first_bad = int(raw.n_found), int(raw.first_bad)
        self.code = code          # STORMCK_OK or STORMCK_EMISMATCH
        self.message = message    # the text of key first_bad's error ("" when there is none)

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return dict({f: getattr(self, f) for f in self.FIELDS}, lookup=self.lookup.as_dict(), space=self.space.tobytes())

    def __repr__(self) -> str:
        return f"GetReport({self.as_dict()})"


def workspace_bytes(n_keys: int, chunks_per_block: int) -> int:
    return int(lib.stormck_get_workspace_bytes(n_keys, chunks_per_block))


def results_numpy(results) -> np.ndarray:
    """A device call's results as RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(RESULT_DTYPE)


def _report(rc: int, raw: GetReportStruct) -> GetReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return GetReport(raw, rc, _lib.last_error() if rc else "")


def get_device(store, layout: ScrubLayout, space_id: int, params: GetParams, keys, offsets=None, lens=None, length=None,
               verify_leaves: bool = True, stream: int = 0, workspace=None, want_objects: bool = True, out_stride=None,
               objects=None):
    """The objects of `keys` (a contiguous uint8 CUDA tensor; `offsets` int64 and `lens` int32 CUDA
    tensors) in space `space_id` of the device-resident store `store` (a CUDA tensor or a raw
    device pointer). Queued on `stream` (0: the null stream); returns when results and rows are
    written. verify_leaves=False reads objectlist and blob leaves without hashing them."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or not keys.is_contiguous() or keys.element_size() != 1:
        raise ValueError("keys must be a contiguous CUDA byte tensor")
    n, stride, length = _addressing(tuple(keys.shape), offsets, lens, length)
    out_stride = params.objects.object_size if out_stride is None else int(out_stride)
    if objects is not None:
        if (not isinstance(objects, torch.Tensor) or not objects.is_cuda or not objects.is_contiguous() or
                objects.element_size() != 1 or tuple(objects.shape) != (n, out_stride)):
            raise ValueError("objects must be a contiguous (n, out_stride) CUDA byte tensor")
    elif want_objects:
        objects = torch.empty((n, out_stride), dtype=torch.uint8, device=device)
    need = workspace_bytes(n, params.keys.chunks_per_block)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 4), dtype=torch.int64, device=device)
    raw = GetReportStruct()
    rc = lib.stormck_get_device(d_store, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw), keys.data_ptr(),
                                stride, offsets.data_ptr() if offsets is not None else None,
                                lens.data_ptr() if lens is not None else None, length, n,
                                0 if verify_leaves else LEAVES_UNVERIFIED, results.data_ptr(),
                                objects.data_ptr() if objects is not None else None, out_stride, workspace.data_ptr(),
                                workspace.numel() * workspace.element_size(), ctypes.byref(raw), stream or None)
    return results, objects, _report(rc, raw)


def get_host(buffer, layout: ScrubLayout, space_id: int, params: GetParams, keys, offsets=None, lens=None, length=None,
             verify_leaves: bool = True, threads: int = 0, want_objects: bool = True, out_stride=None, objects=None):
    """The same over a store in host memory. `keys` is a uint8 numpy array; needs no device."""
    buf = buffer if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, dtype=np.uint8)
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
    n, stride, length = _addressing(keys.shape, offsets, lens, length)
    out_stride = params.objects.object_size if out_stride is None else int(out_stride)
    if objects is not None:
        if (not isinstance(objects, np.ndarray) or objects.dtype != np.uint8 or not objects.flags.c_contiguous or
                objects.shape != (n, out_stride)):
            raise ValueError("objects must be a contiguous (n, out_stride) uint8 array")
    elif want_objects:
        objects = np.zeros((n, out_stride), dtype=np.uint8)
    results = np.zeros(n, dtype=RESULT_DTYPE)
    raw = GetReportStruct()
    rc = lib.stormck_get_host(buf.ctypes.data, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw),
                              keys.ctypes.data, stride, offsets.ctypes.data if offsets is not None else None,
                              lens.ctypes.data if lens is not None else None, length, n,
                              0 if verify_leaves else LEAVES_UNVERIFIED, results.ctypes.data if n else None,
                              objects.ctypes.data if objects is not None and n else None, out_stride, ctypes.byref(raw),
                              threads)
    return results, objects, _report(rc, raw)


# ---- update: storm.Set for keys that already have an object ----------------------------------

UPDATE_NONE, UPDATE_WRITTEN, UPDATE_SUPERSEDED = 0, 1, 2
UPDATE_RESULT_DTYPE = np.dtype([("object_id", "<u8"), ("key_address", "<u8"), ("object_address", "<u8"),
                                ("index", "<u4"), ("stage", "u1"), ("status", "u1"), ("action", "u1"), ("reserved", "u1")])
assert UPDATE_RESULT_DTYPE.itemsize == ctypes.sizeof(UpdateResultStruct) == 32


class UpdateReport:
    """stormck_update_report: ``get`` is the :class:`GetReport` of the get the call ran."""

    FIELDS = ("n_written", "n_superseded", "n_dirty", "bytes_copied", "bytes_hashed", "revision", "last_allocated",
              "first_new", "heights")

    def __init__(self, raw: UpdateReportStruct, code: int, message: str):
        self.get = GetReport(raw.get, _lib.OK, "")
        self.n_written, self.n_superseded = int(raw.n_written), int(raw.n_superseded)
        self.n_dirty = tuple(int(v) for v in raw.n_dirty)
        self.bytes_copied, self.bytes_hashed = int(raw.bytes_copied), int(raw.bytes_hashed)
        self.revision, self.last_allocated = int(raw.revision), int(raw.last_allocated)
        self.first_new, self.heights = int(raw.first_new), int(raw.heights)
        self.code = code          # STORMCK_OK, STORMCK_EMISMATCH or STORMCK_ENOSPC
        self.message = message    # the get's text for its first bad key, or the room check's ("" when there is none)

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return dict({f: getattr(self, f) for f in self.FIELDS}, get=self.get.as_dict())

    def __repr__(self) -> str:
        return f"UpdateReport({self.as_dict()})"


def update_workspace_bytes(n_keys: int, chunks_per_block: int) -> int:
    return int(lib.stormck_update_workspace_bytes(n_keys, chunks_per_block))


def update_results_numpy(results) -> np.ndarray:
    """A device call's results as UPDATE_RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(UPDATE_RESULT_DTYPE)


def _update_report(rc: int, raw: UpdateReportStruct) -> UpdateReport:
    if rc not in (_lib.OK, _lib.EMISMATCH, _lib.ENOSPC):
        _lib.check(rc)
    return UpdateReport(raw, rc, _lib.last_error() if rc else "")


def update_device(store, layout: ScrubLayout, space_id: int, params: GetParams, keys, objects, offsets=None, lens=None,
                  length=None, stream: int = 0, workspace=None, flags: int = 0):
    """Write row i of `objects` (a contiguous (n, in_stride) CUDA byte tensor, in_stride at least
    object_size) over the object of key i in space `space_id` of the device-resident store `store`
    (a CUDA tensor or a raw device pointer), which is changed in place: a new revision. Keys as in
    ``get_device``. Returns when the store is written."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or not keys.is_contiguous() or keys.element_size() != 1:
        raise ValueError("keys must be a contiguous CUDA byte tensor")
    n, stride, length = _addressing(tuple(keys.shape), offsets, lens, length)
    if (not isinstance(objects, torch.Tensor) or not objects.is_cuda or not objects.is_contiguous() or
            objects.element_size() != 1 or objects.dim() != 2 or objects.shape[0] != n):
        raise ValueError("objects must be a contiguous (n, in_stride) CUDA byte tensor")
    need = update_workspace_bytes(n, params.keys.chunks_per_block)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 4), dtype=torch.int64, device=device)
    raw = UpdateReportStruct()
    rc = lib.stormck_update_device(d_store, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw), keys.data_ptr(),
                                   stride, offsets.data_ptr() if offsets is not None else None,
                                   lens.data_ptr() if lens is not None else None, length, n,
                                   objects.data_ptr() if n else None, int(objects.shape[1]), flags, results.data_ptr(),
                                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), ctypes.byref(raw),
                                   stream or None)
    return results, _update_report(rc, raw)


def update_host(buffer, layout: ScrubLayout, space_id: int, params: GetParams, keys, objects, offsets=None, lens=None,
                length=None, threads: int = 0, flags: int = 0):
    """The same over a store in host memory, changed in place: `buffer` is a writable, contiguous
    uint8 numpy array (ValueError otherwise); `keys` and `objects` are uint8 numpy arrays. Needs no
    device."""
    if not isinstance(buffer, np.ndarray) or buffer.dtype != np.uint8 or not buffer.flags.c_contiguous:
        raise ValueError("buffer must be a contiguous uint8 numpy array")
    if not buffer.flags.writeable:
        raise ValueError("buffer is read-only: the update writes the store in place")
    buf = buffer.reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
    n, stride, length = _addressing(keys.shape, offsets, lens, length)
    if (not isinstance(objects, np.ndarray) or objects.dtype != np.uint8 or not objects.flags.c_contiguous or
            objects.ndim != 2 or objects.shape[0] != n):
        raise ValueError("objects must be a contiguous (n, in_stride) uint8 array")
    results = np.zeros(n, dtype=UPDATE_RESULT_DTYPE)
    raw = UpdateReportStruct()
    rc = lib.stormck_update_host(buf.ctypes.data, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw),
                                 keys.ctypes.data, stride, offsets.ctypes.data if offsets is not None else None,
                                 lens.ctypes.data if lens is not None else None, length, n,
                                 objects.ctypes.data if n else None, int(objects.shape[1]), flags,
                                 results.ctypes.data if n else None, ctypes.byref(raw), threads)
    return results, _update_report(rc, raw)


# ---- insert: storm.Set for new keys whose leaves have room ------------------------------------

INSERT_NONE, INSERT_INSERTED, INSERT_REPEATED = 0, 1, 2
(R_NONE, R_SPACE, R_EXISTS, R_NO_LEAF, R_KEY_SPLIT, R_NO_SLOT, R_KEY_FULL, R_MALFORMED, R_CROWDED,
 R_CUT) = range(_lib.INSERT_REASONS)
INSERT_MAX_CHUNKS, INSERT_MAX_PER_LEAF = 1024, 2048
INSERT_RESULT_DTYPE = np.dtype([("object_id", "<u8"), ("key_address", "<u8"), ("object_address", "<u8"),
                                ("key_index", "<u4"), ("object_index", "<u4"), ("stage", "u1"), ("status", "u1"),
                                ("action", "u1"), ("reason", "u1"), ("wrote", "u1"), ("reserved", "u1", (3,))])
assert INSERT_RESULT_DTYPE.itemsize == ctypes.sizeof(InsertResultStruct) == 40


class InsertReport:
    """stormck_insert_report: ``space`` is the space's record, ``lookup`` the lookup's report."""

    FIELDS = ("n_inserted", "n_repeated", "n_none", "first_id", "next_object_id", "cut", "limit", "n_dirty",
              "bytes_copied", "bytes_hashed", "revision", "last_allocated", "first_new", "heights")

    def __init__(self, raw: InsertReportStruct, code: int, message: str):
        self.space = np.frombuffer(bytes(raw.space), dtype=spacestore.RESULT_DTYPE)[0]
        self.lookup = keystore.LookupReport(raw.lookup, _lib.OK, "")
        for f in self.FIELDS:
            v = getattr(raw, f)
            setattr(self, f, int(v) if isinstance(v, int) else tuple(int(x) for x in v))
        self.code = code          # STORMCK_OK, STORMCK_EMISMATCH or STORMCK_ENOSPC
        self.message = message    # the failing stage's text, or the room check's ("" when there is none)

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return dict({f: getattr(self, f) for f in self.FIELDS}, lookup=self.lookup.as_dict(), space=self.space.tobytes())

    def __repr__(self) -> str:
        return f"InsertReport({self.as_dict()})"


def insert_workspace_bytes(n_keys: int, chunks_per_block: int) -> int:
    return int(lib.stormck_insert_workspace_bytes(n_keys, chunks_per_block))


def insert_results_numpy(results) -> np.ndarray:
    """A device call's results as INSERT_RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(INSERT_RESULT_DTYPE)


def _insert_report(rc: int, raw: InsertReportStruct) -> InsertReport:
    if rc not in (_lib.OK, _lib.EMISMATCH, _lib.ENOSPC):
        _lib.check(rc)
    return InsertReport(raw, rc, _lib.last_error() if rc else "")


def insert_device(store, layout: ScrubLayout, space_id: int, params: GetParams, keys, objects, offsets=None, lens=None,
                  length=None, stream: int = 0, workspace=None, flags: int = 0):
    """Insert key i with row i of `objects` (a contiguous (n, in_stride) CUDA byte tensor) into space
    `space_id` of the device-resident store `store`, which is changed in place: a new revision that
    holds every key storm would insert without a split and without a new leaf. Keys as in
    ``get_device``. Synchronous. Returns ``(results, report)``: an int64 tensor of shape (n, 5) that
    ``insert_results_numpy`` views as INSERT_RESULT_DTYPE records, and an :class:`InsertReport`;
    both come back whether or not anything was written."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or not keys.is_contiguous() or keys.element_size() != 1:
        raise ValueError("keys must be a contiguous CUDA byte tensor")
    n, stride, length = _addressing(tuple(keys.shape), offsets, lens, length)
    if (not isinstance(objects, torch.Tensor) or not objects.is_cuda or not objects.is_contiguous() or
            objects.element_size() != 1 or objects.dim() != 2 or objects.shape[0] != n):
        raise ValueError("objects must be a contiguous (n, in_stride) CUDA byte tensor")
    if workspace is None:
        need = insert_workspace_bytes(n, params.keys.chunks_per_block)
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 5), dtype=torch.int64, device=device)
    raw = InsertReportStruct()
    rc = lib.stormck_insert_device(d_store, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw), keys.data_ptr(),
                                   stride, offsets.data_ptr() if offsets is not None else None,
                                   lens.data_ptr() if lens is not None else None, length, n,
                                   objects.data_ptr() if n else None, int(objects.shape[1]), flags, results.data_ptr(),
                                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), ctypes.byref(raw),
                                   stream or None)
    return results, _insert_report(rc, raw)


def insert_host(buffer, layout: ScrubLayout, space_id: int, params: GetParams, keys, objects, offsets=None, lens=None,
                length=None, threads: int = 0, flags: int = 0):
    """The same over a store in host memory, changed in place: `buffer` is a writable, contiguous
    uint8 numpy array (ValueError otherwise); `keys` and `objects` are uint8 numpy arrays. Needs no
    device."""
    if not isinstance(buffer, np.ndarray) or buffer.dtype != np.uint8 or not buffer.flags.c_contiguous:
        raise ValueError("buffer must be a contiguous uint8 numpy array")
    if not buffer.flags.writeable:
        raise ValueError("buffer is read-only: the insert writes the store in place")
    buf = buffer.reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
    n, stride, length = _addressing(keys.shape, offsets, lens, length)
    if (not isinstance(objects, np.ndarray) or objects.dtype != np.uint8 or not objects.flags.c_contiguous or
            objects.ndim != 2 or objects.shape[0] != n):
        raise ValueError("objects must be a contiguous (n, in_stride) uint8 array")
    results = np.zeros(n, dtype=INSERT_RESULT_DTYPE)
    raw = InsertReportStruct()
    rc = lib.stormck_insert_host(buf.ctypes.data, ctypes.byref(layout), int(space_id), ctypes.byref(params.raw),
                                 keys.ctypes.data, stride, offsets.ctypes.data if offsets is not None else None,
                                 lens.ctypes.data if lens is not None else None, length, n,
                                 objects.ctypes.data if n else None, int(objects.shape[1]), flags,
                                 results.ctypes.data if n else None, ctypes.byref(raw), threads)
    return results, _insert_report(rc, raw)
