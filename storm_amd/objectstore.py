"""Objects: objectstore.GetObject for many object IDs at once (include/stormck.h "objects",
DESIGN.md "Objects").

storm traces an object ID down to its blob leaf and probes that leaf by open addressing for the
ID's slot; a Defined slot holds the object. ``get_objects_device`` does that for a batch of IDs
in one call on an image that lives in HBM: the trace's engine, then ``k_object_fetch`` with one
lane per ID, which also moves the found objects into dense rows. ``get_objects_host`` is the
same over an image in host memory on the library's host threads and needs no device.

IDs are a 1-d array of 64-bit integers, or any array whose rows start with the ID
(``id_stride`` bytes apart): a lookup's results (``keystore.RESULT_DTYPE``, stride 32) are read
in place.

Every call returns ``(results, objects, report)``: one ``RESULT_DTYPE`` record per ID, in the
IDs' order (a numpy structured array from the host leg; from the device an int64 tensor of shape
(n, 4) that ``results_numpy`` views as the same records), the rows as a (n, out_stride) uint8
array or tensor (None when ``want_objects`` is False), and an :class:`ObjectsReport`. The first
``object_size`` bytes of a row are the object when the ID is FOUND and zeros otherwise; the rest
of a row is not written. A damaged tree raises nothing: the statuses and the report say what is
wrong. Exceptions are for bad arguments and HIP errors.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, trace
from ._lib import BlobParamsStruct, ObjectResultStruct, ObjectsReportStruct, lib
from .scrub import ScrubLayout, _root
from .trace import ABSENT, DEPTH, FOUND, LEAVES_UNVERIFIED, MISMATCH, RANGE, TYPE  # noqa: F401  (for callers)

NO_SLOT = 2 ** 32 - 1    # STORMCK_LOOKUP_NO_SLOT
MAX_OBJECTS = 4095       # the largest objects_per_block
STATUS_NAMES = trace.STATUS_NAMES
BAD = trace.BAD

RESULT_DTYPE = np.dtype([("object_id", "<u8"), ("address", "<u8"), ("reminder", "<u8"), ("index", "<u4"),
                         ("probes", "<u2"), ("status", "u1"), ("reserved", "u1")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(ObjectResultStruct) == 32


def slot_stride(object_size: int) -> int:
    """unsafe.Sizeof(blob.Object[T]) for unsafe.Sizeof(T) == object_size."""
    return (8 + object_size + 1 + 7) & ~7


class BlobParams:
    """stormck_blob_params: objectsPerBlock and unsafe.Sizeof(T)."""

    def __init__(self, objects_per_block: int, object_size: int):
        self.objects_per_block, self.object_size = int(objects_per_block), int(object_size)
        self.raw = BlobParamsStruct(self.objects_per_block, self.object_size)

    @property
    def stride(self) -> int:
        return slot_stride(self.object_size)


class ObjectsReport:
    """stormck_objects_report; ``trace`` is the trace's report (a trace.TraceReport)."""

    FIELDS = ("n_status", "n_probed", "probes", "first_bad")

    def __init__(self, raw: ObjectsReportStruct, code: int, message: str):
        self.trace = trace.TraceReport(raw.trace, _lib.OK, "")
        self.n_status = tuple(int(v) for v in raw.n_status)
        self.n_probed, self.probes, self.first_bad = int(raw.n_probed), int(raw.probes), int(raw.first_bad)
        self.code = code          # STORMCK_OK or STORMCK_EMISMATCH
        self.message = message    # the text of ID first_bad's error ("" when there is none)

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return dict({f: getattr(self, f) for f in self.FIELDS}, trace=self.trace.as_dict())

    def __repr__(self) -> str:
        return f"ObjectsReport({self.as_dict()})"


def workspace_bytes(n_ids: int) -> int:
    return int(lib.stormck_objects_workspace_bytes(n_ids))


def results_numpy(results) -> np.ndarray:
    """A device call's results as RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(RESULT_DTYPE)


def _report(rc: int, raw: ObjectsReportStruct) -> ObjectsReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return ObjectsReport(raw, rc, _lib.last_error() if rc else "")


def _ids_shape(n_bytes: int, itemsize: int, shape, id_stride):
    """(n, id_stride) of an ID array of `shape`: rows that start with the ID."""
    if id_stride is None:
        id_stride = itemsize if len(shape) == 1 else itemsize * int(np.prod(shape[1:]))
    n = shape[0] if len(shape) else 0
    if n and n_bytes < (n - 1) * id_stride + 8:
        raise ValueError("ids is smaller than n rows of id_stride bytes")
    return int(n), int(id_stride)


def get_objects_device(store, layout: ScrubLayout, root, root_type: int, params: BlobParams, ids, id_stride=None,
                       verify_leaves: bool = True, stream: int = 0, workspace=None, want_objects: bool = True,
                       out_stride=None, objects=None):
    """The objects of `ids` (a contiguous CUDA tensor: 1-d int64, or rows that start with the ID,
    such as a lookup's (n, 4) results) in the object tree at `root` ((checksum, address, birth
    revision) or a Pointer) of block type `root_type` in the device-resident image `store` (a
    CUDA tensor or a raw device pointer). Queued on `stream` (0: the null stream) behind what is
    there; returns when the results and the rows are written. verify_leaves=False probes and
    reads the leaves without hashing them. `out_stride`: bytes per row (default object_size);
    `objects`: a (n, out_stride) uint8 CUDA tensor to write the rows into; `workspace`: a device
    tensor to reuse."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or not ids.is_contiguous() or ids.is_floating_point():
        raise ValueError("ids must be a contiguous CUDA integer tensor")
    n, id_stride = _ids_shape(ids.numel() * ids.element_size(), ids.element_size(), tuple(ids.shape), id_stride)
    out_stride = params.object_size if out_stride is None else int(out_stride)
    if objects is not None:
        if (not isinstance(objects, torch.Tensor) or not objects.is_cuda or not objects.is_contiguous() or
                objects.element_size() != 1 or tuple(objects.shape) != (n, out_stride)):
            raise ValueError("objects must be a contiguous (n, out_stride) CUDA byte tensor")
    elif want_objects:
        objects = torch.empty((n, out_stride), dtype=torch.uint8, device=device)
    need = workspace_bytes(n)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 4), dtype=torch.int64, device=device)
    raw = ObjectsReportStruct()
    r = _root(root)
    rc = lib.stormck_objects_device(d_store, ctypes.byref(layout), ctypes.byref(r), root_type, ctypes.byref(params.raw),
                                    ids.data_ptr(), id_stride, n, 0 if verify_leaves else LEAVES_UNVERIFIED,
                                    results.data_ptr(), objects.data_ptr() if objects is not None else None, out_stride,
                                    workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                    ctypes.byref(raw), stream or None)
    return results, objects, _report(rc, raw)


def get_objects_host(buffer, layout: ScrubLayout, root, root_type: int, params: BlobParams, ids, id_stride=None,
                     verify_leaves: bool = True, threads: int = 0, want_objects: bool = True, out_stride=None,
                     objects=None):
    """The same over an image in host memory, on `threads` library pool threads (0: the pool).
    `ids` is a numpy array (1-d uint64, or rows that start with the ID, such as
    keystore.RESULT_DTYPE records); needs no device."""
    buf = buffer if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, dtype=np.uint8)
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    ids = np.ascontiguousarray(ids)
    if ids.dtype.kind == "f":
        raise ValueError("ids must be integers or records that start with the ID")
    n, id_stride = _ids_shape(ids.nbytes, ids.dtype.itemsize, ids.shape, id_stride)
    out_stride = params.object_size if out_stride is None else int(out_stride)
    if objects is not None:
        if (not isinstance(objects, np.ndarray) or objects.dtype != np.uint8 or not objects.flags.c_contiguous or
                objects.shape != (n, out_stride)):
            raise ValueError("objects must be a contiguous (n, out_stride) uint8 array")
    elif want_objects:
        objects = np.zeros((n, out_stride), dtype=np.uint8)
    results = np.zeros(n, dtype=RESULT_DTYPE)
    raw = ObjectsReportStruct()
    r = _root(root)
    rc = lib.stormck_objects_host(buf.ctypes.data, ctypes.byref(layout), ctypes.byref(r), root_type,
                                  ctypes.byref(params.raw), ids.ctypes.data if n else None, id_stride, n,
                                  0 if verify_leaves else LEAVES_UNVERIFIED, results.ctypes.data if n else None,
                                  objects.ctypes.data if objects is not None and n else None, out_stride,
                                  ctypes.byref(raw), threads)
    return results, objects, _report(rc, raw)
