"""Spaces: spacestore.GetSpace for space IDs (include/stormck.h "spaces", DESIGN.md "Spaces").

storm traces a space ID down to its spacelist leaf and probes that leaf by open addressing for
the space; a Defined space holds the roots of the space's key tree and object tree.
``get_spaces_device`` does that for a batch of IDs in one call on an image that lives in HBM:
the trace's engine, then ``k_space_probe`` with one lane per ID. ``get_spaces_host`` is the same
over an image in host memory and needs no device.

Every call returns ``(results, report)``: one ``RESULT_DTYPE`` record per ID, in the IDs' order
(a numpy structured array from the host leg; from the device an int64 tensor of shape (n, 11)
that ``results_numpy`` views as the same records), and a :class:`SpacesReport`. ``roots`` turns a
FOUND record into the arguments ``keystore`` and ``objectstore`` take. A damaged tree raises
nothing: the statuses and the report say what is wrong.

The library ships no addressing table: the caller passes ``spacelist.AddressingOffsets``, a
permutation of 0..layout.spaces_per_block-1 (the library checks it).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, trace
from ._lib import SpaceResultStruct, SpacesReportStruct, lib
from .scrub import ScrubLayout, _root
from .trace import ABSENT, DEPTH, FOUND, LEAVES_UNVERIFIED, MISMATCH, RANGE, TYPE  # noqa: F401  (for callers)

NO_SLOT = 2 ** 32 - 1    # STORMCK_LOOKUP_NO_SLOT
MAX_SPACES = 32768
BAD = trace.BAD

_POINTER = [("checksum", "<u8"), ("address", "<u8"), ("birth_revision", "<u8")]
RESULT_DTYPE = np.dtype([("key_root", _POINTER), ("object_root", _POINTER), ("next_object_id", "<u8"), ("address", "<u8"),
                         ("reminder", "<u8"), ("index", "<u4"), ("probes", "<u2"), ("key_type", "u1"),
                         ("object_type", "u1"), ("status", "u1"), ("reserved", "u1", (7,))])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(SpaceResultStruct) == 88


class SpacesReport:
    """stormck_spaces_report; ``trace`` is the trace's report (a trace.TraceReport)."""

    FIELDS = ("n_status", "n_probed", "probes", "first_bad")

    def __init__(self, raw: SpacesReportStruct, code: int, message: str):
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
        return f"SpacesReport({self.as_dict()})"


def workspace_bytes(n_ids: int, spaces_per_block: int) -> int:
    return int(lib.stormck_spaces_workspace_bytes(n_ids, spaces_per_block))


def results_numpy(results) -> np.ndarray:
    """A device call's results as RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(RESULT_DTYPE)


def roots(record):
    """((key root, key root type), (object root, object root type)) of a FOUND record: what
    keystore.get_object_ids_* and objectstore.get_objects_* take as root and root_type."""
    if int(record["status"]) != FOUND:
        raise ValueError("the space does not exist")
    k, o = record["key_root"], record["object_root"]
    return (((int(k["checksum"]), int(k["address"]), int(k["birth_revision"])), int(record["key_type"])),
            ((int(o["checksum"]), int(o["address"]), int(o["birth_revision"])), int(record["object_type"])))


def _table(layout: ScrubLayout, addressing_offsets) -> np.ndarray:
    table = np.ascontiguousarray(addressing_offsets, dtype=np.uint16).reshape(-1)
    if table.size < min(layout.spaces_per_block, MAX_SPACES):
        raise ValueError("addressing_offsets is shorter than layout.spaces_per_block")
    return table


def _report(rc: int, raw: SpacesReportStruct) -> SpacesReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return SpacesReport(raw, rc, _lib.last_error() if rc else "")


def get_spaces_device(store, layout: ScrubLayout, root, root_type: int, addressing_offsets, ids,
                      verify_leaves: bool = True, stream: int = 0, workspace=None):
    """The spaces of `ids` (a contiguous 1-d int64 CUDA tensor) in the space tree at `root`
    ((checksum, address, birth revision) or a Pointer) of block type `root_type` in the
    device-resident image `store` (a CUDA tensor or a raw device pointer). Queued on `stream`
    (0: the null stream); returns when the results are written. `workspace`: a device tensor to
    reuse."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if (not isinstance(ids, torch.Tensor) or not ids.is_cuda or not ids.is_contiguous() or ids.dim() != 1 or
            ids.element_size() != 8 or ids.is_floating_point()):
        raise ValueError("ids must be a contiguous 1-d CUDA tensor of 64-bit integers")
    table = _table(layout, addressing_offsets)
    n = ids.numel()
    need = workspace_bytes(n, layout.spaces_per_block)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 11), dtype=torch.int64, device=device)
    raw = SpacesReportStruct()
    r = _root(root)
    rc = lib.stormck_spaces_device(d_store, ctypes.byref(layout), ctypes.byref(r), root_type, table.ctypes.data,
                                   ids.data_ptr(), n, 0 if verify_leaves else LEAVES_UNVERIFIED, results.data_ptr(),
                                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), ctypes.byref(raw),
                                   stream or None)
    return results, _report(rc, raw)


def get_spaces_host(buffer, layout: ScrubLayout, root, root_type: int, addressing_offsets, ids,
                    verify_leaves: bool = True, threads: int = 0):
    """The same over an image in host memory. `ids` is a 1-d uint64 numpy array; needs no device."""
    buf = buffer if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, dtype=np.uint8)
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
    table = _table(layout, addressing_offsets)
    n = ids.size
    results = np.zeros(n, dtype=RESULT_DTYPE)
    raw = SpacesReportStruct()
    r = _root(root)
    rc = lib.stormck_spaces_host(buf.ctypes.data, ctypes.byref(layout), ctypes.byref(r), root_type, table.ctypes.data,
                                 ids.ctypes.data if n else None, n, 0 if verify_leaves else LEAVES_UNVERIFIED,
                                 results.ctypes.data if n else None, ctypes.byref(raw), threads)
    return results, _report(rc, raw)
