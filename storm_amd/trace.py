"""Trace: storm's read path, cache.TraceTagForReading, for many tags at once
(include/stormck.h "trace", DESIGN.md "Trace").

storm walks one tag at a time from a BlockOrigin down the pointer blocks and verifies every
block on the way against the checksum its parent holds. ``trace_device`` walks all the tags
level by level through an image that lives in HBM: per level one hash batch over the distinct
references, then ``k_trace_step`` with one lane per live tag. ``trace_host`` is the same walk
over an image in host memory on the library's host threads and needs no device.
``trace_keys_device`` hashes keys to tags on the device (``engine.key_tags_device``) and traces
them with no host round trip of the tags.

Every call returns ``(results, report)``: one ``RESULT_DTYPE`` record per tag, in the tags'
order (a numpy structured array from the host leg; from the device an int64 tensor of shape
(n, 4) that ``results_numpy`` views as the same records), and a :class:`TraceReport`. A damaged
tree raises nothing: the statuses and the report say what is wrong. Exceptions are for bad
arguments and HIP errors.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._lib import TraceReportStruct, TraceResultStruct, lib
from .scrub import BLOB, OBJECTLIST, POINTER, SPACELIST, ScrubLayout, _root  # noqa: F401  (the kinds, for callers)

# STORMCK_TRACE_* statuses; MISMATCH, RANGE and TYPE have the scrub's numbers
FOUND, MISMATCH, RANGE, TYPE, ABSENT, DEPTH = 0, 1, 2, 3, 5, 6
STATUS_NAMES = {FOUND: "found", MISMATCH: "mismatch", RANGE: "range", TYPE: "type", ABSENT: "absent", DEPTH: "depth"}
BAD = (MISMATCH, RANGE, TYPE, DEPTH)
LEAVES_UNVERIFIED = 1  # STORMCK_TRACE_LEAVES_UNVERIFIED
MAX_DEPTH = 64

RESULT_DTYPE = np.dtype([("address", "<u8"), ("reminder", "<u8"), ("parent", "<u8"), ("slot", "<u4"), ("depth", "<u2"),
                         ("status", "u1"), ("reserved", "u1")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(TraceResultStruct) == 32


class TraceReport:
    """stormck_trace_report. ``leaf_checksums``: per FOUND tag the checksum its parent holds
    for the leaf (numpy uint64, or an int64 tensor on the device), when it was asked for."""

    FIELDS = ("n_status", "blocks_hashed", "bytes_hashed", "first_bad", "levels")

    def __init__(self, raw: TraceReportStruct, code: int, message: str, leaf_checksums=None):
        self.n_status = tuple(int(v) for v in raw.n_status)
        self.blocks_hashed = tuple(int(v) for v in raw.blocks_hashed)
        self.bytes_hashed, self.first_bad, self.levels = int(raw.bytes_hashed), int(raw.first_bad), int(raw.levels)
        self.code = code          # STORMCK_OK or STORMCK_EMISMATCH
        self.message = message    # storm-format text of tag first_bad's error ("" when there is none)
        self.leaf_checksums = leaf_checksums

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self) -> str:
        return f"TraceReport({self.as_dict()})"


def workspace_bytes(n_tags: int) -> int:
    return int(lib.stormck_trace_workspace_bytes(n_tags))


def results_numpy(results) -> np.ndarray:
    """A device call's results as RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(RESULT_DTYPE)


def _report(rc: int, raw: TraceReportStruct, leaf_checksums) -> TraceReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return TraceReport(raw, rc, _lib.last_error() if rc else "", leaf_checksums)


def trace_device(store, layout: ScrubLayout, root, root_type: int, leaf_kind: int, tags, leaf_len: int = 0,
                 verify_leaves: bool = True, stream: int = 0, workspace=None, leaf_checksums: Optional[bool] = None):
    """Trace `tags` (a contiguous int64 or uint64 CUDA tensor) through the tree at `root`
    ((checksum, address, birth revision) or a Pointer) of block type `root_type` in the
    device-resident image `store` (a CUDA tensor or a raw device pointer); the tree's leaves are
    `leaf_kind`, hashed over `leaf_len` bytes (0: the layout's length for that kind). Queued on
    `stream` (0: the null stream) behind what is there; returns when the results are written.
    verify_leaves=False: leaves end FOUND unhashed and the report carries `leaf_checksums`
    (leaf_checksums=True asks for them in any case). `workspace`: a device tensor to reuse."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    if not isinstance(tags, torch.Tensor):
        tags = torch.from_numpy(np.ascontiguousarray(tags, dtype=np.uint64).view(np.int64)).to(device)
    if not tags.is_cuda or not tags.is_contiguous() or tags.element_size() != 8 or tags.is_floating_point():
        raise ValueError("tags must be a contiguous CUDA tensor of 64-bit integers")
    n = tags.numel()
    need = workspace_bytes(n)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 4), dtype=torch.int64, device=device)
    want_cs = (not verify_leaves) if leaf_checksums is None else leaf_checksums
    cs = torch.empty(n, dtype=torch.int64, device=device) if want_cs else None
    raw = TraceReportStruct()
    r = _root(root)
    rc = lib.stormck_trace_device(d_store, ctypes.byref(layout), ctypes.byref(r), root_type, leaf_kind, leaf_len,
                                  tags.data_ptr(), n, 0 if verify_leaves else LEAVES_UNVERIFIED, results.data_ptr(),
                                  cs.data_ptr() if want_cs else None, workspace.data_ptr(),
                                  workspace.numel() * workspace.element_size(), ctypes.byref(raw), stream or None)
    return results, _report(rc, raw, cs)


def trace_keys_device(store, layout: ScrubLayout, root, root_type: int, keys, leaf_kind: int = OBJECTLIST,
                      leaf_len: int = 0, verify_leaves: bool = True, stream: int = 0, workspace=None,
                      leaf_checksums: Optional[bool] = None):
    """keystore's lookup of many keys: `keys` is a contiguous uint8 CUDA tensor of shape
    (n, key length); the tags, xxhash.Sum64(key), are computed on the device into a tensor that
    feeds trace_device on the same stream. Returns (results, report, tags)."""
    import torch
    from . import engine
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or not keys.is_contiguous() or keys.dim() != 2 or \
            keys.element_size() != 1:
        raise ValueError("keys must be a contiguous CUDA byte tensor of shape (n, key length)")
    n, length = keys.shape
    tags = torch.empty(n, dtype=torch.int64, device=keys.device)
    engine.key_tags_device(keys.data_ptr(), n, tags.data_ptr(), stride=length, length=length, stream=stream)
    results, report = trace_device(store, layout, root, root_type, leaf_kind, tags, leaf_len, verify_leaves, stream,
                                   workspace, leaf_checksums)
    return results, report, tags


def trace_host(buffer, layout: ScrubLayout, root, root_type: int, leaf_kind: int, tags, leaf_len: int = 0,
               verify_leaves: bool = True, threads: int = 0, leaf_checksums: Optional[bool] = None):
    """The same trace over an image in host memory, each level's distinct blocks hashed on
    `threads` library pool threads (0: the pool). Needs no device."""
    buf = buffer if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, dtype=np.uint8)
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    if isinstance(tags, np.ndarray) and tags.dtype == np.int64:
        tags = tags.view(np.uint64)
    tags = np.ascontiguousarray(tags, dtype=np.uint64).reshape(-1)
    n = tags.size
    results = np.zeros(n, dtype=RESULT_DTYPE)
    want_cs = (not verify_leaves) if leaf_checksums is None else leaf_checksums
    cs = np.zeros(n, dtype=np.uint64) if want_cs else None
    raw = TraceReportStruct()
    r = _root(root)
    rc = lib.stormck_trace_host(buf.ctypes.data, ctypes.byref(layout), ctypes.byref(r), root_type, leaf_kind, leaf_len,
                                tags.ctypes.data, n, 0 if verify_leaves else LEAVES_UNVERIFIED, results.ctypes.data,
                                cs.ctypes.data if want_cs else None, ctypes.byref(raw), threads)
    return results, _report(rc, raw, cs)
