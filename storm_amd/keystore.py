"""Lookup: keystore.GetObjectID for many keys at once (include/stormck.h "lookup", DESIGN.md
"Lookup").

storm hashes a key to a tag, traces the tag down to its objectlist leaf and probes that leaf by
open addressing for the key's object ID. ``get_object_ids_device`` does the three stages for a
batch of keys in one call on an image that lives in HBM: the key-tag launch, the trace's engine
and ``k_lookup_probe`` with one lane per key. ``get_object_ids_host`` is the same over an image
in host memory on the library's host threads and needs no device.

Keys are addressed as in ``engine.key_tags_device``: a (n, stride) byte array whose rows hold
one key each (``length`` bytes of every row, default the whole row; or ``lens`` per row), or a
flat byte array with ``offsets`` and ``lens``.

Every call returns ``(results, report)``: one ``RESULT_DTYPE`` record per key, in the keys'
order (a numpy structured array from the host leg; from the device an int64 tensor of shape
(n, 4) that ``results_numpy`` views as the same records), and a :class:`LookupReport`. A
damaged tree or a key of a length storm refuses raises nothing: the statuses and the report say
what is wrong. Exceptions are for bad arguments and HIP errors.

The library ships no addressing table (storm's comes from Go's math/rand): the caller passes
``objectlist.AddressingOffsets`` in :class:`ObjectListParams`.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, trace
from ._lib import LookupReportStruct, LookupResultStruct, ObjectListParamsStruct, lib
from .scrub import ScrubLayout, _root
from .trace import ABSENT, DEPTH, FOUND, LEAVES_UNVERIFIED, MISMATCH, RANGE, TYPE  # noqa: F401  (for callers)

KEY = 7                  # STORMCK_LOOKUP_KEY
NO_SLOT = 2 ** 32 - 1    # STORMCK_LOOKUP_NO_SLOT
MAX_KEY = 256            # objectlist.MaxKeyComponentLength
STATUS_NAMES = {**trace.STATUS_NAMES, KEY: "key"}
BAD = trace.BAD + (KEY,)

RESULT_DTYPE = np.dtype([("object_id", "<u8"), ("address", "<u8"), ("reminder", "<u8"), ("index", "<u4"),
                         ("probes", "<u2"), ("status", "u1"), ("reserved", "u1")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(LookupResultStruct) == 32


def leaf_len(chunks_per_block: int) -> int:
    """Bytes of objectlist.Block with that many chunks."""
    return (53 * chunks_per_block + 4 + 7) & ~7


class ObjectListParams:
    """stormck_objectlist_params: ``addressing_offsets`` is objectlist.AddressingOffsets, a
    permutation of 0..chunks_per_block-1 (the library checks it)."""

    def __init__(self, addressing_offsets, chunks_per_block=None):
        self.table = np.ascontiguousarray(addressing_offsets, dtype=np.uint16).reshape(-1)
        self.chunks_per_block = self.table.size if chunks_per_block is None else int(chunks_per_block)
        if self.table.size < min(self.chunks_per_block, 4096):
            raise ValueError("addressing_offsets is shorter than chunks_per_block")
        self.raw = ObjectListParamsStruct(self.table.ctypes.data, self.chunks_per_block, 0)

    @property
    def leaf_len(self) -> int:
        return leaf_len(self.chunks_per_block)


class LookupReport:
    """stormck_lookup_report; ``trace`` is the trace's report (a trace.TraceReport)."""

    FIELDS = ("n_status", "n_probed", "probes", "n_malformed", "first_bad")

    def __init__(self, raw: LookupReportStruct, code: int, message: str, trace_results=None, tags=None):
        self.trace = trace.TraceReport(raw.trace, _lib.OK, "")
        self.n_status = tuple(int(v) for v in raw.n_status)
        self.n_probed, self.probes = int(raw.n_probed), int(raw.probes)
        self.n_malformed, self.first_bad = int(raw.n_malformed), int(raw.first_bad)
        self.code = code          # STORMCK_OK or STORMCK_EMISMATCH
        self.message = message    # the text of key first_bad's error ("" when there is none)
        self.trace_results = trace_results  # when asked for: the trace's results (trace.RESULT_DTYPE)
        self.tags = tags                    # ... and the keys' tags

    @property
    def ok(self) -> bool:
        return self.code == _lib.OK

    def as_dict(self) -> dict:
        return dict({f: getattr(self, f) for f in self.FIELDS}, trace=self.trace.as_dict())

    def __repr__(self) -> str:
        return f"LookupReport({self.as_dict()})"


def workspace_bytes(n_keys: int, chunks_per_block: int) -> int:
    return int(lib.stormck_lookup_workspace_bytes(n_keys, chunks_per_block))


def results_numpy(results) -> np.ndarray:
    """A device call's results as RESULT_DTYPE records on the host."""
    return results.cpu().numpy().reshape(-1).view(RESULT_DTYPE)


def _report(rc: int, raw: LookupReportStruct, trace_results, tags) -> LookupReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return LookupReport(raw, rc, _lib.last_error() if rc else "", trace_results, tags)


def _addressing(shape, offsets, lens, length):
    """(n, stride, uniform length) of a key array of `shape` addressed by offsets / lens / length."""
    if offsets is not None:
        if lens is None:
            raise ValueError("offsets need lens")
        return len(offsets), 0, 0
    if len(shape) != 2:
        raise ValueError("keys must be (n, stride) bytes, or flat bytes with offsets and lens")
    n, stride = shape
    if lens is not None and len(lens) != n:
        raise ValueError("lens must have one entry per key")
    return n, stride, stride if length is None else int(length)


def get_object_ids_device(store, layout: ScrubLayout, root, root_type: int, params: ObjectListParams, keys,
                          offsets=None, lens=None, length=None, verify_leaves: bool = True, stream: int = 0,
                          workspace=None, want_trace: bool = False):
    """Object IDs of `keys` (a contiguous uint8 CUDA tensor) in the key tree at `root` ((checksum,
    address, birth revision) or a Pointer) of block type `root_type` in the device-resident image
    `store` (a CUDA tensor or a raw device pointer). `offsets` (int64) and `lens` (int32) are
    CUDA tensors. Queued on `stream` (0: the null stream) behind what is there; returns when the
    results are written. verify_leaves=False probes the leaves without hashing them.
    want_trace: the report carries the trace's results and the tags as tensors.
    `workspace`: a device tensor to reuse."""
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
    for name, t, size in (("offsets", offsets, 8), ("lens", lens, 4)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or
                              t.element_size() != size or t.is_floating_point() or t.dim() != 1):
            raise ValueError(f"{name} must be a contiguous 1-d CUDA tensor of {size}-byte integers")
    n, stride, length = _addressing(tuple(keys.shape), offsets, lens, length)
    need = workspace_bytes(n, params.chunks_per_block)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    results = torch.empty((n, 4), dtype=torch.int64, device=device)
    tres = torch.empty((n, 4), dtype=torch.int64, device=device) if want_trace else None
    tags = torch.empty(n, dtype=torch.int64, device=device) if want_trace else None
    raw = LookupReportStruct()
    r = _root(root)
    rc = lib.stormck_lookup_device(d_store, ctypes.byref(layout), ctypes.byref(r), root_type, ctypes.byref(params.raw),
                                   keys.data_ptr(), stride, offsets.data_ptr() if offsets is not None else None,
                                   lens.data_ptr() if lens is not None else None, length, n,
                                   0 if verify_leaves else LEAVES_UNVERIFIED, results.data_ptr(),
                                   tres.data_ptr() if want_trace else None, tags.data_ptr() if want_trace else None,
                                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), ctypes.byref(raw),
                                   stream or None)
    return results, _report(rc, raw, tres, tags)


def get_object_ids_host(buffer, layout: ScrubLayout, root, root_type: int, params: ObjectListParams, keys,
                        offsets=None, lens=None, length=None, verify_leaves: bool = True, threads: int = 0,
                        want_trace: bool = False):
    """The same lookup over an image in host memory, on `threads` library pool threads (0: the
    pool). `keys` is a uint8 numpy array; needs no device."""
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
    results = np.zeros(n, dtype=RESULT_DTYPE)
    tres = np.zeros(n, dtype=trace.RESULT_DTYPE) if want_trace else None
    tags = np.zeros(n, dtype=np.uint64) if want_trace else None
    raw = LookupReportStruct()
    r = _root(root)
    rc = lib.stormck_lookup_host(buf.ctypes.data, ctypes.byref(layout), ctypes.byref(r), root_type,
                                 ctypes.byref(params.raw), keys.ctypes.data, stride,
                                 offsets.ctypes.data if offsets is not None else None,
                                 lens.ctypes.data if lens is not None else None, length, n,
                                 0 if verify_leaves else LEAVES_UNVERIFIED, results.ctypes.data,
                                 tres.ctypes.data if want_trace else None, tags.ctypes.data if want_trace else None,
                                 ctypes.byref(raw), threads)
    return results, _report(rc, raw, tres, tags)
