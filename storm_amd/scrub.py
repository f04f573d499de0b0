"""Scrub: walk a committed snapshot from its singularity block and verify every
reachable block (include/stormck.h "scrub", DESIGN.md "Scrub").

In storm a block's expected checksum lives in its parent, so integrity of a snapshot is a
level-synchronous descent, the mirror image of the commit. ``scrub_device`` walks an
image that lives in HBM (frontier levels hashed by the library's batch dispatch,
expanded by ``k_scrub_expand``); ``scrub_host`` walks the same image in host memory on
the library's host threads and needs no device. Both return a :class:`ScrubReport` and
raise nothing on a damaged store: the report says what is wrong. Exceptions are for bad
arguments and HIP errors.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple, Union

import numpy as np

from . import _lib
from ._lib import PointerStruct, ScrubLayoutStruct, ScrubReportStruct, lib

# STORMCK_SCRUB_* block kinds and error codes
POINTER, SPACELIST, OBJECTLIST, BLOB = 0, 1, 2, 3
KIND_NAMES = ("pointer", "spacelist", "objectlist", "blob")
OK, MISMATCH, RANGE, TYPE, DUPLICATE = 0, 1, 2, 3, 4
ERROR_NAMES = ("ok", "mismatch", "range", "type", "duplicate")


class ScrubLayout(ScrubLayoutStruct):
    """stormck_scrub_layout: block `a` lives at base + a * block_size."""

    @classmethod
    def production(cls, n_blocks: int) -> "ScrubLayout":
        """storm's production constants (blocks/*/params.go)."""
        return cls(32768, n_blocks, 1200, 400, 31808, 32768)

    @classmethod
    def test_tag(cls, n_blocks: int) -> "ScrubLayout":
        """The `-tags test` constants (params_testing.go)."""
        return cls(32768, n_blocks, 10, 10, 536, 32768)

    def image_bytes(self) -> int:
        return self.block_size * self.n_blocks

    def bitmap_words(self) -> int:
        return (self.n_blocks + 31) // 32


class ScrubReport:
    """stormck_scrub_report, with the reachable bitmap when it was asked for
    (``reachable``: numpy uint32 words on the host, or an int32 tensor on the device)."""

    FIELDS = ("verified", "bytes_hashed", "n_mismatch", "n_structural", "levels", "first_error", "first_level",
              "first_slot", "first_parent", "first_address", "first_computed", "first_expected")

    def __init__(self, raw: ScrubReportStruct, code: int, message: str, reachable=None):
        self.verified = tuple(int(v) for v in raw.verified)
        for f in self.FIELDS[1:]:
            setattr(self, f, int(getattr(raw, f)))
        self.code = code          # STORMCK_OK or STORMCK_EMISMATCH
        self.message = message    # storm-format text of the first error ("" when intact)
        self.reachable = reachable

    @property
    def ok(self) -> bool:
        return self.n_mismatch + self.n_structural == 0

    @property
    def first_error_name(self) -> str:
        return ERROR_NAMES[self.first_error]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self) -> str:
        return f"ScrubReport({self.as_dict()})"


def workspace_bytes(n_blocks: int) -> int:
    return int(lib.stormck_scrub_workspace_bytes(n_blocks))


def _report(rc: int, raw: ScrubReportStruct, reachable) -> ScrubReport:
    if rc not in (_lib.OK, _lib.EMISMATCH):
        _lib.check(rc)
    return ScrubReport(raw, rc, _lib.last_error() if rc else "", reachable)


def _root(root: Union[PointerStruct, Tuple[int, int, int]]) -> PointerStruct:
    return root if isinstance(root, PointerStruct) else PointerStruct(*root)


def _device_args(store, layout: ScrubLayout, reachable: bool, workspace):
    """(d_store, torch device or None, workspace tensor, bitmap tensor or None)."""
    import torch
    if isinstance(store, torch.Tensor):
        if not store.is_cuda or not store.is_contiguous():
            raise ValueError("store must be a contiguous CUDA tensor")
        if store.numel() * store.element_size() < layout.image_bytes():
            raise ValueError("store tensor is smaller than n_blocks * block_size")
        d_store, device = store.data_ptr(), store.device
    else:
        d_store, device = int(store), torch.device("cuda", torch.cuda.current_device())
    need = workspace_bytes(layout.n_blocks)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    bitmap = torch.empty(layout.bitmap_words(), dtype=torch.int32, device=device) if reachable else None
    return d_store, workspace, bitmap


def scrub_device(store, layout: ScrubLayout, stream: int = 0, reachable: bool = False, workspace=None) -> ScrubReport:
    """Scrub the device-resident image `store` (a CUDA tensor or a raw device pointer) from
    its singularity. Queued on `stream` (0: the null stream) behind what is there;
    returns when the walk has finished. `workspace`: a device tensor to reuse."""
    d_store, workspace, bitmap = _device_args(store, layout, reachable, workspace)
    raw = ScrubReportStruct()
    rc = lib.stormck_scrub_device(d_store, ctypes.byref(layout), workspace.data_ptr(),
                                  workspace.numel() * workspace.element_size(),
                                  bitmap.data_ptr() if reachable else None, ctypes.byref(raw), stream or None)
    return _report(rc, raw, bitmap)


def scrub_tree_device(store, layout: ScrubLayout, root, root_type: int, leaf_kind: int, leaf_len: int = 0,
                      stream: int = 0, reachable: bool = False, workspace=None) -> ScrubReport:
    """One tree from an explicit root ((checksum, address, birth revision) or a Pointer) of
    block type `root_type`; its leaves are `leaf_kind`, hashed over `leaf_len` bytes (0:
    the layout's length for that kind)."""
    d_store, workspace, bitmap = _device_args(store, layout, reachable, workspace)
    raw = ScrubReportStruct()
    r = _root(root)
    rc = lib.stormck_scrub_tree_device(d_store, ctypes.byref(layout), ctypes.byref(r), root_type, leaf_kind, leaf_len,
                                       workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                       bitmap.data_ptr() if reachable else None, ctypes.byref(raw), stream or None)
    return _report(rc, raw, bitmap)


def _host_args(buffer, layout: ScrubLayout, reachable: bool):
    buf = buffer if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, dtype=np.uint8)
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if buf.size < layout.image_bytes():
        raise ValueError("buffer is smaller than n_blocks * block_size")
    bitmap: Optional[np.ndarray] = np.zeros(layout.bitmap_words(), dtype=np.uint32) if reachable else None
    return buf, bitmap


def scrub_host(buffer, layout: ScrubLayout, threads: int = 0, reachable: bool = False) -> ScrubReport:
    """The same walk over an image in host memory, each level hashed on `threads` library
    pool threads (0: the pool). Needs no device."""
    buf, bitmap = _host_args(buffer, layout, reachable)
    raw = ScrubReportStruct()
    rc = lib.stormck_scrub_host(buf.ctypes.data, ctypes.byref(layout), bitmap.ctypes.data if reachable else None,
                                ctypes.byref(raw), threads)
    return _report(rc, raw, bitmap)


def scrub_tree_host(buffer, layout: ScrubLayout, root, root_type: int, leaf_kind: int, leaf_len: int = 0,
                    threads: int = 0, reachable: bool = False) -> ScrubReport:
    buf, bitmap = _host_args(buffer, layout, reachable)
    raw = ScrubReportStruct()
    r = _root(root)
    rc = lib.stormck_scrub_tree_host(buf.ctypes.data, ctypes.byref(layout), ctypes.byref(r), root_type, leaf_kind,
                                     leaf_len, bitmap.ctypes.data if reachable else None, ctypes.byref(raw), threads)
    return _report(rc, raw, bitmap)
