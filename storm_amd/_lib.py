"""ctypes binding of libstormck (include/stormck.h).

Loads the in-tree build ``storm_amd/lib/libstormck.so``. There is no fallback:
if the library is missing, importing this module raises; if no gfx950 device is
present, every batched / device compute call raises :class:`NoDeviceError`
(single calls hash on the host by design: include/stormck.h).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_uint8, c_uint32, c_uint64, c_void_p

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libstormck.so")
# STORMCK_LIBRARY=<path>: load another build of the same ABI instead, e.g. the probe build
# tools/libstormck_probes.so (storm_amd/build.py), whose design knobs the product lacks
LIB_PATH = os.environ.get("STORMCK_LIBRARY") or LIB_PATH

OK = 0
EINVAL = -1
EHIP = -2
ENODEV = -3
ENOMEM = -4
EMISMATCH = -5
ENOSPC = -6

# arena placement modes of stormck_device_alloc_placed: the probe build only (measured and
# rejected in round 4; the product allocates with hipMalloc, stormck_device_alloc)
ALLOC_PLAIN = 0
ALLOC_CONTIGUOUS = 2  # (mode 1, a VMM reservation, was deleted in round 6)
# STORMCK_LEG_* (stormck_commit, stormck_checksum_batch, the route plan)
LEG_NONE, LEG_HOST, LEG_DEVICE, LEG_SPLIT = 0, 1, 2, 3
LEG_NAMES = {LEG_NONE: "none", LEG_HOST: "host", LEG_DEVICE: "device", LEG_SPLIT: "split"}
MEM_PAGEABLE, MEM_PINNED = 0, 1  # STORMCK_MEM_*
RATES_LEARN, RATES_FREEZE = 0, 1  # STORMCK_RATES_*
SPLIT_BALANCED = (1 << 64) - 1    # STORMCK_SPLIT_BALANCED


class StormckError(RuntimeError):
    """A libstormck call failed (code < 0)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"stormck error {code}: {msg}")
        self.code = code


class NoDeviceError(StormckError):
    pass


class RouteRates(ctypes.Structure):
    """stormck_route_rates: the routing model's rates (bytes per microsecond) and the
    devices' start latency in a split (microseconds)."""

    _fields_ = [("host_thread", ctypes.c_double), ("host_memory", ctypes.c_double), ("host_cached", ctypes.c_double),
                ("link_pinned", ctypes.c_double), ("link_pageable", ctypes.c_double),
                ("link_inplace", ctypes.c_double), ("device_latency", ctypes.c_double),
                ("observations", c_uint64)]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class PointerStruct(ctypes.Structure):
    """stormck_pointer == blocks.Pointer (/root/reference/blocks/types.go:35-39)."""

    _fields_ = [("Checksum", c_uint64), ("Address", c_uint64), ("BirthRevision", c_uint64)]


class ShardStruct(ctypes.Structure):
    """stormck_shard: one device-resident shard of stormck_merkle_root_multi."""

    _fields_ = [("d_blocks", c_void_p), ("stride", c_uint64), ("n", c_uint64), ("d_checksums", c_void_p),
                ("leaf_addr_base", c_uint64), ("node_addr_base", c_uint64), ("stream", c_void_p),
                ("device", ctypes.c_int32), ("len", c_uint32)]


class ScrubLayoutStruct(ctypes.Structure):
    """stormck_scrub_layout: the image and block sizes a scrub walks with."""

    _fields_ = [("block_size", c_uint64), ("n_blocks", c_uint64), ("pointer_fanout", c_uint32),
                ("spaces_per_block", c_uint32), ("objectlist_len", c_uint32), ("blob_len", c_uint32)]


class ScrubReportStruct(ctypes.Structure):
    """stormck_scrub_report."""

    _fields_ = [("verified", c_uint64 * 4), ("bytes_hashed", c_uint64), ("n_mismatch", c_uint64),
                ("n_structural", c_uint64), ("levels", c_uint32), ("first_error", c_uint32),
                ("first_level", c_uint32), ("first_slot", c_uint32), ("first_parent", c_uint64),
                ("first_address", c_uint64), ("first_computed", c_uint64), ("first_expected", c_uint64)]


class TraceResultStruct(ctypes.Structure):
    """stormck_trace_result: where one tag's walk ended (32 bytes)."""

    _fields_ = [("address", c_uint64), ("reminder", c_uint64), ("parent", c_uint64), ("slot", c_uint32),
                ("depth", ctypes.c_uint16), ("status", c_uint8), ("reserved", c_uint8)]


class TraceReportStruct(ctypes.Structure):
    """stormck_trace_report."""

    _fields_ = [("n_status", c_uint64 * 7), ("blocks_hashed", c_uint64 * 2), ("bytes_hashed", c_uint64),
                ("first_bad", c_uint64), ("levels", c_uint32), ("reserved", c_uint32)]


class ObjectListParamsStruct(ctypes.Structure):
    """stormck_objectlist_params: objectlist.AddressingOffsets (a host pointer) and ChunksPerBlock."""

    _fields_ = [("addressing_offsets", c_void_p), ("chunks_per_block", c_uint32), ("reserved", c_uint32)]


class LookupResultStruct(ctypes.Structure):
    """stormck_lookup_result: one key's object ID and where its lookup ended (32 bytes)."""

    _fields_ = [("object_id", c_uint64), ("address", c_uint64), ("reminder", c_uint64), ("index", c_uint32),
                ("probes", ctypes.c_uint16), ("status", c_uint8), ("reserved", c_uint8)]


class LookupReportStruct(ctypes.Structure):
    """stormck_lookup_report."""

    _fields_ = [("trace", TraceReportStruct), ("n_status", c_uint64 * 8), ("n_probed", c_uint64), ("probes", c_uint64),
                ("n_malformed", c_uint64), ("first_bad", c_uint64)]


class BlobParamsStruct(ctypes.Structure):
    """stormck_blob_params: objectsPerBlock and unsafe.Sizeof(T) of the blob leaves."""

    _fields_ = [("objects_per_block", c_uint32), ("object_size", c_uint32)]


class ObjectResultStruct(ctypes.Structure):
    """stormck_object_result: where one object ID's GetObject ended (32 bytes)."""

    _fields_ = [("object_id", c_uint64), ("address", c_uint64), ("reminder", c_uint64), ("index", c_uint32),
                ("probes", ctypes.c_uint16), ("status", c_uint8), ("reserved", c_uint8)]


class ObjectsReportStruct(ctypes.Structure):
    """stormck_objects_report."""

    _fields_ = [("trace", TraceReportStruct), ("n_status", c_uint64 * 8), ("n_probed", c_uint64), ("probes", c_uint64),
                ("first_bad", c_uint64)]


class SpaceResultStruct(ctypes.Structure):
    """stormck_space_result: one space ID's two tree roots and where its GetSpace ended (88 bytes)."""

    _fields_ = [("key_root", PointerStruct), ("object_root", PointerStruct), ("next_object_id", c_uint64),
                ("address", c_uint64), ("reminder", c_uint64), ("index", c_uint32), ("probes", ctypes.c_uint16),
                ("key_type", c_uint8), ("object_type", c_uint8), ("status", c_uint8), ("reserved", c_uint8 * 7)]


class SpacesReportStruct(ctypes.Structure):
    """stormck_spaces_report."""

    _fields_ = [("trace", TraceReportStruct), ("n_status", c_uint64 * 8), ("n_probed", c_uint64), ("probes", c_uint64),
                ("first_bad", c_uint64)]


class GetParamsStruct(ctypes.Structure):
    """stormck_get_params: the spaces' table (a host pointer), the lookup's params, the objects call's."""

    _fields_ = [("space_offsets", c_void_p), ("keys", ObjectListParamsStruct), ("objects", BlobParamsStruct)]


class GetResultStruct(ctypes.Structure):
    """stormck_get_result: where one key's storm.Get ended (32 bytes)."""

    _fields_ = [("object_id", c_uint64), ("key_address", c_uint64), ("object_address", c_uint64), ("index", c_uint32),
                ("stage", c_uint8), ("status", c_uint8), ("reserved", ctypes.c_uint16)]


class GetReportStruct(ctypes.Structure):
    """stormck_get_report."""

    _fields_ = [("space", SpaceResultStruct), ("lookup", LookupReportStruct), ("n_selected", c_uint64),
                ("n_status", c_uint64 * 8), ("blocks_hashed", c_uint64 * 2), ("bytes_hashed", c_uint64),
                ("probes", c_uint64), ("levels", c_uint32), ("reserved", c_uint32), ("n_found", c_uint64),
                ("first_bad", c_uint64)]


class UpdateResultStruct(ctypes.Structure):
    """stormck_update_result: stormck_get_result with its reserved field split (32 bytes)."""

    _fields_ = [("object_id", c_uint64), ("key_address", c_uint64), ("object_address", c_uint64), ("index", c_uint32),
                ("stage", c_uint8), ("status", c_uint8), ("action", c_uint8), ("reserved", c_uint8)]


class UpdateReportStruct(ctypes.Structure):
    """stormck_update_report."""

    _fields_ = [("get", GetReportStruct), ("n_written", c_uint64), ("n_superseded", c_uint64), ("n_dirty", c_uint64 * 4),
                ("bytes_copied", c_uint64), ("bytes_hashed", c_uint64), ("revision", c_uint64),
                ("last_allocated", c_uint64), ("first_new", c_uint64), ("heights", c_uint32), ("reserved", c_uint32)]


class InsertResultStruct(ctypes.Structure):
    """stormck_insert_result: what the insert did with one key (40 bytes)."""

    _fields_ = [("object_id", c_uint64), ("key_address", c_uint64), ("object_address", c_uint64), ("key_index", c_uint32),
                ("object_index", c_uint32), ("stage", c_uint8), ("status", c_uint8), ("action", c_uint8),
                ("reason", c_uint8), ("wrote", c_uint8), ("reserved", c_uint8 * 3)]


INSERT_REASONS = 10


class InsertReportStruct(ctypes.Structure):
    """stormck_insert_report."""

    _fields_ = [("space", SpaceResultStruct), ("lookup", LookupReportStruct), ("n_inserted", c_uint64),
                ("n_repeated", c_uint64), ("n_none", c_uint64 * INSERT_REASONS), ("first_id", c_uint64),
                ("next_object_id", c_uint64), ("cut", c_uint64), ("limit", c_uint64), ("n_dirty", c_uint64 * 4),
                ("bytes_copied", c_uint64), ("bytes_hashed", c_uint64), ("revision", c_uint64),
                ("last_allocated", c_uint64), ("first_new", c_uint64), ("heights", c_uint32), ("reserved", c_uint32)]


# name -> (restype, argtypes); mirrors include/stormck.h one to one.
SIGNATURES = {
    "stormck_abi_version": (c_int, []),
    "stormck_build_id": (c_char_p, []),
    "stormck_last_error": (c_char_p, []),
    "stormck_device_count": (c_int, [POINTER(c_int)]),
    "stormck_init": (c_int, [c_int]),
    "stormck_shutdown": (None, []),
    "stormck_device_status": (c_int, [c_void_p]),
    "stormck_device_alloc": (c_int, [c_uint64, POINTER(c_void_p)]),
    "stormck_stream_forget": (c_int, [c_void_p]),
    "stormck_device_free": (c_int, [c_void_p]),
    "stormck_checksum_device": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p]),
    "stormck_checksum_gather_device": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p]),
    "stormck_verify_device": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p]),
    "stormck_checksum_host": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p]),
    "stormck_verify_host": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p]),
    "stormck_checksum_host_multi": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_int]),
    "stormck_verify_host_multi": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "stormck_checksum_batch": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_uint32, POINTER(c_uint32)]),
    "stormck_verify_batch": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32,
                POINTER(c_uint32)]),
    "stormck_checksum_host_leg": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_uint32]),
    "stormck_verify_host_leg": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32]),
    "stormck_xxh64": (c_uint64, [c_void_p, c_uint64]),
    "stormck_checksum": (c_int, [c_void_p, c_uint64, POINTER(c_uint64)]),
    "stormck_checksum_gpu": (c_int, [c_void_p, c_uint64, POINTER(c_uint64)]),
    "stormck_host_register": (c_int, [c_void_p, c_uint64]),
    "stormck_host_unregister": (c_int, [c_void_p]),
    "stormck_host_device_pointer": (c_int, [c_void_p, c_void_p]),
    "stormck_pointer_level_device": (c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_uint8, c_uint32, c_void_p, c_void_p]),
    "stormck_pointer_node_device": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "stormck_pack_pointer_blocks_device": (
        c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_uint8, c_uint32, c_void_p, c_uint64, c_void_p]),
    "stormck_merkle_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_merkle_root_device": (
        c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_uint64, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "stormck_shard_plan": (c_int, [c_uint64, c_uint32, c_void_p, c_int, POINTER(ShardStruct), POINTER(c_uint64)]),
    "stormck_merkle_root_multi": (
        c_int, [POINTER(ShardStruct), c_uint32, c_uint64, c_uint64, c_uint32, POINTER(PointerStruct),
                POINTER(c_uint8), POINTER(PointerStruct), POINTER(c_uint8)]),
    "stormck_multi_layout": (
        c_int, [POINTER(ShardStruct), c_uint32, c_void_p, POINTER(c_uint32), POINTER(c_uint32), c_void_p]),
    "stormck_read_verify_fd": (
        c_int, [c_int, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, c_void_p]),
    "stormck_key_tags_device": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p]),
    "stormck_commit_device": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_uint64), c_void_p, c_void_p]),
    "stormck_commit_host": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_uint64), c_void_p, c_uint32]),
    "stormck_commit": (
        c_int, [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_uint64), c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]),
    "stormck_route_get_rates": (c_int, [POINTER(RouteRates)]),
    "stormck_route_set_rates": (c_int, [POINTER(RouteRates), c_uint32]),
    "stormck_route_devices": (c_int, [c_void_p, c_int]),
    "stormck_route_plan_batch": (
        c_int, [c_uint64, c_void_p, c_uint32, c_uint64, c_uint32, c_uint32, c_uint32, POINTER(c_uint32), c_void_p]),
    "stormck_route_plan_commit": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_uint32, POINTER(c_uint32), c_void_p]),
    "stormck_checksum_split": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_int, c_uint32, c_uint64,
                POINTER(c_uint64)]),
    "stormck_verify_split": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                c_uint32, c_uint64, POINTER(c_uint64)]),
    "stormck_commit_split": (
        c_int, [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_uint64), c_void_p, c_void_p, c_int, c_uint32,
                c_uint64, POINTER(c_uint64)]),
    "stormck_scrub_workspace_bytes": (c_uint64, [c_uint64]),
    "stormck_scrub_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_void_p, c_uint64, c_void_p, POINTER(ScrubReportStruct), c_void_p]),
    "stormck_scrub_tree_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_uint32, c_uint32, c_void_p,
                c_uint64, c_void_p, POINTER(ScrubReportStruct), c_void_p]),
    "stormck_scrub_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_void_p, POINTER(ScrubReportStruct), c_uint32]),
    "stormck_scrub_tree_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_uint32, c_uint32, c_void_p,
                POINTER(ScrubReportStruct), c_uint32]),
    "stormck_trace_workspace_bytes": (c_uint64, [c_uint64]),
    "stormck_trace_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_uint32, c_uint32, c_void_p,
                c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, POINTER(TraceReportStruct), c_void_p]),
    "stormck_trace_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_uint32, c_uint32, c_void_p,
                c_uint64, c_uint32, c_void_p, c_void_p, POINTER(TraceReportStruct), c_uint32]),
    "stormck_lookup_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_lookup_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, POINTER(ObjectListParamsStruct),
                c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p,
                c_void_p, c_uint64, POINTER(LookupReportStruct), c_void_p]),
    "stormck_lookup_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, POINTER(ObjectListParamsStruct),
                c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p,
                POINTER(LookupReportStruct), c_uint32]),
    "stormck_objects_workspace_bytes": (c_uint64, [c_uint64]),
    "stormck_objects_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, POINTER(BlobParamsStruct),
                c_void_p, c_uint64, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64,
                POINTER(ObjectsReportStruct), c_void_p]),
    "stormck_objects_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, POINTER(BlobParamsStruct),
                c_void_p, c_uint64, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64, POINTER(ObjectsReportStruct),
                c_uint32]),
    "stormck_spaces_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_spaces_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_void_p, c_void_p, c_uint64,
                c_uint32, c_void_p, c_void_p, c_uint64, POINTER(SpacesReportStruct), c_void_p]),
    "stormck_spaces_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), POINTER(PointerStruct), c_uint8, c_void_p, c_void_p, c_uint64,
                c_uint32, c_void_p, POINTER(SpacesReportStruct), c_uint32]),
    "stormck_get_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_get_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64,
                POINTER(GetReportStruct), c_void_p]),
    "stormck_get_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64, POINTER(GetReportStruct), c_uint32]),
    "stormck_update_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_update_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64,
                POINTER(UpdateReportStruct), c_void_p]),
    "stormck_update_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, c_uint32, c_void_p, POINTER(UpdateReportStruct),
                c_uint32]),
    "stormck_insert_workspace_bytes": (c_uint64, [c_uint64, c_uint32]),
    "stormck_insert_device": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_uint64,
                POINTER(InsertReportStruct), c_void_p]),
    "stormck_insert_host": (
        c_int, [c_void_p, POINTER(ScrubLayoutStruct), c_uint64, POINTER(GetParamsStruct), c_void_p, c_uint64, c_void_p,
                c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, c_uint32, c_void_p, POINTER(InsertReportStruct),
                c_uint32]),
    "stormck_fill_synthetic_device": (c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_uint64, c_void_p]),
}

# Exported by the probe build only (storm_amd/build.py build_probes_lib), bound when present.
PROBE_SIGNATURES = {
    "stormck_device_alloc_placed": (c_int, [c_uint64, c_uint32, c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
}


def _load() -> ctypes.CDLL:
    # One HIP runtime per process: torch's libtorch_hip NEEDs the unversioned
    # "libamdhip64.so", so if libstormck (NEEDED "libamdhip64.so.7") were loaded first,
    # torch would map a second copy of the runtime and the two would contend for the
    # device. Loading torch first lets libstormck bind to torch's runtime by soname.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libstormck not built ({LIB_PATH} missing): run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in PROBE_SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return lib


lib = _load()


def last_error() -> str:
    msg = lib.stormck_last_error()
    return msg.decode() if msg else ""


def check(rc: int) -> None:
    """Raise on a negative libstormck status."""
    if rc == OK:
        return
    if rc == ENODEV:
        raise NoDeviceError(rc, last_error())
    raise StormckError(rc, last_error())


def device_count() -> int:
    c = c_int(0)
    check(lib.stormck_device_count(ctypes.byref(c)))
    return c.value
