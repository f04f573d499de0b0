"""The argument-error table of the host-memory batch entry points (include/stormck.h):
stormck_checksum_host / _verify_host, the _multi pair, the _host_leg pair, the routed
_batch pair and the _split pair.

Each row is one call with a single defect (or none): the status it must return, the
message stormck_last_error() must hold, and for the verify entries what *first_bad and
*n_bad hold afterwards (both are set to SENTINEL before the call). EXPECTED was recorded
from the library as it stood before the entry points were given one shared validation, and
is a literal on purpose: the shared validation has to reproduce it, row for row.

tests/test_host_batch.py runs the _host_leg rows (no device needed);
tests/test_host_stage_gpu.py runs the others.
"""
import ctypes

import numpy as np

from oracle import oracle as o
from storm_amd import _lib

SENTINEL = 77
BIG_STRIDE = (256 << 20) + 8  # one block step past the 256 MiB staging chunk

# entry -> (verify, takes a device list, split)
ENTRIES = {
    "stormck_checksum_host": (False, False, False),
    "stormck_verify_host": (True, False, False),
    "stormck_checksum_host_multi": (False, True, False),
    "stormck_verify_host_multi": (True, True, False),
    "stormck_checksum_host_leg": (False, False, False),
    "stormck_verify_host_leg": (True, False, False),
    "stormck_checksum_batch": (False, False, False),
    "stormck_verify_batch": (True, False, False),
    "stormck_checksum_split": (False, True, True),
    "stormck_verify_split": (True, True, True),
}
HOST_LEG = ("stormck_checksum_host_leg", "stormck_verify_host_leg")

CASES = ("valid", "null_base", "null_out_or_expected", "null_first_bad", "null_n_bad", "overlap_uniform",
         "overlap_lens", "stride_over_chunk", "device_base", "n_zero", "devices_empty", "devices_65",
         "devices_minus_1")


def cases_of(entry):
    verify, has_list, _ = ENTRIES[entry]
    for c in CASES:
        if c in ("null_first_bad", "null_n_bad") and not verify:
            continue
        if c.startswith("devices_") and not has_list:
            continue
        yield c


def buffer_bytes():
    return BIG_STRIDE + 4096


def run_case(entry, case, buf, device_ptr=None):
    """One call of `entry` with the defect `case` on the host buffer `buf` (zeros, at least
    buffer_bytes() long; registered for the split entries). Returns (status, message,
    first_bad, n_bad): the message only of a failing call, the last two only of a verify
    entry (None where the defect is that pointer itself)."""
    verify, has_list, split = ENTRIES[entry]
    base, stride, length, n = buf.ctypes.data, 64, 64, 2
    lens = None
    if case == "null_base":
        base = None
    elif case == "overlap_uniform":
        length = 128
    elif case == "overlap_lens":
        lens, length, n = np.array([8, 128, 8], dtype=np.uint32), 0, 3
    elif case == "stride_over_chunk":
        stride, length = BIG_STRIDE, 8
    elif case == "device_base":
        base = device_ptr
    elif case == "n_zero":
        n = 0
    out = np.zeros(max(n, 1), dtype=np.uint64)
    # what the blocks of the valid calls hash to (zeros), so that they verify
    exp = o.checksum_batch(buf, n, stride, length) if case in ("valid", "stride_over_chunk") else out.copy()
    fb, nb = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    res = exp.ctypes.data if verify else out.ctypes.data
    if case == "null_out_or_expected":
        res = None
    args = [base, stride, lens.ctypes.data if lens is not None else None, length, n, res]
    if verify:
        args += [None if case == "null_first_bad" else ctypes.addressof(fb),
                 None if case == "null_n_bad" else ctypes.addressof(nb)]
    if has_list:
        devs = {"devices_empty": [], "devices_65": [0] * 65, "devices_minus_1": [-1]}.get(case, [0])
        arr = (ctypes.c_int * max(len(devs), 1))(*devs)
        args += [ctypes.cast(arr, ctypes.c_void_p), len(devs)]
    if split:
        args += [0, 1, None]  # host_threads, device_blocks, device_done
    elif entry in HOST_LEG:
        args += [0]  # threads
    elif entry.endswith("_batch"):
        args += [0, None]  # host_threads, leg_used
    rc = getattr(_lib.lib, entry)(*args)
    msg = _lib.last_error() if rc else ""
    if not verify:
        return rc, msg, None, None
    return (rc, msg, None if case == "null_first_bad" else fb.value, None if case == "null_n_bad" else nb.value)


# (entry, case) -> (status, message, first_bad, n_bad)
EXPECTED = {
    ('stormck_checksum_host', 'valid'): (0, '', None, None),
    ('stormck_checksum_host', 'null_base'): (-1, 'base is null', None, None),
    ('stormck_checksum_host', 'null_out_or_expected'): (-1, 'out is null', None, None),
    ('stormck_checksum_host', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', None, None),
    ('stormck_checksum_host', 'device_base'): (-1, 'base is device memory: use the _device entry points', None, None),
    ('stormck_checksum_host', 'n_zero'): (0, '', None, None),
    ('stormck_verify_host', 'valid'): (0, '', 2, 0),
    ('stormck_verify_host', 'null_base'): (-1, 'base is null', 77, 77),
    ('stormck_verify_host', 'null_out_or_expected'): (-1, 'null argument', 77, 77),
    ('stormck_verify_host', 'null_first_bad'): (-1, 'null argument', None, 77),
    ('stormck_verify_host', 'null_n_bad'): (-1, 'null argument', 77, None),
    ('stormck_verify_host', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_host', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_host', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', 77, 77),
    ('stormck_verify_host', 'device_base'): (-1, 'base is device memory: use the _device entry points', 77, 77),
    ('stormck_verify_host', 'n_zero'): (0, '', 0, 0),
    ('stormck_checksum_host_multi', 'valid'): (0, '', None, None),
    ('stormck_checksum_host_multi', 'null_base'): (-1, 'base is null', None, None),
    ('stormck_checksum_host_multi', 'null_out_or_expected'): (-1, 'out is null', None, None),
    ('stormck_checksum_host_multi', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host_multi', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host_multi', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', None, None),
    ('stormck_checksum_host_multi', 'device_base'): (-1, 'base is device memory: use the _device entry points', None, None),
    ('stormck_checksum_host_multi', 'n_zero'): (0, '', None, None),
    ('stormck_checksum_host_multi', 'devices_empty'): (-1, 'devices: 1..64 entries', None, None),
    ('stormck_checksum_host_multi', 'devices_65'): (-1, 'devices: 1..64 entries', None, None),
    ('stormck_checksum_host_multi', 'devices_minus_1'): (-1, 'devices[0] = -1 is not a visible device', None, None),
    ('stormck_verify_host_multi', 'valid'): (0, '', 2, 0),
    ('stormck_verify_host_multi', 'null_base'): (-1, 'base is null', 77, 77),
    ('stormck_verify_host_multi', 'null_out_or_expected'): (-1, 'null argument', 77, 77),
    ('stormck_verify_host_multi', 'null_first_bad'): (-1, 'null argument', None, 77),
    ('stormck_verify_host_multi', 'null_n_bad'): (-1, 'null argument', 77, None),
    ('stormck_verify_host_multi', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_host_multi', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_host_multi', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', 77, 77),
    ('stormck_verify_host_multi', 'device_base'): (-1, 'base is device memory: use the _device entry points', 77, 77),
    ('stormck_verify_host_multi', 'n_zero'): (0, '', 0, 0),
    ('stormck_verify_host_multi', 'devices_empty'): (-1, 'devices: 1..64 entries', 77, 77),
    ('stormck_verify_host_multi', 'devices_65'): (-1, 'devices: 1..64 entries', 77, 77),
    ('stormck_verify_host_multi', 'devices_minus_1'): (-1, 'devices[0] = -1 is not a visible device', 77, 77),
    ('stormck_checksum_host_leg', 'valid'): (0, '', None, None),
    ('stormck_checksum_host_leg', 'null_base'): (-1, 'base is null', None, None),
    ('stormck_checksum_host_leg', 'null_out_or_expected'): (-1, 'null argument', None, None),
    ('stormck_checksum_host_leg', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host_leg', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_host_leg', 'stride_over_chunk'): (0, '', None, None),
    ('stormck_checksum_host_leg', 'n_zero'): (0, '', None, None),
    ('stormck_checksum_host_leg', 'device_base'): (-1, 'base is not readable host memory', None, None),
    ('stormck_verify_host_leg', 'valid'): (0, '', 2, 0),
    ('stormck_verify_host_leg', 'null_base'): (-1, 'base is null', 2, 0),
    ('stormck_verify_host_leg', 'null_out_or_expected'): (-1, 'null argument', 2, 0),
    ('stormck_verify_host_leg', 'null_first_bad'): (-1, 'null argument', None, 77),
    ('stormck_verify_host_leg', 'null_n_bad'): (-1, 'null argument', 77, None),
    ('stormck_verify_host_leg', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', 2, 0),
    ('stormck_verify_host_leg', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', 3, 0),
    ('stormck_verify_host_leg', 'stride_over_chunk'): (0, '', 2, 0),
    ('stormck_verify_host_leg', 'n_zero'): (0, '', 0, 0),
    ('stormck_verify_host_leg', 'device_base'): (-1, 'base is not readable host memory', 2, 0),
    ('stormck_checksum_batch', 'valid'): (0, '', None, None),
    ('stormck_checksum_batch', 'null_base'): (-1, 'base is null', None, None),
    ('stormck_checksum_batch', 'null_out_or_expected'): (-1, 'null argument', None, None),
    ('stormck_checksum_batch', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_batch', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_batch', 'stride_over_chunk'): (0, '', None, None),
    ('stormck_checksum_batch', 'device_base'): (-1, 'base is device memory: use the _device entry points', None, None),
    ('stormck_checksum_batch', 'n_zero'): (0, '', None, None),
    ('stormck_verify_batch', 'valid'): (0, '', 2, 0),
    ('stormck_verify_batch', 'null_base'): (-1, 'base is null', 77, 77),
    ('stormck_verify_batch', 'null_out_or_expected'): (-1, 'null argument', 77, 77),
    ('stormck_verify_batch', 'null_first_bad'): (-1, 'null argument', None, 77),
    ('stormck_verify_batch', 'null_n_bad'): (-1, 'null argument', 77, None),
    ('stormck_verify_batch', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_batch', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_batch', 'stride_over_chunk'): (0, '', 2, 0),
    ('stormck_verify_batch', 'device_base'): (-1, 'base is device memory: use the _device entry points', 77, 77),
    ('stormck_verify_batch', 'n_zero'): (0, '', 0, 0),
    ('stormck_checksum_split', 'valid'): (0, '', None, None),
    ('stormck_checksum_split', 'null_base'): (-1, 'base is null', None, None),
    ('stormck_checksum_split', 'null_out_or_expected'): (-1, 'null argument', None, None),
    ('stormck_checksum_split', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_split', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', None, None),
    ('stormck_checksum_split', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', None, None),
    ('stormck_checksum_split', 'device_base'): (-1, 'base is device memory: use the _device entry points', None, None),
    ('stormck_checksum_split', 'n_zero'): (0, '', None, None),
    ('stormck_checksum_split', 'devices_empty'): (-1, 'devices: 1..64 entries', None, None),
    ('stormck_checksum_split', 'devices_65'): (-1, 'devices: 1..64 entries', None, None),
    ('stormck_checksum_split', 'devices_minus_1'): (-1, 'devices[0] = -1 is not a visible device', None, None),
    ('stormck_verify_split', 'valid'): (0, '', 2, 0),
    ('stormck_verify_split', 'null_base'): (-1, 'base is null', 77, 77),
    ('stormck_verify_split', 'null_out_or_expected'): (-1, 'null argument', 77, 77),
    ('stormck_verify_split', 'null_first_bad'): (-1, 'null argument', None, 77),
    ('stormck_verify_split', 'null_n_bad'): (-1, 'null argument', 77, None),
    ('stormck_verify_split', 'overlap_uniform'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_split', 'overlap_lens'): (-1, 'stride smaller than a block length (blocks overlap)', 77, 77),
    ('stormck_verify_split', 'stride_over_chunk'): (-1, 'block stride exceeds the staging chunk (256 MiB)', 77, 77),
    ('stormck_verify_split', 'device_base'): (-1, 'base is device memory: use the _device entry points', 77, 77),
    ('stormck_verify_split', 'n_zero'): (0, '', 0, 0),
    ('stormck_verify_split', 'devices_empty'): (-1, 'devices: 1..64 entries', 77, 77),
    ('stormck_verify_split', 'devices_65'): (-1, 'devices: 1..64 entries', 77, 77),
    ('stormck_verify_split', 'devices_minus_1'): (-1, 'devices[0] = -1 is not a visible device', 77, 77),
}
