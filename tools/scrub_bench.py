#!/usr/bin/env python3
"""Time a whole-tree scrub against its hash-only floor on one MI355X.

    python tools/scrub_bench.py [--leaves 1048576] [--reps 10] [--warmup 3] [--out FILE]

Builds a resident tree entirely on the device with existing entry points (synthetic 32 KiB
leaves at addresses 1..n, their checksums, every pointer level packed into the image behind
them, fanout 1200), then times, with HIP events around warmed repeats in one process on one
arena, alternating the two:
  (a) stormck_scrub_tree_device from the root;
  (b) one stormck_checksum_gather_device call over exactly the same offsets and lengths:
      existing code, and the floor a scrub cannot beat (it hashes the same bytes).
Prints one JSON line: both times, their ratio, GiB/s of each, and the scrub's report. The
yardstick is (b) here, not an earlier scrub number and not the HBM peak.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x53544F524D
BS, F, REV = 32768, 1200, 3
POINTER_LEN = (25 * F + 7) & ~7


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from storm_amd import engine, scrub

    n = args.leaves
    levels = []  # (first address, nodes) of every pointer level, bottom-up
    m, addr = n, n + 1
    while m > 1:
        m = (m + F - 1) // F
        levels.append((addr, m))
        addr += m
    n_blocks = addr
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    engine.init(0)
    base = engine.device_alloc(n_blocks * BS)
    try:
        cs = torch.empty(n, dtype=torch.int64, device=dev)
        engine.fill_synthetic_device(base + BS, BS, n, 0, SEED)
        engine.checksum_device(base + BS, BS, n, cs.data_ptr(), BS)
        ws = torch.zeros(max(engine.merkle_workspace_bytes(n, F) // 8, 1), dtype=torch.int64, device=dev)
        root = torch.zeros(4, dtype=torch.int64, device=dev)
        engine.merkle_root_device(cs.data_ptr(), n, 1, n + 1, REV, F, ws.data_ptr(), ws.numel() * 8, root.data_ptr(),
                                  root.data_ptr() + 24)
        # materialise every level: its children's checksums are the leaves', then the workspace rows
        child_cs, child_base, child_n, child_type, row = cs.data_ptr(), 1, n, 2, 0
        for first, nodes in levels:
            engine.pack_pointer_blocks_device(child_cs, child_n, child_base, REV, child_type, F, base + first * BS, BS)
            child_cs, child_base, child_n, child_type = ws.data_ptr() + 8 * row, first, nodes, 1
            row += nodes
        torch.cuda.synchronize()
        r_cs, r_addr, r_rev, r_type = engine.as_tuple(root)

        lay = scrub.ScrubLayout.production(n_blocks)
        work = torch.empty((scrub.workspace_bytes(n_blocks) + 7) // 8, dtype=torch.int64, device=dev)

        def run_scrub():
            return scrub.scrub_tree_device(base, lay, (r_cs, r_addr, r_rev), r_type, scrub.BLOB, workspace=work)

        # (b): the same blocks in the order the scrub reads them (root, upper levels, leaves)
        addrs = torch.cat([torch.arange(first, first + nodes, device=dev) for first, nodes in reversed(levels)] +
                          [torch.arange(1, n + 1, device=dev)])
        offs = (addrs * BS).to(torch.int64)
        n_ptr = sum(nodes for _, nodes in levels)
        lens = torch.cat([torch.full((n_ptr,), POINTER_LEN, dtype=torch.int32, device=dev),
                          torch.full((n,), BS, dtype=torch.int32, device=dev)])
        out = torch.empty(offs.numel(), dtype=torch.int64, device=dev)

        def run_gather():
            engine.checksum_gather_device(base, offs.data_ptr(), offs.numel(), out.data_ptr(), BS, lens.data_ptr(),
                                          check_status=False)

        for _ in range(args.warmup):
            rep = run_scrub()
            run_gather()
        torch.cuda.synchronize()
        if not rep.ok or rep.verified != (n_ptr, 0, 0, n):
            raise SystemExit(f"the scrub of an intact tree reported {rep}")
        engine.device_status()
        total = n_ptr * POINTER_LEN + n * BS
        if rep.bytes_hashed != total:
            raise SystemExit(f"bytes_hashed {rep.bytes_hashed} != {total}")

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        scrub_ms, gather_ms = [], []
        for _ in range(args.reps):  # alternating, so both see the same machine
            scrub_ms.append(timed(run_scrub))
            gather_ms.append(timed(run_gather))
        engine.device_status()
    finally:
        torch.cuda.synchronize()
        engine.device_free(base)

    def med(v):
        s = sorted(v)
        return s[len(s) // 2]

    gib = total / 2.0 ** 30
    line = {
        "tool": "scrub_bench", "leaves": n, "fanout": F, "n_blocks": n_blocks, "pointer_blocks": n_ptr,
        "bytes_hashed": total, "reps": args.reps, "warmup": args.warmup,
        "scrub_ms_median": med(scrub_ms), "scrub_ms_min": min(scrub_ms), "scrub_ms_max": max(scrub_ms),
        "gather_ms_median": med(gather_ms), "gather_ms_min": min(gather_ms), "gather_ms_max": max(gather_ms),
        "ratio_scrub_over_gather": med(scrub_ms) / med(gather_ms),
        "scrub_gib_s": gib / (med(scrub_ms) / 1e3), "gather_gib_s": gib / (med(gather_ms) / 1e3),
        "levels": rep.levels, "report": rep.as_dict(), "library": engine.library_record(),
        "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
