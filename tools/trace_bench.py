#!/usr/bin/env python3
"""Time a batched verified trace against its hash-only floor on one MI355X.

    python tools/trace_bench.py [--leaves 1048576] [--reps 10] [--warmup 3] [--out FILE]

Builds the resident tree tools/scrub_bench.py builds (synthetic 32 KiB leaves at addresses
1..n, fanout 1200, every pointer level packed into the image behind them), then traces one tag
per leaf, in shuffled order, and times, with HIP events around warmed repeats in one process on
one arena, alternating:
  (a) stormck_trace_device of the n tags from the root, leaves verified;
  (b) one stormck_checksum_gather_device call over exactly the distinct offsets and lengths
      the trace hashed, in address order: existing code, the floor of tools/scrub_bench.py;
  (c) the same call with the leaves in the order of the shuffled tags, which is the order the
      trace's leaf level has them in;
  (d) the trace with verify_leaves=False: the pointer path alone (876 blocks hashed), which
      isolates k_trace_step, the table and the per-level read-backs.
Prints one JSON line: the times, trace / floor with the spread the repeats show, GiB/s, the
tags per second of (d), and the trace's report. The yardstick is (b), and beside it the scrub's
ratio over the same floor (profiles/scrub/bench_1m.json).
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

    from storm_amd import engine, scrub, trace

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
        child_cs, child_base, child_n, child_type, row = cs.data_ptr(), 1, n, 2, 0
        for first, nodes in levels:
            engine.pack_pointer_blocks_device(child_cs, child_n, child_base, REV, child_type, F, base + first * BS, BS)
            child_cs, child_base, child_n, child_type = ws.data_ptr() + 8 * row, first, nodes, 1
            row += nodes
        torch.cuda.synchronize()
        r_cs, r_addr, r_rev, r_type = engine.as_tuple(root)

        # leaf i sits at slot i % F of the i // F-th block of the level above, and so on up: the
        # walk takes the root's slot from the tag's lowest digit, so the tag is i's digits reversed
        depth = len(levels)
        leaf = torch.arange(n, dtype=torch.int64, device=dev)
        tags, rest = torch.zeros_like(leaf), leaf.clone()
        for _ in range(depth):
            tags = tags * F + rest % F
            rest = rest // F
        gen = torch.Generator(device=dev)
        gen.manual_seed(SEED)
        perm = torch.randperm(n, device=dev, generator=gen)
        tags, leaf_addr = tags[perm].contiguous(), (leaf + 1)[perm].contiguous()

        lay = scrub.ScrubLayout.production(n_blocks)
        work = torch.empty((trace.workspace_bytes(n) + 7) // 8, dtype=torch.int64, device=dev)
        last = {}

        def run_trace():
            last["res"], last["rep"] = trace.trace_device(base, lay, (r_cs, r_addr, r_rev), r_type, scrub.BLOB, tags,
                                                          workspace=work)

        def run_path():
            last["path_res"], last["path_rep"] = trace.trace_device(base, lay, (r_cs, r_addr, r_rev), r_type, scrub.BLOB,
                                                                    tags, verify_leaves=False, workspace=work)

        n_ptr = sum(nodes for _, nodes in levels)
        upper = [torch.arange(first, first + nodes, device=dev) for first, nodes in reversed(levels)]
        lens = torch.cat([torch.full((n_ptr,), POINTER_LEN, dtype=torch.int32, device=dev),
                          torch.full((n,), BS, dtype=torch.int32, device=dev)])
        offs = (torch.cat(upper + [torch.arange(1, n + 1, device=dev)]) * BS).to(torch.int64)
        offs_shuffled = (torch.cat(upper + [leaf_addr]) * BS).to(torch.int64)
        out = torch.empty(offs.numel(), dtype=torch.int64, device=dev)

        def gather(o):
            return lambda: engine.checksum_gather_device(base, o.data_ptr(), o.numel(), out.data_ptr(), BS,
                                                         lens.data_ptr(), check_status=False)

        runs = {"trace": run_trace, "gather": gather(offs), "gather_shuffled": gather(offs_shuffled), "path": run_path}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        rep, path_rep = last["rep"], last["path_rep"]
        total = n_ptr * POINTER_LEN + n * BS
        if not rep.ok or rep.n_status[trace.FOUND] != n or rep.blocks_hashed != (n_ptr, n) or rep.bytes_hashed != total:
            raise SystemExit(f"the trace of an intact tree reported {rep}")
        if not path_rep.ok or path_rep.n_status[trace.FOUND] != n or path_rep.blocks_hashed != (n_ptr, 0):
            raise SystemExit(f"the pointer-path trace of an intact tree reported {path_rep}")
        res = last["res"]
        if not torch.equal(res[:, 0], leaf_addr) or int(res[:, 1].abs().max()) != 0 or \
                not torch.equal(res, last["path_res"]):
            raise SystemExit("a tag did not end at its own leaf")
        engine.device_status()

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        ms = {k: [] for k in runs}
        for _ in range(args.reps):  # alternating, so all see the same machine
            for k, fn in runs.items():
                ms[k].append(timed(fn))
        engine.device_status()
    finally:
        torch.cuda.synchronize()
        engine.device_free(base)

    def med(v):
        s = sorted(v)
        return s[len(s) // 2]

    gib = total / 2.0 ** 30
    line = {"tool": "trace_bench", "leaves": n, "tags": n, "fanout": F, "n_blocks": n_blocks, "pointer_blocks": n_ptr,
            "bytes_hashed": total, "workspace_bytes": trace.workspace_bytes(n), "reps": args.reps, "warmup": args.warmup}
    for k, v in ms.items():
        line.update({f"{k}_ms_median": med(v), f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    line.update({
        "ratio_trace_over_gather": med(ms["trace"]) / med(ms["gather"]),
        "ratio_min": min(ms["trace"]) / max(ms["gather"]), "ratio_max": max(ms["trace"]) / min(ms["gather"]),
        "ratio_trace_over_gather_shuffled": med(ms["trace"]) / med(ms["gather_shuffled"]),
        "trace_gib_s": gib / (med(ms["trace"]) / 1e3), "gather_gib_s": gib / (med(ms["gather"]) / 1e3),
        "path_tags_per_s": n / (med(ms["path"]) / 1e3),
        "levels": rep.levels, "report": rep.as_dict(), "path_report": path_rep.as_dict(),
        "library": engine.library_record(), "device": torch.cuda.get_device_name(0),
    })
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
