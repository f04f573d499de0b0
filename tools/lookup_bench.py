#!/usr/bin/env python3
"""Time the batched GetObjectID against the trace it contains on one MI355X.

    python tools/lookup_bench.py [--shapes dense,sparse] [--reps 10] [--warmup 3] [--out FILE]

Two key trees at production sizes (block 32768, fan-out 1200, C = 600, 31,808-byte leaves),
built on the host with the test builder (tests/lookup_util.KeyTree) and uploaded:
  dense   1,200 leaves under one pointer block, about 187 keys of 48 bytes in each;
  sparse  65,536 leaves under two pointer levels, one 48-byte key in each.
Every stored key is looked up once, in shuffled order. Timed with HIP events around warmed
repeats in one process on one arena, alternating:
  lookup             get_object_ids_device, leaves verified;
  trace              trace.trace_keys_device over the same keys: the code the lookup adds the
                     probe to, and the yardstick;
  lookup_unverified  the lookup with the leaves probed but not hashed (storm's warm GetObjectID);
  trace_unverified   the trace with verify_leaves=False.
Prints one JSON line: per shape the times, lookup / trace for both pairs with the spread the
repeats show, keys per second, and the lookup's report.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x53544F524D
KEY_LEN = 48


def build(shape, np, lu):
    """(Tree, keys as an (n, 48) array, their object IDs)."""
    rng = np.random.default_rng(SEED)
    depth, per_leaf, leaves = (1, 187, 1200) if shape == "dense" else (2, 1, 65536)
    kt = lu.KeyTree(lu.PRODUCTION_LAYOUT, lu.table(600, 1), depth=depth)
    keys = []
    while len(keys) < per_leaf * leaves:
        k = rng.integers(0, 256, KEY_LEN, dtype=np.uint8).tobytes()
        path, _ = kt.locate(k)
        leaf = kt.leaves.get(path)
        if leaf is None and len(kt.leaves) >= leaves:
            continue
        if leaf is not None and leaf.n_used() >= 2 * per_leaf + (40 if shape == "dense" else 0):
            continue  # dense: about 187 keys a leaf (below storm's SplitTrigger); sparse: one
        kt.add(k, 1 + len(keys))
        keys.append(k)
    tree = kt.build(slack=0)
    rows = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, KEY_LEN)
    order = rng.permutation(len(keys))
    return tree, np.ascontiguousarray(rows[order]), (order + 1).astype(np.int64)


def measure(shape, args, torch, np):
    from storm_amd import engine, keystore as ks, trace
    from storm_amd.scrub import OBJECTLIST
    from tests import lookup_util as lu

    t0 = time.time()
    tree, rows, ids = build(shape, np, lu)
    build_s = time.time() - t0
    dev = torch.device("cuda:0")
    image = torch.from_numpy(np.array(tree.img)).to(dev)
    keys = torch.from_numpy(rows).to(dev)
    n = keys.shape[0]
    lay, root, root_type, params = tree.args()
    work = torch.empty((ks.workspace_bytes(n, 600) + 7) // 8, dtype=torch.int64, device=dev)
    last = {}

    def lookup(verify):
        def run():
            last["lookup", verify] = ks.get_object_ids_device(image, lay, root, root_type, params, keys,
                                                              verify_leaves=verify, workspace=work)
        return run

    def traced(verify):
        def run():
            last["trace", verify] = trace.trace_keys_device(image, lay, root, root_type, keys, OBJECTLIST,
                                                            verify_leaves=verify, workspace=work)
        return run

    runs = {"lookup": lookup(True), "trace": traced(True), "lookup_unverified": lookup(False),
            "trace_unverified": traced(False)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    want = torch.from_numpy(ids).to(dev)
    for verify in (True, False):
        res, rep = last["lookup", verify]
        if not rep.ok or rep.n_status[ks.FOUND] != n or rep.n_probed != n or not torch.equal(res[:, 0], want):
            raise SystemExit(f"{shape}: the lookup of an intact tree reported {rep}")
        tres, trep, _ = last["trace", verify]
        if trep.as_dict() != rep.trace.as_dict() or not torch.equal(tres[:, 0], res[:, 1]):
            raise SystemExit(f"{shape}: the lookup's trace is not the trace's: {trep} / {rep.trace}")
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

    def med(v):
        s = sorted(v)
        return s[len(s) // 2]

    rep = last["lookup", True][1]
    out = {"keys": n, "pointer_blocks": rep.trace.blocks_hashed[0], "leaves": rep.trace.blocks_hashed[1],
           "n_blocks": lay.n_blocks, "host_build_s": round(build_s, 2), "workspace_bytes": ks.workspace_bytes(n, 600)}
    for k, v in ms.items():
        out.update({f"{k}_ms_median": med(v), f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    for pair, a, b in (("verified", "lookup", "trace"), ("unverified", "lookup_unverified", "trace_unverified")):
        out.update({f"ratio_{pair}": med(ms[a]) / med(ms[b]), f"ratio_{pair}_min": min(ms[a]) / max(ms[b]),
                    f"ratio_{pair}_max": max(ms[a]) / min(ms[b]),
                    f"probe_ms_{pair}": med(ms[a]) - med(ms[b])})
    out.update({"lookup_keys_per_s": n / (med(ms["lookup"]) / 1e3),
                "lookup_unverified_keys_per_s": n / (med(ms["lookup_unverified"]) / 1e3),
                "probes_per_key": rep.probes / n, "report": rep.as_dict()})
    del image, keys, work
    torch.cuda.empty_cache()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dense,sparse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from storm_amd import engine

    torch.cuda.set_device(0)
    engine.init(0)
    line = {"tool": "lookup_bench", "key_len": KEY_LEN, "chunks_per_block": 600, "fanout": 1200, "reps": args.reps,
            "warmup": args.warmup,
            # the probe build alone reads it: LDS table + 2 * batched reads (storm_amd/csrc/lookup.h)
            "lookup_variant": os.environ.get("STORMCK_LOOKUP_VARIANT", "shipped")}
    for shape in args.shapes.split(","):
        line[shape] = measure(shape, args, torch, np)
    line.update({"library": engine.library_record(), "device": torch.cuda.get_device_name(0)})
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
