#!/usr/bin/env python3
"""Time the batched GetObject against the trace it contains on one MI355X.

    python tools/get_bench.py [--shapes dense,sparse,get] [--sizes 8,64,256,1024] [--reps 10] [--warmup 3] [--out FILE]

Object trees at production sizes (block 32768, fan-out 1200, blob leaves of 32768 bytes), built
on the host with the test builder (tests/objects_util.ObjectTree) and uploaded, one per shape
and object size S:
  dense   1,200 leaves under one pointer block, N = 100 slots with 70 objects in each (S = 1024:
          N = 31 with 21 objects, the most slots of that size a leaf holds);
  sparse  16,384 leaves under two pointer levels, one object in each.
Every stored object is got once, in shuffled order. Timed with HIP events around warmed repeats
in one process on one arena, alternating:
  objects             get_objects_device, leaves verified;
  trace               trace.trace_device over the same IDs with blob leaves: the call it
                      contains, and the yardstick;
  objects_unverified  the call with the leaves probed and read but not hashed (storm's warm
                      GetObject);
  trace_unverified    the trace with verify_leaves=False;
and, when the loaded library is the probe build (STORMCK_LIBRARY=tools/libstormck_probes.so),
  lane, wave          objects_unverified with STORMCK_FETCH_COPY forcing each form of
                      k_object_fetch's move, in turn.
Shape `get` is storm.Get as one call (stormck_get_device) over the lookup bench's dense key tree
in a whole store whose object tree holds every ID, against the lookup and the objects call made
one after the other (measure_get).
Prints one JSON line: per shape and size the times (median, and the repeats' extremes), objects /
trace for both pairs, the fetch's share, objects per second, and for lane against wave the
difference of the medians beside the spread of each form's repeats.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 0x53544F524D
SPARSE_LEAVES = 16384


def build(shape, S, np, ou):
    """(Tree, the IDs in shuffled order as int64, their objects as an (n, S) array)."""
    rng = np.random.default_rng(SEED + S)
    if shape == "dense":
        N = 100 if ou.stride_of(S) * 100 <= 32760 else 32760 // ou.stride_of(S)
        ot = ou.ObjectTree(ou.PRODUCTION_LAYOUT, N, S, depth=1)
        ids = [slot + 1200 * r for r in range(7 * N // 10) for slot in range(1200)]  # sequential IDs, as storm hands them out
    else:
        ot = ou.ObjectTree(ou.PRODUCTION_LAYOUT, 100 if ou.stride_of(S) * 100 <= 32760 else 31, S, depth=2)
        ids = [int(v) for v in rng.choice(1200 * 1200, SPARSE_LEAVES, replace=False)]  # one per leaf: reminder 0
    objects = rng.integers(1, 255, (len(ids), S), dtype=np.uint8)
    for oid, obj in zip(ids, objects):
        ot.set(oid, obj.tobytes())
    tree = ot.build(slack=0)
    order = rng.permutation(len(ids))
    return tree, np.array(ids, dtype=np.int64)[order], np.ascontiguousarray(objects[order])


def measure(shape, S, args, torch, np, probes):
    from storm_amd import engine, objectstore as obs, trace
    from storm_amd.scrub import BLOB
    from tests import objects_util as ou

    t0 = time.time()
    tree, ids_host, objects_host = build(shape, S, np, ou)
    build_s = time.time() - t0
    dev = torch.device("cuda:0")
    image = torch.from_numpy(np.array(tree.img)).to(dev)
    ids = torch.from_numpy(ids_host).to(dev)
    n = ids.shape[0]
    lay, root, root_type, params = tree.args()
    work = torch.empty((obs.workspace_bytes(n) + 7) // 8, dtype=torch.int64, device=dev)
    rows = torch.empty((n, S), dtype=torch.uint8, device=dev)
    last = {}

    def objects(verify, form=None):
        def run():
            if form is not None:
                os.environ["STORMCK_FETCH_COPY"] = form  # the probe build reads it at every call
            last["objects", verify] = obs.get_objects_device(image, lay, root, root_type, params, ids,
                                                             verify_leaves=verify, workspace=work, objects=rows)
            if form is not None:
                del os.environ["STORMCK_FETCH_COPY"]
        return run

    def traced(verify):
        def run():
            last["trace", verify] = trace.trace_device(image, lay, root, root_type, BLOB, ids, verify_leaves=verify,
                                                       workspace=work)
        return run

    runs = {"objects": objects(True), "trace": traced(True), "objects_unverified": objects(False),
            "trace_unverified": traced(False)}
    if probes:
        runs.update({"lane": objects(False, "0"), "wave": objects(False, "1")})
    want = torch.from_numpy(objects_host).to(dev)
    for _ in range(args.warmup):
        for name, fn in runs.items():
            rows.zero_()
            fn()
            if name not in ("trace", "trace_unverified") and not torch.equal(rows, want):
                raise SystemExit(f"{shape} S={S}: {name} returned other objects than were stored")
    torch.cuda.synchronize()
    for verify in (True, False):
        res, _, rep = last["objects", verify]
        if not rep.ok or rep.n_status[obs.FOUND] != n or rep.n_probed != n or not torch.equal(res[:, 0], ids):
            raise SystemExit(f"{shape} S={S}: the objects of an intact tree reported {rep}")
        tres, trep = last["trace", verify]
        if trep.as_dict() != rep.trace.as_dict() or not torch.equal(tres[:, 0], res[:, 1]):
            raise SystemExit(f"{shape} S={S}: the call's trace is not the trace's: {trep} / {rep.trace}")
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

    rep = last["objects", True][2]
    out = {"ids": n, "object_size": S, "objects_per_block": params.objects_per_block,
           "pointer_blocks": rep.trace.blocks_hashed[0], "leaves": rep.trace.blocks_hashed[1], "n_blocks": lay.n_blocks,
           "host_build_s": round(build_s, 2), "workspace_bytes": obs.workspace_bytes(n)}
    for k, v in ms.items():
        out.update({f"{k}_ms_median": med(v), f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    for pair, a, b in (("verified", "objects", "trace"), ("unverified", "objects_unverified", "trace_unverified")):
        out.update({f"ratio_{pair}": med(ms[a]) / med(ms[b]), f"ratio_{pair}_min": min(ms[a]) / max(ms[b]),
                    f"ratio_{pair}_max": max(ms[a]) / min(ms[b]), f"fetch_ms_{pair}": med(ms[a]) - med(ms[b])})
    out.update({"objects_per_s": n / (med(ms["objects"]) / 1e3),
                "objects_unverified_per_s": n / (med(ms["objects_unverified"]) / 1e3),
                "probes_per_id": rep.probes / n, "report": rep.as_dict()})
    if probes:  # the copy rule: wave ships where its median beats lane's by more than either form's own spread
        spread = max(max(ms["lane"]) - min(ms["lane"]), max(ms["wave"]) - min(ms["wave"]))
        out.update({"lane_minus_wave_ms": med(ms["lane"]) - med(ms["wave"]), "form_spread_ms": spread,
                    "wave_wins": med(ms["lane"]) - med(ms["wave"]) > spread,
                    "lane_wins": med(ms["wave"]) - med(ms["lane"]) > spread})
    del image, ids, work, rows, want
    torch.cuda.empty_cache()
    return out


def measure_get(args, torch, np):
    """Shape (ii): storm.Get over the lookup bench's dense key tree (224,400 keys of 48 bytes in
    1,200 objectlist leaves, C = 600) in a whole store whose object tree holds every ID (8-byte
    objects, 1,200 blob leaves of N = 250 under one pointer block). The yardstick, in the same
    process on the same arena: keystore.get_object_ids_device, then objectstore.get_objects_device
    over its results in place, from the roots one spaces call gave beforehand."""
    import lookup_bench
    from storm_amd import engine, keystore as ks, objectstore as obs, spacestore as sps, storm
    from tests import lookup_util as lu
    from tests import objects_util as ou

    t0 = time.time()
    rng = np.random.default_rng(SEED)
    A = lu.table(600, 1)
    kt = lu.KeyTree(lu.PRODUCTION_LAYOUT, A, depth=1)
    keys = []
    while len(keys) < 187 * 1200:  # lookup_bench.build("dense"), with the KeyTree kept
        k = rng.integers(0, 256, lookup_bench.KEY_LEN, dtype=np.uint8).tobytes()
        leaf = kt.leaves.get(kt.locate(k)[0])
        if leaf is not None and leaf.n_used() >= 2 * 187 + 40:
            continue
        kt.add(k, 1 + len(keys))
        keys.append(k)
    N, S = 250, 8
    ot = ou.ObjectTree(ou.PRODUCTION_LAYOUT, N, S, depth=1)
    objects = rng.integers(1, 255, (len(keys), S), dtype=np.uint8)
    for i, obj in enumerate(objects):
        ot.set(1 + i, obj.tobytes())
    space_id = 4321
    store = ou.Store({space_id: (ou.DEFINED, kt, ot)}, ou.space_table(400, 1), A, lay=ou.PRODUCTION_LAYOUT, blob=(N, S))
    order = rng.permutation(len(keys))
    rows_host = np.ascontiguousarray(np.frombuffer(b"".join(keys), np.uint8).reshape(-1, lookup_bench.KEY_LEN)[order])
    want = torch.from_numpy(np.ascontiguousarray(objects[order])).cuda()
    build_s = time.time() - t0

    dev = torch.device("cuda:0")
    image = torch.from_numpy(np.array(store.img)).to(dev)
    dkeys = torch.from_numpy(rows_host).to(dev)
    n = dkeys.shape[0]
    work = torch.empty((storm.workspace_bytes(n, 600) + 7) // 8, dtype=torch.int64, device=dev)
    rows = torch.empty((n, S), dtype=torch.uint8, device=dev)
    sing = store.img[:72].tobytes()
    import struct
    sres, srep = sps.get_spaces_device(image, store.lay, struct.unpack_from("<QQ", sing, 32) + (1,), sing[56], store.SA,
                                       torch.tensor([space_id], dtype=torch.int64, device=dev))
    (key_root, key_type), (object_root, object_type) = sps.roots(sps.results_numpy(sres)[0])
    last = {}

    def get(verify):
        def run():
            last["get", verify] = storm.get_device(image, store.lay, space_id, store.params, dkeys, verify_leaves=verify,
                                                   workspace=work, objects=rows)
        return run

    def separate(verify):
        def run():
            res, lrep = ks.get_object_ids_device(image, store.lay, key_root, key_type, store.params.keys, dkeys,
                                                 verify_leaves=verify, workspace=work)
            last["separate", verify] = obs.get_objects_device(image, store.lay, object_root, object_type, store.params.objects,
                                                              res, verify_leaves=verify, workspace=work, objects=rows)
        return run

    runs = {"get": get(True), "separate": separate(True), "get_unverified": get(False), "separate_unverified": separate(False)}
    for _ in range(args.warmup):
        for name, fn in runs.items():
            rows.zero_()
            fn()
            if not torch.equal(rows, want):
                raise SystemExit(f"get: {name} returned other objects than were stored")
    rep = last["get", True][2]
    if not rep.ok or rep.n_found != n or rep.n_selected != n:
        raise SystemExit(f"get: an intact store reported {rep}")
    engine.device_status()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    engine.device_status()

    def med(v):
        s = sorted(v)
        return s[len(s) // 2]

    out = {"keys": n, "object_size": S, "objects_per_block": N, "n_blocks": store.lay.n_blocks, "host_build_s": round(build_s, 2),
           "workspace_bytes": storm.workspace_bytes(n, 600)}
    for k, v in ms.items():
        out.update({f"{k}_ms_median": med(v), f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    for pair, a, b in (("verified", "get", "separate"), ("unverified", "get_unverified", "separate_unverified")):
        out.update({f"ratio_{pair}": med(ms[a]) / med(ms[b]), f"ratio_{pair}_min": min(ms[a]) / max(ms[b]),
                    f"ratio_{pair}_max": max(ms[a]) / min(ms[b])})
    out.update({"get_keys_per_s": n / (med(ms["get"]) / 1e3), "get_unverified_keys_per_s": n / (med(ms["get_unverified"]) / 1e3),
                "report": {k: v for k, v in rep.as_dict().items() if k != "space"}})
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dense,sparse,get")
    ap.add_argument("--sizes", default="8,64,256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from storm_amd import _lib, build as sb, engine

    torch.cuda.set_device(0)
    engine.init(0)
    probes = os.path.abspath(_lib.LIB_PATH) == os.path.abspath(sb.PROBES_LIB)
    os.environ.pop("STORMCK_FETCH_COPY", None)  # the four plain runs take the shipped rule
    line = {"tool": "get_bench", "fanout": 1200, "block_size": 32768, "reps": args.reps, "warmup": args.warmup,
            "probe_build": probes}
    for shape in args.shapes.split(","):
        if shape == "get":
            line["get"] = measure_get(args, torch, np)
            continue
        line[shape] = {f"S={S}": measure(shape, int(S), args, torch, np, probes) for S in args.sizes.split(",")}
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
