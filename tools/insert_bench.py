#!/usr/bin/env python3
"""Time the batched insert next to the lookup it contains and the update on one MI355X.

    python tools/insert_bench.py [--sizes 8,256] [--reps 10] [--warmup 3] [--out profiles/insert/bench.json]

A whole store at production sizes (block 32768, fan-out 1200, C = 600), built on the host with
the test builders and uploaded, one per object size S: the lookup bench's dense key tree with room
left in every leaf (1,200 objectlist leaves under one pointer block, 60 keys of 48 bytes in each)
and an object tree that holds every ID (1,200 blob leaves under one pointer block, 60 objects in
each; N = 250 slots for S = 8, N = 120 for S = 256), NextObjectID above every stored ID. The batch
is one new 48-byte key per 3 existing ones (24,000 keys, 20 per leaf), in shuffled order. Timed
with HIP events around warmed repeats in one process, alternating, each on a fresh copy of the
image (the copy is outside the timed region):
  insert   storm.insert_device over the new keys;
  lookup   keystore.get_object_ids_device over the same keys: the call the insert contains;
  update   storm.update_device of as many existing keys on the same store.
Prints one JSON line: per size the times (median, and the repeats' extremes), insert / lookup,
insert / update, keys per second and the insert's report. Context numbers for DESIGN.md "Insert";
there is no threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x53544F524D
KEY_LEN, LEAVES, PER_LEAF, NEW_PER_LEAF = 48, 1200, 60, 20
SPACE = 4321


def build(S, np, lu, ou):
    """(Store, the new keys as rows in shuffled order, as many existing keys likewise)."""
    rng = np.random.default_rng(SEED + S)
    A = lu.table(600, 1)
    kt = lu.KeyTree(lu.PRODUCTION_LAYOUT, A, depth=1)
    N = 250 if S == 8 else 32760 // ou.stride_of(S)
    assert (PER_LEAF + NEW_PER_LEAF) <= N * 3 // 4, "the blob leaves have no room for the batch"
    ot = ou.ObjectTree(ou.PRODUCTION_LAYOUT, N, S, depth=1)
    keys, new = [], []
    filled = {}
    while len(keys) < LEAVES * PER_LEAF or len(new) < LEAVES * NEW_PER_LEAF:
        k = rng.integers(0, 256, KEY_LEN, dtype=np.uint8).tobytes()
        path = kt.locate(k)[0]
        have, fresh = filled.get(path, (0, 0))
        if have < PER_LEAF:
            kt.add(k, len(keys))  # IDs 0 .. 71,999: PER_LEAF in every blob leaf; with_next_object_id puts NextObjectID above
            keys.append(k)
            filled[path] = (have + 1, fresh)
        elif fresh < NEW_PER_LEAF:
            new.append(k)
            filled[path] = (have, fresh + 1)
    objects = rng.integers(1, 255, (len(keys), S), dtype=np.uint8)
    for i, obj in enumerate(objects):
        ot.set(i, obj.tobytes())
    store = ou.Store({SPACE: (ou.DEFINED, kt, ot)}, ou.space_table(400, 1), A, lay=ou.PRODUCTION_LAYOUT, blob=(N, S))
    rows = lambda ks: np.ascontiguousarray(np.frombuffer(b"".join(ks), np.uint8).reshape(-1, KEY_LEN))  # noqa: E731
    new_rows = rows(new)[rng.permutation(len(new))]
    old_rows = rows(keys)[rng.permutation(len(keys))[:len(new)]]
    return store, np.ascontiguousarray(new_rows), np.ascontiguousarray(old_rows), N


def with_next_object_id(store, np, value):
    """The store's image, writable and with room for a revision, its space's NextObjectID set to
    `value` and the path from the spacelist leaf to the singularity signed again (the test
    builder hands out space_id + 1000, below the bench's stored IDs)."""
    from oracle import oracle as o
    from storm_amd.scrub import ScrubLayout
    lay0 = store.lay
    room = 3 * LEAVES + 16
    img = np.zeros((lay0.n_blocks + room) * lay0.block_size, np.uint8)
    img[:lay0.n_blocks * lay0.block_size] = store.img[:lay0.n_blocks * lay0.block_size]
    lay = ScrubLayout(lay0.block_size, lay0.n_blocks + room, lay0.pointer_fanout, lay0.spaces_per_block, lay0.objectlist_len,
                      lay0.blob_len)
    bs, F, S = lay.block_size, lay.pointer_fanout, lay.spaces_per_block
    root = struct.unpack_from("<Q", img, 40)[0]
    slot = SPACE % F
    leaf = struct.unpack_from("<Q", img, root * bs + 24 * slot + 8)[0]
    k = next(k for k in range(S) if img[leaf * bs + 72 * k + 66] == 1 and
             struct.unpack_from("<Q", img, leaf * bs + 72 * k)[0] == SPACE // F)
    struct.pack_into("<Q", img, leaf * bs + 72 * k + 8, value)
    struct.pack_into("<Q", img, root * bs + 24 * slot, o.xxh64(img[leaf * bs:leaf * bs + ((72 * S + 2 + 7) & ~7)]))
    struct.pack_into("<Q", img, 32, o.xxh64(img[root * bs:root * bs + ((25 * F + 7) & ~7)]))
    struct.pack_into("<Q", img, 0, 0)
    struct.pack_into("<Q", img, 0, o.xxh64(img[:72]))
    return img, lay


def measure(S, args, torch, np):
    from storm_amd import engine, keystore as ks, scrub, spacestore as sps, storm
    from tests import lookup_util as lu
    from tests import objects_util as ou

    t0 = time.time()
    store, new_rows, old_rows, N = build(S, np, lu, ou)
    img, lay = with_next_object_id(store, np, LEAVES * PER_LEAF)
    assert scrub.scrub_host(img, lay).ok
    build_s = time.time() - t0
    dev = torch.device("cuda:0")
    pristine = torch.from_numpy(img).to(dev)
    image = pristine.clone()
    d_new, d_old = torch.from_numpy(new_rows).to(dev), torch.from_numpy(old_rows).to(dev)
    n = d_new.shape[0]
    objects = torch.randint(1, 255, (n, S), dtype=torch.uint8, device=dev)
    need = max(storm.insert_workspace_bytes(n, 600), storm.update_workspace_bytes(n, 600))
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    sing = img[:72].tobytes()
    sres, _ = sps.get_spaces_device(image, lay, struct.unpack_from("<QQ", sing, 32) + (1,), sing[56], store.SA,
                                    torch.tensor([SPACE], dtype=torch.int64, device=dev))
    (key_root, key_type), _ = sps.roots(sps.results_numpy(sres)[0])
    last = {}
    runs = {
        "insert": lambda: last.__setitem__("insert", storm.insert_device(image, lay, SPACE, store.params, d_new, objects,
                                                                         workspace=work)),
        "lookup": lambda: last.__setitem__("lookup", ks.get_object_ids_device(image, lay, key_root, key_type, store.params.keys,
                                                                              d_new, workspace=work)),
        "update": lambda: last.__setitem__("update", storm.update_device(image, lay, SPACE, store.params, d_old, objects,
                                                                         workspace=work)),
    }

    def timed(fn):
        image.copy_(pristine)  # every repeat meets the same store
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        for fn in runs.values():
            timed(fn)
    irep, urep = last["insert"][1], last["update"][1]
    if not irep.ok or irep.n_inserted != n or irep.cut != n:
        raise SystemExit(f"S={S}: a store with room in every leaf reported {irep}")
    if not urep.ok or urep.n_written != n:
        raise SystemExit(f"S={S}: the update of existing keys reported {urep}")
    got = storm.get_device(image, lay, SPACE, store.params, d_old)[2]  # the last warm-up call was the update
    if not got.ok:
        raise SystemExit(f"S={S}: the store after the update reported {got}")
    engine.device_status()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):  # alternating, so all see the same machine
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    engine.device_status()

    def med(v):
        s = sorted(v)
        return s[len(s) // 2]

    out = {"keys": n, "existing_keys": LEAVES * PER_LEAF, "key_len": KEY_LEN, "object_size": S, "objects_per_block": N,
           "n_blocks": lay.n_blocks, "host_build_s": round(build_s, 2), "workspace_bytes": storm.insert_workspace_bytes(n, 600)}
    for k, v in ms.items():
        out.update({f"{k}_ms_median": med(v), f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    out.update({"insert_over_lookup": med(ms["insert"]) / med(ms["lookup"]),
                "insert_over_update": med(ms["insert"]) / med(ms["update"]),
                "insert_keys_per_s": n / (med(ms["insert"]) / 1e3),
                "report": {k: v for k, v in irep.as_dict().items() if k != "space"}})
    del image, pristine, work
    torch.cuda.empty_cache()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insert", "bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from storm_amd import engine

    torch.cuda.set_device(0)
    engine.init(0)
    line = {"tool": "insert_bench", "fanout": 1200, "block_size": 32768, "chunks_per_block": 600, "reps": args.reps,
            "warmup": args.warmup}
    for S in args.sizes.split(","):
        line[f"S={S}"] = measure(int(S), args, torch, np)
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
