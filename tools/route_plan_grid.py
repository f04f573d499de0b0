"""The decisions of stormck_route_plan_batch / _plan_commit over one grid, bit for bit.

    python tools/route_plan_grid.py [TREE] > plans.txt

TREE: the checkout whose built library answers (default: the one this file is in). Two trees
that route alike print the same text on the same machine (the pool's size and the CPU count
enter the split's host threads). Every time is printed as the hex of its double.
profiles/route_plan/ keeps the output of the parent and of the tree that moved the model into
route_plan.h. No device is needed.
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import blocks  # noqa: E402
from storm_amd import commit as sc  # noqa: E402

BASE = dict(host_thread=40000.0, host_memory=180000.0, host_cached=180000.0, link_pinned=55000.0,
            link_pageable=50000.0, link_inplace=52000.0, device_latency=120.0)
# the rate sets of tests/test_route.py
RATE_SETS = {
    "base": {},
    "cached90k": dict(host_cached=90000.0),
    "slow_link": dict(link_pinned=500.0, link_pageable=500.0, link_inplace=500.0),
    "margin": dict(device_latency=1.0, host_cached=50000.0, host_thread=50000.0),
    "lat150_cached400k": dict(device_latency=150.0, host_cached=400000.0),
    "lat1_cached100k": dict(device_latency=1.0, host_cached=100000.0),
    "lat40": dict(device_latency=40.0),
    "fast_host": dict(host_thread=400000.0, host_memory=4000000.0, host_cached=4000000.0),
    "priors": None,
}
C5 = [31808] * 1200 + [30000, 72]
TAGS = [536, 728] * 50
L = 32768
# The shapes of tests/cpp/route_plan_test.cpp, each crossed with every rate set: pinned and
# pageable, 1 and 4 threads and the pool, 1, 2 and 8 devices and none, one block (no split),
# 64 MiB (2,048 blocks) and a block either side, a stride beyond the staging chunk.
# (name, n, stride, length, lens, pinned, threads, devices)
BATCHES = [("one", 1, L, L, None, True, 0, 1), ("three", 3, L, 31808, None, True, 0, 1),
           ("tags", 100, L, None, TAGS, False, 0, 1), ("c5", len(C5), L, None, C5, True, 0, 1),
           ("c5", len(C5), L, None, C5, True, 1, 1), ("2047", 2047, L, L, None, True, 4, 1),
           ("2048", 2048, L, L, None, False, 4, 1), ("2049", 2049, L, L, None, True, 4, 2),
           ("2049", 2049, L, L, None, False, 1, 1), ("8gib", 262144, L, L, None, True, 0, 1),
           ("8gib", 262144, L, L, None, True, 0, 8), ("8gib", 262144, L, L, None, False, 1, 2),
           ("8gib", 262144, L, L, None, True, 0, 0), ("wide_stride", 2, 1 << 30, 1 << 30, None, True, 0, 1)]
# (forest, registered, threads, devices)
COMMITS = [("three", True, 0, 1), ("tags", True, 0, 1), ("70", True, 0, 1), ("2047", True, 4, 1), ("2049", True, 4, 2),
           ("2049", False, 1, 1), ("131072", True, 0, 1), ("131072", True, 1, 8), ("131072", False, 0, 1),
           ("131072", True, 0, 0)]


def show(kind, name, rates, mem, th, nd, leg, us):
    print(kind, name, rates, "mem=%d" % mem, "threads=%d" % th, "devices=%d" % nd, "->", leg,
          " ".join(float(u).hex() for u in us))


def forest(n_leaves, leaf_lens=L, fanout=1200):
    return sc.pointer_forest(n_leaves, leaf_lens, fanout, slot=32768, revision=1)[0]


def forest_of_total(total):
    """13 leaves under one pointer block, the first leaf sized so that the lengths sum to `total`."""
    b = forest(13, 1000)
    b["length"][0] += total - int(b["length"].sum())
    assert int(b["length"].sum()) == total
    return b


def set_rates(over):
    if over is None:
        blocks.SetRouteRates(None)
        return
    r = dict(BASE)
    r.update(over)
    blocks.SetRouteRates(r, freeze=True)


def main():
    forests = {"three": forest(2, 31808), "tags": forest(100, np.array(TAGS, dtype=np.uint32), 10), "70": forest(70),
               "2047": forest(2047), "2049": forest(2049), "131072": forest(131072)}
    for rname, over in RATE_SETS.items():
        set_rates(over)
        for name, n, stride, length, lens, pinned, th, nd in BATCHES:
            leg, us = blocks.PlanBatch(n, stride, length, lens=lens, pinned=pinned, host_threads=th, n_devices=nd)
            show("batch", name, rname, pinned, th, nd, leg, us)
        for name, reg, th, nd in COMMITS:
            leg, us = sc.plan_commit(forests[name], registered=reg, host_threads=th, n_devices=nd)
            show("commit", name, rname, reg, th, nd, leg, us)
    # the host-only boundary: totals either side of kHostOnlyUs x host_thread, for rates whose
    # bound is a whole number of bytes, is not, and is `total / 10.0` (tests/test_route.py)
    for ht in (40000.0, 40000.03, 39999.97, 1e9 / 3):
        set_rates(dict(host_thread=ht))
        bound = int(10.0 * ht)
        for total in range(bound - 1, bound + 2):
            leg, us = blocks.PlanBatch(2, 1 << 32, lens=[total - 200000, 200000], pinned=True)
            show("batch", "bound%+d" % (total - bound), "ht=%r" % ht, 1, 0, 1, leg, us)
            leg, us = sc.plan_commit(forest_of_total(total))
            show("commit", "bound%+d" % (total - bound), "ht=%r" % ht, 1, 0, 1, leg, us)
    for total in (int(forests["three"]["length"].sum()), int(forests["tags"]["length"].sum()), 399999, 3 ** 12):
        for div in (10.0, 50.0):
            set_rates(dict(host_thread=total / div))
            leg, us = blocks.PlanBatch(1, total, total, pinned=True)
            show("batch", "total=%d" % total, "ht=total/%g" % div, 1, 0, 1, leg, us)
            leg, us = sc.plan_commit(forest_of_total(total))
            show("commit", "total=%d" % total, "ht=total/%g" % div, 1, 0, 1, leg, us)
    blocks.SetRouteRates(None)


if __name__ == "__main__":
    main()
