"""Irregular dirty forests through the host leg (stormck_commit_host) against storm's serial
loop (the C oracle): the designed shapes of tests/test_commit_fuzz_gpu.py, the smallest
forests, a chain, and 40 seeded cases (tests/commit_util.py). No device needed.

Every forest here has what `pointer_forest` never gives: parents with children at several
heights, children that skip heights, leaves under leaves, many roots (with an origin outside
the batch, with none, bare records), zero-length records, sparse child slots, arena slots in
an order unrelated to the commit order, and upper levels of more than 16,384 blocks, from
which the planner's counting sort runs on the library's pool."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as o
from storm_amd import _lib
from storm_amd import commit as sc
from tests import commit_util as cu

SMALL = {
    "one": dict(counts=[1], slot=1032, align="8", fan=11, irregular=False),
    "pair": dict(counts=[3, 1], slot=1040, align="mixed", fan=11, irregular=False),
    "chain": dict(counts=[5] * 8, slot=1040, align="16", fan=11, irregular=False),
    "deep": dict(counts=[1] * 3000, slot=520, align="8", fan=3, irregular=False, lengths="short"),
}


def _forest(name):
    if name in SMALL:
        d = SMALL[name]
        return cu.random_forest(900 + sorted(SMALL).index(name), d["counts"], d["slot"], d["fan"], d["align"],
                                irregular=d["irregular"], lengths=d.get("lengths", "edge"))
    return cu.designed_forest(name)


def test_level_class_restates_the_dispatch_plan():
    """`level_class` at 256 compute units against the rows tests/cpp/dispatch_plan_test.cpp
    commit_levels() pins for plan_commit_level (kernel, and the waves of an LDS-DMA
    workgroup); 16,384 with the forest both eligible for the LDS-DMA kernel and not."""
    rows = [(256, True, "Wide"), (257, True, "Multi5"), (2048, True, "Multi8"), (2049, True, "Quad"),
            (9983, True, "Quad"), (9984, True, "Glds3"), (16384, True, "Glds1"), (16384, False, "Quad"),
            (24576, True, "Glds3"), (32768, True, "Glds8"), (36864, True, "Glds3"), (107232, True, "Glds8")]
    for cnt, eligible, want in rows:
        assert cu.level_class(cnt, 256, eligible) == want, (cnt, eligible)
    # further rows of commit_levels(): the chunk schedule's neighbours and no CU count
    assert cu.level_class(14000, 256, True) == "Glds1" and cu.level_class(131072, 256, True) == "Glds8"
    assert cu.level_class(1400, 256, True) == "Multi8" and cu.level_class(12000, 256, False) == "Quad"
    assert cu.level_class(9984, 0, True) == "Quad" and cu.level_class(16384, 0, True) == "Glds8"
    assert cu.level0_chunks(140000) == [32768, 107232] and cu.level0_chunks(52000) == [32768, 19232]
    assert cu.level0_chunks(33000) == [33000] and cu.level0_chunks(49151) == [49151]
    assert cu.level0_chunks(49152) == [32768, 16384] and cu.level0_chunks(1) == [1]


def test_designed_shapes_reach_their_classes_on_256_compute_units():
    for name, d in cu.designed(256).items():
        f = _forest(name)
        classes = [c for _, _, c in cu.launch_classes(d["counts"], 256, cu.glds_eligible(0, f.blocks))]
        assert cu.kinds(classes) == d["kinds"], (name, classes)
        assert classes == d.get("waves_256", classes), (name, classes)


@pytest.mark.parametrize("how", cu.ARRANGEMENTS)
@pytest.mark.parametrize("name", list(cu.designed()) + list(SMALL))
def test_host_leg_designed_forests(name, how):
    """Threads 1 (storm's serial loop), 3 and 0 (the pool) against one oracle run."""
    f = _forest(name)
    recs = cu.arrange(f.blocks, how, np.random.default_rng(7), n0=f.counts[0])
    want = cu.expected_commit(f.arena, recs, f.revision, f.last)
    for threads in (1, 3, 0):
        cu.check_commit(cu.host_run(threads), f.arena, recs, f.revision, f.last, want=want)


@pytest.mark.parametrize("name", ["chain", "deep"])
def test_oracle_agrees_with_its_python_restatement(name):
    """The C oracle against oracle.commit_py, once on the chain and once on the 3,000-level
    shape (one block per height: 3,000 levels of one block each for every leg)."""
    f = _forest(name)
    recs = cu.arrange(f.blocks, "shuffled", np.random.default_rng(8), n0=f.counts[0])
    want = cu.expected_commit(f.arena, recs, f.revision, f.last)
    fields = ("data_offset", "origin_pointer", "origin_type", "parent", "address", "birth_revision", "length", "type")
    cols = [recs[k].tolist() for k in fields]
    rows = [dict(zip(fields, v)) for v in zip(*cols)]
    arena = bytearray(f.arena.tobytes())
    cs, last = o.commit_py(arena, rows, f.revision, f.last)
    assert cs == want.checksums.tolist() and last == want.last
    assert [r["address"] for r in rows] == want.records["address"].tolist()
    assert [r["birth_revision"] for r in rows] == want.records["birth_revision"].tolist()
    assert bytes(arena) == want.arena.tobytes()


@pytest.mark.parametrize("seed", range(cu.FUZZ_SEEDS))
def test_host_leg_seeded_forests(seed):
    recs, f, case = cu.seeded_forest(seed)
    leg, _ = sc.plan_commit(recs)  # raises on EINVAL: the router prices every such forest
    assert leg in (_lib.LEG_HOST, _lib.LEG_DEVICE, _lib.LEG_SPLIT)
    want = cu.expected_commit(f.arena, recs, f.revision, f.last)
    for threads in (1, 0):
        cu.check_commit(cu.host_run(threads), f.arena, recs, f.revision, f.last, want=want)


def test_seeded_cases_cover_every_class_and_argument():
    """What the 40 draws reach together, so that a change to the draw cannot quietly narrow it."""
    cases = [cu.seeded_case(s) for s in range(cu.FUZZ_SEEDS)]
    assert {len(c["counts"]) for c in cases} == set(range(1, 7))
    assert {c["align"] for c in cases} == {"16", "8", "mixed"} and {c["how"] for c in cases} == set(cu.ARRANGEMENTS)
    assert {c["p_reloc"] for c in cases} == {0.0, 0.3, 1.0}
    assert {c["lengths"] for c in cases} == {"edge", "short", "long"}
    assert any(c["p_reloc"] == 0.0 and c["how"] == "children_first" for c in cases)  # identity order, plain copy
    seen = set()
    for s, c in enumerate(cases):
        eligible = False
        if c["align"] == "16" and c["slot"] > cu.VAR_MIN_LEN:  # decided by the forest as built, not by the draw
            eligible = cu.glds_eligible(0, cu.seeded_forest(s)[0])
        seen |= {k for _, _, k in cu.launch_classes(c["counts"], 256, eligible)}
    assert {"Wide", "Multi5", "Multi8", "Quad"} <= seen and any(k.startswith("Glds") for k in seen)
    assert max(sum(c["counts"]) * c["slot"] for c in cases) < cu.MAX_ARENA


RANGE, ORIGIN, CYCLE = "parent index out of range", "origin_pointer must be 8-byte aligned", "parent links form a cycle"


@pytest.mark.parametrize("defect,text", [("range", RANGE), ("cycle", CYCLE), ("origin", ORIGIN)])
def test_both_legs_refuse_a_damaged_irregular_forest_alike(defect, text):
    """tests/test_commit.py's refusal rule on seeded forest 12 (six heights, shuffled): a
    parent out of range, a two-cycle among upper blocks, an odd origin_pointer. Both legs
    return EINVAL with the same message and leave the records and the counter as given (the
    device leg validates before it looks for a device; its arena here is no memory at all)."""
    recs, f, case = cu.seeded_forest(12)
    b = recs.copy()
    h = sc.commit_heights(b)
    victim = int(np.flatnonzero((h == 0) & (b["parent"] >= 0))[len(b) // 7])
    if defect == "range":
        b["parent"][victim] = len(b)
    elif defect == "origin":
        b["origin_pointer"][victim] += 5
    else:
        u = int(np.flatnonzero(h == 2)[3])
        v = int(b["parent"][u])
        assert v >= 0 and h[v] > 2
        b["parent"][v] = u  # u -> v -> u
    keep = b.copy()
    cs = np.zeros(len(b), dtype=np.uint64)
    said = []
    for leg in ("device", "host"):
        la = ctypes.c_uint64(f.last)
        if leg == "device":
            rc = _lib.lib.stormck_commit_device(1 << 20, b.ctypes.data, len(b), f.revision, ctypes.byref(la),
                                                cs.ctypes.data, None)
        else:
            rc = _lib.lib.stormck_commit_host(1 << 20, b.ctypes.data, len(b), f.revision, ctypes.byref(la),
                                              cs.ctypes.data, 0)
        assert rc == _lib.EINVAL, leg
        said.append(_lib.last_error())
        assert la.value == f.last and np.array_equal(b, keep) and not cs.any(), leg
    assert said[0] == said[1] and said[0].startswith(text), said
