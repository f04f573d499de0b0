"""Trace under seeded damage, host leg (CPU): trees f10, f64 and f65 after the scrub's
``random_damage`` (tests/scrub_util.py), traced for tag lists that mix present tags, random
ones and near misses of present ones (tests/trace_util.py ``fuzz_case``). For every case and
both ``verify_leaves`` settings the host leg's result records, report and leaf checksums equal
the pure-Python reference's, on one thread and on the pool. The conditions at the end say, from
the reference alone, that the fuzz does not hide behind dead trees and does mix bad statuses in
one call. The same cases run on the device in tests/test_trace_fuzz_gpu.py."""
import numpy as np
import pytest

from storm_amd import _lib, trace
from storm_amd.trace import ABSENT, BAD, FOUND, MISMATCH, RANGE, TYPE
from tests import trace_util as tu

SEEDS = range(tu.FUZZ_SEEDS)
CONDITION_IMAGES = ("f10", "f64")  # f65 has 10 blocks and 4 present tags: exempt


def host(tree, tags, verify_leaves, threads):
    return trace.trace_host(tree.img, *tree.args(), tu.tags_u64(tags), tree.leaf_len, verify_leaves, threads,
                            leaf_checksums=True)


def same_as_reference(tree, tags, verify_leaves):
    want, want_rep, refs, want_cs = tree.reference(tags, verify_leaves)
    res, rep = host(tree, tags, verify_leaves, 0)
    assert tu.as_tuples(res) == want
    assert rep.as_dict() == want_rep
    assert sum(rep.blocks_hashed) == len(refs)
    assert [int(c) for c in rep.leaf_checksums] == want_cs
    assert not res["reserved"].any()
    bad = [i for i, r in enumerate(want) if r[5] in BAD]
    assert rep.first_bad == (bad[0] if bad else len(tags))
    assert rep.code == (_lib.EMISMATCH if bad else _lib.OK) and bool(rep.message) == bool(bad)
    if bad:  # the message is the first bad tag's, not another's
        address, _, parent, slot, _, status = want[bad[0]]
        assert {MISMATCH: "checksum mismatch for block %d," % address,
                RANGE: "block %d does not exist (block %d, slot %d)" % (address, parent, slot),
                TYPE: "block %d, slot %d" % (parent, slot)}[status] in rep.message
    one, rep1 = host(tree, tags, verify_leaves, 1)
    assert one.tobytes() == res.tobytes() and rep1.as_dict() == rep.as_dict()
    assert np.array_equal(rep1.leaf_checksums, rep.leaf_checksums) and (rep1.code, rep1.message) == (rep.code, rep.message)
    return want_rep


@pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", tu.FUZZ_IMAGES)
def test_damage_fuzz(name, seed, verify_leaves):
    tree, tags = tu.fuzz_case(name, seed)
    same_as_reference(tree, tags, verify_leaves)


# ---- conditions on the generator, from the reference alone ---------------------------------------

@pytest.mark.parametrize("name", CONDITION_IMAGES)
def test_fuzz_leaves_most_tags_found(name):
    """In at least 90 % of an image's seeds at least half of the tags end FOUND."""
    alive = 0
    for seed in SEEDS:
        n_status = tu.fuzz_n_status(name, seed)
        alive += 2 * n_status[FOUND] >= sum(n_status)
    assert alive / len(SEEDS) >= 0.9


def test_fuzz_meets_every_status_and_mixes_the_bad_ones():
    """Over all seeds of f10 and f64: each of FOUND, ABSENT, MISMATCH, RANGE and TYPE occurs, and
    at least 10 cases hold two or more different bad statuses in one call."""
    total, mixed = [0] * 7, 0
    for name in CONDITION_IMAGES:
        for seed in SEEDS:
            n_status = tu.fuzz_n_status(name, seed)
            total = [a + b for a, b in zip(total, n_status)]
            mixed += sum(1 for s in BAD if n_status[s]) >= 2
    assert all(total[s] > 0 for s in (FOUND, ABSENT, MISMATCH, RANGE, TYPE)), total
    assert mixed >= 10, mixed
