"""Lookup under fuzz, host leg (CPU): key trees under the scrub's seeded ``random_damage`` and
leaves whose every field may be arbitrary (tests/lookup_util.py ``damaged_tree_case`` and
``leaf_fuzz_case``). For every case and both ``verify_leaves`` settings stormck_lookup_host gives
the records, the report, the return code and the message of the pure-Python reference, on one
thread as on the pool. The conditions at the end say, from the reference alone, what the random
leaves reach. The same cases run on the device in tests/test_lookup_fuzz_gpu.py."""
import pytest

from storm_amd.scrub import POINTER
from storm_amd.trace import ABSENT, FOUND
from tests import lookup_util as lu

VERIFY = pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])


def same_as_reference(case):
    records, report = lu.host_lookup(case)
    lu.check_against_reference(case, records, report)
    one, rep1 = lu.host_lookup(case, threads=1)
    assert one.tobytes() == records.tobytes() and rep1.as_dict() == report.as_dict()
    assert (rep1.code, rep1.message) == (report.code, report.message)
    assert not records["reserved"].any()


@VERIFY
@pytest.mark.parametrize("seed", range(lu.DAMAGED_TREE_SEEDS))
def test_damaged_tree(seed, verify_leaves):
    same_as_reference(lu.damaged_tree_case(seed, verify_leaves))


@VERIFY
@pytest.mark.parametrize("C, seed", lu.leaf_fuzz_ids())
def test_random_leaves(C, seed, verify_leaves):
    case = lu.leaf_fuzz_case(C, seed, verify_leaves)
    same_as_reference(case)
    _, rep, _ = lu.reference_of(case)
    assert rep["n_probed"] == len(case.keys)  # the leaves verify: every key is probed


def test_damaged_trees_mix_key_with_the_trace_statuses():
    """Some call holds a KEY key beside keys the trace ended badly, on either side of it."""
    before = after = 0
    for seed in range(1, lu.DAMAGED_TREE_SEEDS, 2):
        res, rep, _ = lu.reference_of(lu.damaged_tree_case(seed))
        key = next(i for i, r in enumerate(res) if r[5] == lu.KEY)
        bad = [i for i, r in enumerate(res) if r[5] in lu.ks.BAD and i != key]
        assert rep["n_status"][lu.KEY] == 1
        before += bool(bad) and bad[0] < key
        after += bool(bad) and bad[0] > key
    assert before and after, (before, after)


def test_unverified_damaged_trees_probe_blocks_that_are_no_leaves():
    """With the leaves unverified some keys are probed (probes > 0) in a block the intact tree
    holds as a pointer block: its bytes read as a leaf."""
    index = lu._stored_index()
    probed = 0
    for seed in range(lu.DAMAGED_TREE_SEEDS):
        res, _, _ = lu.reference_of(lu.damaged_tree_case(seed, False))
        probed += sum(1 for r in res if r[4] > 0 and r[1] in index and index[r[1]][2] == POINTER)
    assert probed >= 1


def test_random_leaves_reach_what_they_are_for():
    """Over all C = 10 and C = 40 cases: at least 25 % of the keys end FOUND and at least 25 %
    ABSENT, at least 20 % of the cases hold a malformed item, and a key ends NO_SLOT after C
    probes."""
    found = absent = keys = cases = with_malformed = no_slot = 0
    for C, seed in lu.leaf_fuzz_ids():
        if C == 600:
            continue
        res, rep, _ = lu.reference_of(lu.leaf_fuzz_case(C, seed))
        cases += 1
        keys += len(res)
        found += rep["n_status"][FOUND]
        absent += rep["n_status"][ABSENT]
        with_malformed += rep["n_malformed"] >= 1
        no_slot += sum(1 for r in res if r[3] == lu.NO_SLOT and r[4] == C and r[5] == ABSENT)
    assert cases == 120 and found + absent == keys == 6000
    assert found >= 0.25 * keys and absent >= 0.25 * keys, (found, absent)
    assert with_malformed >= 0.2 * cases, with_malformed
    assert no_slot >= 1
