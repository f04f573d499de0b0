"""Objects under fuzz, host leg (CPU): object trees under the scrub's seeded ``random_damage`` and
blob leaves whose states and reminders are edited at random (tests/objects_util.py
``damaged_tree_case`` and ``leaf_fuzz_case``). For every case and both ``verify_leaves`` settings
stormck_objects_host gives the records, the rows, the report, the return code and the message of
the pure-Python reference, on one thread as on the pool. ``test_fuzz_reaches_what_it_is_for`` is
the condition on the inputs, from the reference alone. The same cases run on the device in
tests/test_objects_fuzz_gpu.py."""
import pytest

from storm_amd.scrub import POINTER
from tests import objects_util as ou

VERIFY = pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])


def same_as_reference(case):
    records, objects, report = ou.host_objects(case)
    ou.check_against_reference(case, records, objects, report)
    one, rows1, rep1 = ou.host_objects(case, threads=1)
    assert one.tobytes() == records.tobytes() and rows1.tobytes() == objects.tobytes()
    assert rep1.as_dict() == report.as_dict() and (rep1.code, rep1.message) == (report.code, report.message)


def test_fuzz_reaches_what_it_is_for():
    ou.assert_fuzz_reaches()


@VERIFY
@pytest.mark.parametrize("seed", range(ou.DAMAGED_TREE_SEEDS))
def test_damaged_tree(seed, verify_leaves):
    same_as_reference(ou.damaged_tree_case(seed, verify_leaves))


@VERIFY
@pytest.mark.parametrize("N, S, seed", ou.leaf_fuzz_ids())
def test_random_leaves(N, S, seed, verify_leaves):
    same_as_reference(ou.leaf_fuzz_case(N, S, seed, verify_leaves))


def test_unverified_damaged_trees_read_blocks_that_are_no_leaves():
    """With the leaves unverified some IDs are probed (probes > 0) in a block the intact tree
    holds as a pointer block: its bytes read as a blob leaf."""
    index = ou._stored_index()
    probed = 0
    for seed in range(ou.DAMAGED_TREE_SEEDS):
        res = ou.reference_of(ou.damaged_tree_case(seed, False))[0]
        probed += sum(1 for r in res if r[4] > 0 and r[1] in index and index[r[1]][2] == POINTER)
    assert probed >= 1
