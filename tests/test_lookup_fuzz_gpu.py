"""Lookup under fuzz on the device (MI355X): the cases of tests/test_lookup_fuzz.py through
stormck_lookup_device, which must give the result bytes, the report, the return code and the
message of the host leg and of the pure-Python reference.

Every device call of this module is given the same workspace tensor: sized for the largest
case, filled with 0xA5 bytes once and never cleared, so the trace's table, rows and counters and
the lookup's tags, trace results, table and counters of one case are what the next case finds.

No case can make the device read outside its tensor: each image is uploaded at exactly its
size, n_blocks + SLACK blocks; a reference at or past n_blocks ends RANGE unread; a block that
is probed lies below n_blocks, and a probe stays inside the first leaf_len(C) <= block_size
bytes of it whatever they hold. ``lookup_util.assert_inside`` checks on the host, when a case is
built, that every reference a walk ends at names a block of the tensor."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import keystore as ks  # noqa: E402
from tests import lookup_util as lu  # noqa: E402
from tests import scrub_util as su  # noqa: E402
from tests.test_lookup_gpu import same_everywhere  # noqa: E402

MAX_KEYS = 170
VERIFY = pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])
_workspace = []


def dirty_workspace(case):
    if not _workspace:
        need = max(ks.workspace_bytes(MAX_KEYS, C) for C, _ in lu.LEAF_FUZZ)
        _workspace.append(torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda"))
    ws = _workspace[0]
    assert len(case.keys) <= MAX_KEYS and ws.numel() >= ks.workspace_bytes(len(case.keys), case.tree.C)
    return ws  # large enough: the call uses it and allocates none of its own


def on_device_as_it_is(case):
    t = case.tree
    assert t.img.size == (t.lay.n_blocks + su.SLACK) * t.lay.block_size
    same_everywhere(case, workspace=dirty_workspace(case))


@VERIFY
@pytest.mark.parametrize("seed", range(lu.DAMAGED_TREE_SEEDS))
def test_damaged_tree(seed, verify_leaves):
    on_device_as_it_is(lu.damaged_tree_case(seed, verify_leaves))


@VERIFY
@pytest.mark.parametrize("C, seed", lu.leaf_fuzz_ids())
def test_random_leaves(C, seed, verify_leaves):
    on_device_as_it_is(lu.leaf_fuzz_case(C, seed, verify_leaves))
