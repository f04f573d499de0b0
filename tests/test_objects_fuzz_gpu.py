"""Objects under fuzz on the device (MI355X): the cases of tests/test_objects_fuzz.py through
stormck_objects_device, which must give the result bytes, the row bytes, the report, the return
code and the message of the host leg and of the pure-Python reference, in the dirty workspace of
tests/test_objects_gpu.py.

No case can make the device read outside its tensor: each image is uploaded at exactly its
size, n_blocks + SLACK blocks; a reference at or past n_blocks ends RANGE unread; a block that
is probed lies below n_blocks, and a probe and the object it finds stay inside the first
N * stride <= blob_len - 8 <= block_size bytes of it whatever they hold.
``objects_util.assert_inside`` checks on the host, when a case is built, that every reference a
walk ends at names a block of the tensor. ``test_fuzz_reaches_what_it_is_for`` of
tests/test_objects_fuzz.py is the condition on these inputs; it needs no device."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import objects_util as ou  # noqa: E402
from tests import scrub_util as su  # noqa: E402
from tests.test_objects_gpu import same_everywhere  # noqa: E402

VERIFY = pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])


def on_device_as_it_is(case):
    t = case.tree
    assert t.img.size == (t.lay.n_blocks + su.SLACK) * t.lay.block_size
    same_everywhere(case)


@VERIFY
@pytest.mark.parametrize("seed", range(ou.DAMAGED_TREE_SEEDS))
def test_damaged_tree(seed, verify_leaves):
    on_device_as_it_is(ou.damaged_tree_case(seed, verify_leaves))


@VERIFY
@pytest.mark.parametrize("N, S, seed", ou.leaf_fuzz_ids())
def test_random_leaves(N, S, seed, verify_leaves):
    on_device_as_it_is(ou.leaf_fuzz_case(N, S, seed, verify_leaves))
