"""Trace under seeded damage on the device (MI355X): the cases of tests/test_trace_fuzz.py
through stormck_trace_device, which must give the result bytes, the report, the leaf checksums,
the return code and the message of the host leg and of the pure-Python reference.

Every device call of this module is given the same workspace tensor: sized for the largest tag
count, filled with 0xA5 bytes once and never cleared, so the table keys, the key_row entries,
the rows and the counters one case leaves are what the next case finds.

No case can make the device read outside its tensor: each damaged image is uploaded at exactly
its size, n_blocks + SLACK blocks, a reference at or past n_blocks ends RANGE unread, and
``trace_util.assert_inside`` checks on the host, before the upload, that every entry the damage
wrote names a block of the tensor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import trace  # noqa: E402
from tests import scrub_util as su  # noqa: E402
from tests import trace_util as tu  # noqa: E402
from tests.test_trace_gpu import same_everywhere  # noqa: E402

_workspace = []


def dirty_workspace():
    if not _workspace:
        need = trace.workspace_bytes(max(tu.FUZZ_TAG_COUNTS))
        _workspace.append(torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda"))
    return _workspace[0]


@pytest.mark.parametrize("verify_leaves", [True, False], ids=["verified", "unverified"])
@pytest.mark.parametrize("seed", range(tu.FUZZ_SEEDS))
@pytest.mark.parametrize("name", tu.FUZZ_IMAGES)
def test_damage_fuzz(name, seed, verify_leaves):
    tree, tags = tu.fuzz_case(name, seed)  # asserts that the damage stays inside the image
    ws = dirty_workspace()
    assert ws.numel() >= trace.workspace_bytes(len(tags))  # the call uses it and allocates none of its own
    assert tree.img.size == (tree.lay.n_blocks + su.SLACK) * tree.lay.block_size
    image = torch.from_numpy(np.array(tree.img)).cuda()
    assert image.numel() == tree.img.size
    same_everywhere(tree, tags, image, verify_leaves=verify_leaves, workspace=ws)
