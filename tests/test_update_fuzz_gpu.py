"""The seeded fuzz of tests/test_update_fuzz.py on the device (MI355X): the same seeds, device ==
host leg == reference on the image bytes, results, report, code and message, plus
``check_update`` on the downloaded image."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import update_util as uu  # noqa: E402
from tests.test_update_gpu import device_update  # noqa: E402


@pytest.mark.parametrize("seed", range(uu.FUZZ_SEEDS))
def test_seed(seed):
    uu.run_fuzz(seed, run=device_update)
