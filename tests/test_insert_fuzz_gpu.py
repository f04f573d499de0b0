"""Seeded fuzz of the insert on the device (MI355X): a dozen seeds of tests/test_insert_fuzz.py
through stormck_insert_device, compared with the host leg and the pure-Python reference byte for
byte (tests/test_insert_gpu.py ``device_insert``)."""
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from tests import insert_util as iu  # noqa: E402
from tests.test_insert_gpu import device_insert  # noqa: E402


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(seed):
    iu.run_fuzz(seed, run=device_insert)
