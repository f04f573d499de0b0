"""Seeded fuzz of the insert on the host leg (CPU only): random stores (tree depths, fill levels,
damaged free lists, Invalid and unknown slot states) and random batches (key lengths on both sides
of the chunk size, repeats, existing keys) through stormck_insert_host, against
tests/insert_util.py ``reference_insert`` byte for byte and through ``check_insert``. One test
asserts, from the reference alone, that the generator reaches what it is meant to reach."""
import functools

import pytest

from tests import insert_util as iu
from tests import update_util as uu


@pytest.mark.parametrize("seed", range(iu.FUZZ_SEEDS))
def test_fuzz(seed):
    iu.run_fuzz(seed)


@functools.lru_cache(maxsize=None)
def _reference(seed):
    store, keys, rows, _, space_id = iu.fuzz_case(seed)
    img, lay = uu.roomy(store, 160)
    return iu.reference_insert(img, lay, space_id, store, keys, rows)


def test_the_generator_reaches_every_verdict():
    actions, reasons, inserting, cutting = set(), set(), 0, 0
    for seed in range(iu.FUZZ_SEEDS):
        results, _, rep, code, _, _, _ = _reference(seed)
        assert code == iu.OK
        actions |= {r[7] for r in results}
        reasons |= {r[8] for r in results if r[7] == iu.NONE}
        inserting += rep["n_inserted"] >= 1
        cutting += rep["limit"] < len(results) and any(r[8] == iu.R_CUT for r in results)
    assert actions == {iu.NONE, iu.INSERTED, iu.REPEATED}
    assert reasons >= set(range(1, 10)) - {iu.R_CROWDED}, reasons
    assert 2 * inserting >= iu.FUZZ_SEEDS and 4 * cutting >= iu.FUZZ_SEEDS, (inserting, cutting)
