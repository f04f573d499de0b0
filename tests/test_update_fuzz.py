"""Seeded fuzz of the update on the host leg (CPU only): random subsets of the keys with repeats,
absent keys mixed in and random rows over the get's store and a depth-1 store
(tests/update_util.py ``fuzz_case``). Host leg == ``reference_update``, plus ``check_update``. The
conditions that keep the fuzz from going hollow are asserted on the reference alone."""
import functools

import pytest

from tests import objects_util as ou
from tests import scrub_util as su
from tests import update_util as uu


@pytest.mark.parametrize("seed", range(uu.FUZZ_SEEDS))
def test_seed(seed):
    uu.run_fuzz(seed)


@functools.lru_cache(maxsize=None)
def facts():
    """Per seed, from the reference alone: (n_written, has SUPERSEDED, has NONE, pointer blocks
    with a dirty leaf, every leaf of the tree dirty)."""
    out = []
    for seed in range(uu.FUZZ_SEEDS):
        store, keys, rows, pool = uu.fuzz_case(seed)
        img, lay = uu.roomy(store, 120)
        res, _, rep, code, _, _ = uu.reference_update(img, lay, ou.GET_SPACE, store, keys, rows)
        assert code == uu.OK
        index = su.reference_scrub(img, lay)[2]
        leaves = {r[2] for r in res if r[6] == uu.WRITTEN}
        all_leaves = {int(r["object_address"]) for r in uu._get(img, lay, store, ou.GET_SPACE, pool)[0]}
        out.append((rep["n_written"], any(r[6] == uu.SUPERSEDED for r in res), any(r[6] == uu.NONE for r in res),
                    len({index[a][0] for a in leaves}), leaves == all_leaves))
    return out


def test_the_fuzz_reaches_what_it_is_for():
    f = facts()
    assert len(f) >= 40 and all(w >= 1 for w, _, _, _, _ in f)
    assert sum(s for _, s, _, _, _ in f) >= 10
    assert sum(n for _, _, n, _, _ in f) >= 10
    assert sum(p >= 2 for _, _, _, p, _ in f) >= 10   # dirty leaves under different pointer blocks
    assert sum(a for _, _, _, _, a in f) >= 5          # every leaf of the tree dirty
