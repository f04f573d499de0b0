"""Scrub under mass damage, host leg (CPU): contested references, seeded damage fuzz, entries
past lane 63, rows 8 bytes off a 16-byte boundary and the bytes the library's own commit
wrote. For every case the host leg's report and reachable bitmap, on 1 and on 5 threads,
equal the pure-Python reference's exactly (tests/scrub_util.py). The same cases run on the
device in tests/test_scrub_damage_gpu.py."""
import numpy as np
import pytest

from storm_amd import _lib, commit, scrub
from storm_amd.scrub import MISMATCH
from tests import scrub_util as su


def host(case, threads):
    if case.tree is None:
        return scrub.scrub_host(case.img, case.lay, threads=threads, reachable=True)
    return scrub.scrub_tree_host(case.img, case.lay, *case.tree, threads=threads, reachable=True)


def same_as_reference(case):
    """Host leg on 1 and 5 threads == reference; returns (reference report, index)."""
    want, want_bitmap, index = case.reference()
    for threads in (1, 5):
        rep = host(case, threads)
        assert rep.as_dict() == want, threads
        assert np.array_equal(rep.reachable, want_bitmap), threads
        assert rep.ok == (rep.code == _lib.OK) == (want["n_mismatch"] + want["n_structural"] == 0)
    for field, value in case.expect.items():
        assert want[field] == value, field
    return want, index


@pytest.mark.parametrize("name", list(su.CONTESTED))
def test_contested_references(name):
    want, _ = same_as_reference(su.edited(*su.CONTESTED[name]))
    assert want["n_structural"] + want["n_mismatch"] >= 3


@pytest.mark.parametrize("seed", range(su.FUZZ_SEEDS))
@pytest.mark.parametrize("name", su.FUZZ_IMAGES)
def test_damage_fuzz(name, seed):
    want, index = same_as_reference(su.fuzz_case(name, seed))
    su.check_fuzz_reference(name, seed, want, index)


@pytest.mark.parametrize("name", [n for n in su.FUZZ_IMAGES if su.intact_case(n).lay.n_blocks >= 1000])
def test_damage_fuzz_leaves_most_trees_alive(name):
    """The fuzz does not hide behind dead roots: in at least 90 % of an image's cases the
    reference still verifies at least half of the blocks."""
    def make(seed):
        want, _, index = su.fuzz_case(name, seed).reference()
        su.check_fuzz_reference(name, seed, want, index)
    assert su.still_alive(name, make) >= 0.9


def test_wide_store_is_intact():
    case = su.intact_case("wide_store")
    want, index = same_as_reference(case)
    assert want["first_error"] == 0 and want["n_mismatch"] + want["n_structural"] == 0 and want["levels"] == 4
    assert su.kind_lens(case.lay)[:2] == [3256, 5048]
    kids = dict(su._kids(index, su.wide_pointer_block(index)))
    assert sorted(kids) == [0] + list(su.WIDE_SLOTS)
    entries = dict(su._kids(index, su.wide_first_spacelist(index)))
    assert all(2 * s + which in entries for s, which in su.WIDE_SPACES.items())


@pytest.mark.parametrize("name", list(su.WIDE_DAMAGE))
def test_wide_store_damage_past_lane_63(name):
    parent_of, slot, kind = su.WIDE_DAMAGE[name]
    want, _ = same_as_reference(su.edited("wide_store", su.place_damage(parent_of, slot, kind)))
    assert want["first_slot"] == slot and want["first_parent"] > 0


@pytest.mark.parametrize("name", list(su.F1200_DAMAGE))
def test_f1200_damage_past_lane_63(name):
    want, _ = same_as_reference(su.edited("f1200", su.F1200_DAMAGE[name]))
    assert want["first_slot"] == int(name.split()[1])


def test_rows_8_bytes_off_a_16_byte_boundary():
    img, lay, root, root_type, leaf_len = su.odd_stride_tree()
    assert lay.block_size % 16 == 8
    want, _ = same_as_reference(su.Case(img, lay, (root, root_type, scrub.BLOB, leaf_len),
                                        dict(verified=(66, 0, 0, 300), first_error=0)))
    bad = img.copy()
    bad[151 * lay.block_size + 2055] ^= 1  # the last byte of leaf 151, whose row starts 8 bytes off
    same_as_reference(su.Case(bad, lay, (root, root_type, scrub.BLOB, leaf_len),
                              dict(verified=(66, 0, 0, 299), first_error=MISMATCH, first_address=151, n_mismatch=1)))


@pytest.mark.parametrize("n,F,slot,L", su.ROUND_TRIPS)
def test_commit_then_scrub(n, F, slot, L):
    """stormck_commit_host scatters Pointers and type bytes into the parents; the scrub reads
    them back from the same bytes."""
    blocks, arena, last, levels = su.forest_arena(n, F, slot, L)
    commit.commit_host(arena, blocks, 1, last)
    case = su.committed_tree(arena, n, F, slot, L, levels)
    assert case.tree[0][1] == n + sum(levels) and case.tree[1] == (1 if n > 1 else 2)
    if slot <= 2056:
        same_as_reference(case)
    for threads in (1, 5):
        rep = host(case, threads)
        assert rep.ok and su.popcount(rep.reachable) == case.lay.n_blocks
        for field, value in case.expect.items():
            assert getattr(rep, field) == value, field
