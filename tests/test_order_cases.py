"""The designed inputs of the gather-order tests (tests/order_cases.py) have exactly the
bucket and sub-bucket populations they claim, recomputed here with np.bincount: the GPU
tests (tests/test_gather_order_gpu.py) then cannot silently stop reaching a branch of
k_order_sort (CPU checks)."""
import numpy as np
import pytest

from tests import order_cases as oc

BUILDERS = {"small": oc.small, "designed": oc.designed, "big": oc.big, "arena_lens": oc.arena_lens,
            "arena_uniform_4112": lambda: oc.arena_uniform(4112), "arena_uniform_60000": lambda: oc.arena_uniform(60000)}


def _populations(offs):
    b, s = oc.bucket_of(offs), oc.sub_of(offs)
    count = np.bincount(b, minlength=oc.BUCKETS)
    longest = np.bincount(b * oc.SUBS + s, minlength=oc.BUCKETS * oc.SUBS).reshape(oc.BUCKETS, oc.SUBS).max(axis=1)
    return count, longest


@pytest.fixture(scope="module", params=sorted(BUILDERS))
def case(request):
    return BUILDERS[request.param]()


def test_claimed_populations(case):
    count, longest = _populations(case.offs)
    claimed = set()
    for c in case.claims:
        assert c.bucket not in claimed, c
        claimed.add(c.bucket)
        if c.count < 0:  # filler: far over the sort limit
            assert count[c.bucket] > 10_000, (c, int(count[c.bucket]))
            assert c.path == "placement"
            continue
        assert (int(count[c.bucket]), int(longest[c.bucket])) == (c.count, c.longest), c
        assert oc.sort_path(c.count, c.longest) == (c.path, c.padded), c
    rest = np.ones(oc.BUCKETS, dtype=bool)
    rest[sorted(claimed)] = False
    assert not count[rest].any(), "every unclaimed bucket is empty"
    assert count[0] == 0 and int((count == 0).sum()) >= oc.BUCKETS - 64  # empty buckets, the first included
    # the designed mask marks the claimed, non-filler buckets' entries and nothing else
    designed_buckets = [c.bucket for c in case.claims if c.count >= 0 and "filler" not in c.what]
    assert np.array_equal(case.designed, np.isin(oc.bucket_of(case.offs), designed_buckets))


def test_every_branch_and_boundary_is_in_the_large_cases():
    """The boundaries the order tests exist for, by name and by number."""
    for case in (oc.designed(), oc.big()):
        by = {(c.path, c.count, c.longest, c.padded) for c in case.claims if c.count >= 0}
        assert ("counting", 1, 1, 0) in by                      # a bucket of 1 entry
        assert ("counting", 2048, 2, 0) in by                   # the counting path at kOrderSortMax
        assert ("placement", 2049, 3, 0) in by                  # one over: placement order
        assert any(p == "counting" and l == 16 for p, _, l, _ in by)  # the insertion path at kOrderRunMax
        assert ("bitonic", 1500, 17, 2048) in by                # one run of 17: padded to 2,048
        assert ("bitonic", 2048, 2048, 2048) in by              # the network's size equals the count
        assert ("bitonic", 17, 17, 32) in by                    # ties
        assert ("bitonic", 33, 33, 64) in by                    # padded to 64
        count, _ = _populations(case.offs)
        assert count[4095] > 0                                  # the last bucket
        region_bits = case.offs & np.uint64(oc.REGION - 1)
        assert (region_bits == np.uint64(oc.REGION - 1)).any()  # all 25 region bits set
        assert (case.offs >= np.uint64(1 << 40)).any()          # past 2^40
        ties = case.offs[oc.bucket_of(case.offs) == 7]
        assert ties.size == 17 and np.unique(ties).size == 1
        dense = np.sort(case.offs[oc.bucket_of(case.offs) == 6])
        assert np.all(np.diff(dense) == 16)
        for b in (50, 51):  # one bucket, two regions exactly 128 GiB apart
            regions = np.unique(case.offs[oc.bucket_of(case.offs) == b] >> np.uint64(oc.SHIFT))
            assert regions.tolist() == [b, b + oc.BUCKETS]
        lo = case.offs[(case.offs >> np.uint64(oc.SHIFT)) == 50] & np.uint64(oc.REGION - 1)
        hi = case.offs[(case.offs >> np.uint64(oc.SHIFT)) == 50 + oc.BUCKETS] & np.uint64(oc.REGION - 1)
        assert np.intersect1d(lo, hi).size >= 50                # equal keys from the two regions


def test_sizes_and_parts():
    small, big = oc.small(), oc.big()
    assert small.n == 300 and big.n == (1 << 20) + 37
    # n = 300 over 512 parts: part w holds [300 w / 512, 300 (w + 1) / 512), 0 or 1 element
    sizes = [300 * (w + 1) // 512 - 300 * w // 512 for w in range(512)]
    assert set(sizes) == {0, 1}
    # lengths are carried, never read: the order-only cases use the whole 32-bit range
    assert int(big.lens.max()) > 1 << 31
    count, _ = _populations(big.offs)
    fill = count[oc.FILL_FIRST:oc.FILL_FIRST + oc.FILL_REGIONS]
    assert fill.min() > 10_000 and fill.sum() == big.n - int(big.designed.sum())


def test_arena_cases_fit_the_arena():
    c = oc.arena_lens()
    assert c.n == oc.N_BIG and oc.ARENA_BYTES == 1088 << 20
    ends = c.offs.astype(np.int64) + c.lens.astype(np.int64)
    assert ends.max() <= oc.ARENA_BYTES
    lens = c.lens
    for lo, hi in ((0, 31), (32, 600), (601, 4200)):
        assert ((lens >= lo) & (lens <= hi)).mean() > 0.2
    assert ((lens % 512 == 0) & (lens > 0)).mean() > 0.2 and lens.max() <= 4200
    total = int(lens.astype(np.int64).sum())
    assert 1 << 30 <= total <= 3 << 29, total  # about 1 GiB hashed by the device
    low4 = (c.offs & np.uint64(15)).astype(np.int64)
    share = (low4[~c.designed] != 0).mean()
    assert 0.02 < share < 0.04 and set(np.unique(low4[~c.designed])) == {0, 1, 4, 8, 12}
    pairs = np.unique(np.stack([c.offs, c.lens.astype(np.uint64)]), axis=1).shape[1]
    assert pairs <= 210_000  # what the oracle hashes
    for length in (4112, 60000):
        u = oc.arena_uniform(length)
        assert u.n == oc.N_BIG and np.unique(u.offs).size <= 16384
        assert not (u.offs & np.uint64(15)).any() and int(u.offs.max()) + length <= oc.ARENA_BYTES
        assert np.unique(u.offs).size * length <= 10**9  # the oracle hashes at most 1 GB
