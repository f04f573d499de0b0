"""Designed inputs for the gather's locality order (kernels.h k_order_*): offsets (and
lengths) with a stated population per bucket, built with plain numpy and seeded.

bucket = (off >> 25) & 4095 (a 32 MiB region, wrapping every 128 GiB); sub-bucket =
(off & (2^25 - 1)) >> 15 (a 32 KiB slot of the region). k_order_sort takes, per bucket of
`count` entries whose fullest sub-bucket holds `longest`:

  count > 2048            the bucket stays in placement order        "placement"
  longest <= 16           counting pass + insertion per sub-bucket   "counting"
  otherwise               bitonic network padded to a power of two   "bitonic"

Every case lists what it claims (Claim); tests/test_order_cases.py recomputes the counts
with np.bincount, so the GPU tests cannot silently stop reaching a branch."""
from dataclasses import dataclass, field

import numpy as np

SHIFT, BUCKETS, SUB_SHIFT, SUBS = 25, 4096, 15, 1024
REGION = 1 << SHIFT
SORT_MAX, RUN_MAX = 2048, 16
FILL_REGIONS = 24
FILL_FIRST = 10  # the filler's regions: FILL_FIRST .. FILL_FIRST + FILL_REGIONS - 1
ARENA_BYTES = (FILL_FIRST + FILL_REGIONS) * REGION  # 1,088 MiB: the designed regions and the filler's
N_BIG = (1 << 20) + 37


def bucket_of(offs):
    return ((np.asarray(offs, dtype=np.uint64) >> np.uint64(SHIFT)) & np.uint64(BUCKETS - 1)).astype(np.int64)


def sub_of(offs):
    return ((np.asarray(offs, dtype=np.uint64) & np.uint64(REGION - 1)) >> np.uint64(SUB_SHIFT)).astype(np.int64)


def sort_path(count, longest):
    """The branch k_order_sort takes, and the bitonic network's padded size (0: none)."""
    if count == 0:
        return "empty", 0
    if count > SORT_MAX:
        return "placement", 0
    if longest <= RUN_MAX:
        return "counting", 0
    m = 2
    while m < count:
        m <<= 1
    return "bitonic", m


@dataclass
class Claim:
    bucket: int
    count: int      # entries in the bucket; -1: filler, far over the sort limit
    longest: int    # entries in its fullest sub-bucket (-1: not stated)
    path: str       # sort_path's name for it
    padded: int = 0  # bitonic: the network's size
    what: str = ""


@dataclass
class Case:
    name: str
    offs: np.ndarray  # uint64
    lens: np.ndarray  # uint32
    claims: list = field(default_factory=list)
    designed: np.ndarray = None  # bool per entry: part of a designed bucket (not filler)

    @property
    def n(self):
        return int(self.offs.size)


def _subs(region, per_sub, rng, step=16):
    """Offsets in `region` with per_sub[s] entries in sub-bucket s, 16-byte aligned, distinct
    inside a sub-bucket where it has room."""
    out = []
    for s, c in enumerate(per_sub):
        if c:
            slots = rng.choice((1 << SUB_SHIFT) // step, size=c, replace=False) * step
            out.append(region * REGION + (s << SUB_SHIFT) + slots)
    return np.concatenate(out).astype(np.uint64) if out else np.zeros(0, dtype=np.uint64)


def _pieces(rng, which):
    """The designed buckets: name -> (offsets, Claim). Regions 1..9 lie inside the arena of the
    end-to-end tests; region 0 stays empty."""
    p = {}

    def add(name, offs, bucket, longest, path, padded=0, what=""):
        offs = np.asarray(offs, dtype=np.uint64)
        if name in which:
            p[name] = (offs, Claim(bucket, int(offs.size), longest, path, padded, what))

    add("one", [1 * REGION + 5 * 32768 + 4096], 1, 1, "counting", what="a bucket of 1 entry")
    add("full_counting", _subs(2, [2] * SUBS, rng), 2, 2, "counting", what="2,048 entries, 2 per sub-bucket")
    per = np.full(SUBS, 2)
    per[513] = 3
    add("over", _subs(3, per, rng), 3, 3, "placement", what="2,049 entries: left in placement order")
    per = np.zeros(SUBS, dtype=np.int64)
    per[rng.choice(SUBS, size=100, replace=False)] = rng.integers(1, 4, size=100)
    per[5] = 16
    add("run16", _subs(4, per, rng), 4, 16, "counting", what="the fullest sub-bucket holds exactly 16")
    per = np.zeros(SUBS, dtype=np.int64)
    per[:] = 1
    per[rng.choice(SUBS, size=1500 - 17 - (SUBS - 1), replace=False)] += 1
    top = int(np.argmax(per == 1))
    per[top] = 17
    assert per.sum() == 1500 and per.max() == 17
    add("run17", _subs(5, per, rng), 5, 17, "bitonic", 2048, what="1,500 entries, one sub-bucket of 17")
    add("dense", 6 * REGION + 700 * 32768 + 16 * rng.permutation(2048), 6, 2048, "bitonic", 2048,
        what="2,048 entries 16 bytes apart in one sub-bucket: the network's size equals the count")
    add("ties", np.full(17, 7 * REGION + 9 * 32768 + 512), 7, 17, "bitonic", 32, what="17 entries, one offset")
    add("pad64", _subs(8, [0] * 77 + [33], rng), 8, 33, "bitonic", 64, what="33 entries in one sub-bucket")
    add("all_bits", [9 * REGION + REGION - 1], 9, 1, "counting", what="all 25 region bits set")
    # outside the arena: for the order pass alone
    add("last_bucket", _subs(4095, [0] * 1000 + [1, 0, 2] + [0] * 20 + [2], rng), 4095, 2, "counting",
        what="the last bucket, its last sub-bucket used")
    add("near_2_40", [(1 << 40) + 40 * REGION + 0x12350, (1 << 40) + 40 * REGION + 16], 40, 1, "counting",
        what="offsets past 2^40 (bucket 40 after the wrap)")
    # one bucket fed from two regions exactly 128 GiB apart; equal low bits on both sides
    per = np.zeros(SUBS, dtype=np.int64)
    per[rng.choice(SUBS, size=300, replace=False)] = 2
    lo = _subs(50, per, rng)
    hi = _subs(50 + BUCKETS, per, rng)
    twin = lo[:50] + np.uint64(BUCKETS * REGION)
    both = np.concatenate([lo, hi, twin])
    long50 = int(np.bincount(sub_of(both)).max())
    add("wrap", both, 50, long50, "counting", what="two regions 128 GiB apart in one bucket")
    lo = _subs(51, [0] * 3 + [12], rng)
    hi = _subs(51 + BUCKETS, [0] * 3 + [9, 4], rng)
    add("wrap_bitonic", np.concatenate([lo, hi]), 51, 21, "bitonic", 32,
        what="two regions 128 GiB apart, 21 entries in one sub-bucket")
    return p


IN_ARENA = ("one", "full_counting", "over", "run16", "run17", "dense", "ties", "pad64", "all_bits")
FAR = ("last_bucket", "near_2_40", "wrap", "wrap_bitonic")


def _assemble(name, rng, pieces, fill_offs, fill_claims, fill_lens=None, draw_lens=None):
    """The pieces and the filler in one shuffled batch. Lengths: any 32-bit value (the order
    pass only carries them), or draw_lens(count) with the filler's own fill_lens."""
    offs = np.concatenate([v[0] for v in pieces.values()] + [fill_offs])
    n_designed = offs.size - fill_offs.size
    designed = np.arange(offs.size) < n_designed
    if draw_lens is None:
        lens = rng.integers(0, 1 << 32, size=offs.size, dtype=np.uint64).astype(np.uint32)
    else:
        lens = np.concatenate([draw_lens(n_designed), fill_lens]).astype(np.uint32)
    perm = rng.permutation(offs.size)
    return Case(name, offs[perm], lens[perm], [v[1] for v in pieces.values()] + fill_claims, designed[perm])


def small(seed=1):
    """n = 300: most of the 512 parts hold 0 or 1 element."""
    rng = np.random.default_rng(seed)
    pieces = _pieces(rng, ("one", "ties", "pad64", "all_bits", "last_bucket", "near_2_40", "wrap_bitonic"))
    used = sum(v[0].size for v in pieces.values())
    per = np.zeros(SUBS, dtype=np.int64)
    per[9] = 16  # a run of exactly 16 again, in a small bucket
    per[rng.choice(np.arange(10, SUBS), size=20, replace=False)] = 1
    pieces["run16_small"] = (_subs(4, per, rng), Claim(4, 36, 16, "counting", 0, "36 entries, one run of 16"))
    used += 36
    rest = 300 - used
    regions = FILL_FIRST + rng.integers(0, 4, size=rest)
    fill = (regions * REGION + rng.integers(0, REGION // 16, size=rest) * 16).astype(np.uint64)
    claims = []
    for r in range(FILL_FIRST, FILL_FIRST + 4):
        sel = fill[bucket_of(fill) == r]
        longest = int(np.bincount(sub_of(sel)).max()) if sel.size else 0
        claims.append(Claim(r, int(sel.size), longest, *sort_path(int(sel.size), longest), "random filler"))
    case = _assemble("small", rng, pieces, fill, claims)
    assert case.n == 300
    return case


def designed(seed=2):
    """Every designed bucket, the far ones included, and nothing else (about 10,000 entries)."""
    rng = np.random.default_rng(seed)
    return _assemble("designed", rng, _pieces(rng, IN_ARENA + FAR), np.zeros(0, dtype=np.uint64), [])


def _filler(rng, count, unique=None):
    """count offsets at random in the FILL_REGIONS filler regions (16-byte aligned), drawn
    from `unique` distinct offsets when given."""
    if unique is None:
        regions = FILL_FIRST + rng.integers(0, FILL_REGIONS, size=count)
        return (regions * REGION + rng.integers(0, REGION // 16, size=count) * 16).astype(np.uint64)
    regions = FILL_FIRST + rng.integers(0, FILL_REGIONS, size=unique)
    pool = np.unique((regions * REGION + rng.integers(0, REGION // 16, size=unique) * 16).astype(np.uint64))
    return pool[rng.integers(0, pool.size, size=count)]


def _fill_claims():
    return [Claim(r, -1, -1, "placement", 0, "filler: tens of thousands of entries")
            for r in range(FILL_FIRST, FILL_FIRST + FILL_REGIONS)]


def big(seed=3):
    """2^20 + 37 entries: every designed bucket, and the rest at random in 24 further regions
    (tens of thousands each: far over the sort limit, heavy contention on the cursors)."""
    rng = np.random.default_rng(seed)
    pieces = _pieces(rng, IN_ARENA + FAR)
    used = sum(v[0].size for v in pieces.values())
    case = _assemble("big", rng, pieces, _filler(rng, N_BIG - used), _fill_claims())
    assert case.n == N_BIG
    return case


def _mixed_lens(rng, count):
    """0..31 (no stripe), 32..600, whole multiples of 512, and anything up to 4,200 B."""
    kind = rng.integers(0, 4, size=count)
    return np.where(kind == 0, rng.integers(0, 32, size=count),
                    np.where(kind == 1, rng.integers(32, 601, size=count),
                             np.where(kind == 2, rng.integers(1, 9, size=count) * 512,
                                      rng.integers(601, 4201, size=count))))


def arena_lens(seed=4):
    """The 2^20 + 37 case restricted to the 1,088 MiB arena, with per-block lengths: 0..31,
    32..600, whole multiples of 512 and anything up to 4,200 B, about 1.2 GiB in all; about
    3 % of the filler's starts at +8, +1, +4 or +12 (the designed offsets stay as they are).
    The filler repeats 200,000 (offset, length) pairs, so the oracle hashes far less than
    the device does."""
    rng = np.random.default_rng(seed)
    pieces = _pieces(rng, IN_ARENA)
    used = sum(v[0].size for v in pieces.values())
    uniq = 200_000
    u_offs = _filler(rng, uniq)
    u_lens = _mixed_lens(rng, uniq)
    odd = rng.random(uniq) < 0.03
    u_offs[odd] += rng.choice([8, 1, 4, 12], size=int(odd.sum())).astype(np.uint64)
    pick = rng.integers(0, uniq, size=N_BIG - used)
    case = _assemble("arena_lens", rng, pieces, u_offs[pick], _fill_claims(), u_lens[pick],
                     lambda count: _mixed_lens(rng, count))
    case.lens = np.minimum(case.lens.astype(np.int64), ARENA_BYTES - case.offs.astype(np.int64)).astype(np.uint32)
    assert case.n == N_BIG and int(case.offs.max()) < ARENA_BYTES
    return case


def arena_uniform(length, seed=5):
    """One length, no lens: the designed offsets (the 16-byte aligned ones, once each, so
    their buckets keep their populations) and a filler drawn from so few distinct offsets
    that at most 16,384 are unique in all. Every block ends inside the arena."""
    rng = np.random.default_rng(seed)
    pieces = _pieces(rng, tuple(k for k in IN_ARENA if k != "all_bits"))
    top = np.uint64(9 * REGION + REGION - 16)  # the last 16-byte aligned start of region 9
    pieces["last_aligned"] = (np.array([top], dtype=np.uint64), Claim(9, 1, 1, "counting", 0, "the region's last aligned start"))
    used = sum(v[0].size for v in pieces.values())
    uniq_designed = np.unique(np.concatenate([v[0] for v in pieces.values()])).size
    fill = _filler(rng, N_BIG - used, unique=16384 - uniq_designed)
    fill = np.minimum(fill, np.uint64((ARENA_BYTES - length) & ~15))
    case = _assemble(f"arena_uniform_{length}", rng, pieces, fill, _fill_claims())
    case.lens = np.full(case.n, length, dtype=np.uint32)
    assert case.n == N_BIG and np.unique(case.offs).size <= 16384 and not np.any(case.offs & np.uint64(15))
    assert int(case.offs.max()) + length <= ARENA_BYTES
    return case


ORDER_CASES = {"small": small, "designed": designed, "big": big}
