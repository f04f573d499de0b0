"""Shared pieces of the commit tests: arrangements of a dirty list, the byte-range check,
irregular dirty forests as the stormck_dirty_block contract allows them, the level classes
of dispatch.h's plan_commit_level restated, and the one comparison every leg goes through.

`random_forest` builds, in vectorised numpy, forests the regular `pointer_forest` never
gives: parents whose children sit at several heights, children that skip heights, parents
typed as leaves, several roots (with an origin outside the batch, with none, or the bare
record `cache_records` emits for a block without a PostCommitFunc), zero-length records,
child slots scattered over a table whose unused entries keep the arena's bytes, and arena
slots in an order unrelated to the commit order. Each parent keeps its children's Pointers
inside the bytes it is hashed over, so a parent hashed before one of its children has
stored its Pointer gets a checksum the serial loop never gives.

The generator asserts what it promises from its own output before any library call."""
from collections import namedtuple

import numpy as np

from oracle import oracle as o
from storm_amd import commit as sc

ARRANGEMENTS = ("shuffled", "upper_shuffled", "children_first")


def arrange(b: np.ndarray, how: str, rng, n0=None) -> np.ndarray:
    """Permute the dirty list and remap parent indices. "shuffled": parents may precede
    children; "upper_shuffled": level 0 (the first n0 records; by default the leaves) stays a
    prefix in index order, the blocks after it are shuffled; "children_first": as built."""
    n_leaves = int((b["type"] == sc.LEAF).sum()) if n0 is None else int(n0)
    if how == "children_first":
        return b.copy()
    if how == "shuffled":
        perm = rng.permutation(len(b))
    else:
        perm = np.concatenate([np.arange(n_leaves), n_leaves + rng.permutation(len(b) - n_leaves)])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(b))
    bp = b[perm].copy()
    has = bp["parent"] >= 0
    bp["parent"][has] = inv[bp["parent"][has]]
    return bp


def assert_inside(b, nbytes, shift=0):
    """Every byte range the commit reads or writes lies inside an arena of nbytes: blocks,
    24-byte origin Pointers and origin type bytes (`shift`: bytes before the arena)."""
    assert int((b["data_offset"] + b["length"]).max()) + shift <= nbytes
    has = b["origin_pointer"] != np.uint64(sc.NO_ORIGIN)
    if not has.any():  # a forest of roots that store nothing
        return
    assert int(b["origin_pointer"][has].max()) + 24 + shift <= nbytes
    assert int(b["origin_type"][has].max()) + 1 + shift <= nbytes


def _fast_random_bytes(rng, nbytes):
    return rng.integers(0, 1 << 63, size=(nbytes + 7) // 8, dtype=np.int64).view(np.uint8)[:nbytes]


# ---- dispatch.h's plan_commit_level, restated ----------------------------------------------

COMMIT_WIDE, MULTI_BPW, MULTI_BPW_RING, COMMIT_FLOOR_PER_CU = 256, 5, 8, 39
STREAM_BATCH, BIG_BATCH, BIG_W, VAR_MIN_LEN = 16384, 24576, 131072, 4096
COMMIT_FIRST, COMMIT_GROWTH = 2 * STREAM_BATCH, 3


def busiest_cu_blocks(n, waves, cu):
    per = 16 * waves
    return -(-(-(-n // per)) // cu) * per


def mid_waves_for(n, cu):
    return 1 if busiest_cu_blocks(n, 1, cu) < busiest_cu_blocks(n, 3, cu) else 3


def big_takes_3_waves(n, cu):
    return 4 * busiest_cu_blocks(n, 3, cu) <= 3 * busiest_cu_blocks(n, 8, cu)


def level_class(cnt, cu, glds_levels):
    """The kernel one launch of `cnt` blocks takes on `cu` compute units: "Wide", "Multi5",
    "Multi8", "Quad", or "Glds1" / "Glds3" / "Glds8" (the LDS-DMA kernel and its waves per
    workgroup). glds_levels: the arena base and every data_offset are 16-byte aligned and the
    forest's longest block exceeds 4,096 bytes (`glds_eligible`)."""
    if glds_levels and cu > 0 and cnt >= COMMIT_FLOOR_PER_CU * cu and (
            cnt < BIG_BATCH or (cnt < BIG_W and big_takes_3_waves(cnt, cu))):
        return "Glds%d" % (mid_waves_for(cnt, cu) if cnt < BIG_BATCH else 3)
    if glds_levels and cnt >= STREAM_BATCH:
        return "Glds8"
    if cnt <= COMMIT_WIDE:
        return "Wide"
    if cu > 0 and cnt <= MULTI_BPW * cu:
        return "Multi5"
    if cu > 0 and cnt <= MULTI_BPW_RING * cu:
        return "Multi8"
    return "Quad"


def glds_eligible(base_address, b):
    return base_address % 16 == 0 and not (b["data_offset"] % 16).any() and int(b["length"].max()) > VAR_MIN_LEN


def level0_chunks(n0):
    """commit_plan.h's growing chunk schedule of level 0 on the device."""
    out, nxt = [], COMMIT_FIRST
    while n0 > 0:
        take = min(nxt, n0)
        cnt = n0 if n0 - take < STREAM_BATCH else take
        out.append(cnt)
        n0 -= cnt
        nxt = cnt * COMMIT_GROWTH
    return out


def launch_classes(counts, cu, glds_levels):
    """[(height, blocks, class)] of every launch of the device leg for a forest with
    counts[h] blocks at height h: level 0 chunk by chunk, then one launch per height."""
    rows = [(0, c, level_class(c, cu, glds_levels)) for c in level0_chunks(counts[0])]
    return rows + [(h, c, level_class(c, cu, glds_levels)) for h, c in enumerate(counts) if h > 0]


def kinds(classes):
    """Class names without the wave count ("Glds3" -> "Glds")."""
    return [c.rstrip("138") if c.startswith("Glds") else c for c in classes]


# ---- the generator -------------------------------------------------------------------------

Forest = namedtuple("Forest", "blocks arena last revision counts stats")
Links = namedtuple("Links", "parent rank height stats")

MIN_SKIP, MIN_MIXED, MAX_PARENTLESS = 0.05, 0.10, 0.10
MIXED_SHIFTS = (0, 8, 1, 4, 12, 15)
BARE_ROOTS = 8  # records as cache_records emits them for post_commit is None


def _is_prime(p):
    return p >= 2 and all(p % d for d in range(2, int(p ** 0.5) + 1))


def forest_links(rng, counts, fan, p_root, p_skip=0.0):
    """Parent links of a forest with counts[h] blocks of height h, blocks in height order.
    Every block of height h >= 1 gets one distinct spine child of height h - 1; every other
    block below the top is a root with probability p_root, else draws its parent uniformly
    among all blocks of greater height (with probability p_skip, where two heights lie above
    it, among those at least two heights up). Children are ranked per parent, the spine child
    first; those past `fan` become roots. rank: the child's rank in its parent, -1 for roots."""
    counts = [int(c) for c in counts]
    assert counts and counts[-1] >= 1 and all(a >= b for a, b in zip(counts, counts[1:]))
    nh, n = len(counts), sum(counts)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    height = np.repeat(np.arange(nh, dtype=np.int64), counts)
    parent = np.full(n, -1, dtype=np.int64)
    spine = np.zeros(n, dtype=bool)
    for h in range(1, nh):
        kids = start[h - 1] + rng.permutation(counts[h - 1])[:counts[h]]
        parent[kids] = start[h] + np.arange(counts[h])
        spine[kids] = True
    free = np.flatnonzero(~spine & (height < nh - 1))
    free = free[rng.random(free.size) >= p_root]
    up = np.ones(free.size, dtype=np.int64)
    if p_skip > 0:
        up[(height[free] < nh - 2) & (rng.random(free.size) < p_skip)] = 2
    above = start[height[free] + up]
    parent[free] = above + rng.integers(0, n - above)
    kids = np.flatnonzero(parent >= 0)
    kids = kids[np.lexsort((rng.random(kids.size), ~spine[kids], parent[kids]))]
    p = parent[kids]
    first = np.flatnonzero(np.r_[True, p[1:] != p[:-1]]) if p.size else np.zeros(0, dtype=np.int64)
    r = np.arange(p.size) - np.repeat(first, np.diff(np.r_[first, p.size]))
    assert not (spine[kids] & (r != 0)).any()  # the spine child is first and never dropped
    rank = np.full(n, -1, dtype=np.int64)
    rank[kids] = r
    over = kids[r >= fan]
    parent[over] = -1
    rank[over] = -1
    has = parent >= 0
    # parentless: among the blocks below the top height (those of the top have no parent to draw)
    below = height < nh - 1
    stats = {"blocks": n, "parentless": float((~has & below).sum() / max(1, below.sum())), "skip": 0.0, "mixed": 0.0}
    stats["parentless_all"] = float((~has).mean())
    if has.any():
        stats["skip"] = float((height[parent[has]] - height[has] > 1).mean())
        nch = np.bincount(parent[has], minlength=n)
        cmin, cmax = np.full(n, nh), np.full(n, -1)
        np.minimum.at(cmin, parent[has], height[has])
        np.maximum.at(cmax, parent[has], height[has])
        multi = nch >= 2
        stats["mixed"] = float((cmax[multi] > cmin[multi]).mean()) if multi.any() else 0.0
    return Links(parent, rank, height, stats)


def _free_and_above(counts, p_root):
    """Per height h below the top: the blocks that draw a parent, (counts[h] - counts[h + 1])
    (1 - p_root) in expectation, and the blocks above h they draw among."""
    n = sum(counts)
    return [((counts[h] - counts[h + 1]) * (1 - p_root), n - sum(counts[:h + 1])) for h in range(len(counts) - 1)]


def expected_shares(counts, p_root):
    """(skip, mixed) as the uniform draw gives them in expectation, from the counts alone.
    skip, over all blocks: a drawing block of height h skips when its draw among the blocks
    above it misses the counts[h + 1] of height h + 1. mixed: a parent of height g has its spine
    child at g - 1, Poisson(mu_g) more children of that height and Poisson(lambda_g) of lower
    ones (each drawing block lands on it with probability 1 / above); it has two or more
    children with probability 1 - exp(-(lambda_g + mu_g)) and then children of two heights
    when a lower one is among them, 1 - exp(-lambda_g). Parents of height 1 are never mixed."""
    fa = _free_and_above(counts, p_root)
    skip = sum(f * (1 - counts[h + 1] / a) for h, (f, a) in enumerate(fa[:-1])) / sum(counts)
    multi = mixed = 0.0
    for g in range(1, len(counts)):
        mu = fa[g - 1][0] / fa[g - 1][1]
        lam = sum(f / a for f, a in fa[:g - 1])
        multi += counts[g] * (1 - np.exp(-(lam + mu)))
        mixed += counts[g] * (1 - np.exp(-lam))
    return skip, (mixed / multi if multi else 0.0)


def share_ceilings(counts, fan, p_root):
    """What no draw of this generator can pass, whatever its parents are drawn among: (skip,
    mixed) when every drawing block with two heights above it skips, as far as the fan - 1
    free slots of the blocks two or more heights up hold them. skip is then over the spine
    children and every drawing block that finds a slot; mixed gives each skipping block a
    parent of its own, over the parents with two or more children of expected_shares()."""
    fa = _free_and_above(counts, p_root)
    nh, n = len(counts), sum(counts)
    room = [(fan - 1) * (n - sum(counts[:h + 2])) for h in range(nh - 1)]  # slots two or more heights above h
    skippers = sum(min(f, room[h]) for h, (f, _) in enumerate(fa[:-1]))
    parented = (n - counts[0]) + sum(min(f, (fan - 1) * a) for f, a in fa)
    multi = sum(counts[g] * (1 - np.exp(-sum(f / a for f, a in fa[:g]))) for g in range(1, nh))
    return skippers / max(parented, 1), (min(1.0, skippers / multi) if multi else 0.0)


def condition_floors(counts, fan, p_root):
    """The (skip, mixed) floors a forest of three or more heights must reach: the 5 % and 10 %
    every forest is held to, each lowered to half of expected_shares() only where
    share_ceilings() shows it out of the generator's reach at these counts."""
    e_skip, e_mixed = expected_shares(counts, p_root)
    c_skip, c_mixed = share_ceilings(counts, fan, p_root)
    return (MIN_SKIP if c_skip >= MIN_SKIP else e_skip / 2), (MIN_MIXED if c_mixed >= MIN_MIXED else e_mixed / 2)


def links_meet_conditions(stats, counts, fan, p_root, irregular=True):
    """The generator's promises. With three or more heights: at least 5 % of the parented
    blocks skip a height and at least 10 % of the parents with two or more children hold
    children of two or more heights, or the lower floor condition_floors() derives for a shape
    that cannot reach one of them. With p_root <= 0.05: at most 10 % of the blocks below the
    top height are parentless (those of the top height have no parent to draw), and at most
    10 % of all blocks where the top height holds at most 5 % of them. irregular=False (a
    chain, a pair, whose every block is a spine child): nothing to keep."""
    if not irregular:
        return True
    if len(counts) >= 3:
        min_skip, min_mixed = condition_floors(counts, fan, p_root)
        if stats["skip"] < min_skip or stats["mixed"] < min_mixed:
            return False
    if len(counts) >= 2 and p_root <= 0.05:
        if stats["parentless"] > MAX_PARENTLESS:
            return False
        if counts[-1] <= 0.05 * sum(counts) and stats["parentless_all"] > MAX_PARENTLESS:
            return False
    return True


def palette(slot, name="edge"):
    short = [0, 1, 31, 32, 33, 511, 512, 513, 1024]
    long_ = [slot // 2 + 8, slot - 16, slot - 8, slot]
    return {"edge": short + long_, "short": short, "long": [0, 33] + long_}[name]


def random_forest(seed, counts, slot, fan, align, p_root=0.03, p_reloc=0.3, revision=9, lengths="edge",
                  p_skip=0.0, irregular=True):
    """An irregular dirty forest with counts[h] blocks of height h, in height order (level 0 a
    prefix, the upper blocks by height), its arena and allocation counter.

    Arena: (n + 1) slots of `slot` random bytes; slot 0 is reserved for origins outside the
    batch, block i lives in slot 1 + perm[i] at a start shift set by `align`: "16" every
    data_offset a multiple of 16; "8" the slot size is 8 mod 16, so offsets alternate between
    0 and 8 mod 16; "mixed" childless blocks start at shift 0, 8, 1, 4, 12 or 15, parents at 0
    or 8 (an origin is 8-byte aligned). A parent's table of `fan` (prime) child slots is the
    front of its own bytes: Pointer at 24 k, type byte at 24 fan + k, (25 fan + 7) & ~7 bytes,
    at most the parent's length; child of rank r sits at k = (a_p + r s_p) mod fan.
    `irregular=False` waives links_meet_conditions' promises for a shape whose every block is
    a spine child; the heights, the byte ranges and the table layout are asserted regardless."""
    seed = tuple(np.atleast_1d(seed).tolist())
    assert _is_prime(fan)
    counts = [int(c) for c in counts]
    L = forest_links(np.random.default_rng([*seed, 1]), counts, fan, p_root, p_skip)
    rng = np.random.default_rng([*seed, 2])
    parent, rank, n, nh = L.parent, L.rank, len(L.parent), len(counts)
    has = parent >= 0
    is_parent = np.bincount(parent[has], minlength=n) > 0
    table = sc.pointer_block_size(fan)

    if align == "16":
        assert slot % 16 == 0
        shift = np.zeros(n, dtype=np.int64)
    elif align == "8":
        assert slot % 16 == 8
        shift = np.zeros(n, dtype=np.int64)
    else:
        assert align == "mixed" and slot % 8 == 0
        shift = np.where(is_parent, rng.choice([0, 8], size=n), rng.choice(MIXED_SHIFTS, size=n))
    assert table <= slot - 8
    slots = 1 + rng.permutation(n)  # memory order is unrelated to commit order
    b = np.zeros(n, dtype=sc.DIRTY_DTYPE)
    data = (slots * slot + shift).astype(np.uint64)
    b["data_offset"] = data
    length = rng.choice(palette(slot, lengths), size=n)
    length[is_parent] = np.maximum(length[is_parent], table)
    b["length"] = np.minimum(length, slot - shift)
    b["type"] = rng.integers(1, 3, size=n)  # independent of having children: a parent typed as a leaf
    b["parent"] = parent
    b["origin_pointer"] = sc.NO_ORIGIN
    b["origin_type"] = sc.NO_ORIGIN
    a_p, s_p = rng.integers(0, fan, size=n), rng.integers(1, fan, size=n)
    pp = parent[has]
    k = ((a_p[pp] + rank[has] * s_p[pp]) % fan).astype(np.uint64)
    b["origin_pointer"][has] = data[pp] + np.uint64(24) * k
    b["origin_type"][has] = data[pp] + np.uint64(24 * fan) + k

    roots = rng.permutation(np.flatnonzero(~has))
    bare = roots[~is_parent[roots]][:BARE_ROOTS]  # committed and written, nothing stored anywhere
    b["length"][bare] = 0
    b["type"][bare] = 0
    rest = roots[~np.isin(roots, bare)]
    ext = rest[rng.random(rest.size) >= 0.5][:slot // 32]  # the others keep STORMCK_NO_ORIGIN
    i = np.arange(ext.size, dtype=np.uint64)
    b["origin_pointer"][ext] = np.uint64(32) * i
    b["origin_type"][ext] = np.uint64(32) * i + np.uint64(24)

    first = (1 << 33) + 1 + sum(seed) % 1000
    b["address"] = first + rng.permutation(n)
    last = first + n - 1
    b["birth_revision"] = revision + 1
    old = rng.random(n) < p_reloc
    b["birth_revision"][old] = rng.integers(0, revision + 1, size=int(old.sum()))  # <= revision: relocates
    arena = _fast_random_bytes(rng, (n + 1) * slot)

    # ---- what the generator promises, from its own output
    hist = np.bincount(sc.commit_heights(b), minlength=nh)
    assert hist.tolist() == counts, (hist.tolist(), counts)
    assert links_meet_conditions(L.stats, counts, fan, p_root, irregular), (L.stats, counts, fan, p_root)
    assert_inside(b, arena.size)
    end = data + b["length"]
    assert (data >= np.uint64(slot)).all() and (end <= (slots + 1).astype(np.uint64) * np.uint64(slot)).all()
    op, ot = b["origin_pointer"], b["origin_type"]
    assert not (op[has] % 8).any() and len(np.unique(op[has])) == int(has.sum())
    assert (op[has] + 24 <= data[pp] + 24 * fan).all() and (op[has] >= data[pp]).all()  # inside the table,
    assert (ot[has] >= data[pp] + 24 * fan).all() and (ot[has] < data[pp] + 25 * fan).all()
    assert (b["length"][pp] >= table).all()  # which the parent is hashed over
    assert (ot[ext] < slot).all() and (op[np.setdiff1d(roots, ext)] == np.uint64(sc.NO_ORIGIN)).all()
    stats = dict(L.stats, roots=int(roots.size), external=int(ext.size), bare=int(bare.size),
                 relocating=int(old.sum()), zero_length=int((b["length"] == 0).sum()),
                 leaf_typed_parents=int((is_parent & (b["type"] == sc.LEAF)).sum()))
    return Forest(b, arena, last, revision, counts, stats)


# ---- designed shapes -----------------------------------------------------------------------

def designed(cu=256):
    """The designed forests, sized from the compute-unit count (the numbers in the comments
    are for 256): counts per height, generator arguments and the kernel kind of every launch
    of the device leg (level 0 chunk by chunk, then one per height) on an aligned arena.
    `fan` is sized so that few children find their parent full.

    The floors every shape is held to (condition_floors; thresholds, chunks and quad_at_size
    keep the full 5 % skip and 10 % mixed, and every shape but waves the 10 % mixed):
    - glds_upper: nearly every block is a spine child and the 9,683 drawing blocks of height 3
      find 108 free slots two heights up; if every block that can skip did, 4.8 % would: the
      skip floor is half of the expected 2.8 %.
    - glds_upper_3: 1,000 blocks draw at all, 4.2 % at most: half of the expected 1.4 %.
    - waves: 232 blocks can skip, 0.34 % at most, and only the parents they land on can be
      mixed, 2.2 % at most: half of the expected 0.09 % and 0.72 %.
    - quad_at_size: 2,000 blocks can skip, 5.1 % at most; p_skip = 1 sends each of them two
      heights up, which reaches the 5 %."""
    return {
        # both sides of every small threshold on upper levels: [9000, 2049, 2048, 1281, 1280, 257, 256, 1]
        "thresholds": dict(counts=[35 * cu + 40, 8 * cu + 1, 8 * cu, 5 * cu + 1, 5 * cu, 257, 256, 1], slot=1032,
                           align="8", fan=11,
                           kinds=["Quad", "Quad", "Multi8", "Multi8", "Multi5", "Multi5", "Wide", "Wide"]),
        # three LDS-DMA levels of mixed lengths (0..9 tiles in one workgroup): [12000, 11000, 9984, 9983, 300, 3]
        "glds_upper": dict(counts=[375 * cu // 8, 1375 * cu // 32, 39 * cu, 39 * cu - 1, 300, 3], slot=4608, align="16",
                           fan=37, kinds=["Glds", "Glds", "Glds", "Quad", "Multi5", "Wide"]),
        # level 0 in two chunks, 32,768 (8 waves) then 19,232: [52000, 10500, 2100]
        "chunks": dict(counts=[1625 * cu // 8, 41 * cu + 4, 8 * cu + 52], slot=4608, align="16", fan=11,
                       kinds=["Glds", "Glds", "Glds", "Quad"], waves_256=["Glds8", "Glds1", "Glds3", "Quad"]),
        # an 8-wave, then a 1-wave upper level; 49,152 upper blocks: [33000, 32768, 16384]
        "waves": dict(counts=[128 * cu + 232, 128 * cu, 64 * cu], slot=4608, align="16", fan=11,
                      kinds=["Glds", "Glds", "Glds"], waves_256=["Glds3", "Glds8", "Glds1"]),
        # no LDS-DMA at size, 35,000 upper blocks: [20000, 18000, 17000]
        "quad_at_size": dict(counts=[625 * cu // 8, 1125 * cu // 16, 2125 * cu // 32], slot=1040, align="mixed", fan=11,
                             p_skip=1.0, kinds=["Quad", "Quad", "Quad"]),
        # the first three levels of glds_upper, for an arena 8 bytes off a 16-byte boundary
        "glds_upper_3": dict(counts=[375 * cu // 8, 1375 * cu // 32, 39 * cu], slot=4608, align="16", fan=11,
                             kinds=["Glds", "Glds", "Glds"]),
    }


_designed_cache = {}


def designed_forest(name, cu=256):
    """The Forest of a designed shape (built once per process and never written)."""
    if (name, cu) not in _designed_cache:
        _designed_cache.clear()  # one at a time: the largest arena is 378 MB
        d = designed(cu)[name]
        seed = sorted(designed()).index(name) + 1000
        f = random_forest(seed, d["counts"], d["slot"], d["fan"], d["align"], p_skip=d.get("p_skip", 0.0))
        f.arena.flags.writeable = False
        f.blocks.flags.writeable = False
        _designed_cache[(name, cu)] = f
    return _designed_cache[(name, cu)]


# ---- seeded cases --------------------------------------------------------------------------

FUZZ_SEEDS = 40
MAX_ARENA, MAX_BLOCKS = 256 << 20, 60000
# level sizes per class on 256 compute units; "Big" is the LDS-DMA kernel when the forest is
# eligible for it and the register quad when not
CLASS_RANGES = [("Wide", 1, 256), ("Multi5", 257, 1280), ("Multi8", 1281, 2048), ("Quad", 2049, 9983),
                ("Big", 9984, 36000)]


def seeded_case(seed):
    """Parameters of seeded case `seed`: 1-6 heights, a class per height (non-increasing, a
    count uniform inside the class), alignment, slot, fan, lengths, p_root, p_reloc and an
    arrangement. Draws whose links miss the generator's promises at their full values (5 %
    skip, 10 % mixed), or whose arena would pass 256 MiB, are drawn again from the same seed.

    This biases the seeds: a forest of three or more heights with nearly equal counts, where
    nearly every block is a spine child, is drawn again (5 of the 40 seeds are), so that regime
    is covered by the designed shapes alone (glds_upper, waves, quad_at_size)."""
    for attempt in range(400):
        rng = np.random.default_rng([seed, attempt, 0x5EED])
        nh = int(rng.integers(1, 7))
        align = str(rng.choice(["16", "8", "mixed"]))
        long_blocks = align == "16" and rng.random() < 0.7
        slot = 4608 if long_blocks else {"16": 1040, "8": 1032, "mixed": 1040}[align]
        classes = sorted(rng.integers(0, len(CLASS_RANGES), size=nh).tolist(), reverse=True)
        counts = sorted((int(rng.integers(CLASS_RANGES[c][1], CLASS_RANGES[c][2] + 1)) for c in classes), reverse=True)
        fan = int(rng.choice([11, 37]))
        p_root = float(rng.choice([0.0, 0.02, 0.05, 0.3]))
        p_reloc = float(rng.choice([0.0, 0.3, 1.0]))
        lengths = str(rng.choice(["edge", "edge", "short", "long"]))
        how = str(rng.choice(ARRANGEMENTS))
        if sum(counts) > min(MAX_BLOCKS, MAX_ARENA // slot - 1):
            continue
        if nh >= 3 and condition_floors(counts, fan, p_root) != (MIN_SKIP, MIN_MIXED):
            continue  # a shape that cannot reach the full values
        stats = forest_links(np.random.default_rng([seed, attempt, 1]), counts, fan, p_root).stats
        if not links_meet_conditions(stats, counts, fan, p_root):
            continue
        return dict(seed=(seed, attempt), counts=counts, slot=slot, fan=fan, align=align, p_root=p_root,
                    p_reloc=p_reloc, lengths=lengths, how=how)
    raise AssertionError(f"seed {seed}: no draw met the generator's conditions")


def seeded_forest(seed):
    """(records in the case's arrangement, Forest, case) of seeded case `seed`."""
    case = seeded_case(seed)
    f = random_forest(case["seed"], case["counts"], case["slot"], case["fan"], case["align"], p_root=case["p_root"],
                      p_reloc=case["p_reloc"], lengths=case["lengths"])
    recs = arrange(f.blocks, case["how"], np.random.default_rng([seed, 3]), n0=case["counts"][0])
    return recs, f, case


# ---- the comparison ------------------------------------------------------------------------

Expected = namedtuple("Expected", "checksums records last arena")
SENTINEL, OUT_PAD, GUARD, GUARD_BYTE = 0xA5A5A5A55A5A5A5A, 8, 4096, 0xA5


def expected_commit(arena, records, revision, last):
    """storm's serial loop (the C oracle) on copies; shared among runs, never written."""
    ref_arena, ref_recs = arena.copy(), records.copy()
    cs, ref_last = o.commit(ref_arena, ref_recs, revision, last)
    for a in (cs, ref_recs, ref_arena):
        a.flags.writeable = False
    return Expected(cs, ref_recs, ref_last, ref_arena)


def check_commit(run, arena, records, revision, last, want=None):
    """run(arena, records, revision, last, out) -> (checksums, last_allocated, the arena after)
    commits copies of the given forest; its checksums, the whole record array, the allocation
    counter and every arena byte must equal the oracle's. `out` is a view into a longer array
    whose other words must come back untouched. Returns what `run` returned."""
    want = want or expected_commit(arena, records, revision, last)
    n = len(records)
    buf = np.full(n + 2 * OUT_PAD, SENTINEL, dtype=np.uint64)
    recs = records.copy()
    cs, last2, after = run(arena.copy(), recs, revision, last, buf[OUT_PAD:OUT_PAD + n])
    assert (buf[:OUT_PAD] == SENTINEL).all() and (buf[OUT_PAD + n:] == SENTINEL).all()
    assert np.array_equal(cs, want.checksums), f"{int((cs != want.checksums).sum())} of {n} checksums differ"
    assert np.array_equal(buf[OUT_PAD:OUT_PAD + n], want.checksums)
    assert np.array_equal(recs, want.records)
    assert last2 == want.last
    assert np.array_equal(after, want.arena)
    return cs, last2, recs


def host_run(threads):
    def run(arena, recs, revision, last, out):
        cs, last2 = sc.commit_host(arena, recs, revision, last, threads=threads, out=out)
        return cs, last2, arena
    return run


def hbm_run(dev, base_shift=0, routed=False):
    """The device leg on an HBM arena that sits `base_shift` bytes past a 16-byte boundary,
    between two 4 KiB guard bands that must come back untouched."""
    import torch

    def run(arena, recs, revision, last, out):
        lo = GUARD + base_shift
        t = torch.full((lo + arena.size + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        assert t.data_ptr() % 16 == 0
        t[lo:lo + arena.size] = torch.from_numpy(arena).to(dev)
        assert_inside(recs, t.numel() - GUARD, shift=lo)
        if routed:
            cs, last2, leg = sc.commit(t.data_ptr() + lo, recs, revision, last, out=out)
            run.legs.append(leg)
        else:
            cs, last2 = sc.commit_device(t.data_ptr() + lo, recs, revision, last, out=out)
        got = t.cpu().numpy()
        assert (got[:lo] == GUARD_BYTE).all() and (got[lo + arena.size:] == GUARD_BYTE).all()
        return cs, last2, got[lo:lo + arena.size]
    run.legs = []
    return run


def host_arena_run(commit, registered=True):
    """A page-aligned host arena between two 4 KiB guard bands; with `registered`, guards and
    arena are registered as one range, so the device reaches all of it in place.
    commit(host_arena, device_pointer or None, recs, revision, last, out) -> (checksums, last)."""
    from storm_amd import blocks

    def run(arena, recs, revision, last, out):
        raw = np.full(arena.size + 2 * GUARD + 4096, GUARD_BYTE, dtype=np.uint8)
        off = (-raw.ctypes.data) % 4096
        whole = raw[off:off + arena.size + 2 * GUARD]
        host = whole[GUARD:GUARD + arena.size]
        host[:] = arena
        assert_inside(recs, whole.size - GUARD, shift=GUARD)
        if registered:
            blocks.RegisterHostMemory(whole)
        try:
            d = blocks.HostDevicePointer(whole) + GUARD if registered else None
            cs, last2 = commit(host, d, recs, revision, last, out)
        finally:
            if registered:
                blocks.UnregisterHostMemory(whole)
        assert (whole[:GUARD] == GUARD_BYTE).all() and (whole[GUARD + arena.size:] == GUARD_BYTE).all()
        assert (raw[:off] == GUARD_BYTE).all() and (raw[off + whole.size:] == GUARD_BYTE).all()
        return cs, last2, host
    return run
