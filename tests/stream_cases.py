"""Designed inputs for the two persistent streaming kernels (kernels.h k_xxh64_glds_skew and
k_xxh64_glds_var) launched directly on small grids (tests/hip/stream_kernels.hip): plain
numpy, seeded, no torch and no HIP.

Both kernels walk groups of 16 * W blocks (W waves, a quad of lanes per block) in tiles of
16 stripes (512 bytes per block); a persistent workgroup takes groups wg, wg + G, ... of a
grid of G workgroups, and wave v starts its stream 8 * v tiles late. The classifiers below
restate, from the kernels' own rules, which internal paths a case takes; every case lists
the classes it is there for (`claims`), and tests/test_stream_cases.py checks the claims
against the classifier and that the claims together cover every class, so the GPU tests
cannot silently stop reaching a path.

Every buffer is random bytes from a generator seeded by the case's name, with SLACK bytes
after the last block; block 0 starts base_off bytes into it (a multiple of 16)."""
import zlib
from dataclasses import dataclass, field

import numpy as np

TILE_STRIPES, ROW, WAVE_BLOCKS, WAVES, SKEW = 16, 512, 16, 8, 8
GROUP = WAVE_BLOCKS * WAVES  # 128 blocks: a group of the 8-wave kernels
RAMP = (WAVES - 1) * SKEW    # 56: the last wave's start delay in tile steps
FAR = 4 * RAMP               # a stream "far above" the ramp
SLACK = 64
MAX_BYTES = 64 << 20


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _buffer(name, nbytes):
    assert nbytes <= MAX_BYTES + SLACK + 4096, (name, nbytes)
    return _rng("bytes:" + name).integers(0, 256, size=nbytes, dtype=np.uint8)


def _up16(x):
    return (x + 15) // 16 * 16


# ---------------------------------------------------------------------------------------
# k_xxh64_glds_skew: one length, one stride
# ---------------------------------------------------------------------------------------
@dataclass
class SkewCase:
    name: str
    len: int
    stride: int
    n: int
    grid: int
    base_off: int = 0
    claims: tuple = ()

    @property
    def nbytes(self):
        return self.base_off + (self.n - 1) * self.stride + self.len + SLACK

    def buffer(self):
        return _buffer(self.name, self.nbytes)

    def extents(self):
        """(first byte, one past the last byte) of every block, relative to the buffer."""
        s = self.base_off + np.arange(self.n, dtype=np.int64) * self.stride
        return s, s + self.len


def skew_totals(c):
    """Tile steps of every workgroup that has a group (the kernel's `total`)."""
    ntiles = (c.len // 32) // TILE_STRIPES
    ngroups = -(-c.n // GROUP)
    return [-(-(ngroups - wg) // c.grid) * ntiles for wg in range(min(c.grid, ngroups))]


def skew_classes(c):
    """The classes of the issue's list a skew case falls in."""
    out = set()
    nst = c.len // 32
    ntiles, rem, tail = nst // TILE_STRIPES, nst % TILE_STRIPES, c.len % 32
    ngroups, g = -(-c.n // GROUP), c.grid
    if ntiles == 1: out.add("ntiles=1")
    if 2 <= ntiles <= 7: out.add("ntiles=2..7")
    if ntiles == SKEW: out.add("ntiles=8")
    if 9 <= ntiles <= 55: out.add("ntiles=9..55")
    if ntiles == RAMP: out.add("ntiles=56")
    if ntiles == RAMP + 1: out.add("ntiles=57")
    if ntiles >= 64: out.add("ntiles>=64")
    if ntiles > 128: out.add("ntiles>128")
    if rem in (0, 1, 15): out.add("rem=%d" % rem)
    if tail == 0: out.add("tail=0")
    elif tail == 31: out.add("tail=31")
    elif tail % 8 == 0: out.add("tail=words")
    elif 4 <= tail <= 7: out.add("tail=4..7")
    elif 1 <= tail <= 3: out.add("tail=1..3")
    if g in (1, 2, 3, 7): out.add("G=%d" % g)
    if ngroups < g: out.add("ngroups<G")
    if ngroups == g: out.add("ngroups=G")
    if ngroups % g != 0 and ngroups > g: out.add("ngroups%G!=0")
    if ngroups >= 3 * g: out.add("ngroups>=3G")
    totals = skew_totals(c)
    if min(totals) < RAMP: out.add("total<56")
    if max(totals) >= FAR: out.add("total>>56")
    m = c.n % GROUP
    if m == 0: out.add("n%128=0")
    elif m == 1: out.add("n%128=1")
    elif m < 16: out.add("n%128=2..15")
    elif m == 16: out.add("n%128=16")
    elif m % 16 != 0: out.add("n%128>16,ragged")
    if c.stride == c.len and c.len % 16 == 0: out.add("stride=len")
    if c.stride == _up16(c.len) + 16: out.add("stride=len^16+16")
    if c.stride >= c.len + 2048: out.add("stride=len+KiBs")
    if c.base_off % 512 != 0: out.add("base%512!=0")
    return out


SKEW_REQUIRED = {
    "ntiles=1", "ntiles=2..7", "ntiles=8", "ntiles=9..55", "ntiles=56", "ntiles=57", "ntiles>=64", "ntiles>128",
    "rem=0", "rem=1", "rem=15", "tail=0", "tail=words", "tail=4..7", "tail=1..3", "tail=31",
    "G=1", "G=2", "G=3", "G=7", "ngroups<G", "ngroups=G", "ngroups%G!=0", "ngroups>=3G", "total<56", "total>>56",
    "n%128=0", "n%128=1", "n%128=2..15", "n%128=16", "n%128>16,ragged",
    "stride=len", "stride=len^16+16", "stride=len+KiBs", "base%512!=0",
}

SKEW_CASES = [
    # one tile per block: every group change is one step after the last
    SkewCase("one_tile", len=512, stride=512, n=3 * GROUP, grid=1,
             claims=("ntiles=1", "rem=0", "tail=0", "G=1", "n%128=0", "total<56")),
    # 5 tiles, a remainder stripe, two tail words; padded stride; a lone block in the last group
    SkewCase("five_tiles_lone_block", len=5 * ROW + 32 + 16, stride=_up16(5 * ROW + 48) + 16, n=2 * GROUP + 1, grid=2,
             base_off=16, claims=("rem=1", "tail=words", "G=2", "n%128=1", "stride=len^16+16", "base%512!=0")),
    # a block as long as the skew: wave v hashes group k while wave v + 1 starts it
    SkewCase("skew_tiles_grid_full", len=8 * ROW + 15 * 32 + 5, stride=_up16(8 * ROW + 485) + 4096, n=6 * GROUP + 9, grid=7,
             claims=("ntiles=8", "rem=15", "tail=4..7", "ngroups=G", "n%128=2..15", "stride=len+KiBs")),
    # fewer groups than workgroups: the third returns at once; one full wave in the last group
    SkewCase("thirty_tiles_idle_workgroup", len=30 * ROW + 2, stride=_up16(30 * ROW + 2), n=GROUP + 16, grid=3,
             claims=("ntiles=9..55", "tail=1..3", "ngroups<G", "n%128=16")),
    # a block exactly as long as the start-up ramp, 31 tail bytes, unequal workgroups
    SkewCase("ramp_tiles", len=RAMP * ROW + 31, stride=_up16(RAMP * ROW + 31) + 16, n=2 * GROUP + 37, grid=2,
             claims=("ntiles=56", "tail=31", "ngroups%G!=0", "n%128>16,ragged")),
    SkewCase("ramp_plus_one", len=(RAMP + 1) * ROW, stride=(RAMP + 1) * ROW, n=2 * GROUP + 44, grid=3,
             claims=("ntiles=57", "G=3", "stride=len")),
    # storm's 32 KiB slots on one workgroup: 256 steps, the regime of the shipped dispatch
    SkewCase("slots_long_stream", len=32768, stride=32768, n=4 * GROUP, grid=1,
             claims=("ntiles>=64", "total>>56")),
    SkewCase("over_64k", len=130 * ROW + 32 + 24, stride=_up16(130 * ROW + 56) + 16, n=GROUP + 2, grid=7,
             claims=("ntiles>128", "G=7")),
    # the production shape the issue names (uniform 1 KiB blocks): waves many groups apart
    SkewCase("kib_blocks_many_groups", len=1024, stride=1024, n=21 * GROUP + 1, grid=7, base_off=48,
             claims=("ntiles=2..7", "ngroups>=3G")),
]


# ---------------------------------------------------------------------------------------
# k_xxh64_glds_var: per-block lengths and / or offsets
# ---------------------------------------------------------------------------------------
@dataclass
class Form:
    waves: int        # 1, 3 or 8
    persistent: bool  # 8 waves only: `grid` workgroups, waves 8 tiles apart
    grid: int = 1
    n: int = 0        # a prefix of the case (0: all of it)

    @property
    def tag(self):
        return "p" if self.persistent else "w%d" % self.waves


@dataclass
class VarCase:
    name: str
    n: int
    nbytes: int
    base_off: int = 0
    stride: int = 0
    len: int = 0
    lens: np.ndarray = None   # uint32, or None: one length
    offs: np.ndarray = None   # uint64 from the base, or None: i * stride
    order: np.ndarray = None  # uint32: the output slot of block i (the ordered gather)
    forms: list = field(default_factory=list)
    claims: tuple = ()

    def buffer(self):
        return _buffer(self.name, self.nbytes)

    def lengths(self):
        return np.full(self.n, self.len, dtype=np.int64) if self.lens is None else self.lens.astype(np.int64)

    def starts(self):
        o = np.arange(self.n, dtype=np.int64) * self.stride if self.offs is None else self.offs.astype(np.int64)
        return self.base_off + o

    def extents(self):
        s = self.starts()
        return s, s + self.lengths()


def var_classes(c):
    """'<form>:<class>' for every form of the case; the buffer is taken as 16-byte aligned."""
    out = set()
    entry = "ORD" if c.order is not None else "LENS+OFFS" if c.lens is not None and c.offs is not None else \
        "LENS" if c.lens is not None else "OFFS"
    if c.order is not None and c.lens is None:
        entry = "ORD,one-length"
    for f in c.forms:
        n = f.n or c.n
        start, L = c.starts()[:n], c.lengths()[:n]
        staged = start % 16 == 0
        sb = np.where(staged, (L >> 5) * 32, 0)
        tiles = -(-sb // ROW)
        bpw = WAVE_BLOCKS * f.waves
        ngroups = -(-n // bpw)
        G = f.grid if f.persistent else ngroups
        has = set()
        has.add(entry)
        if f.persistent:
            has.add("G=%d" % G)
            if ngroups < G: has.add("ngroups<G")
            # several groups per workgroup, unequally many, a ragged last group (and, below, waves
            # far apart that pass over groups)
            many = G >= 2 and ngroups >= 3 * G and ngroups % G != 0 and n % bpw != 0
        if set(range(32)) <= set(L[L < 32].tolist()): has.add("len0..31")
        if (staged & (L >= ROW) & (L % ROW == 0)).any(): has.add("len=k*512")
        if ((sb > ROW) & (sb % ROW != 0)).any(): has.add("partial_last_tile")
        if (tiles > 64).any(): has.add("len>64tiles")
        for k in (8, 1, 4, 12):
            if ((start % 16 == k) & (L >= 32)).any(): has.add("start+%d" % k)
        if n % bpw != 0 and bpw - n % bpw >= WAVE_BLOCKS: has.add("dead_wave")

        def pad(a, fill):
            return np.concatenate([a, np.full(ngroups * bpw - n, fill, dtype=a.dtype)]).reshape(ngroups, f.waves, WAVE_BLOCKS)
        live, p_sb, p_st, p_L = pad(np.ones(n, bool), False), pad(sb, -1), pad(staged, False), pad(L, 0)
        t = pad(tiles, 0).max(axis=2)  # tiles of wave w in group g
        full = live.all(axis=2)
        if (full & p_st.all(axis=2) & (p_sb.min(axis=2) == p_sb.max(axis=2)) & (p_sb.min(axis=2) > 0)).any():
            has.add("wave_uniform")
        lo = np.where(live, p_sb, p_sb.max()).min(axis=2)
        if ((t > 0) & (lo != p_sb.max(axis=2))).any(): has.add("wave_masked")
        unst = full & ~p_st.any(axis=2) & (p_L >= 32).any(axis=2)
        if unst.any(): has.add("unstaged_wave")
        if unst.all(axis=1).any(): has.add("unstaged_group")
        for wg in range(min(G, ngroups)):
            tw = t[wg::G]  # this workgroup's groups in order
            per_group, per_wave = tw.sum(axis=1), tw.sum(axis=0)
            if per_group.sum() == 0:
                has.add("wg_no_tile")
                continue
            if ((tw[0] == 0) & (per_wave > 0)).any(): has.add("wave_late_start")
            if (per_wave == 0).any(): has.add("wave_no_tile")
            busy = np.flatnonzero(per_group > 0)
            if (per_group[busy[0]:busy[-1]] == 0).any(): has.add("empty_group_between")
            if per_wave.max() - per_wave.min() > RAMP: has.add("stream_diff>56")
            for w in range(f.waves):  # a wave that passes over a group while other waves stream it
                on = np.flatnonzero(tw[:, w] > 0)
                if on.size and (tw[on[0]:on[-1], w] == 0).any() and (per_group[on[0]:on[-1]] > 0).all():
                    has.add("wave_skips_group")
        if f.persistent and many and {"stream_diff>56", "wave_skips_group"} <= has: has.add("many_groups")
        out |= {f.tag + ":" + h for h in has}
    return out


_P_CLASSES = ("len0..31", "len=k*512", "partial_last_tile", "len>64tiles", "wave_uniform", "wave_masked",
              "start+8", "start+1", "start+4", "start+12", "unstaged_wave", "unstaged_group",
              "wave_late_start", "wave_no_tile", "empty_group_between", "wg_no_tile", "stream_diff>56",
              "ngroups<G", "many_groups", "dead_wave", "LENS", "OFFS", "LENS+OFFS", "ORD", "ORD,one-length", "G=1", "G=2", "G=3", "G=5")
# the non-persistent forms at small n: the per-block paths, a wave without a tile beside waves
# with tiles, and a wave wholly past n where a workgroup has more than one wave
_W_CLASSES = ("len0..31", "partial_last_tile", "len>64tiles", "wave_uniform", "wave_masked", "start+1", "unstaged_wave",
              "wave_no_tile", "LENS+OFFS")
VAR_REQUIRED = {"p:" + c for c in _P_CLASSES} | {"w%d:%s" % (w, c) for w in (1, 3, 8) for c in _W_CLASSES} - \
    {"w1:wave_no_tile"} | {"w3:dead_wave", "w8:dead_wave", "w1:LENS", "w3:OFFS", "w8:ORD", "w8:ORD,one-length"}


def _layout(specs, base_off=0):
    """Blocks one after another: block i is specs[i] = (length, misalignment) and starts at the
    next 16-byte boundary (of base_off + offset) plus its misalignment. -> offs, lens, nbytes."""
    offs, lens, cur = [], [], 0
    for length, mis in specs:
        o = _up16(cur) + mis
        offs.append(o)
        lens.append(length)
        cur = o + length
    return np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), base_off + cur + SLACK


def _mixed():
    """Long, short, empty and unaligned blocks in one workgroup (group 0, wave by wave), a group
    of unstaged blocks only, a random group and a partial one."""
    r = _rng("mixed")
    g0 = [(k, 0) for k in range(16)]                                  # wave 0: lengths 0..15, no tile
    g0 += [(k, 0) for k in range(16, 32)]                             # wave 1: 16..31, no tile
    g0 += [(int(r.integers(0, 6000)), int(r.choice([0, 0, 0, 8, 1]))) for _ in range(16)]  # wave 2: mixed
    g0 += [(2048, 0)] * 16                                            # wave 3: the same staged length
    g0 += [(1000, 8)] * 16                                            # wave 4: no block staged
    g0 += [(ROW * k, 0) for k in range(1, 17)]                        # wave 5: whole tiles, 1..16
    g0 += [(40000, 0)] + [(100, 0)] * 15                              # wave 6: 78 tiles beside 0
    g0 += [(int(r.integers(700, 3000)), (1, 4, 12, 8)[k % 4]) for k in range(16)]  # wave 7: starts off by 1, 4, 12, 8
    g1 = [(int(r.integers(33, 2000)), int(r.choice([8, 1, 4, 12]))) for _ in range(GROUP)]  # nothing staged
    g2 = [(int(r.integers(0, 5000)), int(r.choice([0, 0, 0, 0, 8, 4]))) for _ in range(GROUP)]
    g3 = [(int(r.integers(0, 3000)), 0) for _ in range(40)]           # waves 3..7 wholly past n
    offs, lens, nbytes = _layout(g0 + g1 + g2 + g3, 32)
    n = len(offs)
    return VarCase("mixed", n, nbytes, base_off=32, lens=lens, offs=offs,
                   forms=[Form(8, True, 1), Form(8, True, 2), Form(8, True, 3), Form(8, True, 5), Form(8, False),
                          Form(3, False, n=8 * 48 + 20), Form(1, False, n=GROUP + 5)],
                   claims=tuple("p:" + c for c in ("len0..31", "len=k*512", "partial_last_tile", "len>64tiles",
                                                   "wave_uniform", "wave_masked", "start+8", "start+1", "start+4",
                                                   "start+12", "unstaged_wave", "unstaged_group", "wave_late_start",
                                                   "empty_group_between", "stream_diff>56", "dead_wave", "LENS+OFFS",
                                                   "G=1")) +
                   tuple("w%d:%s" % (w, c) for w in (1, 3, 8) for c in _W_CLASSES if (w, c) != (1, "wave_no_tile")) +
                   ("w3:dead_wave", "w8:dead_wave"))


def _sparse():
    """Two workgroups: the odd groups have no tile at all (short or unstaged blocks), and in
    the even ones wave 7 never has one."""
    r = _rng("sparse")
    specs = []
    for g in range(6):
        for w in range(WAVES):
            for _ in range(WAVE_BLOCKS):
                if g % 2 == 1:
                    specs.append((int(r.integers(0, 32)), 0) if w % 2 else (int(r.integers(32, 900)), 8))
                elif w == 7:
                    specs.append((int(r.integers(0, 32)), 0))
                else:
                    specs.append((int(r.integers(32, 4000)), 0))
    offs, lens, nbytes = _layout(specs)
    return VarCase("sparse", len(offs), nbytes, lens=lens, offs=offs, forms=[Form(8, True, 2), Form(8, True, 3)],
                   claims=("p:wg_no_tile", "p:wave_no_tile", "p:G=2"))


def _strided():
    """Per-block lengths at a fixed stride, fewer groups than workgroups, a lone last block."""
    r = _rng("strided")
    n, stride = 2 * GROUP + 1, 4096 + 16
    lens = r.integers(0, stride + 1, size=n).astype(np.uint32)
    lens[:4] = (stride, 0, 31, 4096)
    return VarCase("strided", n, 16 + n * stride + SLACK, base_off=16, stride=stride,
                   lens=lens, forms=[Form(8, True, 5), Form(1, False, n=50), Form(3, False, n=100)],
                   claims=("p:ngroups<G", "p:LENS", "p:G=5", "w1:LENS"))


def _gathered():
    """Offsets with one length: shuffled slots, every eighth start off by 8."""
    r = _rng("gathered")
    n, length, slot = 7 * GROUP + 77, 5000, 5024
    perm = r.permutation(n).astype(np.uint64)
    offs = perm * np.uint64(slot) + np.where(np.arange(n) % 8 == 5, 8, 0).astype(np.uint64)
    return VarCase("gathered", n, n * slot + SLACK, offs=offs, len=length,
                   forms=[Form(8, True, 3), Form(3, False, n=200)], claims=("p:OFFS", "p:G=3", "w3:OFFS"))


def _ordered(name, one_length):
    """The ordered gather's instances: offsets (and lengths) in an order of their own, order[i]
    the output slot of block i."""
    r = _rng(name)
    n = 4 * GROUP + 19
    if one_length:
        length, slot = 3000, 3008
        offs, lens, nbytes = r.permutation(n).astype(np.uint64) * np.uint64(slot), None, n * slot + SLACK
    else:
        length = 0
        offs, lens, nbytes = _layout([(int(r.integers(0, 9000)), int(r.choice([0, 0, 0, 8]))) for _ in range(n)])
    tag = "ORD,one-length" if one_length else "ORD"
    return VarCase(name, n, nbytes, offs=offs, lens=lens, len=length, order=r.permutation(n).astype(np.uint32),
                   forms=[Form(8, True, 2), Form(8, False)], claims=("p:" + tag, "w8:" + tag))


def _streams():
    """Eleven groups and a few blocks on two and on three workgroups: every wave draws, group by
    group, nothing to stage, short blocks, one long block among short ones, or 16 equal blocks,
    so the waves' streams drift apart by tens of tiles and skip groups at different times."""
    r = _rng("streams")
    specs = []
    for _ in range(10 * WAVES):
        kind = int(r.integers(0, 4))
        for k in range(WAVE_BLOCKS):
            mis = 8 if r.integers(0, 20) == 0 else 0
            if kind == 0:
                specs.append((int(r.integers(0, 32)), mis))
            elif kind == 1:
                specs.append((int(r.integers(0, 2000)), mis))
            elif kind == 2:
                specs.append((int(r.integers(16000, 33000)) if k == 5 else int(r.integers(0, 700)), 0))
            else:
                specs.append((4096, 0))
    specs += [(int(r.integers(0, 6000)), 0) for _ in range(3)]
    offs, lens, nbytes = _layout(specs, 48)
    return VarCase("streams", len(offs), nbytes, base_off=48, lens=lens, offs=offs,
                   forms=[Form(8, True, 2), Form(8, True, 3)], claims=("p:many_groups",))


VAR_CASES = [_mixed(), _sparse(), _strided(), _gathered(), _ordered("ordered", False), _ordered("ordered_one_length", True),
             _streams()]
