"""Irregular dirty forests through every level kernel and every leg of the commit on the
device (MI355X): the forests of tests/commit_util.py, compared byte for byte with storm's
serial loop (the C oracle) by `check_commit`.

The designed cases name the kernel of every launch; `level_class` (dispatch.h's
plan_commit_level restated, pinned on the CPU by tests/test_commit_fuzz.py) gives it from the
device's compute-unit count, and a case that does not reach the class it names fails. Shapes
are written in compute units; the numbers in the docstrings are for 256.

Every device call works on an arena between two 4 KiB guard bands of 0xA5 and writes its
checksums into the middle of a longer array of sentinels; `check_commit` and the runners of
commit_util assert that both come back untouched. No call can reach outside its arena: the
generator asserts, before any library call, that every block, Pointer and type byte of a
forest lies inside it, and the runners assert the same for the arena as placed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, engine  # noqa: E402
from storm_amd import commit as sc  # noqa: E402
from tests import commit_util as cu  # noqa: E402

DESIGNED = ["thresholds", "glds_upper", "chunks", "waves", "quad_at_size"]
REGISTERED_SEEDS, SPLIT_SEEDS, ROUTED_SEEDS = range(0, 10), range(10, 20), range(20, 25)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _designed(name, how, base_shift=0):
    """(records, Forest) of a designed shape at this device's size, after asserting the
    kernel of every launch from the device's compute-unit count."""
    ncu = engine._cu_count()
    d = cu.designed(ncu)[name]
    f = cu.designed_forest(name, ncu)
    eligible = cu.glds_eligible(base_shift, f.blocks)
    classes = [c for _, _, c in cu.launch_classes(d["counts"], ncu, eligible)]
    want = d["kinds"] if base_shift == 0 else ["Quad"] * len(d["kinds"])
    assert cu.kinds(classes) == want, (name, ncu, classes)
    if ncu == 256 and base_shift == 0:
        assert classes == d.get("waves_256", classes), (name, classes)
    return cu.arrange(f.blocks, how, np.random.default_rng(7), n0=f.counts[0]), f


@pytest.mark.parametrize("how", cu.ARRANGEMENTS)
@pytest.mark.parametrize("name", DESIGNED)
def test_device_leg_designed_forests(dev, name, how):
    """thresholds [9000, 2049, 2048, 1281, 1280, 257, 256, 1], slots of 1,032 bytes: Quad,
    Quad, Multi8, Multi8, Multi5, Multi5, Wide, Wide; both sides of every small threshold on
    upper levels. glds_upper [12000, 11000, 9984, 9983, 300, 3], slots of 4,608: three LDS-DMA
    levels with lengths of 0..9 tiles in one workgroup, then Quad, Multi5, Wide. chunks
    [52000, 10500, 2100]: level 0 as two LDS-DMA launches, 32,768 (8 waves) then 19,232 (1
    wave), 10,500 on 3 waves, Quad. waves [33000, 32768, 16384]: 3-, 8- and 1-wave levels and
    49,152 upper blocks, so the planner's counting sort runs on the pool. quad_at_size [20000,
    18000, 17000], mixed start shifts: Quad at every level, the threaded sort again."""
    recs, f = _designed(name, how)
    cu.check_commit(cu.hbm_run(dev), f.arena, recs, f.revision, f.last)


@pytest.mark.parametrize("how", cu.ARRANGEMENTS)
def test_device_leg_arena_8_bytes_off_a_16_byte_boundary(dev, how):
    """[12000, 11000, 9984] in 16-byte aligned slots of 4,608 bytes, the arena 8 bytes into a
    16-byte aligned allocation: no LDS-DMA level, the register quad at every one."""
    recs, f = _designed("glds_upper_3", how, base_shift=8)
    cu.check_commit(cu.hbm_run(dev, base_shift=8), f.arena, recs, f.revision, f.last)


@pytest.mark.parametrize("seed", range(cu.FUZZ_SEEDS))
def test_device_leg_seeded_forests(dev, seed):
    """The seeds of tests/test_commit_fuzz.py on an HBM arena: the device leg must give the
    oracle's result, and so the host leg's."""
    recs, f, case = cu.seeded_forest(seed)
    want = cu.expected_commit(f.arena, recs, f.revision, f.last)
    cs_h, last_h, recs_h = cu.check_commit(cu.host_run(0), f.arena, recs, f.revision, f.last, want=want)
    cs_d, last_d, recs_d = cu.check_commit(cu.hbm_run(dev), f.arena, recs, f.revision, f.last, want=want)
    assert np.array_equal(cs_d, cs_h) and last_d == last_h and np.array_equal(recs_d, recs_h)


def _cases(names, seeds):
    return ([pytest.param(("designed", n), id=n) for n in names] +
            [pytest.param(("seed", s), id=f"seed{s}") for s in seeds])


def _case(case):
    kind, which = case
    if kind == "designed":
        return _designed(which, "shuffled")
    recs, f, _ = cu.seeded_forest(which)
    return recs, f


def _in_place(host, d_arena, recs, revision, last, out):
    return sc.commit_device(d_arena, recs, revision, last, out=out)


@pytest.mark.parametrize("case", _cases(DESIGNED[:2], REGISTERED_SEEDS))
def test_device_leg_in_place_on_a_registered_host_arena(dev, case):
    """The level kernels read the blocks and store the Pointers over the link, through
    HostDevicePointer; the guard bands are part of the registered range."""
    recs, f = _case(case)
    cu.check_commit(cu.host_arena_run(_in_place), f.arena, recs, f.revision, f.last)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", _cases([DESIGNED[0], DESIGNED[-1]], SPLIT_SEEDS))
def test_split_leg_every_share(dev, case):
    """commit_split with none, 7, half and all of level 0 on the device, and the share the
    library's rates give; the upper levels on the host threads."""
    recs, f = _case(case)
    n0 = f.counts[0]
    want = cu.expected_commit(f.arena, recs, f.revision, f.last)
    for share in (0, 7, n0 // 2, n0, None):
        done = []

        def split(host, d_arena, r, revision, last, out):
            cs, last2, d = sc.commit_split(host, r, revision, last, device_leaves=share, out=out)
            done.append(d)
            return cs, last2
        cu.check_commit(cu.host_arena_run(split), f.arena, recs, f.revision, f.last, want=want)
        assert len(done) == 1 and 0 <= done[0] <= n0, (share, done)
        if share is not None:
            assert done[0] == share, (share, done)


@pytest.mark.parametrize("kind", ["hbm", "pageable", "registered"])
@pytest.mark.parametrize("seed", ROUTED_SEEDS)
def test_routed_commit_any_leg(dev, seed, kind):
    """stormck_commit: an HBM arena takes the device leg, a pageable one the host leg, a
    registered one the leg the cost model picks; whichever, the oracle's result."""
    recs, f, _ = cu.seeded_forest(seed)
    legs = []

    def routed(host, d_arena, r, revision, last, out):
        cs, last2, leg = sc.commit(host.ctypes.data, r, revision, last, out=out)
        legs.append(leg)
        return cs, last2
    if kind == "hbm":
        run = cu.hbm_run(dev, routed=True)
        legs = run.legs
    else:
        run = cu.host_arena_run(routed, registered=kind == "registered")
    cu.check_commit(run, f.arena, recs, f.revision, f.last)
    assert len(legs) == 1
    if kind == "hbm":
        assert legs[0] == _lib.LEG_DEVICE
    elif kind == "pageable":
        assert legs[0] == _lib.LEG_HOST
    else:
        assert legs[0] in (_lib.LEG_HOST, _lib.LEG_DEVICE, _lib.LEG_SPLIT)
