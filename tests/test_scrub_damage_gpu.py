"""Scrub under mass damage, on the device (MI355X): the cases of tests/test_scrub_damage.py
through stormck_scrub_device / stormck_scrub_tree_device. The device's report, return code,
message and reachable bitmap equal the host leg's and the pure-Python reference's exactly,
and a second run on the same workspace gives the same again: the order in which the rows
reach the queue differs from run to run, the result must not. Every address the edits
write is below n_blocks + SLACK, so it is rejected as out of range before any read or lies
inside the tensor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storm_amd import _lib, commit, engine, scrub  # noqa: E402
from storm_amd.scrub import BLOB, MISMATCH  # noqa: E402
from tests import scrub_util as su  # noqa: E402
from tests.test_scrub_damage import host  # noqa: E402


def device(case, image, workspace=None):
    if case.tree is None:
        return scrub.scrub_device(image, case.lay, reachable=True, workspace=workspace)
    return scrub.scrub_tree_device(image, case.lay, *case.tree, reachable=True, workspace=workspace)


def same_everywhere(case, image=None):
    """Device (twice on one workspace) == host leg == reference; returns the device's report."""
    assert case.img.size >= (case.lay.n_blocks + su.SLACK) * case.lay.block_size  # wrong addresses stay inside
    want, want_bitmap, index = case.reference()
    h = host(case, 5)
    if image is None:
        image = torch.from_numpy(np.array(case.img)).cuda()
    ws = torch.empty(scrub.workspace_bytes(case.lay.n_blocks) // 8 + 1, dtype=torch.int64, device="cuda")
    for run in range(2):
        dev = device(case, image, ws)
        bitmap = dev.reachable.cpu().numpy().view(np.uint32)
        assert dev.as_dict() == want, run
        assert dev.as_dict() == h.as_dict() and dev.code == h.code and dev.message == h.message, run
        assert np.array_equal(bitmap, want_bitmap) and np.array_equal(bitmap, h.reachable), run
    for field, value in case.expect.items():
        assert getattr(dev, field) == value, field
    return dev, want, index


@pytest.mark.parametrize("name", list(su.CONTESTED))
def test_contested_references(name):
    dev, _, _ = same_everywhere(su.edited(*su.CONTESTED[name]))
    assert dev.code == _lib.EMISMATCH


@pytest.mark.parametrize("seed", range(su.FUZZ_SEEDS))
@pytest.mark.parametrize("name", su.FUZZ_IMAGES)
def test_damage_fuzz(name, seed):
    _, want, index = same_everywhere(su.fuzz_case(name, seed))
    su.check_fuzz_reference(name, seed, want, index)


@pytest.mark.parametrize("name", [n for n in su.FUZZ_IMAGES if su.intact_case(n).lay.n_blocks >= 1000])
def test_damage_fuzz_leaves_most_trees_alive(name):
    def make(seed):
        want, _, index = su.fuzz_case(name, seed).reference()
        su.check_fuzz_reference(name, seed, want, index)
    assert su.still_alive(name, make) >= 0.9


def test_wide_store_is_intact():
    dev, _, _ = same_everywhere(su.intact_case("wide_store"))
    assert dev.ok and dev.levels == 4


@pytest.mark.parametrize("name", list(su.WIDE_DAMAGE))
def test_wide_store_damage_past_lane_63(name):
    parent_of, slot, kind = su.WIDE_DAMAGE[name]
    dev, _, _ = same_everywhere(su.edited("wide_store", su.place_damage(parent_of, slot, kind)))
    assert dev.first_slot == slot and dev.first_parent > 0


@pytest.mark.parametrize("name", list(su.F1200_DAMAGE))
def test_f1200_damage_past_lane_63(name):
    dev, _, _ = same_everywhere(su.edited("f1200", su.F1200_DAMAGE[name]))
    assert dev.first_slot == int(name.split()[1])


def test_rows_8_bytes_off_a_16_byte_boundary():
    """block_size = 8 (mod 16) and the image 8 bytes into a tensor: the gathered rows are not
    16-byte aligned and k_scrub_expand's 8-byte loads sit at the least alignment allowed."""
    img, lay, root, root_type, leaf_len = su.odd_stride_tree()
    buf = torch.zeros(img.size + 32, dtype=torch.uint8, device="cuda")
    off = (8 - buf.data_ptr()) % 16
    image = buf[off:off + img.size]
    image.copy_(torch.from_numpy(np.array(img)))
    assert image.data_ptr() % 16 == 8 and image.is_contiguous()
    tree = (root, root_type, BLOB, leaf_len)
    dev, _, _ = same_everywhere(su.Case(img, lay, tree, dict(verified=(66, 0, 0, 300), first_error=0)), image)
    assert dev.ok
    bad = img.copy()
    bad[151 * lay.block_size + 2055] ^= 1
    image[151 * lay.block_size + 2055] ^= 1
    same_everywhere(su.Case(bad, lay, tree, dict(verified=(66, 0, 0, 299), first_error=MISMATCH, first_address=151,
                                                 n_mismatch=1)), image)


def _mixed_level_leaves():
    """Leaves for a level of per-block lengths that takes the LDS-DMA kernel with per-wave
    tile counts: plan_checksum (dispatch.h) sends a gather with lengths there from
    max(kMidBatch, 44 per CU) rows, and from more than 16 per CU (tests/cpp/dispatch_plan_test.cpp
    "scrub level": 11,302 rows at 256 CUs)."""
    cu = engine._cu_count()
    return max(10240, 44 * cu, 16 * cu + 1) + 36


def test_device_built_level_of_mixed_kinds():
    """Built on the device by existing entry points: a root over pointer blocks A_0..A_k, which
    hold n synthetic 32 KiB leaves, and B, which holds the pointer blocks C_1 and C_2 with three
    leaves each. Level 2 is n leaves and two 30,000-byte pointer blocks: mixed lengths for the
    hash, and k_scrub_expand over thousands of rows that only take the compare."""
    n, F, bs, rev = _mixed_level_leaves(), 1200, 32768, 3
    k = (n + F - 1) // F                # A_0 .. A_(k-1)
    p = n + 7                           # leaves 1..n, C's leaves n+1..n+6, then A's, B, C_1, C_2, the root
    B, C1, C2, root_addr = p + k, p + k + 1, p + k + 2, p + k + 3
    n_blocks = root_addr + 1
    image = torch.zeros((n_blocks + 1, bs), dtype=torch.uint8, device="cuda")
    base = image.data_ptr()

    def at(address):
        return base + address * bs

    cs = torch.empty(n + 6, dtype=torch.int64, device="cuda")
    engine.fill_synthetic_device(at(1), bs, n + 6, 0, su.o.SYNTH_SEED)
    engine.checksum_device(at(1), bs, n + 6, cs.data_ptr(), bs)
    engine.pack_pointer_blocks_device(cs.data_ptr(), n, 1, rev, 2, F, at(p), bs)
    engine.pack_pointer_blocks_device(cs.data_ptr() + 8 * n, 3, n + 1, rev, 2, F, at(C1), bs)
    engine.pack_pointer_blocks_device(cs.data_ptr() + 8 * (n + 3), 3, n + 4, rev, 2, F, at(C2), bs)
    pcs = torch.empty(k + 4, dtype=torch.int64, device="cuda")  # A's, B, C_1, C_2, the root
    engine.checksum_device(at(C1), bs, 2, pcs.data_ptr() + 8 * (k + 1), 30000)
    engine.pack_pointer_blocks_device(pcs.data_ptr() + 8 * (k + 1), 2, C1, rev, 1, F, at(B), bs)
    engine.checksum_device(at(p), bs, k + 1, pcs.data_ptr(), 30000)
    engine.pack_pointer_blocks_device(pcs.data_ptr(), k + 1, p, rev, 1, F, at(root_addr), bs)
    engine.checksum_device(at(root_addr), bs, 1, pcs.data_ptr() + 8 * (k + 3), 30000)
    torch.cuda.synchronize()
    root = (int(engine.u64(pcs)[k + 3]), root_addr, rev)
    lay = scrub.ScrubLayout.production(n_blocks)
    ws = torch.empty(scrub.workspace_bytes(n_blocks) // 8 + 1, dtype=torch.int64, device="cuda")
    rep = scrub.scrub_tree_device(image, lay, root, 1, BLOB, reachable=True, workspace=ws)
    assert rep.ok and rep.first_error == 0 and rep.levels == 4
    assert rep.verified == (k + 4, 0, 0, n + 6)
    assert rep.bytes_hashed == (k + 4) * 30000 + (n + 6) * bs
    assert su.popcount(rep.reachable.cpu().numpy().view(np.uint32)) == n_blocks

    victims = [200 + i * ((n - 400) // 36) for i in range(37)]  # 37 leaves spread over level 2
    assert len(set(victims)) == 37 and 1 <= victims[0] and victims[-1] <= n
    for v in victims:
        image[v, (v * 37) % bs] ^= 0x80
    image[n + 5, 77] ^= 0x01  # and one leaf under C_2, a level deeper
    damaged = torch.empty(1, dtype=torch.int64, device="cuda")
    engine.checksum_device(at(victims[0]), bs, 1, damaged.data_ptr(), bs)
    for run in range(2):
        rep = scrub.scrub_tree_device(image, lay, root, 1, BLOB, reachable=True, workspace=ws)
        assert rep.code == _lib.EMISMATCH and rep.n_mismatch == 38 and rep.n_structural == 0
        assert rep.verified == (k + 4, 0, 0, n + 6 - 38) and rep.levels == 4
        first = victims[0]  # the A's addresses ascend with their leaves': the smallest (parent, slot)
        assert (rep.first_error, rep.first_address, rep.first_level) == (MISMATCH, first, 2)
        assert (rep.first_parent, rep.first_slot) == (p + (first - 1) // F, (first - 1) % F)
        assert rep.first_computed == int(engine.u64(damaged)[0])
        assert rep.first_expected == int(engine.u64(cs)[first - 1])
        assert su.popcount(rep.reachable.cpu().numpy().view(np.uint32)) == n_blocks


@pytest.mark.parametrize("n,F,slot,L", su.ROUND_TRIPS)
def test_commit_then_scrub(n, F, slot, L):
    """stormck_commit_device scatters Pointers and type bytes into the parents in HBM; the
    scrub reads them back from the same bytes."""
    blocks, arena, last, levels = su.forest_arena(n, F, slot, L)
    d_arena = torch.from_numpy(arena).cuda()
    commit.commit_device(d_arena.data_ptr(), blocks, 1, last)
    torch.cuda.synchronize()
    back = d_arena.cpu().numpy()
    case = su.committed_tree(back, n, F, slot, L, levels)
    total = n + sum(levels)
    assert case.tree[0][1] == total and case.tree[1] == (1 if n > 1 else 2)
    ws = torch.empty(scrub.workspace_bytes(case.lay.n_blocks) // 8 + 1, dtype=torch.int64, device="cuda")
    dev = device(case, d_arena, ws)
    h = host(case, 0)
    assert dev.as_dict() == h.as_dict() and dev.code == h.code == _lib.OK
    assert su.popcount(dev.reachable.cpu().numpy().view(np.uint32)) == total + 1
    for field, value in case.expect.items():
        assert getattr(dev, field) == value, field

    v = n // 2 + 1
    d_arena[v * slot + L - 1] ^= 0x10
    dev = device(case, d_arena, ws)
    assert dev.code == _lib.EMISMATCH and (dev.n_mismatch, dev.n_structural) == (1, 0)
    assert (dev.first_error, dev.first_address, dev.first_level) == (MISMATCH, v, len(levels))
    assert (dev.first_parent, dev.first_slot) == ((n + 1 + (v - 1) // F, (v - 1) % F) if n > 1 else (0, 0))
    assert dev.verified == (sum(levels), 0, 0, n - 1)
