"""What the designed cases of tests/stream_cases.py cover, without a GPU (CPU checks).

tests/test_stream_kernels_gpu.py launches k_xxh64_glds_skew and k_xxh64_glds_var directly
on these cases. Here the classifiers of stream_cases.py recompute which paths every case
takes: each case reaches what it claims, the claims together cover every class of the list,
and every case is the only one to claim at least one class, so dropping or bending a case
fails here, with the class that lost its member, before any GPU run."""
import os
import re

import numpy as np
import pytest

from tests import stream_cases as sc
from tests.conftest import ROOT

ALL = sc.SKEW_CASES + sc.VAR_CASES


def _classes(c):
    return sc.skew_classes(c) if isinstance(c, sc.SkewCase) else sc.var_classes(c)


def test_names_are_unique():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_case_reaches_what_it_claims(c):
    missing = set(c.claims) - _classes(c)
    assert not missing, (c.name, sorted(missing))


@pytest.mark.parametrize("cases,required", [(sc.SKEW_CASES, sc.SKEW_REQUIRED), (sc.VAR_CASES, sc.VAR_REQUIRED)],
                         ids=["skew", "var"])
def test_claims_cover_every_class(cases, required):
    claimed = set().union(*(c.claims for c in cases))
    assert not required - claimed, "classes no case is there for: %s" % sorted(required - claimed)
    assert not claimed - required, "claims outside the list: %s" % sorted(claimed - required)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_every_case_is_the_only_claimant_of_a_class(c):
    same = sc.SKEW_CASES if isinstance(c, sc.SkewCase) else sc.VAR_CASES
    others = set().union(*(o.claims for o in same if o is not c))
    assert set(c.claims) - others, c.name


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_conventions(c):
    """At most 64 MiB of block data, SLACK bytes after the last block, every block inside the
    buffer, a 16-byte aligned base; what the kernels require of a strided batch."""
    first, end = c.extents()
    assert first.min() >= 0 and end.max() + sc.SLACK <= c.nbytes <= sc.MAX_BYTES + sc.SLACK + 4096
    assert c.base_off % 16 == 0
    if isinstance(c, sc.SkewCase):
        assert c.len >= 512 and c.stride >= c.len and c.stride % 16 == 0 and c.n > 0 and c.grid > 0
    else:
        assert c.lens is None or (c.lens.dtype == np.uint32 and c.lens.size == c.n)
        assert c.offs is None or (c.offs.dtype == np.uint64 and c.offs.size == c.n)
        assert c.offs is not None or c.stride % 16 == 0
        if c.order is not None:
            assert c.offs is not None and np.array_equal(np.sort(c.order), np.arange(c.n, dtype=np.uint32))
        for f in c.forms:
            assert f.waves in (1, 3, 8) and (not f.persistent or f.waves == 8) and 0 <= f.n <= c.n
            assert c.order is None or f.waves == 8
        assert any(f.persistent for f in c.forms)


def test_some_bases_are_not_512_aligned():
    assert any(c.base_off % 512 for c in sc.SKEW_CASES) and any(c.base_off % 512 for c in sc.VAR_CASES)


def test_buffers_are_seeded():
    c = sc.SKEW_CASES[0]
    a, b = c.buffer(), c.buffer()
    assert a.dtype == np.uint8 and a.size == c.nbytes and np.array_equal(a, b)
    assert not np.array_equal(a[:256], sc.SKEW_CASES[1].buffer()[:256])


def test_plan_query_shows_the_library_cases_on_the_skew_kernel():
    """tests/cpp/plan_query.cpp (dispatch.h alone, the probe build's knobs from the
    environment): the library-level GPU test's batches plan as k_xxh64_glds_skew on one
    workgroup per CU under STORMCK_SKEW_MIN_STEPS=1, and not under the shipped threshold."""
    import subprocess
    from tests import stream_run as sr
    query = sr.build_plan_query()
    env = {k: v for k, v in os.environ.items() if not k.startswith("STORMCK_")}

    def plan(n, ln, stride, cu, **knobs):
        r = subprocess.run([query, str(n), str(ln), str(stride), "0", str(cu)], env=dict(env, **knobs),
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return r.stdout.split()
    for cu in (256, 304):
        cases = sr.library_cases(cu)
        assert {c[1] for c in cases} == {512, 1000, 4136} and len({c[0] for c in cases}) == 3
        assert all(n * stride <= 256 << 20 and stride % 16 == 0 and stride >= ln for n, ln, stride in cases)
        assert cases[0][0] == 128 * (cu - 1) + 1 and any(n >= 131072 and n % 128 for n, _, _ in cases)
        for n, ln, stride in cases:
            assert plan(n, ln, stride, cu, STORMCK_SKEW_MIN_STEPS="1") == ["glds-skew", str(cu), "512"], (cu, n, ln)
            assert plan(n, ln, stride, cu)[0] == "glds", (cu, n, ln)
    # the shipped threshold: 3,584 tile steps per workgroup
    assert plan(256 * 128 * 56, 32768, 32768, 256) == ["glds-skew", "256", "512"]
    assert plan(256 * 128 * 55, 32768, 32768, 256)[0] == "glds"
    assert subprocess.run([query], capture_output=True).returncode == 2


def test_launch_constants_match_the_dispatch():
    """The harness restates dispatch.h's launch constants; stream_cases.py its geometry."""
    disp = open(os.path.join(ROOT, "storm_amd", "csrc", "dispatch.h")).read()
    harness = open(os.path.join(ROOT, "tests", "hip", "stream_kernels.hip")).read()
    want = {"kTileStripes": sc.TILE_STRIPES, "kAuxNT": 2, "kGldsWaves": sc.WAVES, "kSkewTiles": sc.SKEW}
    for name, value in want.items():
        for text in (disp, harness):
            m = re.search(r"constexpr int %s = (\d+);" % name, text)
            assert m and int(m.group(1)) == value, name
    assert sc.GROUP == 16 * sc.WAVES and sc.RAMP == (sc.WAVES - 1) * sc.SKEW and sc.ROW == 32 * sc.TILE_STRIPES
