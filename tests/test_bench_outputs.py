"""bench.py --dump-outputs / --full, the parts that need no GPU: the options, the seeded
sample of a large checksum array, the exact float64 form of 64-bit words and the size
limit of a dump (the GPU side is tests/test_bench_gpu.py)."""
import sys

import numpy as np
import pytest

import bench


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_options_default_to_a_plain_run(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs == ""
    a = _parse(["--full", "--dump-outputs", "somewhere"], monkeypatch)
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_is_refused_for_other_workloads(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "keytags", "--dump-outputs", "x"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "--dump-outputs" in str(e.value)


def test_dump_indices_small_outputs_are_written_whole():
    assert bench.dump_indices(0).size == 0
    assert bench.dump_indices(40001).tolist() == list(range(40001))
    assert bench.dump_indices(bench.DUMP_SAMPLE).size == bench.DUMP_SAMPLE


def test_dump_indices_sample_is_fixed_sorted_and_holds_both_ends():
    n = bench.C3_BLOCKS
    idx = bench.dump_indices(n)
    assert idx.dtype == np.int64 and bench.DUMP_SAMPLE - 2 <= idx.size <= bench.DUMP_SAMPLE
    assert idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, bench.dump_indices(n))  # the same in every run
    # spread over the whole output, not a prefix: every sixteenth of it is sampled
    assert np.all(np.bincount(idx * 16 // n, minlength=16) > idx.size // 32)


def test_u64_halves_are_exact():
    words = np.array([0, 1, 0xFFFFFFFF, 1 << 32, 0xD423DE13A105E824, (1 << 64) - 1], dtype=np.uint64)
    h = bench.u64_halves(words)
    assert h.dtype == np.float64 and h.shape == (6, 2)
    back = [(int(a) << 32) | int(b) for a, b in h.tolist()]
    assert back == [int(w) for w in words]
    # the int64 view a device tensor comes back as gives the same words
    assert np.array_equal(bench.u64_halves(words.view(np.int64)), h)
    assert bench.u64_halves(bench.root_words((0xD423DE13A105E824, 0x10036AA, 1, 1))).tolist() == \
        [[float(0xD423DE13), float(0xA105E824)], [0.0, float(0x10036AA)], [0.0, 1.0], [0.0, 1.0]]


def test_dump_outputs_writes_float64_and_keeps_the_limit(tmp_path):
    out = tmp_path / "a" / "b"
    bench.dump_outputs(str(out), {"x": np.arange(6, dtype=np.int64).reshape(3, 2), "y": [1.5]})
    assert sorted(p.name for p in out.iterdir()) == ["x.npy", "y.npy"]
    x = np.load(out / "x.npy")
    assert x.dtype == np.float64 and x.tolist() == [[0, 1], [2, 3], [4, 5]]
    # the largest dump the bench makes (a full sample: halves + indices, and the root) fits
    assert (bench.DUMP_SAMPLE * 3 + 8) * 8 <= bench.DUMP_LIMIT
    big = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(bench.DUMP_LIMIT // 8 + 1,), strides=(0,))
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"z": big})
    assert not (tmp_path / "big" / "z.npy").exists()
