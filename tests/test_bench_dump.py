"""CPU: bench.py's --dump-outputs writer (the size cap and its seeded sample) and its refusal of a step count that
would time nothing -- neither needs a GPU."""
import os
import subprocess
import sys

import numpy as np

from dcp_testlib import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_below_the_cap_is_whole(tmp_path):
    a, b = np.arange(1000, dtype=np.float32), -np.arange(1000, dtype=np.float64)
    info = bench.dump_outputs(str(tmp_path), {"null_cost": a, "alt_cost": b}, 0, 1)
    assert info["sampled"] is False and info["windows"] == info["written"] == 1000
    assert np.array_equal(np.load(tmp_path / "null_cost.npy"), a)
    got = np.load(tmp_path / "alt_cost.npy")
    assert got.dtype == np.float32 and np.array_equal(got, b.astype(np.float32))


def test_dump_above_the_cap_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    n = 100_000
    a = np.arange(n, dtype=np.float32)  # each value is its window's index
    runs = []
    for world, rank, d in ((1, 0, "x"), (1, 0, "y"), (2, 1, "z")):
        info = bench.dump_outputs(str(tmp_path / d), {"null_cost": a, "alt_cost": a + 1}, rank, world)
        assert info["sampled"] is True and info["windows"] == n
        files = sorted(os.listdir(tmp_path / d))
        assert files == (["alt_cost.npy", "null_cost.npy"] if world == 1 else ["alt_cost_rank1.npy", "null_cost_rank1.npy"])
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) * world <= 40_000
        nul = np.load(tmp_path / d / files[1])
        assert len(nul) == info["written"] and np.array_equal(np.load(tmp_path / d / files[0]), nul + 1)
        assert np.all(np.diff(nul) > 0) and nul[-1] < n  # a subset of the windows, in window order
        runs.append(nul)
    assert np.array_equal(runs[0], runs[1])  # the same sample every run


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
