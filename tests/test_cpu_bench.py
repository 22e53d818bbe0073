"""-m "not gpu": the host side of bench.py - the --dump-outputs writer and the refusal of a run without timed steps."""
import os

import numpy as np
import pytest

import bench


def test_dump_outputs_float32_and_budget(tmp_path, monkeypatch):
    a = np.arange(6 * 4, dtype=np.float64).reshape(6, 4)
    bench.dump_outputs(str(tmp_path / "small"), {"features": a})
    got = np.load(tmp_path / "small" / "features.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a)           # under the budget: every row, as float32
    # over the budget: a seeded sample of rows, in row order, the same on every run, the files within the budget
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * (4096 + 64 * 16 * 4))     # 64 rows of 16 float32 per array
    big = np.random.default_rng(1).standard_normal((1000, 16)).astype(np.float32)
    for d in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / d), {"features": big, "gathered_features": big[::-1]})
    for name in ("features", "gathered_features"):
        s1, s2 = (np.load(tmp_path / d / (name + ".npy")) for d in ("r1", "r2"))
        assert s1.shape == (64, 16) and s1.dtype == np.float32 and np.array_equal(s1, s2)
        src = big if name == "features" else big[::-1]
        rows = [int(np.flatnonzero((src == r).all(1))[0]) for r in s1]
        assert all(i < j for i, j in zip(rows, rows[1:]))
    assert sum(os.path.getsize(tmp_path / "r1" / f) for f in os.listdir(tmp_path / "r1")) <= bench.DUMP_BYTES


def test_bench_refuses_zero_steps():
    with pytest.raises(SystemExit, match="at least one timed step"):
        bench.run(["--steps", "0"])
