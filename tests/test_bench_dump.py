"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files within 64 MB, the same in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dumped(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_budget_and_sample(tmp_path):
    """arrays over their share of the budget become a seeded sample; the small ones are written whole, shape kept; the dtypes hold the values exactly"""
    import bench
    rng = np.random.default_rng(3)
    n = 3_000_000
    flags = rng.integers(0, 1 << 12, n).astype(np.uint16)
    perm = rng.permutation(n).astype(np.uint32)
    ctr = rng.integers(0, 1 << 40, (5, 7)).astype(np.int64)
    qual = rng.integers(2, 42, 40 * n).astype(np.uint8)
    arrays = [("flags", flags, np.float32), ("permutation", perm, np.float64), ("dup_counters", ctr, np.float64), ("qual", qual, np.float32)]
    budget = 8_000_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget)
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert sorted(a) == ["dup_counters", "flags", "permutation", "qual"]
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= budget + 4 * 128
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["dup_counters"].shape == (5, 7) and np.array_equal(a["dup_counters"], ctr.astype(np.float64))
    assert 0 < a["permutation"].size < n and np.unique(a["permutation"]).size == a["permutation"].size
    assert set(np.unique(a["qual"]).astype(int)) <= set(range(2, 42))


@pytest.mark.gpu
@pytest.mark.fresh_only
def test_bench_dump_outputs_repeat(tmp_path):
    """two runs with the same arguments: the same number of timed steps as asked for, and the same outputs, every one under the budget"""
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "300000",
                            "--full", "--no-extra", "--c4-reads", "0", "--cpu-reads", "100000", "--dump-outputs", str(d)],
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["verify"]["ok"]
        runs.append((line, _dumped(d)))
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
    (l0, a), (_, b) = runs
    assert sorted(a) == ["context_table", "cycle_table", "dup_counters", "flags", "permutation", "qual", "qual_table"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    n = l0["config"]["reads_per_gpu"]
    assert a["flags"].shape == (n,) and np.array_equal(np.sort(a["permutation"]), np.arange(n))
    assert a["qual_table"][..., 0].sum() > 0 and a["dup_counters"].sum() > 0


@pytest.mark.gpu
@pytest.mark.fresh_only
def test_bench_plain_run_is_the_headline_only(tmp_path):
    """without --full the run stages, warms up, times the steps and writes its outputs: the line carries the headline fields, and none of
    the measurements that take runs of their own (serial order, side measurements, CPU baseline, verify)"""
    d = tmp_path / "plain"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "300000",
                        "--dump-outputs", str(d)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert "extra" not in line and "cpu_baseline" not in line and "verify" not in line and line["serial_order"] is None
    assert sorted(_dumped(d)) == ["context_table", "cycle_table", "dup_counters", "flags", "permutation", "qual", "qual_table"]
