"""bench.py --dump-outputs: what the last timed step computed, written as .npy files within a size limit, the same on every
run of the same command; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_arrays_whole_under_the_limit(tmp_path):
    import bench
    arrays = {"stats": np.array([1.5, 7.0, 9.0], dtype=np.float32), "params": np.linspace(-1, 1, 1000, dtype=np.float64)}
    got = bench.dump_outputs(str(tmp_path), arrays)
    assert got == {"stats": (3, 3), "params": (1000, 1000)}
    for k, a in arrays.items():
        b = np.load(os.path.join(tmp_path, k + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b)


def test_dump_outputs_samples_large_arrays_to_the_limit(tmp_path):
    import bench
    n, limit = 1 << 20, 1 << 21
    arrays = {"stats": np.arange(3, dtype=np.float32), "params": np.arange(n, dtype=np.float32),
              "exp_avg": -np.arange(n, dtype=np.float32), "big64": np.arange(n // 2, dtype=np.float64)}
    got = bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    assert sum(_sizes(tmp_path / "a").values()) <= limit
    assert got["stats"] == (3, 3) and all(got[k][0] < got[k][1] for k in ("params", "exp_avg", "big64"))
    p, e = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "exp_avg.npy")
    assert p.dtype == np.float32 and np.load(tmp_path / "a" / "big64.npy").dtype == np.float64
    assert (np.diff(p) > 0).all() and p[0] >= 0 and p[-1] < n          # distinct entries, in index order
    assert np.array_equal(e, -p)                                          # the same indices for arrays of the same length
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)          # the same entries on every call
    for f in _sizes(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_dump_outputs_refuses_other_dtypes(tmp_path):
    import bench
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), {"counts": np.arange(4, dtype=np.int32)})


@pytest.mark.gpu
@pytest.mark.parametrize("module", ["cogmen", "dagerc"])
def test_bench_dump_outputs_repeat(tmp_path, module):
    """Two runs of the same bench command time --steps steps and dump the same outputs of the last one: the stats the step
    returns (the line's loss), the updated parameters and both optimizer moments, float32, 64 MB at most (DAG-ERC's 6.4 M
    parameters x 3 buffers exceed it: sampled)."""
    lines = []
    for run in ("a", "b"):
        res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--module", module, "--steps", "3", "--warmup", "2",
                              "--no_cpu_baseline", "--no_fp32_path", "--kernel_reps", "2", "--dump-outputs", str(tmp_path / run)],
                             cwd=REPO, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines.append(json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1]))
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
    names = sorted(_sizes(tmp_path / "a"))
    assert names == ["exp_avg.npy", "exp_avg_sq.npy", "params.npy", "stats.npy"] and names == sorted(_sizes(tmp_path / "b"))
    assert sum(_sizes(tmp_path / "a").values()) <= 64 * 1000 * 1000
    stats = np.load(tmp_path / "a" / "stats.npy")
    assert stats.shape == (3,) and float(stats[0]) == lines[0]["config"]["loss"]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), f
        assert float(np.abs(a - b).max()) <= 1e-5 * max(1e-30, float(np.abs(a).max())), f


def test_bench_refuses_zero_timed_steps():
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 2 and "--steps" in res.stderr and not res.stdout.strip()
