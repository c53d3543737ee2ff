"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy
files that two builds of the project can be compared on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def _outputs(rows):
    rng = np.random.default_rng(1)
    return ({"Q": rng.normal(size=(rows, 4)), "S": (rng.random(rows) > 0.5).astype(np.float32)},
            {"x": np.array([0.25, -1.5])})


def test_dump_writes_whole_arrays_when_they_fit(tmp_path):
    per_row, whole = _outputs(1000)
    info = bench.dump_outputs(str(tmp_path), per_row, whole)
    assert info["sampled_rows"] is None
    assert sorted(os.listdir(str(tmp_path))) == ["Q.npy", "S.npy", "x.npy"]
    for name, a in list(per_row.items()) + list(whole.items()):
        got = np.load(str(tmp_path / (name + ".npy")))
        assert got.dtype in (np.float32, np.float64)
        assert np.array_equal(got, a)


def test_dump_samples_the_same_rows_under_the_limit(tmp_path, monkeypatch):
    """A larger output is cut to a fixed, seeded sample of its rows: the same rows on
    every run, every file together within the limit, the indices in rows.npy."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200000)
    per_row, whole = _outputs(50000)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        info = bench.dump_outputs(d, per_row, whole)
        assert 0 < info["sampled_rows"] < 50000
        assert _sizes(d) <= bench.DUMP_LIMIT_BYTES
    rows = np.load(os.path.join(dirs[0], "rows.npy"))
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    for name, a in per_row.items():
        assert np.array_equal(np.load(os.path.join(dirs[0], name + ".npy")), a[r])
    for f in os.listdir(dirs[0]):
        assert np.array_equal(np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f)))
    assert np.array_equal(np.load(os.path.join(dirs[0], "x.npy")), whole["x"])


def test_bench_refuses_zero_steps():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"],
                         capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_twice(hip_device, tmp_path):
    """Two runs with the same arguments: the number of timed steps asked for, the chosen
    point of the last one in x.npy, and identical files (a 40000-row grid: the sweep and
    set passes of the large-grid path)."""
    runs = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--config", "2",
                              "--side", "200", "--steps", "3", "--warmup", "1", "--no-extras",
                              "--no-cpu-baseline", "--no-check-chosen", "--dump-outputs", d],
                             capture_output=True, text=True, timeout=600, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        res = json.loads(out.stdout.strip().splitlines()[-1])
        assert res["steps"] == 3
        assert res["dumped_outputs"]["sampled_rows"] is None
        runs.append((d, res))
    (d, res), (d2, _) = runs
    assert sorted(os.listdir(d)) == ["G.npy", "M.npy", "Q.npy", "S.npy", "x.npy"]
    assert np.array_equal(np.load(os.path.join(d, "x.npy")), res["chosen_x"])
    Q, S = np.load(os.path.join(d, "Q.npy")), np.load(os.path.join(d, "S.npy"))
    assert Q.shape == (40000, 2) and Q.dtype == np.float64 and S.dtype == np.float32
    assert np.array_equal(S, (Q[:, 0] > 0.0).astype(np.float32))
    for f in os.listdir(d):
        assert np.array_equal(np.load(os.path.join(d, f)), np.load(os.path.join(d2, f))), f


def test_bench_offers_full():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0 and "--full" in out.stdout


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(hip_device):
    """Without --full the run stops at the headline: no per-launch pass, no shared-factor
    pass, no CPU baseline or oracle check behind the timed steps."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--config", "2",
                          "--side", "200", "--steps", "3", "--warmup", "1"],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 3 and res["warmup"] == 1 and res["value"] > 0
    for key in ("roofline", "shared_factor", "per_rank_sweep_ms", "cpu_baseline", "parity"):
        assert key not in res, key
