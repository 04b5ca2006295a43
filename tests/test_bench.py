"""bench.py's plain run (the headline only) and --dump-outputs (what the timed path computed in its last step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")


class _Session:
    """Stands in for mavmap_amd.Session: get_params() / result() are all dump_outputs reads."""

    def __init__(self, ni, nc, np_):
        rng = np.random.default_rng(5)
        self.params = rng.normal(size=(ni, 6)), rng.normal(size=(nc, 9)), rng.normal(size=(np_, 3))

    def get_params(self):
        return tuple(a.copy() for a in self.params)

    def result(self):
        return dict(initial_cost=10.0, final_cost=2.5)


def test_dump_outputs_writes_float64_arrays_and_a_seeded_sample_above_the_limit(tmp_path, monkeypatch):
    import bench
    sess = _Session(7, 2, 1000)
    bench.dump_outputs(str(tmp_path / "all"), sess, 0, 1)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["cost", "intrinsics", "points", "poses"]
    assert all(a.dtype == np.float64 for a in got.values())
    for a, b in zip((got["poses"], got["intrinsics"], got["points"]), sess.params):
        assert np.array_equal(a, b)
    assert np.array_equal(got["cost"], [10.0, 2.5])

    # above the limit: the points are a fixed sample of rows, their indices beside them, everything within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 12 * 1024)
    samples = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), sess, 0, 1)
        files = sorted(os.listdir(tmp_path / run))
        assert files == ["cost.npy", "intrinsics.npy", "points.npy", "points_index.npy", "poses.npy"]
        assert sum(np.load(tmp_path / run / f).nbytes for f in files) <= 12 * 1024
        idx, pts = np.load(tmp_path / run / "points_index.npy"), np.load(tmp_path / run / "points.npy")
        assert 0 < len(idx) < 1000 and len(idx) == len(pts) and np.all(np.diff(idx) > 0)
        assert np.array_equal(pts, sess.params[2][idx.astype(np.int64)])
        samples.append(idx)
    assert np.array_equal(*samples)


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(mavba, tmp_path):
    """`bench.py --steps K --warmup W` without --full: ONE JSON line holding the headline keys and none of --full's; K is the
    number of timed steps; --dump-outputs writes the last timed step's parameters and cost, identical from run to run."""
    from mavmap_amd import synth
    p = synth.make_config("C2", scale=0.2)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--config", "C2",
                              "--scale", "0.2", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        r = json.loads(lines[0])
        assert set(r) == set(HEADLINE), sorted(r)
        assert r["steps"] == 7 and r["warmup"] == 2 and r["n_gpus"] == 1 and r["value"] > 0 and r["dtype"] == "f64"
        assert r["unit"] == "iter/s" and r["higher_is_better"] is True
        assert abs(r["ms_per_step"] * r["value"] - 1e3) < 1.0
        got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert sorted(got) == ["cost", "intrinsics", "points", "poses"]
        assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
        assert got["poses"].shape == (p.num_images, 6) and got["intrinsics"].shape == (p.num_cameras, 9)
        assert got["points"].shape == (p.num_points, 3)
        assert got["cost"][1] <= got["cost"][0]
        dumps.append(got)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
