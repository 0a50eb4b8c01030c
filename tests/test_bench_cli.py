"""bench.py's two modes: a plain run prints the headline line only; --full appends the objects that take runs of
their own (roofline, breakdown, sub-runs, CPU baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_aggregate", "breakdown_ms_per_step", "power", "f32_exact", "other_configs",
             "stationary", "train_step", "cpu_baseline")


def test_pmc_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--pmc"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
           "--workload", "tgv2d", "--repeats", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "rollout particle-steps/sec" and d["unit"] == "particle-steps/s" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 2 and d["repeats"]["n"] == 2 and d["dtype"].startswith("f32")
    n = d["config"]["n_particles"]
    assert abs(d["value"] - 2 * n * 3 / (d["ms_per_step"] * 3e-3)) <= 1e-6 * d["value"]
    assert np.isfinite(d["mse20_mean"]) and d["config"]["edges_per_traj_mean"] > 0
    assert not [k for k in FULL_ONLY if k in d], sorted(d)
    assert sorted(os.listdir(tmp_path)) == ["mse.npy", "pred.npy", "pred_last_step.npy"]
    assert np.load(tmp_path / "pred.npy").shape == (2, 3, n, 2)
