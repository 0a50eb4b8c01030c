"""``python -m lagrangebench_amd`` end to end, the way a reference user starts a run (main.py): one child process trains the
Linear baseline on the LJ set from a YAML file that extends LAGRANGEBENCH_DEFAULTS plus command-line overrides, a second one
runs inference from the checkpoint directory the first one left (``load_ckp=<run>/best``)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

yaml = pytest.importorskip("yaml")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ = os.path.join(ROOT, "tests", "golden", "3D_LJ_3_1214every1")


def _run(argv, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return subprocess.run([sys.executable, "-m", "lagrangebench_amd"] + argv, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def test_train_from_a_config_file_then_infer_from_the_checkpoint(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(LJ, ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    md.setdefault("write_every", 1)
    json.dump(md, open(ds_dir / "metadata.json", "w"))
    (tmp_path / "lj.yaml").write_text(
        "extends: LAGRANGEBENCH_DEFAULTS\n\n"
        "dataset:\n  src: 3D_LJ_3_1214every1\n\n"          # relative to the working directory, like the reference's files
        "model:\n  input_seq_length: 3\n\n"
        "train:\n  noise_std: 0.0\n  optimizer:\n    lr_start: 1e-3\n\n"
        "eval:\n  n_rollout_steps: 5\n  train:\n    n_trajs: 2\n    metrics_stride: 5\n"
        "  infer:\n    n_trajs: 2\n    metrics: [mse]\n    out_type: none\n\n"
        "logging:\n  log_steps: 1\n  eval_steps: 5\n  ckp_dir: ckp\n")
    r = _run(["config=lj.yaml", "model.name=linear", "train.step_max=10", "logging.run_name=cli", "gpu=0"], str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Starting a LagrangeBench run with the following configs:" in r.stdout and "gpu / xla_mem_fraction are ignored" in r.stdout
    assert "  name: linear" in r.stdout and "  step_max: 10" in r.stdout and "lr_start: 0.001" in r.stdout
    assert "Start training..." in r.stdout and "Start inference..." in r.stdout and "train/loss" in r.stdout
    best = tmp_path / "ckp" / "cli" / "best"
    for f in ("config.yaml", "params_tree.pkl", "metadata_ckp.json"):
        assert (best / f).is_file(), f
    assert (tmp_path / "ckp" / "cli" / "config.yaml").is_file()

    r2 = _run(["load_ckp=ckp/cli/best", "mode=infer"], str(tmp_path))
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "mode: infer" in r2.stdout and "load_ckp: ckp/cli/best" in r2.stdout and "  name: linear" in r2.stdout
    assert "Start training..." not in r2.stdout and "Start inference..." in r2.stdout
    assert "Metrics of ckp/cli/best on valid split:" in r2.stdout and "mse" in r2.stdout.split("Metrics of")[1]
