"""Wall time of one Trainer step whose push-forward unroll runs from host weights or from the device weights
(train.device_unroll).

    python tools/unroll_bench.py --case tgv2d|tgv3d|rpf2d-egnn [--device-unroll 0|1] [--steps 200] [--warmup 20]

GNS-10-128 on the synthetic TGV2D-2.5k / TGV3D-8k cases, EGNN-5-128 on RPF2D, batch_size 1, evaluation off, noise_std 3e-4,
pushforward {"steps": [-1, -1], "unrolls": [0, 1], "probs": [0, 1]}: EVERY step unrolls once.  A step is timed from one
entry of model.loss_grad to the next - one whole turn of the Trainer's loop: sample, noise, neighbor list, the unroll
(weights to the model, forward, integrate, neighbor list again), loss, backward, AdamW; loss_grad returns the loss as a host
float, so the stream is empty at every mark.  Prints one JSON line: median / quartiles of the steps after the warm-up.
The script runs on a tree without train.device_unroll as well (--device-unroll 0), which is how the parent commit is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="tgv2d", choices=["tgv2d", "tgv3d", "rpf2d-egnn"])
    ap.add_argument("--device-unroll", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN, GNS
    from lagrangebench_amd.train import Trainer

    isl, extra = 6, 2
    name = args.case.split("-")[0]
    ds = make_case(name, n_trajs=8, extra_seq_length=extra, input_seq_length=isl)
    dim = len(ds.box)
    case = case_builder(ds.box, ds.metadata, isl, cfg_neighbors={"multiplier": ds.multiplier},
                        cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=3e-4, external_force_fn=ds.force)
    cfg_train = {"batch_size": 1, "noise_std": 3e-4, "pushforward": {"steps": [-1, -1], "unrolls": [0, 1], "probs": [0, 1]}}
    if args.device_unroll:
        cfg_train["device_unroll"] = True
    if args.case == "rpf2d-egnn":
        model = EGNN(128, 1, ds.metadata["dt"] * ds.metadata["write_every"], isl - 1,
                     normalization_stats=case.normalization_stats, num_mp_steps=5)
        cfg_train["loss_weight"] = {"pos": 1.0, "vel": 0.0, "acc": 0.0}
    else:
        model = GNS(dim, 128, 2, 10, 16)
    marks = []
    inner = model.loss_grad

    def timed(*a, **k):
        marks.append(time.perf_counter())
        return inner(*a, **k)

    model.loss_grad = timed
    n = args.warmup + args.steps
    trainer = Trainer(model, case, ds, ds, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": extra, "train": {"n_trajs": 1, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 10**9, "eval_steps": 10**9}, input_seq_length=isl, seed=0)
    trainer.train(step_max=n)
    torch.cuda.synchronize()
    dt = np.diff(np.asarray(marks))[args.warmup:] * 1e3
    q = np.percentile(dt, [25, 50, 75])
    print(json.dumps({"label": args.label, "case": args.case, "device_unroll": bool(args.device_unroll), "steps": int(dt.size),
                      "N": int(ds.metadata["num_particles_max"]), "step_ms_median": round(float(q[1]), 4),
                      "step_ms_q25": round(float(q[0]), 4), "step_ms_q75": round(float(q[2]), 4),
                      "step_ms_min": round(float(dt.min()), 4)}), flush=True)


if __name__ == "__main__":
    main()
