#!/usr/bin/env python
"""PaiNN-5-128 training-step time on the device (csrc/lb_train_painn.h).

    python tools/painn_train_bench.py [--warmup 3] [--repeats 20] [--only rpf2d_b1_runner] [--out FILE]

Workloads: RPF2D-3.2k B = 1 and TGV3D-8k B = 1 (synthetic cases of lagrangebench_amd.data, seeded inputs and weights),
each at the runner's radius 1.5 * default_connectivity_radius (few edges live: the network's norms are in units of the
connectivity radius) and at radius 1.5 (every edge live).  A step is zero_grad + loss_grad + adamw_step on one
preprocessed batch; per workload `--warmup` untimed steps (allocation, operand packing, code objects), then `--repeats`
timed steps, each a host clock around the step, which ends in a device synchronise.  Prints the median and the spread
in ms per step.  The kernel trace is a separate run:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/painn_train_bench.py --only rpf2d_b1_live --repeats 5
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"rpf2d_b1_runner": ("rpf2d", 1, "runner"), "rpf2d_b1_live": ("rpf2d", 1, 1.5),
             "tgv3d_b1_runner": ("tgv3d", 1, "runner"), "tgv3d_b1_live": ("tgv3d", 1, 1.5)}


def run(name, case, B, radius, warmup, repeats, L=5, H=128):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    ds = make_case(case, n_trajs=B, extra_seq_length=1, vel_amp=0.03)   # (as tools/painn_bench.py)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm, "magnitude_features": True},
                         noise_std=ds.noise_std, external_force_fn=ds.force)
    pos = np.stack([ds[i][0] for i in range(B)]).astype(np.float64)
    pt = np.stack([ds[i][1] for i in range(B)])
    key = torch.Generator()
    key.manual_seed(0)
    key, feats, target, _ = hcase.allocate(key, (pos, pt), ds.noise_std)
    r = 1.5 * ds.metadata["default_connectivity_radius"] if radius == "runner" else float(radius)   # runner.py:272
    model = PaiNN(H, 1, L, gaussian_rbf(20, r, trainable=True), cosine_cutoff(r), ds.input_seq_length - 1)
    params, state = model.init_params(0, ds.external_force_fn is not None)
    th = model.train_handle(feats.engine, params, state)

    def step():
        th.zero_grad()
        th.loss_grad(target["acc"], 1.0)   # (host-synchronous: ends in a stream synchronise)
        th.adamw_step(5e-4)
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        step()
        ms.append((time.perf_counter() - t0) * 1e3)
    st = feats.engine.stats()
    th.close()
    return (f"{name:16s} N={ds.metadata['num_particles_max']:5d} B={B} E={st['n_edges_total']:7d} radius {r:.4g} "
            f"ms/train step median {statistics.median(ms):.3f} min {min(ms):.3f} max {max(ms):.3f} "
            f"(warm-up {warmup}, repeats {repeats})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("painn_train_bench: needs a HIP device (no CPU timing)")
    names = [a.only] if a.only else list(WORKLOADS)
    lines = [f"PaiNN-5-128 training step (zero_grad + loss_grad + adamw_step), {torch.cuda.get_device_name(0)}"]
    for n in names:
        lines.append(run(n, *WORKLOADS[n], a.warmup, a.repeats))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
