#!/usr/bin/env python
"""PaiNN-5-128 rollout step time on the device (csrc/lb_painn.hip).

    python tools/painn_bench.py [--steps 20] [--repeats 10] [--only rpf2d_b1] [--out FILE]

Workloads: RPF2D-3.2k B = 1, RPF2D-3.2k B = 8, TGV3D-8k B = 1 (synthetic cases of lagrangebench_amd.data, seeded
inputs, untrained seeded weights, the runner's radius 1.5 * default_connectivity_radius).  Per workload: one warm-up
rollout of the same length (allocation, code-object load), then
`--repeats` timed rollouts of `--steps` steps, each a host clock around lb_painn_rollout, which ends in a device
synchronise.  Prints the median and the spread in ms per rollout step.  The kernel trace is a separate run:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/painn_bench.py --only rpf2d_b1 --repeats 3
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"rpf2d_b1": ("rpf2d", 1), "rpf2d_b8": ("rpf2d", 8), "tgv3d_b1": ("tgv3d", 1)}


def run(name, case, B, steps, repeats, L=5, H=128):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    # vel_amp 0.03: the particles stay near their lattice sites, so the neighbour count is the dataset's own
    ds = make_case(case, n_trajs=B, extra_seq_length=steps, vel_amp=0.03)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm, "magnitude_features": True},
                         noise_std=ds.noise_std, external_force_fn=ds.force)
    pos = np.stack([ds[i][0] for i in range(B)]).astype(np.float64)
    pt = np.stack([ds[i][1] for i in range(B)])
    r = 1.5 * ds.metadata["default_connectivity_radius"]  # runner.py:272
    model = PaiNN(H, 1, L, gaussian_rbf(20, r, trainable=True), cosine_cutoff(r), ds.input_seq_length - 1)
    params, state = model.init_params(0, ds.external_force_fn is not None)
    eng = hcase.engine(B)
    eng.set_particle_type(pt)
    traj = eng.prepare_traj(pos)
    h = model.handle(eng, params, state)
    eng.rollout(h, traj, steps)  # warm-up: neighbour-list allocation, code objects
    torch.cuda.synchronize()
    ms = []
    n_realloc = 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, nre = eng.rollout(h, traj, steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
        n_realloc += nre
    st = eng.stats()
    med = statistics.median(ms)
    return (f"{name:9s} N={ds.metadata['num_particles_max']:5d} B={B} E/step={st['n_edges_total']:7d} "
            f"ms/step median {med:.4f} min {min(ms):.4f} max {max(ms):.4f} (repeats {repeats} x {steps} steps, "
            f"reallocs {n_realloc})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("painn_bench: needs a HIP device (no CPU timing)")
    names = [a.only] if a.only else list(WORKLOADS)
    lines = [f"PaiNN-5-128 rollout, {torch.cuda.get_device_name(0)}"]
    for n in names:
        lines.append(run(n, *WORKLOADS[n], a.steps, a.repeats))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
