#!/usr/bin/env python
"""Linear baseline rollout step time on the device (csrc/lb_linear.hip), by the method of tools/painn_bench.py.

    python tools/linear_bench.py [--steps 200] [--repeats 10] [--only rpf2d_b1] [--out FILE]

Workloads: RPF2D-3.2k B = 1, RPF2D-3.2k B = 8, TGV3D-8k B = 1 (synthetic cases of lagrangebench_amd.data, seeded inputs,
seeded initial weights scaled down for a calm rollout, magnitude features on).  Per workload: one warm-up rollout of the same
length (allocation, code-object load), then `--repeats` timed rollouts of `--steps` steps, each a host clock around
lb_linear_rollout, which ends in a device synchronise.  Prints the median and the spread in ms per rollout step.  A step is
three launches (node features, k_ln_forward, integrator) and no neighbor search, so the figure is launch overhead: it is a
baseline, there is no bar on it.
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


def run(name, case, B, steps, repeats):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import Linear
    ds = make_case(case, n_trajs=B, extra_seq_length=steps, vel_amp=0.03)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm, "magnitude_features": True},
                         noise_std=ds.noise_std, external_force_fn=ds.force)
    pos = np.stack([ds[i][0] for i in range(B)]).astype(np.float64)
    pt = np.stack([ds[i][1] for i in range(B)])
    eng = hcase.engine(B)
    eng.set_particle_type(pt)
    model = Linear(len(ds.box))
    params = model.init_params(0, eng.node_in + 1)
    params["linear"]["w"] *= np.float32(0.01)
    traj = eng.prepare_traj(pos)
    h = model.handle(eng, params)
    eng.rollout(h, traj, steps)  # warm-up: code objects (and the one list allocation lb_linear_rollout leaves behind)
    torch.cuda.synchronize()
    eng.edge_accounting(reset=True)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.rollout(h, traj, steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    builds = eng.edge_accounting()["builds"]
    med = statistics.median(ms)
    return (f"{name:9s} N={ds.metadata['num_particles_max']:5d} B={B} inputs={eng.node_in + 1} "
            f"ms/step median {med:.4f} min {min(ms):.4f} max {max(ms):.4f} (repeats {repeats} x {steps} steps, "
            f"neighbor-list builds in the timed rollouts {builds})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_bench: needs a HIP device (no CPU timing)")
    names = [a.only] if a.only else list(WORKLOADS)
    lines = [f"Linear rollout, {torch.cuda.get_device_name(0)}"]
    for n in names:
        lines.append(run(n, *WORKLOADS[n], a.steps, a.repeats))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
