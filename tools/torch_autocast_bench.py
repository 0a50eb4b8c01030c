#!/usr/bin/env python
"""One loss_grad of the README's MyMP (h = 128) through models.TorchModel on RPF2D-3.2k, B = 1, with and without
``autocast=torch.bfloat16``: the end-to-end figure beside tools/graph_ops_bench.py --dtype bf16.

    python tools/torch_autocast_bench.py [--repeats 20] [--hidden 128] [--out FILE]

ms per ``model.loss_grad`` (features, forward, loss, backward into the training handle's gradient blob; the call returns the
loss as a float, so each one is complete when it returns): the median of `--repeats` calls after three warm-up calls, with
their spread.  Reported, not gated.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("torch_autocast_bench: needs a HIP device (no CPU timing)")
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import TorchModel

    class MyMP(torch.nn.Module):
        def __init__(self, node_in, dim, h):
            super().__init__()
            self.enc, self.dec = torch.nn.Linear(node_in, h), torch.nn.Linear(h, dim)
            self.edge, self.node = torch.nn.Linear(2 * h + dim + 1, h), torch.nn.Linear(2 * h, h)

        def forward(self, features, particle_type, graph):
            x = torch.nn.functional.silu(self.enc(features["vel_hist"]))
            e = torch.cat([graph.gather(x, "senders"), graph.gather(x, "receivers"), features["rel_disp"], features["rel_dist"]], -1)
            agg = graph.segment_sum(torch.nn.functional.silu(self.edge(e)), "receivers")
            return self.dec(x + torch.nn.functional.silu(self.node(torch.cat([x, agg], -1))))

    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=1)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=ds.noise_std, external_force_fn=ds.force)
    pos, pt = ds[0]
    isl, dim = ds.input_seq_length, pos.shape[-1]
    feats, _ = hcase.allocate_eval((pos[None, :, :isl].astype(np.float64), pt[None]))
    eng = feats.engine
    target = {"acc": torch.randn((1, eng.N, dim), generator=torch.Generator().manual_seed(0)).to(eng.device)}
    lines = [f"MyMP (h = {a.hidden}) on RPF2D-3.2k, N = {eng.N}, E_cap = {eng.e_cap}, {torch.cuda.get_device_name(0)}; ms per "
             f"loss_grad, median of {a.repeats}"]
    med = {}
    for name, flag in (("float32", None), ("autocast bfloat16", torch.bfloat16)):
        model = TorchModel(MyMP((isl - 1) * dim, dim, a.hidden), autocast=flag)
        params, _ = model.init(np.array([0]), None)
        th = model.train_handle(eng, params)
        ms = []
        for i in range(3 + a.repeats):
            th.zero_grad()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = model.loss_grad(th, target, {"acc": 1.0})
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(1e3 * (time.perf_counter() - t0))
        th.close()
        med[name] = statistics.median(ms)
        lines.append(f"  {name:18s} median {med[name]:7.3f} ms  (min {min(ms):7.3f}  max {max(ms):7.3f})  loss {loss:.6e}")
    lines.append(f"  autocast / float32 = {med['autocast bfloat16'] / med['float32']:.2f}x")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
