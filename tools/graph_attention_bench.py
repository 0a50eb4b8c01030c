#!/usr/bin/env python
"""The attention ops of csrc/lb_graph.hip beside the same quantities written in torch alone, in the protocol of
tools/graph_ops_bench.py.

    python tools/graph_attention_bench.py [--repeats 20] [--inner 50] [--only rpf2d] [--heads 8] [--head-dim 16] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1, H = 8 heads of D = 16 columns (C = H D = 128).  Per workload and role:

  segment_softmax            logits (E_cap, C) -> (E_cap, C), graph.Graph.segment_softmax
  attend forward             logits (E_cap, H), values (E_cap, H, D) -> (N, H, D), graph.Graph.attend
  attend forward + backward  the same with requires_grad leaves and one backward

each beside (a) torch only, over the REAL slots only (a prefix at B = 1): scatter_reduce("amax"), exp, index_add_, divide,
multiply, index_add_, and their autograd for the backward figure - float atomics, no pad handling; and (b), for information,
the composition of this library's own separate ops, segment_sum(segment_softmax(l)[..., None] * v).  Each figure is the
median of `--repeats` windows of `--inner` calls between two device events (after one warm-up window), with the spread
(min .. max) of the windows.  The graph.Graph figures include its Python wrapper and autograd node, as the torch ones do.

Bytes are those the op has to move, from the shapes: the softmax reads E C-rows and writes E_cap; attend reads E (H + H D)
floats and writes N (H D + 2 H); its backward reads the same inputs and N H D of d_out and writes E_cap (H + H D); plus the
int32 indices.  The fraction is of the 8.0 TB/s HBM3E peak; these tensors fit the 256 MiB Infinity Cache.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.graph_ops_bench import WORKLOADS, line, windows  # noqa: E402


def run(case, H, D, repeats, inner):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    ds = make_case(case, n_trajs=1, extra_seq_length=1)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=ds.noise_std, external_force_fn=ds.force)
    pos, pt = ds[0]
    feats, _ = hcase.allocate_eval((pos[None, :, :ds.input_seq_length].astype(np.float64), pt[None]))
    eng = feats.engine
    g = Graph(feats)
    N, E_cap, C = eng.N, eng.e_cap, H * D
    idx, ne = eng.nl_idx()
    E = int(ne[0])
    gen = torch.Generator(device=eng.device).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=eng.device, generator=gen)   # noqa: E731
    wide, logits, values, w = 3 * rnd(1, E_cap, C), 3 * rnd(1, E_cap, H), rnd(1, E_cap, H, D), rnd(1, N, H, D)
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, H = {H}, D = {D} (C = {C})"]
    for role, r in (("receivers", 0), ("senders", 1)):
        add = idx[0, r, :E].long().contiguous()

        def t_softmax(x):                       # x (E, K): real slots only
            K = x.shape[1]
            m = x.new_zeros((N, K)).scatter_reduce(0, add[:, None].expand(-1, K), x.detach(), "amax", include_self=False)
            e = torch.exp(x - m[add])
            return e / x.new_zeros((N, K)).index_add_(0, add, e)[add]

        def t_attend(l, v):                     # (E, H), (E, H, D)
            return v.new_zeros((N, H, D)).index_add_(0, add, t_softmax(l)[..., None] * v)

        def own_composition(l, v):
            return g.segment_sum(g.segment_softmax(l, role)[..., None] * v, role)

        def fwd_bwd(fn, l, v, d):
            l.grad = v.grad = None
            fn(l, v).backward(d)

        # the three routes agree before they are timed
        ours = g.attend(logits, values, role)
        assert torch.equal(ours, own_composition(logits, values))
        assert torch.allclose(ours[0], t_attend(logits[0, :E], values[0, :E]), rtol=1e-4, atol=1e-5)
        assert torch.allclose(g.segment_softmax(wide, role)[0, :E], t_softmax(wide[0, :E]), rtol=1e-4, atol=1e-6)
        idx_b = 4 * (N + 1) + (4 * (E + N + 1) if r else 0)
        b_soft = 4 * C * (E + E_cap) + idx_b
        b_fwd = 4 * E * (H + C) + 4 * N * (C + 2 * H) + idx_b
        b_bwd = 4 * E * (H + C) + 4 * N * (C + 2 * H) + 4 * E_cap * (H + C) + idx_b + 4 * (E + 2)
        lg, vg = logits.clone().requires_grad_(), values.clone().requires_grad_()
        lr_, vr_ = logits[0, :E].clone().requires_grad_(), values[0, :E].clone().requires_grad_()
        wr = w[0]
        rows = [("segment_softmax", b_soft, lambda: g.segment_softmax(wide, role), lambda: t_softmax(wide[0, :E]), None),
                ("attend forward", b_fwd, lambda: g.attend(logits, values, role), lambda: t_attend(logits[0, :E], values[0, :E]),
                 lambda: own_composition(logits, values)),
                ("attend forward + backward", b_fwd + b_bwd, lambda: fwd_bwd(lambda l, v: g.attend(l, v, role), lg, vg, w),
                 lambda: fwd_bwd(t_attend, lr_, vr_, wr), lambda: fwd_bwd(own_composition, lg, vg, w))]
        for tag, nbytes, ours_fn, torch_fn, comp_fn in rows:
            l1, o_ms = line(f"{tag}({role}) ours", windows(ours_fn, repeats, inner), nbytes)
            l2, t_ms = line(f"{tag}({role}) torch only", windows(torch_fn, repeats, inner), nbytes)
            out += [l1, l2]
            note = f"  {tag} over {role}: ours / torch only = {o_ms / t_ms:.2f}x"
            if comp_fn is not None:
                l3, c_ms = line(f"{tag}({role}) own separate ops", windows(comp_fn, repeats, inner), nbytes)
                out.append(l3)
                note += f", ours / own separate ops = {o_ms / c_ms:.2f}x"
            out.append(note)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=16)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_attention_bench: needs a HIP device (no CPU timing)")
    lines = [f"graph attention ops, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.heads, a.head_dim, a.repeats, a.inner)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
