#!/usr/bin/env python
"""The window gradient of a user's torch network (csrc/lb_graph.hip: lb_graph_features_backward; autograd.TorchModule), in the
protocol of tools/graph_ops_bench.py.

    python tools/torch_window_grad_bench.py [--repeats 20] [--inner 50] [--only rpf2d] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1.  Per workload:

  (a) features_backward      engine.graph_features_backward with every cotangent the case has, beside the same transposition
                             written in torch alone on the device: the velocity (and wall) terms by slicing, float64 index_add_
                             of +h over the receivers and -h over the senders of the REAL slots into zeros (float atomics)
  (b) one step               a TinyMP (hidden 32) forward + backward through TorchModule, window.requires_grad off and on
  (c) two-step unroll        p1 = mod(w1); p2 = mod(advance_window(w1, p1)); forward and backward timed apart: the backward
                             holds the one reload of w1 with its list rebuild

Each figure is the median of `--repeats` windows of `--inner` calls between device events (after one warm-up window), with the
spread (min .. max) of the windows; (b) and (c) include Python, torch's dense layers and autograd.  Bytes of (a) are what the
op has to move, from the shapes: per edge its fp32 feature row and cotangents (dim + 1 floats each) once as a receiver and
once as a sender, the node cotangents, the fp64 result, the int32 rows; the fraction is of the 8.0 TB/s HBM peak (these
tensors fit the Infinity Cache).
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.graph_ops_bench import WORKLOADS, line, windows  # noqa: E402


def split_windows(first, second, repeats, inner):
    """ms per call of first() and of second(), called in turn: `repeats` windows of `inner` pairs, each half between its own
    device events, after one warm-up window."""
    import torch
    for _ in range(inner):
        first()
        second()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(inner)]
        for a, b, c in ev:
            a.record()
            first()
            b.record()
            second()
            c.record()
        torch.cuda.synchronize()
        out[0].append(sum(a.elapsed_time(b) for a, b, c in ev) / inner)
        out[1].append(sum(b.elapsed_time(c) for a, b, c in ev) / inner)
    return out


def tline(tag, ms):
    med = statistics.median(ms)
    return f"  {tag:46s} median {med * 1e3:9.2f} us  (min {min(ms) * 1e3:9.2f}  max {max(ms) * 1e3:9.2f})", med


def run(case, repeats, inner):
    import torch
    from lagrangebench_amd.autograd import TorchModule, advance_window
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import TorchModel
    from tests._torch_models import TinyMP, node_in_of
    ds = make_case(case, n_trajs=1, extra_seq_length=2)
    isl = ds.input_seq_length
    hcase = case_builder(ds.box, ds.metadata, isl, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=ds.noise_std, external_force_fn=ds.force)
    pos, pt = ds[0]
    window = torch.as_tensor(pos[None, :, :isl].astype(np.float64))
    feats, _ = hcase.allocate_eval((window.numpy(), pt[None]))
    eng = feats.engine
    N, E_cap, dim, K = eng.N, eng.e_cap, eng.dim, isl - 1
    idx, ne = eng.nl_idx()
    E = int(ne[0])
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, isl = {isl}, dim = {dim}"]
    gen = torch.Generator(device=eng.device).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=eng.device, generator=gen)   # noqa: E731

    # ---- (a) the op beside torch alone
    cot = {"d_abs_pos": rnd(N, isl, dim), "d_vel_hist": rnd(N, K * dim), "d_rel_disp": rnd(E_cap, dim), "d_rel_dist": rnd(E_cap, 1)}
    if eng.has_vel_mag:
        cot["d_vel_mag"] = rnd(N, K)
    if eng.has_bound:
        cot["d_bound"] = rnd(N, 2 * dim)
    recv, send = idx[0, 0, :E].long().contiguous(), idx[0, 1, :E].long().contiguous()
    rd, rr = feats["rel_disp"][0, :E].float(), feats["rel_dist"][0, :E].float()
    nf = eng.node_features()
    vh = nf["vel_hist"][0].float().reshape(N, K, dim)
    vm = nf["vel_mag"][0].float() if eng.has_vel_mag else None
    bd = nf["bound"][0].float() if eng.has_bound else None
    inv_std = 1.0 / torch.as_tensor(np.asarray(hcase.normalization_stats["velocity"]["std"], np.float64), device=eng.device)
    rc = float(ds.metadata["default_connectivity_radius"])

    def torch_only():
        res = cot["d_abs_pos"].double()
        g = cot["d_vel_hist"].reshape(N, K, dim).double()
        if vm is not None:
            m = vm.double()[..., None]
            g = g + torch.where(m != 0, cot["d_vel_mag"].double()[..., None] / m, torch.zeros_like(m)) * vh.double()
        g = g * inv_std
        res[:, 1:] += g
        res[:, :-1] -= g
        new = res[:, -1]
        if bd is not None:
            inside = ((bd > -1) & (bd < 1)).double() * cot["d_bound"].double() / rc
            new += inside[:, :dim] - inside[:, dim:]
        dist = rr.double()
        w = torch.where(dist != 0, cot["d_rel_dist"][:E].double() / dist, torch.zeros_like(dist))
        h = (cot["d_rel_disp"][:E].double() + w * rd.double()) / rc
        new.index_add_(0, recv, h)
        new.index_add_(0, send, -h)
        return res

    ours = eng.graph_features_backward(**cot)[0]
    ref = torch_only()
    assert float((ours - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), "the two transpositions disagree"
    nbytes = 2 * E * 4 * 2 * (dim + 1) + N * 4 * (isl * dim + K * dim) + N * isl * dim * 8 + 4 * (3 * (N + 1) + E)
    l1, o_ms = line("(a) features_backward, ours", windows(lambda: eng.graph_features_backward(**cot), repeats, inner), nbytes)
    l2, t_ms = line("(a) features_backward, torch only", windows(torch_only, repeats, inner), nbytes)
    out += [l1, l2, f"  (a) ours / torch only = {o_ms / t_ms:.2f}x"]

    # ---- (b) one step of a TinyMP through TorchModule
    model = TorchModel(TinyMP(node_in_of(eng), dim, 32))
    params, state = model.init(np.array([7]), None)
    mod = TorchModule(model, hcase, params, 1, state=state)
    pt_dev = torch.as_tensor(pt[None]).to(eng.device)
    w_plain = window.to(eng.device)
    w_grad = w_plain.clone().requires_grad_(True)
    d_out = rnd(1, N, dim)

    def step(w):
        mod.zero_grad()
        w.grad = None
        mod(w, pt_dev)["acc"].backward(d_out)

    l3, p_ms = tline("(b) forward + backward, window.requires_grad off", windows(lambda: step(w_plain), repeats, inner))
    l4, g_ms = tline("(b) forward + backward, window.requires_grad on", windows(lambda: step(w_grad), repeats, inner))
    out += [l3, l4, f"  (b) the window gradient costs {1e3 * (g_ms - p_ms):.2f} us a step ({g_ms / p_ms:.2f}x)"]

    # ---- (c) the two-step unroll, forward and backward apart
    hold = {}

    def unroll_forward():
        mod.zero_grad()
        w_grad.grad = None
        p1 = mod(w_grad, pt_dev)["acc"]
        p2 = mod(advance_window(hcase, w_grad, p1, "acc"))["acc"]
        hold["loss"] = (p1 * d_out).sum() + (p2 * d_out).sum()

    def unroll_backward():
        hold["loss"].backward()

    restored0 = mod.restored
    f_ms, b_ms = split_windows(unroll_forward, unroll_backward, repeats, inner)
    assert mod.restored - restored0 == (repeats + 1) * inner          # one reload + rebuild per backward
    l5, uf = tline("(c) two-step unroll, forward", f_ms)
    l6, ub = tline("(c) two-step unroll, backward (one list rebuild)", b_ms)
    out += [l5, l6, f"  (c) unroll forward + backward {1e3 * (uf + ub):.2f} us = {(uf + ub) / g_ms:.2f}x one step with the window gradient"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("torch_window_grad_bench: needs a HIP device (no CPU timing)")
    lines = [f"torch window gradient, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.repeats, a.inner)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
