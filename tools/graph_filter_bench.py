#!/usr/bin/env python
"""filter_conv of csrc/lb_graph.hip - the continuous-filter convolution with its Linear inside - beside the composition a
user writes without it: torch.nn.functional.linear(f, weight.T), then graph.conv.

    python tools/graph_filter_bench.py [--dtype f32|bf16] [--repeats 20] [--inner 50] [--only tgv3d] [--columns 128] [--basis 20]
                                       [--trial] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1 (synthetic cases of lagrangebench_amd.data, seeded), C = 128 columns, R = 20 basis
functions - the protocol of tools/graph_pair_bench.py.  Per workload and role (receivers, senders), at K = 1 (x (N, C)) and
K = 3 (x (N, 3, C)):

    fused      graph.filter_conv(x, f, weight, role)
    composed   graph.conv(x, torch.nn.functional.linear(f, weight.T), role)

forward alone, forward plus backward through autograd with all three gradients (x, f, weight; a fixed cotangent), and forward
plus backward with x and weight only (f a constant of the step: no gradient to the window).  Each figure is the median of
`--repeats` windows of `--inner` calls between two device events (after a warm-up of at least one window and 0.3 s), with the
spread (min .. max) of the windows; for forward plus backward the two sides alternate, half the windows each in two rounds.
`--trial` times only the fused forward plus backward with all three gradients and the two d_weight launches: one run per library
build of the chunk-size trial (profiles/graph_filter_chunk_trial.txt).  The fused side's launches - the forward / d_x kernel, the d_f kernel, the two d_weight
launches - are also timed alone, through the library entries with preallocated outputs (a ctypes call per launch, so the
device queue stays full): the "kernels alone" lines.  Their sum against the fused forward plus backward says how much of that
figure is the host's dispatch.

Before anything is timed the two sides are compared: they differ in the order of the sums over r, c and the slots (the
library GEMMs state none), so float32 is held to 1e-5 of the largest entry (d_weight, a sum over every slot of the list, to
1e-4) and bfloat16 - where the composition rounds the filter to bfloat16 and filter_conv does not - to 2^-6 of it.

Bytes are those each side has to move, from the shapes: a node tensor read through the cache counts once (N rows), an
edge-shaped tensor counts its real slots when read by a graph kernel and every slot when a GEMM reads or writes it; the
composed side counts the filter it writes and reads back and conv's d_w.  Indices: 4 bytes per entry read.

The verdict line per configuration states the fused side's SLOWEST window against the composition's FASTEST window.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.graph_pair_bench import WORKLOADS, line, windows  # noqa: E402


def filter_bytes(N, E, E_cap, K, R, C, esize, sender, chunks):
    """{(side, what): bytes} of one layer; what = fwd, bwd3 (all three gradients), bwd2 (x and weight), and for the fused side
    its launches alone."""
    row = esize * C
    walk = 4 * (N + 1 + E) + (4 * (E + N + 1) if sender else 0)
    node, real, slots = N * K * row, E * row, E_cap * row
    f_real, f_slots, wt, part = E * R * esize, E_cap * R * esize, R * row, chunks * R * C * 4
    conv = f_real + wt + 2 * node + walk                       # f once, x through the cache, the node rows out
    d_f = 2 * node + wt + f_slots + 8 * E
    d_w = 2 * node + f_real + 8 * E + 2 * part + wt
    gemm_fwd = f_slots + wt + slots
    conv_c = real + 2 * node + walk
    pair = 2 * node + slots + 8 * E                            # conv's d_w
    gemm_dw, gemm_df = slots + f_slots + wt, slots + wt + f_slots
    return {("fused", "fwd"): conv, ("fused", "bwd3"): conv + d_f + d_w, ("fused", "bwd2"): conv + d_w, ("fused", "d_f"): d_f,
            ("fused", "d_w"): d_w, ("composed", "fwd"): gemm_fwd + conv_c,
            ("composed", "bwd3"): conv_c + pair + gemm_dw + gemm_df, ("composed", "bwd2"): conv_c + pair + gemm_dw}


def run(case, C, R, repeats, inner, dtype="f32", trial=False):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtype]
    code = {"f32": 0, "bf16": 1}[dtype]
    ds = make_case(case, n_trajs=1, extra_seq_length=1)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=ds.noise_std, external_force_fn=ds.force)
    pos, pt = ds[0]
    feats, _ = hcase.allocate_eval((pos[None, :, :ds.input_seq_length].astype(np.float64), pt[None]))
    eng = feats.engine
    g = Graph(feats)
    N, E_cap = eng.N, eng.e_cap
    E = int(eng.nl_idx()[1][0])
    gen = torch.Generator(device=eng.device).manual_seed(0)

    def rand(*shape, scale=1.0):
        return (torch.randn(shape, device=eng.device, generator=gen) * scale).to(dt).requires_grad_()

    n_part = int(eng.lib.lb_graph_filter_partials(eng._h, R, C))
    chunks = n_part // (R * C)
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, C = {C}, R = {R}, {dtype}; the filter f @ weight "
           f"would be {E_cap * esize * C / 1e6:.1f} MB; d_weight's partials: {chunks} chunks, {n_part * 4 / 1e6:.2f} MB"]
    f, weight = rand(1, E_cap, R), rand(R, C, scale=R ** -0.5)
    tol = 1e-5 if dtype == "f32" else 2.0 ** -6
    verdicts = []
    med = statistics.median
    for K in (1, 3):
        x = rand(1, N, C) if K == 1 else rand(1, N, K, C)
        d = torch.randn(x.shape, device=eng.device, generator=gen).to(dt)
        for role in ("receivers", "senders"):
            def fused():
                return g.filter_conv(x, f, weight, role)

            def composed():
                return g.conv(x, torch.nn.functional.linear(f, weight.T), role)

            def fb(fn, with_f=True):
                def step():
                    x.grad = f.grad = weight.grad = None
                    f.requires_grad_(with_f)
                    fn().backward(d)
                    f.requires_grad_(True)
                return step

            r = 0 if role == "receivers" else 1
            tag = f"({role}, K = {K})"
            nb = filter_bytes(N, E, E_cap, K, R, C, esize, role == "senders", chunks)
            nb_dx = filter_bytes(N, E, E_cap, K, R, C, esize, role != "senders", chunks)["fused", "fwd"]
            for what in ("bwd3", "bwd2"):   # (a backward adds the d_x launch over the other role to its side)
                nb["fused", what] += nb_dx
            xf, df_ = x.detach().reshape(N, K, C), d.reshape(N, K, C).contiguous()
            o_x, o_f, o_w = torch.empty_like(xf), torch.empty_like(f.detach()), torch.empty_like(weight.detach())
            part = torch.empty(n_part, device=eng.device)
            p = [v.data_ptr() for v in (xf, df_, f.detach(), weight.detach())]
            conv, grad = eng.lib.lb_graph_filter_conv, eng.lib.lb_graph_filter_conv_grad

            def raw(entry, *args):
                def call():
                    rc = entry(eng._h, *args)
                    assert rc == 0, rc
                return call

            d_w_alone = raw(grad, r, p[0], p[1], p[2], p[3], None, o_w.data_ptr(), part.data_ptr(), n_part, K, R, C, code)
            if trial:   # the chunk-size trial: the fused forward + backward and the two d_weight launches, nothing else
                out += [line(f"filter_conv {tag} forward + backward (x, f, weight)", windows(fb(fused), repeats, inner), nb["fused", "bwd3"]),
                        line(f"kernels alone: k_graph_filter_dw + finish {tag}", windows(d_w_alone, repeats, inner), nb["fused", "d_w"])]
                continue
            # ---- the two sides agree before they are timed
            fb(fused)()
            got = (fused().detach(), x.grad.clone(), f.grad.clone(), weight.grad.clone())
            fb(composed)()
            want = (composed().detach(), x.grad.clone(), f.grad.clone(), weight.grad.clone())
            for a, b, what in zip(got, want, ("forward", "d_x", "d_f", "d_weight")):
                assert torch.isfinite(a).all(), (case, role, K, what)
                err = float((a.float() - b.float()).abs().max() / b.float().abs().max())
                assert err <= (1e-4 if what == "d_weight" and dtype == "f32" else tol), (case, role, K, what, err)
            fb(fused, False)()
            assert f.grad is None and torch.equal(weight.grad, got[3]) and torch.equal(x.grad, got[1])
            with torch.no_grad():
                t = {("fused", "fwd"): windows(fused, repeats, inner), ("composed", "fwd"): windows(composed, repeats, inner)}
            # forward + backward: the two sides alternate, two rounds of half the windows each, so that a change of the host's
            # pace between rounds shows as a spread on both sides and not as a difference between them
            for what, with_f in (("bwd3", True), ("bwd2", False)):
                t["fused", what], t["composed", what] = [], []
                for _ in range(2):
                    for side, fn in (("fused", fused), ("composed", composed)):
                        t[side, what] += windows(fb(fn, with_f), (repeats + 1) // 2, inner)
            # ---- the fused side's launches alone: the entries with preallocated outputs
            t["fused", "k_fwd"] = windows(raw(conv, r, p[0], p[2], p[3], o_x.data_ptr(), K, R, C, code), repeats, inner)
            t["fused", "k_dx"] = windows(raw(conv, 1 - r, p[1], p[2], p[3], o_x.data_ptr(), K, R, C, code), repeats, inner)
            t["fused", "d_f"] = windows(raw(grad, r, p[0], p[1], p[2], p[3], o_f.data_ptr(), None, None, 0, K, R, C, code), repeats, inner)
            t["fused", "d_w"] = windows(d_w_alone, repeats, inner)
            names = {"fwd": "forward", "bwd3": "forward + backward (x, f, weight)", "bwd2": "forward + backward (x, weight)"}
            for what, name in names.items():
                out += [line(f"filter_conv {tag} {name}", t["fused", what], nb["fused", what]),
                        line(f"linear, conv {tag} {name}", t["composed", what], nb["composed", what])]
            out += [line(f"kernels alone: k_graph_filter_conv {tag}", t["fused", "k_fwd"], nb["fused", "fwd"]),
                    line(f"kernels alone: k_graph_filter_conv, d_x of {tag}", t["fused", "k_dx"], nb_dx),
                    line(f"kernels alone: k_graph_filter_df {tag}", t["fused", "d_f"], nb["fused", "d_f"]),
                    line(f"kernels alone: k_graph_filter_dw + finish {tag}", t["fused", "d_w"], nb["fused", "d_w"])]
            alone = sum(med(t["fused", k]) for k in ("k_fwd", "k_dx", "d_f", "d_w"))
            parts = []
            for what, name in names.items():
                tf, tc = t["fused", what], t["composed", what]
                parts.append(f"{name}: composed / fused = {med(tc) / med(tf):.2f}x, fused slowest window {max(tf) * 1e3:.2f} us against "
                             f"composed fastest {min(tc) * 1e3:.2f} us ({'faster' if max(tf) < min(tc) else 'NOT faster'})")
            verdicts.append(f"  filter_conv {tag}: " + "; ".join(parts) + f"; its launches alone {alone * 1e3:.2f} us = "
                            f"{100 * alone / med(t['fused', 'bwd3']):.0f} % of the fused forward + backward (x, f, weight), the rest is "
                            f"the host's dispatch")
    out += verdicts
    if trial:
        return out
    out.append(f"  sender views built by the radix sort: {eng.graph_sender_sorts()}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--columns", type=int, default=128)
    ap.add_argument("--basis", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--trial", action="store_true", help="only the fused forward + backward and the d_weight launches (chunk-size trial)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_filter_bench: needs a HIP device (no CPU timing)")
    lines = [f"filter_conv, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.columns, a.basis, a.repeats, a.inner, a.dtype, a.trial)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
