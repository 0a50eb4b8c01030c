#!/usr/bin/env python
"""The multi-aggregator of csrc/lb_graph.hip - graph.aggregate: sum, mean, max, min, std of one message from one launch -
beside the same layer written with this library's own separate ops: what a user writes without it.

    python tools/graph_aggregate_bench.py [--dtype f32|bf16] [--repeats 20] [--inner 50] [--only tgv3d] [--columns 32,128] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1 (synthetic cases of lagrangebench_amd.data, seeded), C = 32 and 128 columns - the
protocol of tools/graph_vec_bench.py.  Per workload, C, role (receivers, senders) and op set:

    pna5        fused      graph.aggregate(msg, role, ("sum", "mean", "max", "min", "std"))
                composed   torch.stack([segment_sum, m = segment_mean, segment_max, segment_min,
                                        sqrt((segment_mean(msg * msg) - m * m).clamp(min=0) + eps)], 2)
                separate   the same five results without the stack (forward only)
    mean_std    fused      graph.aggregate(msg, role, ("mean", "std"))
                composed   torch.stack([m, sqrt(...)], 2) as above

forward alone, and forward plus backward through autograd (the gradient to msg, a fixed cotangent).  Each figure is the median
of `--repeats` windows of `--inner` calls between two device events (after a warm-up of at least one window and 0.3 s), with
the spread (min .. max) of the windows.  The two launches of the fused op - k_graph_aggregate and k_graph_aggregate_bwd - are
also timed alone, through the library entry with preallocated outputs (a ctypes call per launch, so the device queue stays
full): the "kernels alone" lines.  Their sum over the fused forward-plus-backward time is the device's share of that figure;
the rest is the host's autograd dispatch.

Before anything is timed the two sides are compared.  float32: the sum / mean / max / min planes equal the separate ops bit for
bit; std is held to 1e-3 of its largest entry (the composition's one-pass variance is the less accurate side).  bfloat16: the
fused result is held to its own contract, the rounded float32 op of the widened inputs.

Bytes are those each side has to move, from the shapes: the message counts its real slots once per launch that reads it (the
fused second walk re-reads lines it just read: not counted again), a node-shaped tensor counts N rows, an edge-shaped tensor
written counts every slot; the composed side counts every intermediate it writes and reads back, autograd's included, at one
read and one write per elementwise op.  Indices: 4 bytes per entry read.

The verdict line states the one condition set for this op: on TGV3D-8k at C = 128 the fused five-op forward median is below
the median of the five separate forwards together.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"rpf2d": "RPF2D-3.2k", "tgv3d": "TGV3D-8k"}
HBM_PEAK = 8.0e12
WARM_S = 0.3
ROLE_CODE = {"receivers": 0, "senders": 1}
SETS = {"pna5": ("sum", "mean", "max", "min", "std"), "mean_std": ("mean", "std")}
CODES = {"sum": 1, "mean": 2, "max": 3, "min": 4, "std": 5, "var": 6}
EPS = 1e-5


def windows(fn, repeats, inner):
    """ms per call of fn(): `repeats` windows of `inner` calls between device events, after a warm-up of at least one window
    and WARM_S seconds."""
    import torch
    t0, n = time.perf_counter(), 0
    while n < inner or time.perf_counter() - t0 < WARM_S:
        fn()
        n += 1
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def line(tag, ms, nbytes):
    med = statistics.median(ms)
    return (f"  {tag:72s} median {med * 1e3:8.2f} us  (min {min(ms) * 1e3:8.2f}  max {max(ms) * 1e3:8.2f})  "
            f"{nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:5.1f} % of HBM peak")


def agg_bytes(N, E, E_cap, C, esize, ops, sender):
    """{"fwd", "bwd": the two fused launches; "c_f", "c_fb": the composition forward and forward plus backward}."""
    row = esize * C
    walk = 4 * (N + 1) + (4 * (E + N + 1) if sender else 0)              # row pointers (+ the sender view)
    node, real, slots = N * row, E * row, E_cap * row
    side = N * 2 * 4 * C                                                  # win, or stats: (N, 2, C) of 4 bytes
    A = len(ops)
    ext, mom = ("max" in ops or "min" in ops), ("std" in ops or "var" in ops)
    b = {"fwd": real + A * node + walk + (side if ext else 0) + (side if mom else 0),
         "bwd": A * node + (real + side if mom else 0) + (side if ext else 0) + slots + 4 * E + 4 * (N + 1) + (walk if sender else 0)}
    seg = real + node + walk                                              # one separate segment reduction
    mean = seg + 3 * node + 4 * N                                         # ... then degree, clamp and the division
    f = 0
    if "sum" in ops:
        f += seg
    f += mean                                                             # m: a plane of its own and the mean inside std
    for op in ("max", "min"):
        if op in ops:
            f += seg + N * 4 * C                                          # its win
    f += (real + slots) + mean + 4 * 2 * node                             # msg * msg, its mean, four elementwise steps to std
    f += 2 * A * node                                                     # the stack
    b["c_f"] = f
    g = A * node + slots * (A + 2)                                        # unstack; one edge-shaped gradient per reduction ...
    g += 2 * (A - 1) * slots * 3 // 2                                     # ... which autograd adds pairwise (two reads, one write)
    g += 3 * slots + 8 * node                                             # d(msg * msg) = 2 msg d; the elementwise steps back
    b["c_fb"] = f + g
    return b


def run(case, C, repeats, inner, dtype="f32"):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    dt, esize, code = {"f32": (torch.float32, 4, 0), "bf16": (torch.bfloat16, 2, 1)}[dtype]
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
    msg = torch.randn((1, E_cap, C), device=eng.device, generator=gen).to(dt).requires_grad_()
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, C = {C}, {dtype}; the (E_cap, C) message is "
           f"{E_cap * esize * C / 1e6:.1f} MB"]
    med = statistics.median
    verdicts = []
    for role in ("receivers", "senders"):
        def std_of(m):
            return torch.sqrt((g.segment_mean(msg * msg, role) - m * m).clamp(min=0) + EPS)

        def separate():
            m = g.segment_mean(msg, role)
            return [g.segment_sum(msg, role), m, g.segment_max(msg, role), g.segment_min(msg, role), std_of(m)]

        def mean_std():
            m = g.segment_mean(msg, role)
            return [m, std_of(m)]

        for name, ops in SETS.items():
            nb = agg_bytes(N, E, E_cap, C, esize, ops, role == "senders")
            parts = separate if name == "pna5" else mean_std
            fused = lambda: g.aggregate(msg, role, ops, EPS)                         # noqa: E731
            composed = lambda: torch.stack(parts(), 2)                              # noqa: E731
            d = torch.randn((1, N, len(ops), C), device=eng.device, generator=gen).to(dt)

            def fb(fn):
                def step():
                    msg.grad = None
                    fn().backward(d)
                return step

            # ---- the two sides agree before they are timed
            fb(fused)()
            f, f_grad = fused().detach(), msg.grad.clone()
            fb(composed)()
            c, c_grad = composed().detach(), msg.grad.clone()
            assert torch.isfinite(f).all() and torch.isfinite(f_grad).all(), (case, role, name)
            if dtype == "f32":
                exact = [a for a, op in enumerate(ops) if op != "std"]
                assert torch.equal(f[:, :, exact], c[:, :, exact]), (case, role, name)
                assert (f - c).abs().max() <= 1e-3 * c.abs().max() and (f_grad - c_grad).abs().max() <= 1e-3 * c_grad.abs().max()
            else:
                with torch.no_grad():
                    wide = g.aggregate(msg.float(), role, ops, EPS).to(dt)
                assert torch.equal(f, wide), (case, role, name)
            # ---- the two launches alone
            word = sum(CODES[op] << (4 * a) for a, op in enumerate(ops))
            flat = msg.detach().reshape(E_cap, C)
            o_out, o_d = torch.empty((N, len(ops), C), dtype=dt, device=eng.device), torch.empty_like(flat)
            o_win = torch.empty((N, 2, C), dtype=torch.int32, device=eng.device)
            o_st = torch.empty((N, 2, C), dtype=torch.float32, device=eng.device)
            d_flat = d.reshape(N, len(ops), C).contiguous()
            r = ROLE_CODE[role]

            def k_fwd():
                if eng.lib.lb_graph_aggregate(eng._h, r, flat.data_ptr(), o_out.data_ptr(), o_win.data_ptr(), o_st.data_ptr(), C, word,
                                              ctypes.c_float(EPS), code) != 0:
                    raise RuntimeError("lb_graph_aggregate")

            def k_bwd():
                if eng.lib.lb_graph_aggregate_backward(eng._h, r, d_flat.data_ptr(), flat.data_ptr(), o_win.data_ptr(), o_st.data_ptr(),
                                                       o_d.data_ptr(), C, word, code) != 0:
                    raise RuntimeError("lb_graph_aggregate_backward")

            t_kf, t_kb = windows(k_fwd, repeats, inner), windows(k_bwd, repeats, inner)
            with torch.no_grad():
                t_ff, t_cf = windows(fused, repeats, inner), windows(composed, repeats, inner)
                t_sf = windows(parts, repeats, inner)
            t_fb, t_cb = windows(fb(fused), repeats, inner), windows(fb(composed), repeats, inner)
            tag = f"{name} ({role})"
            out += [line(f"kernels alone: k_graph_aggregate, {tag}", t_kf, nb["fwd"]),
                    line(f"kernels alone: k_graph_aggregate_bwd, {tag}", t_kb, nb["bwd"]),
                    line(f"aggregate {tag} forward", t_ff, nb["fwd"]),
                    line(f"separate ops of {tag} forward, not stacked", t_sf, nb["c_f"] - 2 * len(ops) * N * esize * C),
                    line(f"composition of {tag} forward", t_cf, nb["c_f"]),
                    line(f"aggregate {tag} forward + backward", t_fb, nb["fwd"] + nb["bwd"]),
                    line(f"composition of {tag} forward + backward", t_cb, nb["c_fb"])]
            dev = med(t_kf) + med(t_kb)
            text = (f"  {tag} C = {C}: separate / fused = {med(t_sf) / med(t_ff):.2f}x forward (stacked: {med(t_cf) / med(t_ff):.2f}x), "
                    f"{med(t_cb) / med(t_fb):.2f}x forward + backward; the two kernels alone {dev * 1e3:.2f} us = "
                    f"{100 * dev / med(t_fb):.0f} % of the fused forward + backward, host dispatch the other "
                    f"{max(0.0, 100 - 100 * dev / med(t_fb)):.0f} %")
            if case == "tgv3d" and C == 128 and name == "pna5":
                holds = med(t_ff) < med(t_sf)
                text += (f"; THE CONDITION (fused five-op forward median {med(t_ff) * 1e3:.2f} us below the five separate forwards' "
                         f"{med(t_sf) * 1e3:.2f} us) {'holds' if holds else 'DOES NOT HOLD'}")
            verdicts.append(text)
    out += verdicts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--columns", default="32,128")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_aggregate_bench: needs a HIP device (no CPU timing)")
    lines = [f"multi-aggregator, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        for C in [int(c) for c in a.columns.split(",")]:
            lines += run(case, C, a.repeats, a.inner, a.dtype)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
