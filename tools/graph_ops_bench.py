#!/usr/bin/env python
"""The graph ops of csrc/lb_graph.hip beside torch's index_select / index_add_ on the same tensors.

    python tools/graph_ops_bench.py [--dtype f32|bf16] [--repeats 20] [--inner 50] [--only rpf2d] [--columns 128] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1 (synthetic cases of lagrangebench_amd.data, seeded), C = 128 columns.  Per
workload and role (receivers, senders): lb_graph_gather and lb_graph_segment_sum - the forward and the backward of
graph.Graph.gather are these two launches in this order, of graph.Graph.segment_sum the same two in the other order, so
"forward plus backward" of either op is their sum - beside torch.index_select (pad slots read row 0) and zero_ +
index_add_ over the REAL slots only, with the same indices; index_add_ is also timed alone, accumulating into a warm
buffer.  `--dtype bf16` runs every line, torch's included, on bfloat16 tensors (bytes from the 2-byte element).  One more
line per role: the fused lb_graph_attend at H = 8, D = 16 (logits (E_cap, 8), values (E_cap, 8, 16); it reads both once per
real slot and writes the node rows, m and s).  Each figure is the median of `--repeats` windows of `--inner` launches between two device events (after one
warm-up window), with the spread (min .. max) of the windows.

Bytes are those the op has to move, from the shapes: gather reads one C-row per real slot and writes every slot (pads are
zero-filled), segment_sum reads one C-row per real slot and writes one per node, plus the int32 indices either reads;
torch's index_add_ reads and writes the node rows (atomics are read-modify-write: N more rows; the zero_ in its window
is not counted).  The fraction is of the 8.0 TB/s HBM3E peak (a float4 copy measures 6.3 TB/s on this chip); the tensors
of these workloads fit the 256 MiB Infinity Cache, so a fraction above the copy rate is cache traffic, not an error.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"rpf2d": "RPF2D-3.2k", "tgv3d": "TGV3D-8k"}
HBM_PEAK = 8.0e12


def windows(fn, repeats, inner):
    """ms per call of fn(): `repeats` windows of `inner` calls between device events, after one warm-up window."""
    import torch
    for _ in range(inner):
        fn()
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
    return (f"  {tag:34s} median {med * 1e3:8.2f} us  (min {min(ms) * 1e3:8.2f}  max {max(ms) * 1e3:8.2f})  "
            f"{nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:5.1f} % of HBM peak"), med


def run(case, C, repeats, inner, dtype="f32"):
    import torch
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtype]
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    ds = make_case(case, n_trajs=1, extra_seq_length=1)
    hcase = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
                         cfg_model={"isotropic_norm": ds.isotropic_norm}, noise_std=ds.noise_std, external_force_fn=ds.force)
    pos, pt = ds[0]
    feats, _ = hcase.allocate_eval((pos[None, :, :ds.input_seq_length].astype(np.float64), pt[None]))
    eng = feats.engine
    N, E_cap = eng.N, eng.e_cap
    idx, ne = eng.nl_idx()
    E = int(ne[0])
    gen = torch.Generator(device=eng.device).manual_seed(0)
    x = torch.randn((N, C), device=eng.device, generator=gen).to(dt)
    msg = torch.randn((E_cap, C), device=eng.device, generator=gen).to(dt)
    H, D = 8, 16
    logits = torch.randn((E_cap, H), device=eng.device, generator=gen).to(dt)
    values = torch.randn((E_cap, H, D), device=eng.device, generator=gen).to(dt)
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, C = {C}, {dtype}"]
    row = esize * C
    for role, r in (("receivers", 0), ("senders", 1)):
        flat = idx[0, r].long()
        real = torch.arange(E_cap, device=eng.device) < E
        sel = torch.where(real, flat, torch.zeros_like(flat))            # index_select: pad slots read row 0
        # index_add_ over the REAL slots only (at B = 1 they are a prefix): what a torch user would write.  Sending the pad
        # slots into one spare row would serialise a fifth of the atomics on one row and measure that row, not torch.
        add, msg_real = flat[:E].contiguous(), msg[:E]
        acc = torch.zeros((N, C), device=eng.device, dtype=dt)
        b_gather = E * row + E_cap * row + 4 * (E + 2)
        b_sum = E * row + N * row + 4 * (N + 1) + (4 * (E + N + 1) if r else 0)
        # the ops agree before they are timed (the ordered sum and the atomic one differ in the last bits only)
        ours, theirs = eng.graph_segment_sum(r, msg), acc.zero_().index_add_(0, add, msg_real)
        if dtype == "f32":
            assert torch.allclose(ours, theirs, rtol=1e-4, atol=1e-4)
        else:   # (the atomic bfloat16 sum keeps 8 bits along the way: only the float32 ordered sum is held to anything)
            assert torch.equal(ours, eng.graph_segment_sum(r, msg.float()).to(dt))
        assert torch.equal(eng.graph_gather(r, x)[:E], x.index_select(0, sel)[:E])
        l1, g_ms = line(f"lb_graph_gather({role})", windows(lambda: eng.graph_gather(r, x), repeats, inner), b_gather)
        l2, s_ms = line(f"lb_graph_segment_sum({role})", windows(lambda: eng.graph_segment_sum(r, msg), repeats, inner), b_sum)
        l3, tg_ms = line(f"torch.index_select({role})", windows(lambda: x.index_select(0, sel), repeats, inner), b_gather)
        l4, ts_ms = line(f"torch zero_ + index_add_({role})",
                         windows(lambda: acc.zero_().index_add_(0, add, msg_real), repeats, inner), b_sum + N * row)
        l5, ta_ms = line(f"torch index_add_ alone({role})",
                         windows(lambda: acc.index_add_(0, add, msg_real), repeats, inner), b_sum + N * row)
        b_att = E * esize * H * (D + 1) + N * esize * H * D + 8 * N * H + 4 * (N + 1) + (4 * (E + N + 1) if r else 0)
        l6, _ = line(f"lb_graph_attend({role}, {H}x{D})", windows(lambda: eng.graph_attend(r, logits, values), repeats, inner), b_att)
        out += [l1, l2, l3, l4, l5, l6,
                f"  forward + backward of gather or segment_sum over {role}: ours {1e3 * (g_ms + s_ms):.2f} us, torch "
                f"{1e3 * (tg_ms + ts_ms):.2f} us (ordered sum / atomic sum = {s_ms / ts_ms:.2f}x, gather / index_select = "
                f"{g_ms / tg_ms:.2f}x)"]
    out.append(f"  sender views built by the radix sort: {eng.graph_sender_sorts()}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--columns", type=int, default=128)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_ops_bench: needs a HIP device (no CPU timing)")
    lines = [f"graph ops, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} launches (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.columns, a.repeats, a.inner, a.dtype)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
