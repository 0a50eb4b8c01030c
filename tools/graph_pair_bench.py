#!/usr/bin/env python
"""The fused edge messages of csrc/lb_graph.hip - conv, pair_mul, pair_add - beside the same layers written with this
library's gather / segment_sum and torch's elementwise ops: what a user writes without them.

    python tools/graph_pair_bench.py [--dtype f32|bf16] [--repeats 20] [--inner 50] [--only tgv3d] [--columns 128] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1 (synthetic cases of lagrangebench_amd.data, seeded), C = 128 columns - the
protocol of tools/graph_ops_bench.py.  Per workload and role (receivers, senders), at K = 1 (x (N, C)) and K = 3
(x (N, 3, C), w broadcast):

    fused      graph.conv(x, w, role)
    composed   graph.segment_sum(graph.gather(x, other role) * w[..., None, :], role)

forward alone, and forward plus backward through autograd (gradients to x and w, a fixed cotangent).  Then, once per
workload, pair_add(a, b) beside gather(a, "senders") + gather(b, "receivers") and pair_mul beside the product of the two
gathers, forward and forward plus backward.  Each figure is the median of `--repeats` windows of `--inner` calls between two
device events (after a warm-up of at least one window and 0.3 s), with the spread (min .. max) of the windows.

Before anything is timed the two sides are compared.  float32: forward and d_x equal bit for bit, d_w bit for bit at K = 1
(at K > 1 autograd reduces the broadcast w in an order of its own: held to 1e-5 of the largest entry).  bfloat16: conv is
not the composition (it keeps the products in float32), so the fused result is held to its own contract, the rounded
float32 conv of the widened inputs; pair_mul / pair_add equal their compositions in either dtype.

Bytes are those each side has to move, from the shapes: a node tensor read through the cache counts once (N rows), an
edge-shaped tensor counts its real slots when read and every slot when written; the composed side counts every
intermediate it writes and reads back, autograd's included.  Indices: 4 bytes per entry read.

The verdict line per role states the condition this tool was written to check: on TGV3D-8k in float32 the fused conv's
SLOWEST window is faster than the composition's FASTEST window, forward and forward plus backward.
"""
import argparse
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
OTHER = {"receivers": "senders", "senders": "receivers"}


def windows(fn, repeats, inner):
    """ms per call of fn(): `repeats` windows of `inner` calls between device events, after a warm-up of at least one window
    and WARM_S seconds (the first autograd windows of a process ran 2.5x slower for a fifth of a second)."""
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
    return (f"  {tag:64s} median {med * 1e3:8.2f} us  (min {min(ms) * 1e3:8.2f}  max {max(ms) * 1e3:8.2f})  "
            f"{nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:5.1f} % of HBM peak")


def conv_bytes(N, E, E_cap, K, row, sender):
    """(fused forward, fused forward + backward, composed forward, composed forward + backward) bytes of one conv layer."""
    walk = 4 * (N + 1 + E) + (4 * (E + N + 1) if sender else 0)          # row pointers and the other role's list (+ the view)
    node, real, slots = N * K * row, E * row, E_cap * row
    f_fwd = real + 2 * node + walk                                          # w once, x through the cache, the node rows out
    f_bwd = (real + 2 * node + walk) + (2 * node + slots + 8 * E)           # d_x: the same kernel; d_w: pair_mul
    gather = node + K * slots + 4 * E
    mul = 2 * K * slots + slots                                             # reads gathered x and w, writes the messages
    seg = K * real + node + walk
    c_fwd = gather + mul + seg
    # autograd: gather(d_out), d_gx = d_m * w, d_w = sum_k(d_m * gx) (the product written, then reduced when K > 1), the
    # ordered sum of d_gx
    reduce_k = (K * slots + slots) if K > 1 else 0
    c_bwd = gather + (2 * K * slots + slots) + (3 * K * slots + reduce_k) + seg
    return f_fwd, f_fwd + f_bwd, c_fwd, c_fwd + c_bwd


def pair_bytes(N, E, E_cap, row):
    """(fused forward, fused forward + backward, composed forward, composed forward + backward) of pair_add; pair_mul's
    backward reads the two node tensors more on either side (not told apart here)."""
    node, real, slots = N * row, E * row, E_cap * row
    f_fwd = 2 * node + slots + 8 * E
    f_bwd = 2 * (real + node + 4 * (N + 1 + E)) + 4 * (E + N + 1)
    c_fwd = 2 * (node + slots + 4 * E) + 3 * slots
    return f_fwd, f_fwd + f_bwd, c_fwd, c_fwd + f_bwd


def run(case, C, repeats, inner, dtype="f32"):
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtype]
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

    def rand(*shape):
        return torch.randn(shape, device=eng.device, generator=gen).to(dt).requires_grad_()

    row = esize * C
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, C = {C}, {dtype}; one edge-shaped row set is "
           f"{E_cap * row / 1e6:.1f} MB"]
    w = rand(1, E_cap, C)
    verdicts = []
    for K in (1, 3):
        x = rand(1, N, C) if K == 1 else rand(1, N, K, C)
        d = torch.randn(x.shape, device=eng.device, generator=gen).to(dt)
        wb = (lambda: w) if K == 1 else (lambda: w[:, :, None, :])
        for role in ("receivers", "senders"):
            other = OTHER[role]

            def fused():
                return g.conv(x, w, role)

            def composed():
                return g.segment_sum(g.gather(x, other) * wb(), role)

            def fb(fn):
                def step():
                    x.grad = w.grad = None
                    fn().backward(d)
                return step

            # ---- the two sides agree before they are timed
            fb(fused)()
            f_out, f_dx, f_dw = fused().detach(), x.grad.clone(), w.grad.clone()
            fb(composed)()
            c_out, c_dx, c_dw = composed().detach(), x.grad.clone(), w.grad.clone()
            assert torch.isfinite(f_out).all() and torch.isfinite(f_dx).all() and torch.isfinite(f_dw).all()
            if dtype == "f32":
                assert torch.equal(f_out, c_out) and torch.equal(f_dx, c_dx), (case, role, K)
                if K == 1:
                    assert torch.equal(f_dw, c_dw), (case, role, K)
                else:
                    assert (f_dw - c_dw).abs().max() <= 1e-5 * c_dw.abs().max(), (case, role, K)
            else:
                with torch.no_grad():
                    assert torch.equal(f_out, g.conv(x.float(), w.float(), role).to(dt)), (case, role, K)
            with torch.no_grad():
                t_ff, t_cf = windows(fused, repeats, inner), windows(composed, repeats, inner)
            t_fb, t_cb = windows(fb(fused), repeats, inner), windows(fb(composed), repeats, inner)
            b_ff, b_fb, b_cf, b_cb = conv_bytes(N, E, E_cap, K, row, role == "senders")
            tag = f"({role}, K = {K})"
            out += [line(f"conv {tag} forward", t_ff, b_ff), line(f"gather * w, segment_sum {tag} forward", t_cf, b_cf),
                    line(f"conv {tag} forward + backward", t_fb, b_fb),
                    line(f"gather * w, segment_sum {tag} forward + backward", t_cb, b_cb)]
            med = statistics.median
            holds = max(t_ff) < min(t_cf) and max(t_fb) < min(t_cb)
            verdicts.append(f"  conv {tag}: composed / fused = {med(t_cf) / med(t_ff):.2f}x forward, {med(t_cb) / med(t_fb):.2f}x forward + "
                            f"backward; fused slowest window {max(t_ff) * 1e3:.2f} / {max(t_fb) * 1e3:.2f} us against composed fastest "
                            f"{min(t_cf) * 1e3:.2f} / {min(t_cb) * 1e3:.2f} us: the condition {'holds' if holds else 'DOES NOT HOLD'}")
    # ---- pair_add and pair_mul beside the two gathers and torch's add / multiply
    a, b = rand(1, N, C), rand(1, N, C)
    de = torch.randn((1, E_cap, C), device=eng.device, generator=gen).to(dt)
    b_pf, b_pfb, b_cf, b_cfb = pair_bytes(N, E, E_cap, row)
    for name, op in (("pair_add", torch.add), ("pair_mul", torch.mul)):
        def fused():
            return getattr(g, name)(a, b)

        def composed():
            return op(g.gather(a, "senders"), g.gather(b, "receivers"))

        def fb(fn):
            def step():
                a.grad = b.grad = None
                fn().backward(de)
            return step

        fb(fused)()
        f_out, f_da, f_db = fused().detach(), a.grad.clone(), b.grad.clone()
        fb(composed)()
        assert torch.equal(f_out, composed().detach()), (case, name)
        if dtype == "f32":   # (bfloat16: conv's float32 products against the composition's rounded ones)
            assert torch.equal(f_da, a.grad) and torch.equal(f_db, b.grad), (case, name)
        with torch.no_grad():
            t_ff, t_cf = windows(fused, repeats, inner), windows(composed, repeats, inner)
        t_fb, t_cb = windows(fb(fused), repeats, inner), windows(fb(composed), repeats, inner)
        sym = "+" if name == "pair_add" else "*"
        out += [line(f"{name} forward", t_ff, b_pf), line(f"gather {sym} gather forward", t_cf, b_cf),
                line(f"{name} forward + backward", t_fb, b_pfb), line(f"gather {sym} gather forward + backward", t_cb, b_cfb)]
        med = statistics.median
        verdicts.append(f"  {name}: composed / fused = {med(t_cf) / med(t_ff):.2f}x forward, {med(t_cb) / med(t_fb):.2f}x forward + backward")
    out += verdicts
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
        sys.exit("graph_pair_bench: needs a HIP device (no CPU timing)")
    lines = [f"edge messages, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.columns, a.repeats, a.inner, a.dtype)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
