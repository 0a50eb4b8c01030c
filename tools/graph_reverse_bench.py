#!/usr/bin/env python
"""The edge-pair ops of csrc/lb_graph.hip - the reverse map, swap, symmetrize, antisymmetrize - beside the same thing written in
torch on the same commit: what a user writes without them.

    python tools/graph_reverse_bench.py [--dtype f32|bf16] [--repeats 20] [--inner 50] [--only tgv3d] [--columns 128] [--out FILE]

Workloads: RPF2D-3.2k and TGV3D-8k, B = 1 (synthetic cases of lagrangebench_amd.data, seeded), C = 128 columns - the protocol
and the window statistics of tools/graph_pair_bench.py: each figure is the median of `--repeats` windows of `--inner` calls
between two device events (after a warm-up of at least one window and 0.3 s), with the spread (min .. max) of the windows.

The map.  The engine builds it once per list build, at its first use, so it is timed with the list build in front of it:

    list build + first graph op     eng.nl_update(); eng.graph_degree(0)      (the read-back every first graph op of a build makes)
    ... + the map                   eng.nl_update(); eng.graph_degree(0); eng.graph_reverse()
    ... + the map in torch          eng.nl_update(); eng.graph_degree(0); a searchsorted over receiver * (N + 1) + sender keys of nl_idx()

and the map's cost is the difference of the medians to the first line.  The two maps are compared integer for integer first.

The ops, forward and forward plus backward through autograd (a fixed cotangent):

    fused      graph.swap / symmetrize / antisymmetrize (msg)
    composed   torch.where(rev >= 0, msg +- take_along_dim(msg, rev.clamp(min=0)), 0)        (swap: the taken rows alone)

float32: forward and gradient are compared bit for bit before anything is timed; bfloat16: the forward.

Bytes are those each side has to move, from the shapes.  Fused: the real rows of msg streamed (not for swap), one scattered
row read per real slot (the partner's: 512 bytes at C = 128 in float32), every slot written, 12 bytes of indices per slot; the
backward is the same launch.  Composed: every edge-shaped tensor each torch kernel reads or writes, autograd's included (an
estimate: take_along_dim 2 row sets, the add 3, where 2; backward about 10) plus its index tensors.
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
MODES = ("swap", "symmetrize", "antisymmetrize")


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


def line(tag, ms, nbytes=None):
    med = statistics.median(ms)
    text = f"  {tag:64s} median {med * 1e3:8.2f} us  (min {min(ms) * 1e3:8.2f}  max {max(ms) * 1e3:8.2f})"
    if nbytes is not None:
        text += (f"  {nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = "
                 f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:5.1f} % of HBM peak")
    return text


def torch_reverse(idx, N):
    """idx (B, 2, E_cap) of nl_idx() (receivers, senders, local to the trajectory; pad slots hold N) -> (B, E_cap) int32: per
    trajectory a searchsorted of the transposed key sender * (N + 1) + receiver in the row's own ascending keys receiver *
    (N + 1) + sender (the pads' key is the largest)."""
    import torch
    r, s = idx[:, 0].to(torch.int64), idx[:, 1].to(torch.int64)
    keys, query = r * (N + 1) + s, s * (N + 1) + r
    pos = torch.searchsorted(keys, query).clamp(max=keys.shape[1] - 1)
    found = (torch.take_along_dim(keys, pos, 1) == query) & (r < N)
    return torch.where(found, pos, torch.full_like(pos, -1)).to(torch.int32)


def torch_edge_pair(mode, msg, rev):
    import torch
    other = torch.take_along_dim(msg, rev.clamp(min=0).to(torch.int64)[..., None], 1)
    val = other if mode == "swap" else (msg + other if mode == "symmetrize" else msg - other)
    return torch.where((rev >= 0)[..., None], val, torch.zeros((), dtype=msg.dtype, device=msg.device))


def op_bytes(mode, E, E_cap, row):
    """(fused forward, fused forward + backward, composed forward, composed forward + backward)"""
    real, slots = E * row, E_cap * row
    fused = (real if mode == "swap" else 2 * real) + slots + 12 * E_cap
    c_fwd = (4 if mode == "swap" else 7) * slots + (8 + 12 + 8 + 5 + 1) * E_cap
    c_bwd = 10 * slots + (8 + 1) * E_cap
    return fused, 2 * fused, c_fwd, c_fwd + c_bwd


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
    idx, ne = eng.nl_idx()
    E = int(ne[0])
    rev = g.reverse
    row = esize * C
    med = statistics.median
    out = [f"{WORKLOADS[case]}: N = {N}, E = {E} real slots of E_cap = {E_cap}, C = {C}, {dtype}; one edge-shaped row set is "
           f"{E_cap * row / 1e6:.1f} MB; slots without a transpose: {int((rev[0, :E] < 0).sum())}"]
    gen = torch.Generator(device=eng.device).manual_seed(0)
    msg = torch.randn((1, E_cap, C), device=eng.device, generator=gen).to(dt).requires_grad_()
    de = torch.randn((1, E_cap, C), device=eng.device, generator=gen).to(dt)
    verdicts = []
    # ---- the ops (before the map: its timing builds new lists, which leaves `g` stale)
    for mode in MODES:
        def fused():
            return getattr(g, mode)(msg)

        def composed():
            return torch_edge_pair(mode, msg, rev)

        def fb(fn):
            def step():
                msg.grad = None
                fn().backward(de)
            return step

        fb(fused)()
        f_out, f_d = fused().detach(), msg.grad.clone()
        fb(composed)()
        c_out, c_d = composed().detach(), msg.grad.clone()
        assert torch.isfinite(f_out).all() and torch.isfinite(f_d).all()
        assert torch.equal(f_out, c_out), (case, mode)
        if dtype == "f32":
            assert torch.equal(f_d, c_d), (case, mode)
        with torch.no_grad():
            t_ff, t_cf = windows(fused, repeats, inner), windows(composed, repeats, inner)
        t_fb, t_cb = windows(fb(fused), repeats, inner), windows(fb(composed), repeats, inner)
        b_ff, b_fb, b_cf, b_cb = op_bytes(mode, E, E_cap, row)
        out += [line(f"{mode} forward", t_ff, b_ff), line(f"torch composition of {mode} forward", t_cf, b_cf),
                line(f"{mode} forward + backward", t_fb, b_fb), line(f"torch composition of {mode} forward + backward", t_cb, b_cb)]
        verdicts.append(f"  {mode}: composed / fused = {med(t_cf) / med(t_ff):.2f}x forward, {med(t_cb) / med(t_fb):.2f}x forward + "
                        f"backward")
    # ---- the map, behind a list build
    assert torch.equal(torch_reverse(idx, N), rev), case

    def build():
        eng.nl_update()
        eng.graph_degree(0)

    def build_map():
        build()
        return eng.graph_reverse()

    def build_torch_map():
        build()
        return torch_reverse(eng.nl_idx()[0], N)

    inner_map = max(inner // 5, 5)
    t_b, t_m, t_t = windows(build, repeats, inner_map), windows(build_map, repeats, inner_map), windows(build_torch_map, repeats, inner_map)
    assert torch.equal(build_map().reshape(1, E_cap), build_torch_map())
    out += [line("list build + first graph op", t_b), line("list build + first graph op + the reverse map", t_m),
            line("list build + first graph op + the map in torch (searchsorted)", t_t)]
    verdicts.append(f"  the map: {1e3 * (med(t_m) - med(t_b)):.2f} us over the list build, the torch map {1e3 * (med(t_t) - med(t_b)):.2f} us "
                    f"(differences of medians; the kernel writes {4 * E_cap / 1e3:.0f} kB)")
    out += verdicts
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
        sys.exit("graph_reverse_bench: needs a HIP device (no CPU timing)")
    lines = [f"edge pairs, {torch.cuda.get_device_name(0)}; median of {a.repeats} windows of {a.inner} calls (device events; the map: "
             f"{max(a.inner // 5, 5)} calls)"]
    for case in ([a.only] if a.only else list(WORKLOADS)):
        lines += run(case, a.columns, a.repeats, a.inner, a.dtype)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
