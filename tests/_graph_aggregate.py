"""Restatements of graph.Graph.aggregate for the tests: the numpy float32 twin of the forward and of the backward, which states
every rounding of the contract (lagrangebench_amd/graph.py, "Multi-aggregator") as a loop over the real slots in ascending
order; three mutated twins that break one rule each; the same op in differentiable float64 torch on the padded list
(`CpuAggGraph`); the planted rows; and `TinyPNA`, a small PNA network for ``models.TorchModel``.

Everything works on an exported padded list as tests/_graph_attention.py does: `idx` (B, E_cap), the role index of every slot
(pad slots hold N), and `ne` (B,).  Pad slots are never read.
"""
import numpy as np
import torch
from torch import nn

from tests._graph_attention import CpuAttnGraph, node_slots, np_degree, rank_steps
from tests._torch_models import NODE_KEYS

OPS = ("sum", "mean", "max", "min", "std", "var")
MUTANTS = ("one_pass", "late_ties", "eps_outside")
F = np.float32


def same_bits(a, b):
    """Equal bit for bit, or a NaN in both (the payload of a NaN that an op produced or passed on is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def np_aggregate(msg, idx, ne, N, ops=OPS, eps=1e-5, mutant=None):
    """msg (B, E_cap, C) float32 -> (out (B, N, A, C) float32, win (B, N, 2, C) int32: max then min, stats (B, N, 2, C) float32:
    mean then std).  Every operation is one float32 operation of numpy - correctly rounded, as the kernel's.  `mutant` breaks
    one rule: "one_pass" var = E[x^2] - m^2; "late_ties" an equal value replaces the winner; "eps_outside" std = sqrt(var) + eps."""
    assert mutant in (None,) + MUTANTS
    msg = np.asarray(msg, F)
    B, _, C = msg.shape
    s, q = np.zeros((B, N, C), F), np.zeros((B, N, C), F)
    ext = [np.zeros((B, N, C), F), np.zeros((B, N, C), F)]
    win = np.full((B, N, 2, C), -1, np.int32)
    steps = rank_steps(idx, ne, N)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, st in enumerate(steps):
            for n, (nodes, slots) in enumerate(st):
                a, j = msg[b, slots], slots[:, None].astype(np.int32)
                if n == 0:                                   # every reduction STARTS from the first slot
                    s[b, nodes], ext[0][b, nodes], ext[1][b, nodes] = a, a, a
                    win[b, nodes, 0], win[b, nodes, 1] = j, j
                    continue
                s[b, nodes] = s[b, nodes] + a
                for k in (0, 1):
                    v = ext[k][b, nodes]
                    beats = ((a < v) if k else (a > v)) | (np.isnan(a) & ~np.isnan(v))
                    if mutant == "late_ties":
                        beats |= a == v
                    ext[k][b, nodes] = np.where(beats, a, v)
                    win[b, nodes, k] = np.where(beats, j, win[b, nodes, k])
        deg = np_degree(idx, ne, N)
        dd = np.maximum(deg, 1).astype(F)[..., None]
        m = s / dd
        for b, st in enumerate(steps):                       # the second walk: centred squares
            for n, (nodes, slots) in enumerate(st):
                a = msg[b, slots]
                t = a if mutant == "one_pass" else a - m[b, nodes]
                q[b, nodes] = t * t if n == 0 else q[b, nodes] + t * t
        var = q / dd
        if mutant == "one_pass":
            var = var - m * m
        std = np.sqrt(var) + F(eps) if mutant == "eps_outside" else np.sqrt(var + F(eps))
        std = np.where(deg[..., None] > 0, std, F(0))        # a node without slots: +0.0, not sqrt(eps)
    planes = {"sum": s, "mean": m, "max": ext[0], "min": ext[1], "std": std, "var": var}
    assert all(p.dtype == F for p in planes.values())
    return np.stack([planes[o] for o in ops], 2), win, np.stack([m, std], 2)


def np_aggregate_backward(d_out, msg, win, stats, idx, ne, ops=OPS):
    """d_msg (B, E_cap, C) float32: per real slot the present terms in the contract's fixed order, the first present one
    starting the sum; +0.0 where no term is present and in the pad slots."""
    d_out, msg = np.asarray(d_out, F), np.asarray(msg, F)
    B, N, _, C = d_out.shape
    d = np.zeros((B, msg.shape[1], C), F)
    deg = np_degree(idx, ne, N)
    pos = {o: a for a, o in enumerate(ops)}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            n = int(ne[b])
            i, j = idx[b, :n], np.arange(n)[:, None]
            dd = np.maximum(deg[b, i], 1).astype(F)[:, None]
            acc, seen = np.zeros((n, C), F), np.zeros((n, C), bool)

            def add(term, mask=True):
                nonlocal acc, seen
                mask = np.broadcast_to(mask, acc.shape)
                acc = np.where(mask, np.where(seen, acc + term, term), acc)
                seen = seen | mask

            if "sum" in pos:
                add(d_out[b, i, pos["sum"]])
            if "mean" in pos:
                add(d_out[b, i, pos["mean"]] / dd)
            if "max" in pos:
                add(d_out[b, i, pos["max"]], win[b, i, 0] == j)
            if "min" in pos:
                add(d_out[b, i, pos["min"]], win[b, i, 1] == j)
            t = msg[b, :n] - stats[b, i, 0]
            if "std" in pos:
                add((d_out[b, i, pos["std"]] * t) / (dd * stats[b, i, 1]))
            if "var" in pos:
                add(((F(2) * d_out[b, i, pos["var"]]) * t) / dd)
            assert acc.dtype == F
            d[b, :n] = acc
    return d


class CpuAggGraph(CpuAttnGraph):
    """CpuAttnGraph plus aggregate / segment_std / segment_var in differentiable torch (any float dtype; float64 is the
    yardstick).  Ties share the gradient here, so it stands in for the device op only where no two slots of a node are equal."""

    def aggregate(self, msg, role, ops=("sum", "mean", "max", "min", "std"), eps=1e-5):
        shape = msg.shape
        x = torch.where(self.real[..., None], msg.reshape(self.B, self.E, -1), torch.zeros((), dtype=msg.dtype))
        deg = self.degree(role)
        dd = deg.clamp(min=1).to(msg.dtype)[..., None]
        planes = {"sum": self.segment_sum(x, role)}
        planes["mean"] = planes["sum"] / dd
        for op in ("max", "min"):
            if op in ops:
                planes[op] = self._extreme(x, role, "a" + op)
        if "std" in ops or "var" in ops:
            t = torch.where(self.real[..., None], x - self.gather(planes["mean"], role), torch.zeros((), dtype=msg.dtype))
            planes["var"] = self.segment_sum(t * t, role) / dd
            planes["std"] = torch.sqrt(planes["var"] + eps) * (deg > 0).to(msg.dtype)[..., None]
        return torch.stack([planes[o] for o in ops], 2).reshape((self.B, self.N, len(ops)) + tuple(shape[2:]))

    def segment_std(self, msg, role, eps=1e-5):
        return self.aggregate(msg, role, ("std",), eps)[:, :, 0]

    def segment_var(self, msg, role):
        return self.aggregate(msg, role, ("var",))[:, :, 0]


# ------------------------------------------------------------------------------------------------ the planted rows
# name: the least degree of a node that can hold it.  "tie": the first two slots tie at the top (even columns) and at the bottom
# (odd columns); "zeros": -0.0, +0.0, then -1 (even columns: the maximum stays -0.0) or +1 (odd: the minimum does); "equal":
# every slot 1.5 - sums and mean exact, var exactly 0, std = sqrt_rn(eps), the std gradient term exactly 0; "big": 4096 + j / 4,
# exact in float32, whose squares are not (ulp 2): the one-pass variance is garbage; "nan": one real slot is NaN; "deg1": a node
# with a single slot, left as it is.  NaN goes into every pad slot.
PLANTS = (("tie", 2), ("zeros", 2), ("equal", 2), ("big", 2), ("nan", 1), ("deg1", 1))


def plant_rows(msg, idx, ne, N):
    """Write the planted rows into the real slots of chosen nodes of msg (B, E_cap, C), in place, NaN into every pad slot, and
    return {name: (b, node, its slots)} for the rows that found a node: the nodes by falling degree, each used once; "nan"
    prefers a node with two slots, "deg1" takes one with exactly one."""
    rows = [(len(s), b, i, s) for b, row in enumerate(node_slots(idx, ne, N)) for i, s in enumerate(row) if len(s)]
    rows.sort(key=lambda r: (-r[0], r[1], r[2]))
    used, placed = set(), {}

    def take(ok):
        for d, b, i, s in rows:
            if (b, i) not in used and ok(d):
                used.add((b, i))
                return b, i, s
        return None

    for name, least in PLANTS:
        got = take(lambda d: d == 1) if name == "deg1" else None
        if name == "nan":
            got = take(lambda d: d >= 2)
        if got is None and name != "deg1":
            got = take(lambda d: d >= least)
        if got is None:
            continue
        b, i, s = got
        placed[name] = got
        if name == "tie":
            msg[b, s[:2], 0::2], msg[b, s[:2], 1::2] = 64.0, -64.0
        elif name == "zeros":
            msg[b, s, 0::2], msg[b, s, 1::2] = -1.0, 1.0
            msg[b, s[0]], msg[b, s[1]] = -0.0, 0.0
        elif name == "equal":
            msg[b, s] = 1.5
        elif name == "big":
            msg[b, s] = (4096.0 + 0.25 * (1 + np.arange(len(s), dtype=F)))[:, None]
        elif name == "nan":
            msg[b, s[len(s) // 2]] = np.nan
    for b in range(msg.shape[0]):
        msg[b, ne[b]:] = np.nan
    return placed


class TinyPNA(nn.Module):
    """TinyMP's encoder and decoder (tests/_torch_models.py) around one PNA layer: the edge message aggregated over receivers
    by sum, mean, max, min and std in one `aggregate`, flattened and scaled by the degree scalers of PNA (identity,
    amplification, attenuation) computed in torch from `graph.degree`."""

    OPS = ("sum", "mean", "max", "min", "std")

    def __init__(self, node_in: int, dim: int, hidden: int = 32):
        super().__init__()
        self.enc = nn.Linear(node_in, hidden)
        self.edge = nn.Linear(2 * hidden + dim + 1, hidden)
        self.node = nn.Sequential(nn.Linear(hidden + 3 * len(self.OPS) * hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.dec = nn.Linear(hidden, dim)
        self.register_buffer("in_scale", torch.ones(node_in))

    def forward(self, features, particle_type, graph):
        dt = self.enc.weight.dtype
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        h = nn.functional.silu(self.enc(x * self.in_scale))
        hs, hr = graph.gather(h, "senders"), graph.gather(h, "receivers")
        e = nn.functional.silu(self.edge(torch.cat([hs, hr, features["rel_disp"].to(dt), features["rel_dist"].to(dt)], -1)))
        agg = graph.aggregate(e, "receivers", self.OPS).flatten(-2)
        s = torch.log(graph.degree("receivers").to(agg.dtype) + 1.0)[..., None] / 2.5
        agg = torch.cat([agg, agg * s, agg / s.clamp(min=0.25)], -1)
        return self.dec(h + self.node(torch.cat([h.to(agg.dtype), agg], -1)))
