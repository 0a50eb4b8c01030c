"""Restatements of graph.Graph's ``filter_conv`` for the tests: numpy loops that state its order contracts bit for bit - the
r-loop of the filter, ``conv``'s sum over the slots, the blocked ``d_f`` and the chunked ``d_weight`` -, the op in differentiable
torch on the CPU (`CpuFilterGraph`, any dtype), and `TinyFilter`, a small SchNet-style network for ``models.TorchModel``.

Everything works on an exported padded list: per role `idx` (B, E_cap) int, the role's node of every slot (pad slots hold
N), and `ne` (B,), the real slots of every trajectory.  Pad slots are never read.  The numpy twins compute in the dtype of
their first argument: float32 states the device's bits, float64 the adjoint identities.
"""
import math
import os
import re

import numpy as np
import torch
from torch import nn

from tests._graph_attention import rank_steps
from tests._graph_vec import OTHER, CpuVecGraph, du_block  # noqa: F401  (OTHER is re-exported)
from tests._torch_models import NODE_KEYS

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lbhip.h")


def header_constant(name: str) -> int:
    with open(_HEADER) as f:
        return int(re.search(r"^#define\s+%s\s+(\d+)" % name, f.read(), flags=re.M).group(1))


def filter_chunk() -> int:
    """LB_GRAPH_FILTER_CHUNK of include/lbhip.h: the slots of one partial sum of d_weight - the one place the twins read it
    from."""
    return header_constant("LB_GRAPH_FILTER_CHUNK")


def np_filter(f, weight):
    """f (n, R), weight (R, C) -> wf (n, C): f[:, 0] * weight[0], then one add per further r of the rounded product."""
    wf = (f[:, 0:1] * weight[0]).astype(f.dtype)
    for r in range(1, f.shape[1]):
        wf = wf + (f[:, r:r + 1] * weight[r]).astype(f.dtype)
    return wf


def np_filter_conv(x, f, weight, idx_role, idx_other, ne, N):
    """x (B, N, K, C), f (B, E_cap, R), weight (R, C) -> (B, N, K, C).  Per node the real slots j whose `idx_role` is the node,
    ascending; the term of a slot is x[idx_other[j]] * wf[j] with wf of np_filter, rounded to the dtype; the first term starts
    the sum, every further one is one add.  An empty row is +0.0."""
    out = np.zeros(x.shape, x.dtype)
    for b, steps in enumerate(rank_steps(idx_role, ne, N)):
        for n, (nodes, slots) in enumerate(steps):
            term = (x[b, idx_other[b, slots]] * np_filter(f[b, slots], weight)[:, None, :]).astype(x.dtype)
            out[b, nodes] = term if n == 0 else out[b, nodes] + term
    return out


def np_filter_g(x, d, idx_role, idx_other, b, n):
    """g (n, C) of trajectory b's n real slots: x[other, 0] * d[role, 0], then one add per further k of the rounded product."""
    xo, dn = x[b, idx_other[b, :n]], d[b, idx_role[b, :n]]
    g = (xo[:, 0] * dn[:, 0]).astype(x.dtype)
    for k in range(1, x.shape[2]):
        g = g + (xo[:, k] * dn[:, k]).astype(x.dtype)
    return g


def np_filter_edge_grad(x, d, f, weight, idx_role, idx_other, ne, e_cap, block=None, chunk=None, from_first=False):
    """x, d (B, N, K, C) - x read at idx_other, the cotangent d at idx_role -, f (B, E_cap, R), weight (R, C) -> (d_f (B, E_cap,
    R), d_weight (R, C)) with g of np_filter_g:
      d_f[j, r] = the sum over c of weight[r, c] * g[j, c]: consecutive blocks of `block` columns (the last may be short), c
                  ascending inside a block from its first product, the block sums added in ascending order from the first;
                  +0.0 in the pad slots;
      d_weight[r, c] = the sum over the real slots of f[j, r] * g[j, c]: the flat padded slots b * e_cap + j in consecutive
                  chunks of `chunk`; a chunk's partial starts at +0.0 and takes its real slots' terms in ascending order; the
                  total starts at +0.0 and takes the partials in ascending chunk order.
    `from_first` is NOT the contract: both levels start from their first term instead of +0.0 (a neighbouring order the tests
    tell apart)."""
    block = du_block() if block is None else block
    chunk = filter_chunk() if chunk is None else chunk
    B, _, _, C = x.shape
    R = f.shape[2]
    dt = x.dtype
    d_f = np.zeros((B, e_cap, R), dt)
    g_all = np.zeros((B * e_cap, C), dt)
    real = np.zeros(B * e_cap, bool)
    for b in range(B):
        n = int(ne[b])
        g = np_filter_g(x, d, idx_role, idx_other, b, n)
        g_all[b * e_cap:b * e_cap + n], real[b * e_cap:b * e_cap + n] = g, True
        prod = (weight[None, :, :] * g[:, None, :]).astype(dt)                       # (n, R, C)
        total = None
        for c0 in range(0, C, block):
            part = prod[:, :, c0]
            for c in range(c0 + 1, min(c0 + block, C)):
                part = part + prod[:, :, c]
            total = part if total is None else total + part
        d_f[b, :n] = total
    # every chunk's loop at once, one position of the chunk at a time
    n_chunks = -(-B * e_cap // chunk)
    pad = n_chunks * chunk - B * e_cap
    ff = np.concatenate([f.reshape(B * e_cap, R), np.zeros((pad, R), dt)]).reshape(n_chunks, chunk, R)
    gg = np.concatenate([g_all, np.zeros((pad, C), dt)]).reshape(n_chunks, chunk, C)
    rr = np.concatenate([real, np.zeros(pad, bool)]).reshape(n_chunks, chunk)
    partial = np.zeros((n_chunks, R, C), dt)
    started = np.zeros(n_chunks, bool)
    with np.errstate(invalid="ignore"):
        for p in range(chunk):
            term = (ff[:, p, :, None] * gg[:, p, None, :]).astype(dt)                 # (chunks, R, C); NaN where f is a pad's
            take = rr[:, p]
            new = np.where((started | (not from_first))[:, None, None], partial + term, term)
            partial = np.where(take[:, None, None], new, partial)
            started |= take
    if from_first:
        live = [q for q in range(n_chunks) if started[q]]
        d_weight = np.zeros((R, C), dt) if not live else partial[live[0]].copy()
        for q in live[1:]:
            d_weight = d_weight + partial[q]
        return d_f, d_weight
    d_weight = np.zeros((R, C), dt)
    for q in range(n_chunks):
        d_weight = d_weight + partial[q]
    return d_f, d_weight


class CpuFilterGraph(CpuVecGraph):
    """CpuVecGraph plus filter_conv in differentiable torch: conv on f @ weight.  The pad slots of f are masked before the
    product, so NaN there reaches neither a value nor a gradient."""

    def filter_conv(self, x, f, weight, role):
        return self.conv(x, self._masked(f) @ weight.to(f.dtype), role)


class TinyFilter(nn.Module):
    """A SchNet-style layer between TinyMP's encoder and decoder (tests/_torch_models.py): the per-edge basis is `n_rbf`
    Gaussians of rel_dist times a cosine cutoff plus the cutoff envelope itself as the bias column; two continuous-filter
    convolutions over "senders" - one on the scalar channels, one at K = dim on vector features (B, N, dim, hidden) - with
    their (n_rbf + 1, hidden) weights as plain Parameters; SiLU throughout.  rel_dist reaches the output only through f."""

    def __init__(self, node_in: int, dim: int, hidden: int = 32, n_rbf: int = 7):
        super().__init__()
        self.dim, self.hidden, self.n_rbf = dim, hidden, n_rbf
        self.enc = nn.Linear(node_in, hidden)
        self.vec = nn.Linear(hidden, dim * hidden)
        self.w_s = nn.Parameter(torch.empty(n_rbf + 1, hidden))
        self.w_v = nn.Parameter(torch.empty(n_rbf + 1, hidden))
        self.node = nn.Sequential(nn.Linear((2 + dim) * hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.dec = nn.Linear(hidden, dim)
        self.gain = nn.Parameter(torch.ones(hidden))
        self.register_buffer("in_scale", torch.ones(node_in))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.gain.fill_(1.0)
            bound = 1.0 / math.sqrt(self.n_rbf + 1)
            self.w_s.uniform_(-bound, bound)
            self.w_v.uniform_(-bound, bound)

    def basis(self, rel_dist):
        """rel_dist (..., 1), in units of the cutoff -> f (..., n_rbf + 1) = [rbf * fcut, fcut]."""
        mu = torch.linspace(0.0, 1.0, self.n_rbf, dtype=rel_dist.dtype, device=rel_dist.device)
        fcut = 0.5 * (torch.cos(math.pi * rel_dist.clamp(0.0, 1.0)) + 1.0)
        return torch.cat([torch.exp(-0.5 * (self.n_rbf * (rel_dist - mu)) ** 2) * fcut, fcut], -1)

    def forward(self, features, particle_type, graph):
        dt = self.gain.dtype
        silu = nn.functional.silu
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        h = silu(self.enc(x * self.in_scale))
        f = self.basis(features["rel_dist"].to(dt)).to(h.dtype)                      # (under autocast h is bfloat16)
        v = silu(self.vec(h)).reshape(h.shape[:-1] + (self.dim, self.hidden))
        ds = graph.filter_conv(h, f, self.w_s, "senders")
        dv = graph.filter_conv(v, f, self.w_v, "senders")
        agg = torch.cat([h, ds, dv.reshape(h.shape[:-1] + (self.dim * self.hidden,))], -1)
        return self.dec(h + self.gain * self.node(agg))
