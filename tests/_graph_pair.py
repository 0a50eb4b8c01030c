"""Restatements of graph.Graph's edge-message ops for the tests: numpy loops that state the order contracts of ``conv``,
``pair_mul`` (with its K-reduction) and ``pair_add`` bit for bit, the same ops in differentiable torch on the CPU
(`CpuPairGraph`, any dtype), and `TinyConv`, a small PaiNN-style network for ``models.TorchModel``.

Everything works on an exported padded list: per role `idx` (B, E_cap) int, the role's node of every slot (pad slots hold
N), and `ne` (B,), the real slots of every trajectory.  Pad slots are never read.  The numpy twins compute in the dtype of
their first argument: float32 states the device's bits, float64 the adjoint identities.
"""
import numpy as np
import torch
from torch import nn

from tests._graph_attention import CpuAttnGraph, rank_steps
from tests._torch_models import NODE_KEYS

OTHER = {"receivers": "senders", "senders": "receivers"}


def np_conv(x, w, idx_role, idx_other, ne, N):
    """x (B, N, K, C), w (B, E_cap, C) -> (B, N, K, C).  The contract as a loop, one step of every node's loop at a time: per
    node the real slots j whose `idx_role` is the node, ascending; the term of a slot is x[idx_other[j]] * w[j], rounded to
    the dtype; the first term starts the sum, every further one is one add.  An empty row is +0.0."""
    out = np.zeros(x.shape, x.dtype)
    for b, steps in enumerate(rank_steps(idx_role, ne, N)):
        for n, (nodes, slots) in enumerate(steps):
            term = (x[b, idx_other[b, slots]] * w[b, slots][:, None, :]).astype(x.dtype)
            out[b, nodes] = term if n == 0 else out[b, nodes] + term
    return out


def np_pair_mul(a, b, idx_a, idx_b, ne, e_cap):
    """a, b (B, N, K, C) -> (B, E_cap, C): per real slot a[idx_a[j], 0] * b[idx_b[j], 0], then one add per further k of the
    rounded product a[.., k] * b[.., k], k ascending; +0.0 in the pad slots."""
    B, _, K, C = a.shape
    out = np.zeros((B, e_cap, C), a.dtype)
    for t in range(B):
        ia, ib = idx_a[t, :ne[t]], idx_b[t, :ne[t]]
        s = (a[t, ia, 0] * b[t, ib, 0]).astype(a.dtype)
        for k in range(1, K):
            s = s + (a[t, ia, k] * b[t, ib, k]).astype(a.dtype)
        out[t, :ne[t]] = s
    return out


def np_pair_add(a, b, idx_a, idx_b, ne, e_cap):
    """a, b (B, N, C) -> (B, E_cap, C): a[idx_a[j]] + b[idx_b[j]] in the real slots, +0.0 in the pad slots."""
    B, _, C = a.shape
    out = np.zeros((B, e_cap, C), a.dtype)
    for t in range(B):
        out[t, :ne[t]] = a[t, idx_a[t, :ne[t]]] + b[t, idx_b[t, :ne[t]]]
    return out


class CpuPairGraph(CpuAttnGraph):
    """CpuAttnGraph plus conv / pair_mul / pair_add in differentiable torch (index_select / index_add through gather and
    segment_sum).  The pad slots of w are masked before they are multiplied, so NaN there reaches neither a value nor a
    gradient."""

    def _gather_rows(self, x, role):
        """x (B, N, ...) -> (B, E_cap, ...)."""
        rest = tuple(x.shape[2:])
        return self.gather(x.reshape(self.B, self.N, -1), role).reshape((self.B, self.E) + rest)

    def conv(self, x, w, role):
        wm = torch.where(self.real.reshape((self.B, self.E) + (1,) * (w.dim() - 2)), w, torch.zeros((), dtype=w.dtype))
        xg = self._gather_rows(x, OTHER[role])
        if x.dim() == w.dim() + 1:
            wm = wm.unsqueeze(-2)
        msg = xg * wm
        return self.segment_sum(msg.reshape(self.B, self.E, -1), role).reshape(x.shape)

    def pair_mul(self, a, b):
        return self._gather_rows(a, "senders") * self._gather_rows(b, "receivers")

    def pair_add(self, a, b):
        return self._gather_rows(a, "senders") + self._gather_rows(b, "receivers")


class TinyConv(nn.Module):
    """A PaiNN-style layer between TinyMP's encoder and decoder (tests/_torch_models.py): the edge encoder is a `pair_add` of
    two node Linears plus an edge Linear - Linear(cat[h_s, h_r, e]) with its GEMMs on N rows -, the filter is gated by a
    `pair_mul`, one scalar `conv` and one K = dim `conv` on vector features (B, N, dim, hidden) run over "senders"; SiLU
    throughout."""

    def __init__(self, node_in: int, dim: int, hidden: int = 32):
        super().__init__()
        self.dim, self.hidden = dim, hidden
        self.enc = nn.Linear(node_in, hidden)
        self.edge_s = nn.Linear(hidden, hidden, bias=False)
        self.edge_r = nn.Linear(hidden, hidden, bias=False)
        self.edge_e = nn.Linear(dim + 1, hidden)
        self.gate_s = nn.Linear(hidden, hidden)
        self.gate_r = nn.Linear(hidden, hidden)
        self.filt = nn.Linear(hidden, 2 * hidden)
        self.vec = nn.Linear(hidden, dim * hidden)
        self.node = nn.Sequential(nn.Linear((2 + dim) * hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.dec = nn.Linear(hidden, dim)
        self.gain = nn.Parameter(torch.ones(hidden))
        self.register_buffer("in_scale", torch.ones(node_in))

    def reset_parameters(self):
        with torch.no_grad():
            self.gain.fill_(1.0)

    def forward(self, features, particle_type, graph):
        dt = self.gain.dtype
        silu = nn.functional.silu
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        h = silu(self.enc(x * self.in_scale))
        geo = torch.cat([features["rel_disp"].to(dt), features["rel_dist"].to(dt)], -1)
        e = silu(graph.pair_add(self.edge_s(h), self.edge_r(h)) + self.edge_e(geo))
        gate = silu(graph.pair_mul(silu(self.gate_s(h)), silu(self.gate_r(h))))
        w = self.filt(e)
        w_s, w_v = w[..., :self.hidden] * gate, w[..., self.hidden:] * gate
        v = silu(self.vec(h)).reshape(h.shape[:-1] + (self.dim, self.hidden))
        ds = graph.conv(h, w_s, "senders")
        dv = graph.conv(v, w_v, "senders")
        agg = torch.cat([h, ds, dv.reshape(h.shape[:-1] + (self.dim * self.hidden,))], -1)
        return self.dec(h + self.gain * self.node(agg))
