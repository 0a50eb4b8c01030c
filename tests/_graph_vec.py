"""Restatements of graph.Graph's vector-message ops for the tests: numpy loops that state the order contracts of ``conv_vec``,
``conv_dot`` and their shared edge gradients bit for bit, the two ops in differentiable torch on the CPU (`CpuVecGraph`, any
dtype), and `TinyVec`, a small equivariant network for ``models.TorchModel``.

Everything works on an exported padded list: per role `idx` (B, E_cap) int, the role's node of every slot (pad slots hold
N), and `ne` (B,), the real slots of every trajectory.  Pad slots are never read.  The numpy twins compute in the dtype of
their first argument: float32 states the device's bits, float64 the adjoint identities.
"""
import os
import re

import numpy as np
import torch
from torch import nn

from tests._graph_attention import rank_steps
from tests._graph_pair import OTHER, CpuPairGraph  # noqa: F401  (OTHER is re-exported)
from tests._torch_models import NODE_KEYS

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lbhip.h")


def du_block() -> int:
    """LB_GRAPH_DU_BLOCK of include/lbhip.h: the column block of the d_u sum - the one place the twins read it from."""
    with open(_HEADER) as f:
        return int(re.search(r"^#define\s+LB_GRAPH_DU_BLOCK\s+(\d+)", f.read(), flags=re.M).group(1))


def _vec_dot(vg, ug):
    """vg (n, K, C), ug (n, K) -> t (n, C): vg[:, 0] * ug[:, 0], then one add per further k of the rounded product."""
    t = (vg[:, 0] * ug[:, 0:1]).astype(vg.dtype)
    for k in range(1, vg.shape[1]):
        t = t + (vg[:, k] * ug[:, k:k + 1]).astype(vg.dtype)
    return t


def np_conv_vec(x, w, u, idx_role, idx_other, ne, N):
    """x (B, N, C), w (B, E_cap, C), u (B, E_cap, K) -> (B, N, K, C).  Per node the real slots j whose `idx_role` is the node,
    ascending; the term of a slot is (x[idx_other[j]] * w[j]) * u[j, k], each product rounded to the dtype; the first term
    starts the sum, every further one is one add.  An empty row is +0.0."""
    B, _, C = x.shape
    out = np.zeros((B, N, u.shape[2], C), x.dtype)
    for b, steps in enumerate(rank_steps(idx_role, ne, N)):
        for n, (nodes, slots) in enumerate(steps):
            xw = (x[b, idx_other[b, slots]] * w[b, slots]).astype(x.dtype)
            term = (xw[:, None, :] * u[b, slots][:, :, None]).astype(x.dtype)
            out[b, nodes] = term if n == 0 else out[b, nodes] + term
    return out


def np_conv_dot(v, w, u, idx_role, idx_other, ne, N):
    """v (B, N, K, C), w (B, E_cap, C), u (B, E_cap, K) -> (B, N, C): per slot t = v[idx_other[j], 0] * u[j, 0] + ... (k
    ascending, the first product starts the sum), the term w[j] * t; per node the terms of its slots added in ascending order
    from the first one."""
    B, _, _, C = v.shape
    out = np.zeros((B, N, C), v.dtype)
    for b, steps in enumerate(rank_steps(idx_role, ne, N)):
        for n, (nodes, slots) in enumerate(steps):
            term = (w[b, slots] * _vec_dot(v[b, idx_other[b, slots]], u[b, slots])).astype(v.dtype)
            out[b, nodes] = term if n == 0 else out[b, nodes] + term
    return out


def np_vec_edge_grad(s, v, w, u, idx_s, idx_v, ne, e_cap, block=None):
    """s (B, N, C) read at idx_s, v (B, N, K, C) read at idx_v, w (B, E_cap, C), u (B, E_cap, K) -> (d_w (B, E_cap, C), d_u
    (B, E_cap, K)), +0.0 in the pad slots:
      d_w[j] = s * t, t as in np_conv_dot;
      d_u[j, k] = the sum over c of (s[c] * w[j, c]) * v[k, c]: consecutive blocks of `block` columns (the last may be short),
                  c ascending inside a block from its first product, the block sums added in ascending order from the first."""
    block = du_block() if block is None else block
    B, _, K, C = v.shape
    d_w, d_u = np.zeros((B, e_cap, C), s.dtype), np.zeros((B, e_cap, K), s.dtype)
    for t in range(B):
        n = int(ne[t])
        sg, vg, wg, ug = s[t, idx_s[t, :n]], v[t, idx_v[t, :n]], w[t, :n], u[t, :n]
        d_w[t, :n] = (sg * _vec_dot(vg, ug)).astype(s.dtype)
        prod = ((sg * wg).astype(s.dtype)[:, None, :] * vg).astype(s.dtype)          # (n, K, C)
        total = None
        for c0 in range(0, C, block):
            part = prod[:, :, c0]
            for c in range(c0 + 1, min(c0 + block, C)):
                part = part + prod[:, :, c]
            total = part if total is None else total + part
        d_u[t, :n] = total
    return d_w, d_u


class CpuVecGraph(CpuPairGraph):
    """CpuPairGraph plus conv_vec / conv_dot in differentiable torch.  The pad slots of w and u are masked before they are
    multiplied, so NaN there reaches neither a value nor a gradient."""

    def _masked(self, t):
        return torch.where(self.real.reshape((self.B, self.E) + (1,) * (t.dim() - 2)), t, torch.zeros((), dtype=t.dtype))

    def conv_vec(self, x, w, u, role):
        xw = self._gather_rows(x, OTHER[role]) * self._masked(w)                      # (B, E, C)
        msg = xw[:, :, None, :] * self._masked(u)[:, :, :, None]                      # (B, E, K, C)
        K, C = u.shape[-1], w.shape[-1]
        return self.segment_sum(msg.reshape(self.B, self.E, K * C), role).reshape(self.B, self.N, K, C)

    def conv_dot(self, v, w, u, role):
        t = (self._gather_rows(v, OTHER[role]) * self._masked(u)[:, :, :, None]).sum(2)
        return self.segment_sum(self._masked(w) * t, role)


class TinyVec(nn.Module):
    """An equivariant layer between TinyMP's encoder and decoder (tests/_torch_models.py): two filters from a `pair_add` edge
    encoder as in TinyConv; v = conv_vec(s, w_vs, rel_disp, "senders") lifts the scalars to vectors along the edge directions,
    s' = s + conv_dot(v, w_sv, rel_disp, "senders") brings them back; the output is a vector readout of v - a bias-free
    Linear over channels - plus dec(s')."""

    def __init__(self, node_in: int, dim: int, hidden: int = 32):
        super().__init__()
        self.dim, self.hidden = dim, hidden
        self.enc = nn.Linear(node_in, hidden)
        self.edge_s = nn.Linear(hidden, hidden, bias=False)
        self.edge_r = nn.Linear(hidden, hidden, bias=False)
        self.edge_e = nn.Linear(dim + 1, hidden)
        self.filt = nn.Linear(hidden, 2 * hidden)
        self.read = nn.Linear(hidden, 1, bias=False)
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
        s = silu(self.enc(x * self.in_scale))
        r = features["rel_disp"].to(dt)
        geo = torch.cat([r, features["rel_dist"].to(dt)], -1)
        e = silu(graph.pair_add(self.edge_s(s), self.edge_r(s)) + self.edge_e(geo))
        w = self.filt(e)
        w_vs, w_sv = w[..., :self.hidden], w[..., self.hidden:]
        v = graph.conv_vec(s, w_vs, r, "senders")                                    # (B, N, dim, hidden)
        s2 = s + self.gain * graph.conv_dot(v, w_sv, r, "senders")
        return self.read(v)[..., 0] + self.dec(s2)
