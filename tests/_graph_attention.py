"""Restatements of graph.Graph's attention ops for the tests: numpy float32 loops that state the order contracts bit for bit
(degree, segment_mean, segment_max / segment_min and their backward), float64 restatements of segment_softmax and attend
with their backward, the same ops in differentiable torch on the CPU (`CpuAttnGraph`, any dtype), and `TinyAttn`, a small
attention network for ``models.TorchModel``.

Everything works on an exported padded list: `idx` (B, E_cap) int, the role index of every slot (pad slots hold N), and
`ne` (B,), the real slots of every trajectory.  Pad slots are never read.
"""
import numpy as np
import torch
from torch import nn

from tests._torch_models import NODE_KEYS, CpuGraph
from tests.test_graph_ops_gpu import np_segment_sum


def node_slots(idx, ne, N):
    """[b][i] -> the real slots of trajectory b whose role index is i, ascending."""
    out = []
    for b in range(idx.shape[0]):
        real = np.asarray(idx[b, :ne[b]])
        order = np.argsort(real, kind="stable")
        out.append(np.split(order, np.searchsorted(real[order], np.arange(1, N))))
    return out


def rank_steps(idx, ne, N):
    """[b] -> [(nodes, slots) for n = 0, 1, ...]: the nodes that have an n-th real slot (in ascending slot order) and that
    slot - one step of every node's loop at a time."""
    out = []
    for b in range(idx.shape[0]):
        real = np.asarray(idx[b, :ne[b]])
        order = np.argsort(real, kind="stable")
        nodes = real[order]
        rank = np.arange(len(order)) - np.searchsorted(nodes, nodes)
        out.append([(nodes[rank == n], order[rank == n]) for n in range(int(rank.max()) + 1 if len(rank) else 0)])
    return out


def np_degree(idx, ne, N):
    return np.array([[len(s) for s in row] for row in node_slots(idx, ne, N)], np.int32)


def np_segment_mean(msg, idx, ne, N):
    """The ordered float32 sum, then ONE float32 division by max(degree, 1)."""
    deg = np.maximum(np_degree(idx, ne, N), 1).astype(np.float32)
    return (np_segment_sum(msg, idx, ne, N) / deg[..., None]).astype(np.float32)


def np_segment_max(msg, idx, ne, N, minimum=False):
    """msg (B, E_cap, C) -> (out (B, N, C) float32, win (B, N, C) int32).  The order contract, stated as a loop: start from
    the node's first real slot; a further slot, ascending, replaces the value only if it is strictly greater (smaller), or
    if it is a NaN and the value is not (np.maximum's NaN rule).  Empty row: +0.0 and -1."""
    B, C = msg.shape[0], msg.shape[2]
    out, win = np.zeros((B, N, C), np.float32), np.full((B, N, C), -1, np.int32)
    for b, steps in enumerate(rank_steps(idx, ne, N)):
        for n, (nodes, slots) in enumerate(steps):
            a, j = msg[b, slots], slots[:, None].astype(np.int32)
            if n == 0:
                out[b, nodes], win[b, nodes] = a, j
                continue
            s = out[b, nodes]
            with np.errstate(invalid="ignore"):
                beats = ((a < s) if minimum else (a > s)) | (np.isnan(a) & ~np.isnan(s))
            out[b, nodes] = np.where(beats, a, s)
            win[b, nodes] = np.where(beats, j, win[b, nodes])
    return out, win


def np_segment_max_backward(d_out, win, idx, ne, e_cap):
    """d_msg (B, E_cap, C): d_out[node] where the slot won, +0.0 in every other slot."""
    B, N, C = d_out.shape
    d = np.zeros((B, e_cap, C), np.float32)
    for b in range(B):
        j = np.arange(int(ne[b]))
        i = idx[b, :ne[b]]
        d[b, :ne[b]] = np.where(win[b, i] == j[:, None], d_out[b, i], np.float32(0))
    return d


def softmax64(logits, idx, ne, N):
    """(B, E_cap, C) float64: per node and column the softmax over the node's real slots; 0 in the pad slots."""
    x = np.asarray(logits, np.float64)
    y = np.zeros_like(x)
    for b, row in enumerate(node_slots(idx, ne, N)):
        for slots in row:
            if len(slots):
                e = np.exp(x[b, slots] - x[b, slots].max(0))
                y[b, slots] = e / e.sum(0)
    return y


def softmax_backward64(y, d_y, idx, ne, N):
    y, d_y = np.asarray(y, np.float64), np.asarray(d_y, np.float64)
    d = np.zeros_like(y)
    for b, row in enumerate(node_slots(idx, ne, N)):
        for slots in row:
            if len(slots):
                d[b, slots] = y[b, slots] * (d_y[b, slots] - (d_y[b, slots] * y[b, slots]).sum(0))
    return d


def attend64(logits, values, idx, ne, N):
    """logits (B, E_cap, H), values (B, E_cap, H, D) -> (B, N, H, D) float64."""
    a = softmax64(logits, idx, ne, N)
    v = np.asarray(values, np.float64)
    out = np.zeros((v.shape[0], N) + v.shape[2:])
    for b, row in enumerate(node_slots(idx, ne, N)):
        for i, slots in enumerate(row):
            if len(slots):
                out[b, i] = (a[b, slots][..., None] * v[b, slots]).sum(0)
    return out


def attend_backward64(logits, values, d_out, idx, ne, N):
    """-> (d_logits (B, E_cap, H), d_values (B, E_cap, H, D), the bound's scale max over the real slots of sum_d |d_out v|)."""
    a = softmax64(logits, idx, ne, N)
    v, g = np.asarray(values, np.float64), np.asarray(d_out, np.float64)
    d_l, d_v, scale = np.zeros_like(a), np.zeros(v.shape), 0.0
    for b, row in enumerate(node_slots(idx, ne, N)):
        for i, slots in enumerate(row):
            if len(slots):
                d_v[b, slots] = a[b, slots][..., None] * g[b, i]
                t = (g[b, i] * v[b, slots]).sum(-1)
                scale = max(scale, np.abs(g[b, i] * v[b, slots]).sum(-1).max())
                d_l[b, slots] = a[b, slots] * (t - (a[b, slots] * t).sum(0))
    return d_l, d_v, scale


class CpuAttnGraph(CpuGraph):
    """CpuGraph plus the attention ops in differentiable torch: scatter_reduce for the extrema (an empty row keeps 0),
    exp / index_add for the softmax.  Ties share the gradient here (torch's amax rule), so it stands in for the device ops
    only where no two slots of a node are equal."""

    def degree(self, role):
        ones = self.real.to(torch.float64)[..., None]
        return self.segment_sum(ones, role)[..., 0].to(torch.int32)

    def _extreme(self, msg, role, how):
        shape = msg.shape
        m = torch.where(self.real[..., None], msg.reshape(self.B, self.E, -1), torch.zeros((), dtype=msg.dtype))
        C = m.shape[-1]
        index = self.flat[role][:, None].expand(-1, C)
        out = msg.new_zeros((self.B * self.N + 1, C)).scatter_reduce(0, index, m.reshape(self.B * self.E, C), how, include_self=False)
        return out[:-1].reshape((self.B, self.N) + tuple(shape[2:]))

    def segment_max(self, msg, role):
        return self._extreme(msg, role, "amax")

    def segment_min(self, msg, role):
        return self._extreme(msg, role, "amin")

    def segment_mean(self, msg, role):
        return self.segment_sum(msg, role) / self.degree(role).clamp(min=1).to(msg.dtype)[..., None]

    def segment_softmax(self, logits, role):
        x = torch.where(self.real[..., None], logits, torch.zeros((), dtype=logits.dtype))
        e = torch.exp(x - self.gather(self.segment_max(x, role).detach(), role))
        e = torch.where(self.real[..., None], e, torch.zeros((), dtype=logits.dtype))
        s = self.gather(self.segment_sum(e, role), role)
        return e / torch.where(self.real[..., None], s, torch.ones((), dtype=logits.dtype))

    def attend(self, logits, values, role):
        H, D = values.shape[-2:]
        a = self.segment_softmax(logits, role)
        v = torch.where(self.real[..., None, None], values, torch.zeros((), dtype=values.dtype))
        return self.segment_sum((a[..., None] * v).reshape(self.B, self.E, H * D), role).reshape(self.B, self.N, H, D)


class TinyAttn(nn.Module):
    """TinyMP's encoder and decoder (tests/_torch_models.py) around one `attend` layer over receivers - `heads` heads of
    hidden / heads columns, logits and values from an edge Linear - and one `segment_max` of the edge values over senders."""

    def __init__(self, node_in: int, dim: int, hidden: int = 32, heads: int = 4):
        super().__init__()
        self.heads = heads
        self.enc = nn.Linear(node_in, hidden)
        self.edge = nn.Linear(2 * hidden + dim + 1, hidden + heads)
        self.node = nn.Sequential(nn.Linear(3 * hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.dec = nn.Linear(hidden, dim)
        self.gain = nn.Parameter(torch.ones(hidden))
        self.register_buffer("in_scale", torch.ones(node_in))

    def reset_parameters(self):
        with torch.no_grad():
            self.gain.fill_(1.0)

    def forward(self, features, particle_type, graph):
        dt = self.gain.dtype
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        h = nn.functional.silu(self.enc(x * self.in_scale))
        hs, hr = graph.gather(h, "senders"), graph.gather(h, "receivers")
        e = self.edge(torch.cat([hs, hr, features["rel_disp"].to(dt), features["rel_dist"].to(dt)], -1))
        logits, values = e[..., :self.heads], nn.functional.silu(e[..., self.heads:])
        att = graph.attend(logits, values.reshape(values.shape[:-1] + (self.heads, -1)), "receivers")
        agg = torch.cat([h, att.reshape(h.shape), graph.segment_max(values, "senders")], -1)
        return self.dec(h + self.gain * self.node(agg))
