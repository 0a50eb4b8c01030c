"""A momentum-conserving message-passing layer for ``models.TorchModel``, the worked example of the edge-pair ops
(graph.Graph.antisymmetrize; README "Your own network"), and the CPU graph it is restated on.

``MomentumMP``: a scalar edge magnitude from a ``pair_add`` edge encoder times the edge's displacement, antisymmetrised, summed
over receivers:

    e = silu(graph.pair_add(self.ws(x), self.wr(x)) + self.we(features["rel_dist"]))
    m = graph.antisymmetrize(self.dec(e) * features["rel_disp"])      # (B, E_cap, dim): m_ij = -m_ji exactly
    acc = graph.segment_sum(m, "receivers")

The antisymmetrisation is the LAST edge-shaped step on purpose: m_ij = -m_ji then rests on the op alone - one float32
subtraction of the same two numbers in either order - and not on a GEMM giving equal rows equal bits.  So the sum of acc over
the particles of a trajectory is zero up to the rounding of the ordered row sums, on every list, one-directional edges included
(their slots get +0.0).  ``antisym=False`` is the control: the same network without the op.

``CpuReverseGraph`` is tests/_graph_pair.CpuPairGraph plus reverse / swap / symmetrize / antisymmetrize in differentiable torch
(``take_along_dim`` over the dict-built map of tests/_graph_reverse.py), any float dtype.
"""
import numpy as np
import torch
from torch import nn

from tests import _graph_reverse as GR
from tests._graph_pair import CpuPairGraph
from tests._torch_models import NODE_KEYS


class MomentumMP(nn.Module):
    """forward(features, particle_type, graph) -> (B, N, dim).  `tap`: the module keeps the edge field m and the output of its
    last forward in MomentumMP.last (a class attribute: TorchModel runs a deep copy of the module)."""
    last = None

    def __init__(self, node_in: int, dim: int, hidden: int = 32, antisym: bool = True, tap: bool = False):
        super().__init__()
        self.antisym, self.tap = antisym, tap
        self.enc = nn.Linear(node_in, hidden)
        self.ws = nn.Linear(hidden, hidden, bias=False)
        self.wr = nn.Linear(hidden, hidden, bias=False)
        self.we = nn.Linear(1, hidden)
        self.dec = nn.Linear(hidden, 1)
        self.gain = nn.Parameter(torch.ones(hidden))
        self.register_buffer("in_scale", torch.ones(node_in))

    def reset_parameters(self):
        with torch.no_grad():
            self.gain.fill_(1.0)

    def forward(self, features, particle_type, graph):
        dt = self.gain.dtype
        silu = nn.functional.silu
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        x = silu(self.enc(x * self.in_scale))
        e = silu(graph.pair_add(self.ws(x), self.wr(x)) + self.we(features["rel_dist"].to(dt)))
        m = self.dec(self.gain * e) * features["rel_disp"].to(dt)
        if self.antisym:
            m = graph.antisymmetrize(m)                               # (B, E_cap, dim): m_ij = -m_ji exactly
        acc = graph.segment_sum(m, "receivers")
        if self.tap:
            MomentumMP.last = (m.detach(), acc.detach())
        return acc


class CpuReverseGraph(CpuPairGraph):
    def __init__(self, senders, receivers, n_edges, n_nodes):
        super().__init__(senders, receivers, n_edges, n_nodes)
        self.reverse = torch.as_tensor(GR.np_reverse(np.asarray(receivers), np.asarray(senders), np.asarray(n_edges).reshape(-1)))

    def _clean(self, msg):
        """(NaN in a pad slot must reach neither a value nor a gradient: 0 * NaN is NaN in torch.where's backward)"""
        return torch.where(self.real[..., None], msg, torch.zeros((), dtype=msg.dtype))

    def swap(self, msg):
        return GR.torch_edge_pair("swap", self._clean(msg), self.reverse)

    def symmetrize(self, msg):
        return GR.torch_edge_pair("symmetrize", self._clean(msg), self.reverse)

    def antisymmetrize(self, msg):
        return GR.torch_edge_pair("antisymmetrize", self._clean(msg), self.reverse)
