"""Graph primitives with autograd on the engine's current neighbor list (csrc/lb_graph.hip).

What a message-passing network written in torch needs from the graph: ``x[senders]``, ``x[receivers]`` and
``jraph.segment_sum(msg, receivers | senders, N)``.  ``Graph`` runs them as HIP kernels on the list the ``FeatureDict``
describes, in the padded layout of ``features["senders"]`` / ``["receivers"]`` ((B, E_cap), pad slots hold N):

    g = Graph(features)                      # binds features.engine and features.version
    xs = g.gather(x, "senders")              # (B, N, C) -> (B, E_cap, C); pad slots are +0.0
    agg = g.segment_sum(msg, "receivers")    # (B, E_cap, C) -> (B, N, C); pad slots are never read
    g.n_edges, g.senders, g.receivers        # (B,), (B, E_cap), (B, E_cap)

(with un-batched features the leading B is dropped: (N, C) -> (E_cap, C)).  Trailing dimensions beyond C are folded into C.

The sum is ordered: per node its real slots in ascending slot order, one float32 add after the other, no atomics - the
result equals a numpy float32 loop bit for bit and two calls give the same bits (torch's ``index_add_`` on the GPU uses
float atomics and does not).  The two ops are each other's adjoints - gather's backward is ``segment_sum`` over the same
role, ``segment_sum``'s backward is ``gather`` - so forward and backward are the same two kernels with the same bits.

Tensors are float32 on the engine's device (``TypeError`` otherwise) and are made contiguous here.  A forward or a
backward after the engine's list moved on raises ``RuntimeError``: the staleness rule of ``FeatureDict``.  The ops are once
differentiable: a double backward through them (``create_graph=True``) raises.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

__all__ = ["Graph"]

_ROLES = {"receivers": 0, "senders": 1}
_GATHER, _SEGMENT_SUM = 0, 1


class _Op(torch.autograd.Function):
    """gather (kind 0) or segment_sum (kind 1) over `role`; the backward is the other kind over the same role."""

    @staticmethod
    def forward(ctx, x, graph, role, kind):
        ctx.graph, ctx.role, ctx.kind = graph, role, kind
        return graph._run(kind, role, x)

    @staticmethod
    @once_differentiable   # (the backward runs the kernel on detached data: a double backward raises instead of giving zeros)
    def backward(ctx, d):
        return ctx.graph._run(1 - ctx.kind, ctx.role, d), None, None, None


class Graph:
    """The engine's current list behind `features` (a FeatureDict), as differentiable gather / segment_sum.
    `batched`: whether the tensors carry the leading B (default: as the features do)."""

    def __init__(self, features, batched: Optional[bool] = None):
        engine = getattr(features, "engine", None)
        if engine is None:
            raise TypeError("graph.Graph needs the FeatureDict returned by case.preprocess* / allocate* (it names the "
                            "engine and the list to run on)")
        self.features, self.engine, self.version = features, engine, features.version
        self.batched = bool(features.batched if batched is None else batched)
        if not self.batched and engine.B != 1:
            raise ValueError(f"graph.Graph: un-batched tensors on an engine of batch {engine.B}")
        self._idx = None

    # ------------------------------------------------------------------ the list
    def _check_fresh(self, what: str) -> None:
        if self.engine.version != self.version:
            raise RuntimeError(f"graph.{what}: the engine's neighbor list changed since these features were produced "
                               "(features are stale)")

    def _export(self):
        if self._idx is None:
            self._check_fresh("Graph")
            self._idx = self.engine.nl_idx()
        return self._idx

    def _lead(self, t: torch.Tensor) -> torch.Tensor:
        return t if self.batched else t[0]

    @property
    def n_edges(self) -> torch.Tensor:
        return self._lead(self._export()[1])

    @property
    def receivers(self) -> torch.Tensor:
        return self._lead(self._export()[0][:, 0])

    @property
    def senders(self) -> torch.Tensor:
        return self._lead(self._export()[0][:, 1])

    # ------------------------------------------------------------------ the ops
    @staticmethod
    def _role(role) -> int:
        if role not in _ROLES:
            raise ValueError(f"role must be 'senders' or 'receivers', got {role!r}")
        return _ROLES[role]

    def _run(self, kind: int, role: int, t: torch.Tensor) -> torch.Tensor:
        name = "segment_sum" if kind == _SEGMENT_SUM else "gather"
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"graph.{name}: float32 tensors only, got {getattr(t, 'dtype', type(t))}")
        e = self.engine
        if t.device != e.device:
            raise TypeError(f"graph.{name}: the tensor is on {t.device}, the engine on {e.device}")
        self._check_fresh(name)
        rows = e.e_cap if kind == _SEGMENT_SUM else e.N
        lead = (e.B, rows) if self.batched else (rows,)
        if tuple(t.shape[:len(lead)]) != lead or t.dim() <= len(lead) or t.numel() == 0:
            raise ValueError(f"graph.{name}: expected {lead + ('C',)} (C >= 1), got {tuple(t.shape)}")
        rest = tuple(t.shape[len(lead):])
        flat = t.detach().contiguous().reshape(e.B * rows, -1)
        out = (e.graph_segment_sum if kind == _SEGMENT_SUM else e.graph_gather)(role, flat)
        out_rows = e.N if kind == _SEGMENT_SUM else e.e_cap
        return out.reshape(((e.B, out_rows) if self.batched else (out_rows,)) + rest)

    def gather(self, x: torch.Tensor, role: str) -> torch.Tensor:
        """x (B, N, C) -> (B, E_cap, C): x[b, role index of slot (b, j)] in the real slots, +0.0 in the pad slots."""
        return _Op.apply(x, self, self._role(role), _GATHER)

    def segment_sum(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): per node the ordered float32 sum of the real slots whose role index it is."""
        return _Op.apply(msg, self, self._role(role), _SEGMENT_SUM)
