"""numpy twins of the edge-pair ops of graph.Graph (csrc/lb_graph.hip: k_graph_reverse, k_graph_edge_pair) for the tests:

* ``np_reverse``: the reverse map from a Python dict over (receiver, sender) per trajectory - no bisection, no sorted rows, so
  it shares nothing with the kernel but the statement: slot j of (r, s) maps to the slot of (s, r) of the same trajectory, a
  self-edge to itself, -1 without such an edge and in every pad slot.
* ``np_edge_pair``: swap / symmetrize / antisymmetrize as plain float32 loops over the real slots; +0.0 in a slot without a
  partner and in the pads, which are never read.  Each op is its own adjoint, so ``np_edge_pair_grad`` is the same loop on the
  cotangent (stated separately so that a test names what it compares).
* ``np_edge_pair_bf16``: the bfloat16 contract through tests/_graph_bf16.py - widen, the float32 loop, one rounding; swap
  copies the bits.
* ``MUTANTS``: wrong twins, each the mistake one check of tests/test_graph_reverse.py is there to catch.
* ``torch_edge_pair``: the ops written in torch from the map alone - what tools/graph_reverse_bench.py times them against.
The momentum-conserving model and the CPU graph it is restated on are in tests/_graph_reverse_models.py.
"""
import numpy as np
import torch

from tests import _graph_bf16 as GB

MODES = ("swap", "symmetrize", "antisymmetrize")


def np_reverse(receivers, senders, ne):
    """receivers, senders (B, E_cap) int, ne (B,) -> (B, E_cap) int32."""
    receivers, senders = np.asarray(receivers), np.asarray(senders)
    B, E = receivers.shape
    rev = np.full((B, E), -1, np.int32)
    for b in range(B):
        n = int(ne[b])
        where = {(int(receivers[b, j]), int(senders[b, j])): j for j in range(n)}
        assert len(where) == n, "an edge twice in one trajectory"
        for j in range(n):
            rev[b, j] = where.get((int(senders[b, j]), int(receivers[b, j])), -1)
    return rev


def np_edge_pair(mode, msg, rev, ne, mutant=None):
    """msg (B, E_cap, C) float32 -> (B, E_cap, C) float32: one float32 operation per real, paired slot and column."""
    assert mode in MODES and msg.dtype == np.float32
    B, E, C = msg.shape
    out = np.zeros((B, E, C), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            for j in range(int(ne[b])):
                p = int(rev[b, j])
                if p < 0:
                    if mutant == "unpaired_pass_through":
                        out[b, j] = msg[b, j]
                    continue
                if mutant == "self_edge_skipped" and p == j:
                    continue
                if mode == "swap":
                    out[b, j] = msg[b, p]
                elif mode == "symmetrize":
                    out[b, j] = msg[b, j] + msg[b, p]
                elif mutant == "antisymmetrize_adds":
                    out[b, j] = msg[b, j] + msg[b, p]
                else:
                    out[b, j] = msg[b, j] - msg[b, p]
        if mutant == "pads_copied":
            for b in range(B):
                out[b, int(ne[b]):] = msg[b, int(ne[b]):]
    return out


MUTANTS = ("unpaired_pass_through", "self_edge_skipped", "antisymmetrize_adds", "pads_copied")


def np_edge_pair_grad(mode, d_out, rev, ne):
    """The gradient of msg: the op itself on the cotangent (swap' = swap, symmetrize' = symmetrize; for antisymmetrize the
    transpose of (I - P) is (I - P^T) = (I - P) on the paired slots, P being an involution there)."""
    return np_edge_pair(mode, d_out, rev, ne)


def np_edge_pair_bf16(mode, msg_bits, rev, ne):
    """msg_bits (B, E_cap, C) uint16 -> uint16: round_to_bf16(the float32 op(widen)); swap is a copy of the bits."""
    msg_bits = np.asarray(msg_bits, np.uint16)
    if mode == "swap":
        out = np.zeros_like(msg_bits)
        for b in range(msg_bits.shape[0]):
            for j in range(int(ne[b])):
                if rev[b, j] >= 0:
                    out[b, j] = msg_bits[b, rev[b, j]]
        return out
    return GB.round_bf16(np_edge_pair(mode, GB.widen(msg_bits), rev, ne))


def same_bits(a, b):
    """float32 arrays equal in bits, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def torch_edge_pair(mode, msg, rev):
    """The same thing written in torch with the map (what a user would write with Graph.reverse alone): msg (B, E_cap, C), rev
    (B, E_cap) integer.  One float32 operation per element, so on float32 it has the ops' bits."""
    other = torch.take_along_dim(msg, rev.clamp(min=0).to(torch.int64)[..., None], 1)
    val = other if mode == "swap" else (msg + other if mode == "symmetrize" else msg - other)
    return torch.where((rev >= 0)[..., None], val, torch.zeros((), dtype=msg.dtype, device=msg.device))
