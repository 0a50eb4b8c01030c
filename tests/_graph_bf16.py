"""Restatements of the bfloat16 contract of graph.Graph for the tests:

    the bfloat16 op  ==  round_to_bf16( the float32 op( upcast(inputs) ) )        bit for bit

`round_bf16` is the rounding by integer arithmetic on the float32 bits (round to nearest even, NaN stays NaN, beyond the
range +-inf, subnormals kept), `widen` its exact inverse direction; `np_segment_sum_bf16` is the float32 loop of
tests/test_graph_ops_gpu.np_segment_sum on the widened terms, rounded once; `CpuGraphBf16` is tests/_torch_models.CpuGraph
whose segment_sum follows that contract (float32 accumulation, one rounding), so that the CPU restatement of a network under
``torch.autocast("cpu", dtype=torch.bfloat16)`` states what the device ops do and not ``index_add`` in bfloat16.  The two
mutated twins (`np_segment_sum_bf16_acc`: the partial sums held in bfloat16; `reverse=True`: descending slot order) are the
wrong implementations the planted rows must tell from the contract.
"""
import numpy as np
import torch

from tests._graph_attention import CpuAttnGraph
from tests.test_graph_ops_gpu import np_segment_sum

# rows of one node's terms whose sum shows what an implementation does: [256, 1, 1, 1, 1] is 260 with a float32 accumulator
# (a tie at 258 on the way would stay 256 in bfloat16: 256 + 1 rounds back to 256 every time); the other two hold the same
# terms in two orders and give 0 and 1 (2^24 + 1 is a float32 tie that rounds to 2^24); descending, the first of them gives 1.
PLANTED_ROWS = ([256.0, 1.0, 1.0, 1.0, 1.0], [2.0 ** 24, 1.0, -2.0 ** 24], [1.0, -2.0 ** 24, 2.0 ** 24])
PLANTED_SUMS = (260.0, 0.0, 1.0)


def round_bf16(x):
    """float32 array -> uint16 array: the bfloat16 bits of round-to-nearest-even(x)."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = np.where(nan, (u >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def widen(bits):
    """uint16 bfloat16 bits -> float32 (exact)."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16_values(x):
    """float32 -> the float32 array of the values rounded to bfloat16."""
    return widen(round_bf16(x))


def torch_bits(t):
    """a bfloat16 torch tensor -> its uint16 bits as numpy."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(bits, device=None, requires_grad=False):
    """uint16 bits -> a bfloat16 torch tensor holding them."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(bits, np.uint16)).view(np.int16).copy()).view(torch.bfloat16)
    if device is not None:
        t = t.to(device)
    return t.requires_grad_(requires_grad)


def same_bits(a, b):
    """uint16 arrays equal, a NaN matching any NaN (its payload is not specified)."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    na, nb = (a & 0x7FFF) > 0x7F80, (b & 0x7FFF) > 0x7F80
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def np_segment_sum_bf16(msg_bits, idx, ne, N, reverse=False):
    """msg_bits (B, E_cap, C) uint16 -> (B, N, C) uint16: the float32 loop on the widened terms, rounded once.  `reverse`: a
    mutated twin that adds in descending slot order."""
    msg = widen(msg_bits)
    if reverse:
        msg, idx = msg.copy(), np.array(idx).copy()
        for b in range(idx.shape[0]):
            msg[b, :ne[b]], idx[b, :ne[b]] = msg[b, :ne[b]][::-1].copy(), idx[b, :ne[b]][::-1].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return round_bf16(np_segment_sum(msg, idx, ne, N))


def np_segment_sum_bf16_acc(msg_bits, idx, ne, N):
    """A mutated twin: the running sum is rounded to bfloat16 after every add (what a bfloat16 accumulator does)."""
    msg = widen(msg_bits)
    B, E = idx.shape
    out = np.zeros((B, N, msg.shape[2]), np.float32)
    seen = np.zeros((B, N), bool)
    for b in range(B):
        for j in range(int(ne[b])):
            i = idx[b, j]
            out[b, i] = to_bf16_values(out[b, i] + msg[b, j]) if seen[b, i] else msg[b, j]
            seen[b, i] = True
    return round_bf16(out)


class CpuGraphBf16(CpuAttnGraph):
    """CpuAttnGraph under the bfloat16 contract: a bfloat16 input is widened, the op runs in float32 and the result is rounded
    once.  Other dtypes pass through unchanged (the float64 and float32 restatements use the same class)."""

    def _wide(self, op, *tensors):
        if tensors[0].dtype != torch.bfloat16:
            return op(*tensors)
        return op(*[t.float() for t in tensors]).to(torch.bfloat16)

    def segment_sum(self, msg, role):
        return self._wide(lambda m: CpuAttnGraph.segment_sum(self, m, role), msg)

    def segment_mean(self, msg, role):
        if msg.dtype != torch.bfloat16:
            return CpuAttnGraph.segment_mean(self, msg, role)
        deg = self.degree(role).clamp(min=1).to(torch.float32)[..., None]
        return (self.segment_sum(msg, role).float() / deg).to(torch.bfloat16)

    def segment_max(self, msg, role):
        return self._wide(lambda m: CpuAttnGraph.segment_max(self, m, role), msg)

    def segment_min(self, msg, role):
        return self._wide(lambda m: CpuAttnGraph.segment_min(self, m, role), msg)

    def segment_softmax(self, logits, role):
        return self._wide(lambda x: CpuAttnGraph.segment_softmax(self, x, role), logits)

    def attend(self, logits, values, role):
        return self._wide(lambda l, v: CpuAttnGraph.attend(self, l, v, role), logits, values)
