"""graph.Graph's filter_conv without a device: the numpy twins of tests/_graph_filter.py - the contracts the device tests hold
the kernels to bit for bit - against float64 torch autograd of `CpuFilterGraph`, the blocked d_f and the chunked d_weight
against the any-order summation bound, the neighbouring orders the device test must be able to tell from the contract, and the
declarations of the new library entries and constants.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_filter as GF  # noqa: E402
from tests.test_graph_vec import ROLES, _nan_pads, _random_list  # noqa: E402


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("R,C,K", [(1, 1, 1), (3, 5, 3), (20, 37, 1), (32, 18, 2)])
def test_float64_twins_equal_float64_autograd_of_the_cpu_graph(R, C, K):
    """Forward, d_x, d_f and d_weight over both roles on the small random list of tests/test_graph_vec.py: the loops of the
    contract and torch's autograd through index_select / index_add / matmul agree to 1e-12 of the largest entry in float64
    (they differ only in the order of the sums) - with the header's chunk (one chunk here) and with chunks of 16 slots (five,
    one of them real and pad slots, the last pads only)."""
    rng = np.random.default_rng(100 * R + 10 * K + C)
    B, N, E = 2, 9, 40
    ne = np.array([31, 17])
    idx = _random_list(rng, B, N, E, ne)
    x, d = rng.standard_normal((B, N, K, C)), rng.standard_normal((B, N, K, C))
    f, weight = _nan_pads(rng.standard_normal((B, E, R)), ne), rng.standard_normal((R, C))
    g = GF.CpuFilterGraph(idx["senders"], idx["receivers"], ne, N)
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), what
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-12, (what, err)

    for role in ROLES:
        other = GF.OTHER[role]
        tx, tf, tw = (torch.tensor(a, requires_grad=True) for a in (x, f, weight))
        out = g.filter_conv(tx, tf, tw, role)
        out.backward(torch.tensor(d))
        close(GF.np_filter_conv(x, f, weight, idx[role], idx[other], ne, N), out.detach(), (role, "forward"))
        close(GF.np_filter_conv(d, f, weight, idx[other], idx[role], ne, N), tx.grad, (role, "d_x"))
        for chunk in (None, 16):
            d_f, d_weight = GF.np_filter_edge_grad(x, d, f, weight, idx[role], idx[other], ne, E, chunk=chunk)
            close(d_f, tf.grad, (role, chunk, "d_f"))
            close(d_weight, tw.grad, (role, chunk, "d_weight"))
        assert all((d_f[b, ne[b]:].view(np.uint64) == 0).all() for b in range(B))     # +0.0 in the pad slots
    print(f"[graph filter twins R={R} C={C} K={K}] worst deviation / largest entry {worst:.2e}")


def _gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


@pytest.mark.parametrize("R,C,K", [(1, 1, 1), (3, 5, 3), (20, 64, 1), (32, 130, 3)])
def test_float32_blocked_d_f_and_chunked_d_weight_stay_within_the_any_order_summation_bound(R, C, K):
    """The float32 twins against float64 on the same float32 inputs.  Every elementary term x d w (or x d f) is rounded once per
    operation on its way into the result: K operations inside g (K products, K - 1 adds - K at most on the way of one product),
    one product with weight (f), and the adds of the outer sum - at most C for d_f in any order, and for d_weight at most the
    slots of a chunk plus the chunks (the adds to +0.0 counted).  So |error| <= gamma_n sum|terms| with n that count of
    roundings, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability, section 4.2: any order)."""
    rng = np.random.default_rng(7 * R + C + K)
    B, N, E = 2, 24, 300
    ne = np.array([290, 170])
    idx = _random_list(rng, B, N, E, ne)
    x, d = (rng.standard_normal((B, N, K, C)).astype(np.float32) for _ in range(2))
    f, weight = _nan_pads(rng.standard_normal((B, E, R)).astype(np.float32), ne), rng.standard_normal((R, C)).astype(np.float32)
    chunk = GF.filter_chunk()
    n_chunks = -(-B * E // chunk)
    ir, io = idx["senders"], idx["receivers"]
    got_f, got_w = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E)
    want_f, want_w = GF.np_filter_edge_grad(*(a.astype(np.float64) for a in (x, d, f, weight)), ir, io, ne, E)
    assert got_f.dtype == got_w.dtype == np.float32
    sum_w = np.zeros((R, C))
    for b in range(B):
        n = int(ne[b])
        absg = np.abs(x[b, io[b, :n]].astype(np.float64) * d[b, ir[b, :n]].astype(np.float64)).sum(1)      # (n, C): sum_k |x d|
        bound_f = _gamma(K + 1 + C) * (absg[:, None, :] * np.abs(weight.astype(np.float64))[None]).sum(-1)
        err_f = np.abs(got_f[b, :n].astype(np.float64) - want_f[b, :n])
        assert (err_f <= bound_f).all(), (b, float((err_f / bound_f).max()))
        sum_w += (np.abs(f[b, :n].astype(np.float64))[:, :, None] * absg[:, None, :]).sum(0)
    bound_w = _gamma(K + 1 + min(chunk, int(ne.sum())) + n_chunks) * sum_w
    err_w = np.abs(got_w.astype(np.float64) - want_w)
    print(f"[graph filter bound R={R} C={C} K={K}] d_weight: largest error / bound {float((err_w / bound_w).max()):.3f} "
          f"({n_chunks} chunks of {chunk})")
    assert (err_w <= bound_w).all()


def test_neighbouring_orders_give_other_bits_than_the_contract():
    """What the device test can tell apart: a twin with another chunk, a twin with another column block, and a twin whose sums
    start from their first term instead of +0.0 - that one on an input whose every term is -0.0: the contract's total is +0.0
    (+0.0 + -0.0), the first-term twin's -0.0."""
    rng = np.random.default_rng(5)
    B, N, E, K, R, C = 2, 24, 300, 2, 20, 64
    ne = np.array([290, 170])
    idx = _random_list(rng, B, N, E, ne)
    ir, io = idx["receivers"], idx["senders"]
    x, d = (rng.standard_normal((B, N, K, C)).astype(np.float32) for _ in range(2))
    f, weight = _nan_pads(rng.standard_normal((B, E, R)).astype(np.float32), ne), rng.standard_normal((R, C)).astype(np.float32)
    chunk = GF.filter_chunk()
    assert chunk in (64, 256, 1024)
    d_f, d_w = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E)
    for wrong in {64, 256, 1024, 32} - {chunk}:
        if min(wrong, chunk) >= B * E:
            continue                                           # (both are one chunk of this list)
        other_f, other_w = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E, chunk=wrong)
        assert np.array_equal(_u32(other_f), _u32(d_f)) and not np.array_equal(_u32(other_w), _u32(d_w)), wrong
    other_f, other_w = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E, block=C)
    assert not np.array_equal(_u32(other_f), _u32(d_f)) and np.array_equal(_u32(other_w), _u32(d_w))
    # every term -0.0: x = 1, d = -0.0, f = 1
    ones = np.ones((B, N, 1, C), np.float32)
    f1 = _nan_pads(np.ones((B, E, R), np.float32), ne)
    _, zero = GF.np_filter_edge_grad(ones, -0.0 * ones, f1, weight, ir, io, ne, E)
    _, first = GF.np_filter_edge_grad(ones, -0.0 * ones, f1, weight, ir, io, ne, E, from_first=True)
    assert (_u32(zero) == 0).all() and (_u32(first) == 0x80000000).all()
    # and on ordinary input the two agree (adding to +0.0 is exact), so only such an input tells them apart
    _, same = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E, from_first=True)
    assert np.array_equal(_u32(same), _u32(d_w))


def test_the_new_entries_and_constants_are_declared():
    from lagrangebench_amd import _lib, graph
    from lagrangebench_amd.engine import _GRAPH_OPS, RolloutEngine
    assert GF.header_constant("LB_GRAPH_MAX_R") == 32 == graph._MAX_R
    assert GF.filter_chunk() in (64, 256, 1024)
    header = open(GF._HEADER).read()
    table = next(v for v in vars(_lib).values()
                 if isinstance(v, dict) and "lb_graph_conv" in v and isinstance(v["lb_graph_conv"], tuple))
    for symbol, extra in (("lb_graph_filter_conv", 0), ("lb_graph_filter_conv_grad", 0)):
        assert symbol in table and symbol in _GRAPH_OPS and ("int %s(" % symbol) in header, symbol
        entry, ins, outs, sizes, _ = _GRAPH_OPS[symbol]
        assert entry == symbol and sizes[-3:] == ("K", "R", "C")                     # no float32-only twin
        assert len(table[symbol][1]) == 2 + len(ins) + len(outs) + len(sizes) + 1    # handle, role, tensors, sizes, dtype
        assert callable(getattr(RolloutEngine, symbol[3:]))
    assert "lb_graph_filter_partials" in table and "int64_t lb_graph_filter_partials(" in header
    assert callable(graph.Graph.filter_conv)
