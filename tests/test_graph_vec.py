"""graph.Graph's vector-message ops without a device: the numpy twins of tests/_graph_vec.py - the contracts the device tests
hold the kernels to bit for bit - against float64 torch autograd of `CpuVecGraph`, the blocked d_u order against the
any-order summation bound, and the declarations of the three new library entries.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_vec as GV  # noqa: E402

ROLES = ("receivers", "senders")


def _random_list(rng, B, N, E, ne):
    """A padded list in canonical (receiver, sender) order without self edges or duplicates; some nodes have no edge; not
    symmetric, so the two roles walk different rows."""
    idx = {r: np.full((B, E), N, np.int64) for r in ROLES}
    for b in range(B):
        pairs = np.array([(r, s) for r in range(N - 2) for s in range(N) if r != s])
        take = np.sort(rng.choice(len(pairs), ne[b], replace=False))
        idx["receivers"][b, :ne[b]], idx["senders"][b, :ne[b]] = pairs[take, 0], pairs[take, 1]
    return idx


def _nan_pads(a, ne):
    a = a.copy()
    for b in range(a.shape[0]):
        a[b, ne[b]:] = np.nan
    return a


@pytest.mark.parametrize("K,C", [(1, 1), (3, 5), (5, 37)])
def test_float64_twins_equal_float64_autograd_of_the_cpu_graph(K, C):
    """Forward, d_x / d_v, d_w and d_u of both ops over both roles: the loops of the contract and torch's autograd through
    index_select / index_add agree to 1e-12 of the largest entry in float64 (they differ only in the order of the sums)."""
    rng = np.random.default_rng(10 * K + C)
    B, N, E = 2, 9, 40
    ne = np.array([31, 17])
    idx = _random_list(rng, B, N, E, ne)
    x, v = rng.standard_normal((B, N, C)), rng.standard_normal((B, N, K, C))
    w, u = _nan_pads(rng.standard_normal((B, E, C)), ne), _nan_pads(rng.standard_normal((B, E, K)), ne)
    dv, ds = rng.standard_normal((B, N, K, C)), rng.standard_normal((B, N, C))
    g = GV.CpuVecGraph(idx["senders"], idx["receivers"], ne, N)
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), what
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-12, (what, err)

    for role in ROLES:
        other = GV.OTHER[role]
        # ---- conv_vec
        tx, tw, tu = (torch.tensor(a, requires_grad=True) for a in (x, w, u))
        out = g.conv_vec(tx, tw, tu, role)
        out.backward(torch.tensor(dv))
        close(GV.np_conv_vec(x, w, u, idx[role], idx[other], ne, N), out.detach(), (role, "conv_vec"))
        close(GV.np_conv_dot(dv, w, u, idx[other], idx[role], ne, N), tx.grad, (role, "conv_vec d_x"))
        d_w, d_u = GV.np_vec_edge_grad(x, dv, w, u, idx[other], idx[role], ne, E)
        close(d_w, tw.grad, (role, "conv_vec d_w"))
        close(d_u, tu.grad, (role, "conv_vec d_u"))
        # ---- conv_dot
        tv, tw, tu = (torch.tensor(a, requires_grad=True) for a in (v, w, u))
        out = g.conv_dot(tv, tw, tu, role)
        out.backward(torch.tensor(ds))
        close(GV.np_conv_dot(v, w, u, idx[role], idx[other], ne, N), out.detach(), (role, "conv_dot"))
        close(GV.np_conv_vec(ds, w, u, idx[other], idx[role], ne, N), tv.grad, (role, "conv_dot d_v"))
        d_w, d_u = GV.np_vec_edge_grad(ds, v, w, u, idx[role], idx[other], ne, E)
        close(d_w, tw.grad, (role, "conv_dot d_w"))
        close(d_u, tu.grad, (role, "conv_dot d_u"))
        for a in (d_w, d_u):                                 # +0.0 in the pad slots
            assert all((a[b, ne[b]:].view(np.uint64) == 0).all() for b in range(B))
    print(f"[graph vec twins K={K} C={C}] worst deviation / largest entry {worst:.2e}")


@pytest.mark.parametrize("C", [1, 5, 16, 17, 130, 520])
def test_float32_blocked_d_u_stays_within_the_any_order_summation_bound(C):
    """The float32 twin of d_u - blocks of LB_GRAPH_DU_BLOCK columns, then the block sums - against float64 on the same float32
    inputs: any order of n - 1 adds of n rounded terms stays within (n + 1) 2^-24 sum|terms| to first order (two roundings per
    term, at most n - 1 adds on the way of any term)."""
    rng = np.random.default_rng(C)
    B, N, E, K = 1, 6, 24, 3
    ne = np.array([20])
    idx = _random_list(rng, B, N, E, ne)
    s = rng.standard_normal((B, N, C)).astype(np.float32)
    v = rng.standard_normal((B, N, K, C)).astype(np.float32)
    w = _nan_pads(rng.standard_normal((B, E, C)).astype(np.float32), ne)
    u = _nan_pads(rng.standard_normal((B, E, K)).astype(np.float32), ne)
    assert GV.du_block() == 16
    _, got = GV.np_vec_edge_grad(s, v, w, u, idx["senders"], idx["receivers"], ne, E)
    _, want = GV.np_vec_edge_grad(*(a.astype(np.float64) for a in (s, v, w, u)), idx["senders"], idx["receivers"], ne, E)
    assert got.dtype == np.float32
    n = int(ne[0])
    sg, vg = s[0, idx["senders"][0, :n]].astype(np.float64), v[0, idx["receivers"][0, :n]].astype(np.float64)
    terms = np.abs(sg[:, None, :] * w[0, :n, None, :].astype(np.float64) * vg).sum(-1)
    bound = (C + 1) * 2.0 ** -24 * terms
    err = np.abs(got[0, :n].astype(np.float64) - want[0, :n])
    print(f"[graph vec d_u C={C}] largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # the blocking is what is stated: one plain loop over c gives other bits once a later block has two columns to add first
    # (at C = 17 the two orders are the same sequence of adds)
    if C > 17:
        _, other = GV.np_vec_edge_grad(s, v, w, u, idx["senders"], idx["receivers"], ne, E, block=C)
        assert not np.array_equal(other.view(np.uint32), got.view(np.uint32))


def test_the_new_entries_are_declared():
    from lagrangebench_amd import _lib
    from lagrangebench_amd.engine import _GRAPH_OPS, RolloutEngine
    from lagrangebench_amd.graph import Graph
    table = next(v for v in vars(_lib).values()
                 if isinstance(v, dict) and "lb_graph_conv" in v and isinstance(v["lb_graph_conv"], tuple))
    for symbol in ("lb_graph_conv_vec", "lb_graph_conv_dot", "lb_graph_conv_vec_edge_grad"):
        assert symbol in table and symbol in _GRAPH_OPS, symbol
        assert _GRAPH_OPS[symbol][0] == symbol and _GRAPH_OPS[symbol][3] == ("K", "C")       # no float32-only twin
        assert len(table[symbol][1]) == 2 + len(_GRAPH_OPS[symbol][1]) + len(_GRAPH_OPS[symbol][2]) + 3
        assert callable(getattr(RolloutEngine, symbol[3:]))
    assert callable(Graph.conv_vec) and callable(Graph.conv_dot)
