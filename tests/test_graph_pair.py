"""The edge-message ops of graph.Graph (conv, pair_mul, pair_add) without a device: the public surface, the C ABI, and the
yardsticks themselves - the numpy twins of tests/_graph_pair.py against the composition they replace, and the adjoint
identities the device code relies on against float64 autograd - on the tiny hand-written padded lists of
tests/test_graph_attention.py (B = 2, N = 4, E_cap = 8; `IDX` sorted, `IDX2` scattered, a node without edges, NaN in every
pad slot)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_pair as GP  # noqa: E402
from tests.test_graph_attention import E_CAP, IDX, IDX2, N, NE  # noqa: E402
from tests.test_graph_ops_gpu import np_gather, np_segment_sum  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ("conv", "pair_mul", "pair_add")
NEW_SYMBOLS = ("lb_graph_conv", "lb_graph_pair_mul", "lb_graph_pair_add")
LISTS = {"receivers": IDX, "senders": IDX2}      # the two roles of one padded list
ROLES = ("receivers", "senders")
REAL = np.arange(E_CAP)[None, :] < NE[:, None]


def _node(shape, seed, dtype=np.float32):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def _edge(C_, seed, dtype=np.float32):
    """(B, E_cap, C) with NaN in every pad slot."""
    w = (3 * np.random.default_rng(seed).standard_normal((2, E_CAP, C_))).astype(dtype)
    w[~REAL] = np.nan
    return w


def test_graph_has_the_new_ops():
    from lagrangebench_amd.graph import Graph
    for name in NEW_OPS:
        assert callable(getattr(Graph, name, None)), name


@pytest.fixture(scope="module")
def lib():
    from lagrangebench_amd import build
    build.build()
    from lagrangebench_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from lagrangebench_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lb_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGS and hasattr(lib, name), name
        assert _lib._SIGS[name][1][-1] is C.c_int32          # the trailing dtype
        assert name + "_t" not in _lib._SIGS                  # no float32-only twin, so no _t entry either


def test_new_entries_refuse_a_null_engine(lib):
    from lagrangebench_amd import _lib
    for name in NEW_SYMBOLS:
        args = [None] + [1 if t is C.c_int32 else None for t in _lib._SIGS[name][1][1:]]
        assert getattr(lib, name)(*args) == -1, name
        assert b"null" in lib.lb_last_error()


@pytest.mark.parametrize("C_", [1, 5])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("role", ROLES)
def test_np_conv_is_the_composition_bit_for_bit(role, K, C_):
    other = GP.OTHER[role]
    x, w = _node((2, N, K, C_), 1), _edge(C_, 2)
    got = GP.np_conv(x, w, LISTS[role], LISTS[other], NE, N)
    with np.errstate(invalid="ignore"):
        msg = np_gather(x.reshape(2, N, K * C_), LISTS[other], NE).reshape(2, E_CAP, K, C_) * w[:, :, None, :]
    want = np_segment_sum(msg.reshape(2, E_CAP, K * C_), LISTS[role], NE, N).reshape(2, N, K, C_)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    empty = [(b, i) for b in range(2) for i in range(N) if not (LISTS[role][b, :NE[b]] == i).any()]
    assert (0, 2) in empty                                   # the node without edges, in either role
    for b, i in empty:
        assert (got[b, i].view(np.uint32) == 0).all()
    # pair_mul with K = 1 and pair_add are numpy indexing on the real slots, +0.0 in the pads
    a, c = _node((2, N, 1, C_), 3), _node((2, N, 1, C_), 4)
    pm = GP.np_pair_mul(a, c, LISTS["senders"], LISTS["receivers"], NE, E_CAP)
    pa = GP.np_pair_add(a[:, :, 0], c[:, :, 0], LISTS["senders"], LISTS["receivers"], NE, E_CAP)
    for b in range(2):
        s, r = LISTS["senders"][b, :NE[b]], LISTS["receivers"][b, :NE[b]]
        assert np.array_equal(pm[b, :NE[b]], a[b, s, 0] * c[b, r, 0]) and np.array_equal(pa[b, :NE[b]], a[b, s, 0] + c[b, r, 0])
    assert (pm[~REAL].view(np.uint32) == 0).all() and (pa[~REAL].view(np.uint32) == 0).all()


def _cpu_graph():
    return GP.CpuPairGraph(LISTS["senders"], LISTS["receivers"], NE, N)


@pytest.mark.parametrize("C_", [1, 5])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("role", ROLES)
def test_conv_adjoints_are_conv_with_the_role_swapped_and_pair_mul_with_the_k_sum(role, K, C_):
    other = GP.OTHER[role]
    x, w, d = _node((2, N, K, C_), 5, np.float64), _edge(C_, 6, np.float64), _node((2, N, K, C_), 7, np.float64)
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    shaped = xt if K > 1 else xt.reshape(2, N, C_)           # K = 1: the (B, N, C) form of the call
    out = _cpu_graph().conv(shaped, wt, role)
    assert np.abs(out.detach().numpy().reshape(x.shape) - GP.np_conv(x, w, LISTS[role], LISTS[other], NE, N)).max() <= 1e-12
    out.backward(torch.tensor(d).reshape(out.shape))
    d_x = GP.np_conv(d, w, LISTS[other], LISTS[role], NE, N)                        # conv(d_out, w, other(role))
    d_w = GP.np_pair_mul(x, d, LISTS[other], LISTS[role], NE, E_CAP)                # the K-reducing pair_mul
    assert np.abs(xt.grad.numpy() - d_x).max() <= 1e-12
    assert np.abs(wt.grad.numpy() - d_w).max() <= 1e-12 and not wt.grad.numpy()[~REAL].any()
    assert np.isfinite(xt.grad.numpy()).all() and np.abs(d_x).max() > 0 and np.abs(d_w).max() > 0


@pytest.mark.parametrize("C_", [1, 5])
def test_pair_adjoints_are_the_conv_pair_and_the_two_segment_sums(C_):
    a, b, d = _node((2, N, C_), 8, np.float64), _node((2, N, C_), 9, np.float64), _edge(C_, 10, np.float64)
    s_idx, r_idx = LISTS["senders"], LISTS["receivers"]
    for name in ("pair_mul", "pair_add"):
        at, bt = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
        out = getattr(_cpu_graph(), name)(at, bt)
        twin = GP.np_pair_mul(a[:, :, None], b[:, :, None], s_idx, r_idx, NE, E_CAP) if name == "pair_mul" \
            else GP.np_pair_add(a, b, s_idx, r_idx, NE, E_CAP)
        assert np.abs(out.detach().numpy() - twin).max() <= 1e-12 and not out.detach().numpy()[~REAL].any()
        out.backward(torch.tensor(d))                                               # NaN in the pad slots of the cotangent
        if name == "pair_mul":      # d_a = conv(b, d, "senders"), d_b = conv(a, d, "receivers")
            d_a = GP.np_conv(b[:, :, None], d, s_idx, r_idx, NE, N)[:, :, 0]
            d_b = GP.np_conv(a[:, :, None], d, r_idx, s_idx, NE, N)[:, :, 0]
        else:                       # the ordered sums of d over the two roles (a conv with x = 1)
            one = np.ones((2, N, 1, C_))
            d_a = GP.np_conv(one, d, s_idx, r_idx, NE, N)[:, :, 0]
            d_b = GP.np_conv(one, d, r_idx, s_idx, NE, N)[:, :, 0]
        assert np.abs(at.grad.numpy() - d_a).max() <= 1e-12 and np.abs(bt.grad.numpy() - d_b).max() <= 1e-12, name


def test_shape_and_dtype_refusals_come_before_any_device_call():
    """A Graph over a stub engine without a library: every refusal below is raised from the shapes and dtypes alone."""
    from lagrangebench_amd.graph import Graph
    engine = types.SimpleNamespace(B=2, N=N, e_cap=E_CAP, device=torch.device("cpu"), version=3)
    g = Graph(types.SimpleNamespace(engine=engine, version=3, batched=True))
    x, x4, w = torch.zeros((2, N, 5)), torch.zeros((2, N, 3, 5)), torch.zeros((2, E_CAP, 5))
    for bad_x, bad_w in ((torch.zeros((2, N, 4)), w), (torch.zeros((2, N, 3, 4)), w), (x, torch.zeros((2, E_CAP, 3, 5))),
                         (torch.zeros((2, N, 2, 3, 5)), w), (x4, torch.zeros((2, E_CAP, 5, 3)))):
        with pytest.raises(ValueError, match=re.escape(str(tuple(bad_x.shape))) + ".*" + re.escape(str(tuple(bad_w.shape)))):
            g.conv(bad_x, bad_w, "senders")
    with pytest.raises(ValueError, match="expected"):
        g.conv(torch.zeros((2, N + 1, 5)), w, "senders")
    with pytest.raises(ValueError, match="role"):
        g.conv(x, w, "nodes")
    for op in (g.pair_mul, g.pair_add):
        with pytest.raises(ValueError, match="one shape"):
            op(x, torch.zeros((2, N, 4)))
        with pytest.raises(ValueError, match="expected"):
            op(w, w)
        with pytest.raises(TypeError, match="one dtype"):
            op(x, x.to(torch.bfloat16))
        for dt in (torch.float16, torch.float64):
            with pytest.raises(TypeError, match="float32 or bfloat16"):
                op(x.to(dt), x.to(dt))
    with pytest.raises(TypeError, match="one dtype"):
        g.conv(x, w.to(torch.bfloat16), "receivers")
    with pytest.raises(TypeError, match="one dtype"):
        g.conv(x.to(torch.float16), w, "receivers")
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            g.conv(x4.to(dt), w.to(dt), "receivers")
    engine.version = 4                                       # the list moved on: the staleness rule, before any launch
    with pytest.raises(RuntimeError, match="stale"):
        g.pair_add(x, x)
