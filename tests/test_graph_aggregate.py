"""graph.Graph.aggregate without a device: the public surface and its refusals, the C ABI, and the yardsticks themselves - the
numpy float32 twin of tests/_graph_aggregate.py against the existing twins of sum, mean, max and min (bit for bit) and against
float64 autograd of the torch restatement (to a bound derived from the number of roundings), and the three mutated twins,
which must differ from the contract twin on the planted rows.  The lists are the tiny hand-written ones of
tests/test_graph_attention.py: B = 2, N = 4, E_cap = 8, sorted and scattered, a node without edges."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_aggregate as AG  # noqa: E402
from tests import _graph_attention as GA  # noqa: E402
from tests.test_graph_attention import E_CAP, IDX, IDX2, N, NE  # noqa: E402
from tests.test_graph_ops_gpu import np_segment_sum  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lb_graph_aggregate", "lb_graph_aggregate_backward")
ULP = 2.0 ** -24
EPS = 1e-5
COLS = 4


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _inputs(idx, seed=0):
    """random values with the planted rows in the real slots and NaN in every pad slot -> (msg, {name: (b, node, slots)})"""
    msg = (3 * np.random.default_rng(seed).standard_normal((2, E_CAP, COLS))).astype(np.float32)
    return msg, AG.plant_rows(msg, idx, NE, N)


def _cpu_graph():
    """graph.Graph over a stand-in for the FeatureDict and its engine: what the surface checks before it reaches the device."""
    from lagrangebench_amd.graph import Graph
    engine = types.SimpleNamespace(B=2, N=N, e_cap=E_CAP, version=3, device=torch.device("cpu"))
    return Graph(types.SimpleNamespace(engine=engine, version=3, batched=True))


def test_surface_exists_and_refuses_bad_ops():
    from lagrangebench_amd.graph import Graph
    for name in ("aggregate", "segment_std", "segment_var"):
        assert callable(getattr(Graph, name, None)), name
    g = _cpu_graph()
    msg = torch.zeros((2, E_CAP, 3))
    for ops, eps, what in (((), 1e-5, "empty"), (("sum", "sum"), 1e-5, "twice"), (("sum", "median"), 1e-5, "unknown"),
                           (("mean", "std"), 0.0, "eps"), (("std",), -1.0, "eps")):
        with pytest.raises(ValueError, match=what):
            g.aggregate(msg, "receivers", ops, eps)
    with pytest.raises(ValueError, match="eps"):
        g.segment_std(msg, "receivers", 0.0)
    with pytest.raises(ValueError, match="role"):
        g.aggregate(msg, "nodes", ("sum",))
    # the checks of Graph._flat come next: dtype, then shape
    with pytest.raises(TypeError, match="float32"):
        g.aggregate(msg.double(), "receivers", ("var",), 0.0)     # (eps is not looked at without std)
    with pytest.raises(ValueError, match="expected"):
        g.aggregate(torch.zeros((2, E_CAP + 1, 3)), "receivers", ("sum",))


@pytest.fixture(scope="module")
def lib():
    from lagrangebench_amd import build
    build.build()
    from lagrangebench_amd import _lib
    return _lib.load()


def test_symbols_are_declared_bound_and_exported_and_refuse_a_null_engine(lib):
    from lagrangebench_amd import _lib
    from lagrangebench_amd.engine import _GRAPH_OPS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lb_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib._SIGS and hasattr(lib, name) and name in _GRAPH_OPS, name
        args = [None] + [1 if t is C.c_int32 else (1.0 if t is C.c_float else None) for t in _lib._SIGS[name][1][1:]]
        assert getattr(lib, name)(*args) == -1, name
        assert b"null" in lib.lb_last_error()


@pytest.mark.parametrize("idx", [IDX, IDX2], ids=["sorted", "scattered"])
def test_twin_equals_the_existing_twins_bit_for_bit(idx):
    msg, placed = _inputs(idx)
    assert set(placed) == {name for name, _ in AG.PLANTS}, placed
    out, win, stats = AG.np_aggregate(msg, idx, NE, N, AG.OPS, EPS)
    assert out.shape == (2, N, 6, COLS) and out.dtype == np.float32
    assert AG.same_bits(out[:, :, 0], np_segment_sum(msg, idx, NE, N))
    assert AG.same_bits(out[:, :, 1], GA.np_segment_mean(msg, idx, NE, N))
    for k, minimum in ((2, False), (3, True)):
        want, w = GA.np_segment_max(msg, idx, NE, N, minimum)
        assert AG.same_bits(out[:, :, k], want) and np.array_equal(win[:, :, k - 2], w)
    # the order of ops is the order of the planes; single ops are the planes
    perm = ("std", "max", "sum", "min", "mean", "var")
    out2, _, _ = AG.np_aggregate(msg, idx, NE, N, perm, EPS)
    for a, op in enumerate(perm):
        assert AG.same_bits(out2[:, :, a], out[:, :, AG.OPS.index(op)])
        assert AG.same_bits(AG.np_aggregate(msg, idx, NE, N, (op,), EPS)[0][:, :, 0], out2[:, :, a])
    # single-op gradients of sum, mean, max, min: gather, gather / degree, the winner's
    d_out = np.random.default_rng(5).standard_normal((2, N, 1, COLS)).astype(np.float32)
    deg = np.maximum(GA.np_degree(idx, NE, N), 1).astype(np.float32)[..., None]
    for op, want in (("sum", d_out[:, :, 0]), ("mean", (d_out[:, :, 0] / deg).astype(np.float32))):
        d = AG.np_aggregate_backward(d_out, msg, win, stats, idx, NE, (op,))
        for b in range(2):
            assert np.array_equal(_bits(d[b, :NE[b]]), _bits(want[b, idx[b, :NE[b]]])) and not _bits(d[b, NE[b]:]).any()
    for k, op in ((0, "max"), (1, "min")):
        d = AG.np_aggregate_backward(d_out, msg, win, stats, idx, NE, (op,))
        assert np.array_equal(_bits(d), _bits(GA.np_segment_max_backward(d_out[:, :, 0], win[:, :, k], idx, NE, E_CAP)))
    # ---- what the planted rows say
    b, i, s = placed["equal"]
    assert not _bits(out[b, i, 5]).any()                                      # var exactly +0.0
    assert np.array_equal(_bits(out[b, i, 4]), _bits(np.full(COLS, np.sqrt(np.float32(EPS)), np.float32)))
    d = AG.np_aggregate_backward(np.ones((2, N, 1, COLS), np.float32), msg, win, stats, idx, NE, ("std",))
    assert not d[b, s].any()                                                  # its std gradient exactly 0
    b, i, s = placed["deg1"]
    assert len(s) == 1 and not _bits(out[b, i, 5]).any() and (out[b, i, 4] == np.sqrt(np.float32(EPS))).all()
    b, i, s = placed["zeros"]
    assert np.signbit(out[b, i, 2, 0]) and np.signbit(out[b, i, 3, 1]) and win[b, i, 0, 0] == s[0] and win[b, i, 1, 1] == s[0]
    b, i, s = placed["tie"]
    assert (win[b, i, 0, 0::2] == s[0]).all() and (win[b, i, 1, 1::2] == s[0]).all() and (out[b, i, 2, 0::2] == 64).all()
    b, i, s = placed["nan"]
    assert np.isnan(out[b, i]).all()
    empty = GA.np_degree(idx, NE, N) == 0
    assert empty.sum() >= 1 and not _bits(out[empty]).any() and (win[empty] == -1).all() and not _bits(stats[empty]).any()
    assert np.isnan(out).sum() == 6 * COLS                                    # the pads' NaN reached nothing: only "nan"'s row


@pytest.mark.parametrize("idx", [IDX, IDX2], ids=["sorted", "scattered"])
def test_twin_agrees_with_float64_autograd(idx):
    """The bound, from the roundings (u = 2^-24, d <= 4 slots a node, X = max(1, max|x|), so |t| <= 2 X):
    the sum takes d - 1 adds and the mean one division: |m - m64| <= d u X; t = x - m adds one rounding and inherits the mean's
    error: |t - t64| <= (d + 2) u X; q is d products and d - 1 adds of terms <= 4 X^2 that each inherit 2 |t| |dt|:
    |q - q64| <= d (4 (d + 2) + 4 d) u X^2; var adds a division, std an add and a root (derivative <= 1 / (2 sqrt(eps))).  The
    comparison runs at eps = 1, where the root and 1 / std amplify nothing; then every plane is within F = (8 d^2 + 8 d + 4) u X^2.
    A backward term is a cotangent (|g| <= G) times a quantity that is within F, or the quotient of two such, and takes at most
    3 further roundings: within G (2 F + 3 u X^2); six terms of size <= 2 G X and five adds of partial sums <= 12 G X^2 give
    G (12 F + (18 + 60) u X^2).  (At eps = 1e-5 the factor 1 / sqrt(eps) = 316 on t / std makes a derived bound useless on rows
    that are nearly equal; there the bits are what the device tests hold.)"""
    eps = 1.0
    rng = np.random.default_rng(11)
    msg = rng.standard_normal((2, E_CAP, COLS)).astype(np.float32)    # no planted rows: ties share the gradient in torch
    for b in range(2):
        msg[b, NE[b]:] = np.nan
    ops = ("std", "max", "sum", "min", "mean", "var")
    out, win, stats = AG.np_aggregate(msg, idx, NE, N, ops, eps)
    d_out = rng.standard_normal(out.shape).astype(np.float32)
    d = AG.np_aggregate_backward(d_out, msg, win, stats, idx, NE, ops)
    g = AG.CpuAggGraph(idx, idx, NE, N)
    xt = torch.tensor(np.nan_to_num(msg), dtype=torch.float64, requires_grad=True)
    o64 = g.aggregate(xt, "senders", ops, eps)
    (o64 * torch.tensor(d_out, dtype=torch.float64)).sum().backward()
    real = np.arange(E_CAP)[None, :] < NE[:, None]
    top = max(1.0, float(np.abs(msg[real]).max()))
    deg = 4
    fwd = np.abs(out - o64.detach().numpy()).max()
    bwd = np.abs(d[real] - xt.grad.numpy()[real]).max()
    coef = 8 * deg * deg + 8 * deg + 4
    fwd_bound = coef * ULP * top ** 2
    bwd_bound = (12 * coef + 78) * ULP * float(np.abs(d_out).max()) * top ** 2
    print(f"[aggregate twin vs float64] forward {fwd:.2e} (bound {fwd_bound:.2e}); backward {bwd:.2e} (bound {bwd_bound:.2e})")
    assert fwd <= fwd_bound and bwd <= bwd_bound
    assert not _bits(d[~real]).any()
    # segment_std / segment_var of the restatement are its planes
    assert torch.equal(g.segment_std(xt, "senders", eps), o64[:, :, 0]) and torch.equal(g.segment_var(xt, "senders"), o64[:, :, 5])


@pytest.mark.parametrize("idx", [IDX, IDX2], ids=["sorted", "scattered"])
def test_each_mutant_differs_on_a_planted_row(idx):
    msg, placed = _inputs(idx)
    out, win, stats = AG.np_aggregate(msg, idx, NE, N, AG.OPS, EPS)
    d_out = np.ones(out.shape, np.float32)
    d = AG.np_aggregate_backward(d_out, msg, win, stats, idx, NE, AG.OPS)
    where = {"one_pass": "big", "late_ties": "tie", "eps_outside": "equal"}
    for mutant in AG.MUTANTS:
        out_m, win_m, stats_m = AG.np_aggregate(msg, idx, NE, N, AG.OPS, EPS, mutant)
        d_m = AG.np_aggregate_backward(d_out, msg, win_m, stats_m, idx, NE, AG.OPS)
        b, i, s = placed[where[mutant]]
        differs = not AG.same_bits(out_m[b, i], out[b, i]) or not np.array_equal(win_m[b, i], win[b, i]) \
            or not AG.same_bits(d_m[b, s], d[b, s])
        assert differs, mutant
    # ... and each in its own way: the one-pass variance has no correct digit on the big row (off by half the variance or more)
    b, i, s = placed["big"]
    one = AG.np_aggregate(msg, idx, NE, N, ("var",), EPS, "one_pass")[0][b, i, 0]
    exact = np.var(msg[b, s].astype(np.float64), 0)
    assert np.abs(out[b, i, 5] - exact).max() <= 4 * ULP * exact.max() and np.abs(one - exact).max() >= 0.5 * exact.max()
    b, i, s = placed["tie"]
    late = AG.np_aggregate(msg, idx, NE, N, ("max", "min"), EPS, "late_ties")[1]
    assert (late[b, i, 0, 0::2] == s[1]).all() and (late[b, i, 1, 1::2] == s[1]).all()
    b, i, s = placed["equal"]
    outside = AG.np_aggregate(msg, idx, NE, N, ("std",), EPS, "eps_outside")[0][b, i, 0]
    assert (outside == np.float32(EPS)).all() and (out[b, i, 4] == np.sqrt(np.float32(EPS))).all()
