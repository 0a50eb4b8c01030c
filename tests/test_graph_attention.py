"""The attention ops of graph.Graph without a device: the public surface, the C ABI, and the yardsticks themselves - the numpy
and float64 restatements of tests/_graph_attention.py against torch.softmax, torch.amax and autograd on a tiny hand-written
padded list (B = 2, N = 4; a node with a single edge, a node without one, a planted tie, NaN in every pad slot)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_attention as GA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ("degree", "segment_mean", "segment_max", "segment_min", "segment_softmax", "attend")
NEW_SYMBOLS = ("lb_graph_degree", "lb_graph_segment_max", "lb_graph_segment_min", "lb_graph_segment_max_backward",
               "lb_graph_segment_softmax", "lb_graph_segment_softmax_backward", "lb_graph_attend", "lb_graph_attend_backward")

N, E_CAP = 4, 8
# receivers of the slots (pad slots hold N): trajectory 0 - node 0 three edges, node 1 one edge, node 2 none, node 3 two;
# trajectory 1 - node 0 none, node 1 four, node 2 one, node 3 two
IDX = np.array([[0, 0, 0, 1, 3, 3, N, N], [1, 1, 1, 1, 2, 3, 3, N]])
NE = np.array([6, 7])
# a second role on the same slots, not sorted: the slots of a node are not contiguous
IDX2 = np.array([[3, 1, 0, 0, 1, 0, N, N], [2, 3, 1, 0, 1, 3, 1, N]])


def _inputs(C_, seed=0):
    rng = np.random.default_rng(seed)
    x = (3 * rng.standard_normal((2, E_CAP, C_))).astype(np.float32)
    x[0, 1, 0] = x[0, 0, 0]                      # a tie inside node 0's row (receivers), column 0
    for b in range(2):
        x[b, NE[b]:] = np.nan
    return x


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


def test_new_entries_refuse_a_null_engine(lib):
    from lagrangebench_amd import _lib
    for name in NEW_SYMBOLS:
        args = [None] + [1 if t is C.c_int32 else None for t in _lib._SIGS[name][1][1:]]
        assert getattr(lib, name)(*args) == -1, name
        assert b"null" in lib.lb_last_error()


@pytest.mark.parametrize("idx", [IDX, IDX2], ids=["sorted", "scattered"])
def test_extrema_restatement_against_torch_amax(idx):
    x = _inputs(3)
    assert GA.np_degree(idx, NE, N).tolist() == [[int((idx[b, :NE[b]] == i).sum()) for i in range(N)] for b in range(2)]
    for minimum, red in ((False, torch.amax), (True, torch.amin)):
        out, win = GA.np_segment_max(x, idx, NE, N, minimum)
        for b in range(2):
            for i in range(N):
                slots = np.flatnonzero(idx[b, :NE[b]] == i)
                if len(slots) == 0:
                    assert (win[b, i] == -1).all() and (out[b, i].view(np.uint32) == 0).all()
                    continue
                assert np.array_equal(out[b, i], red(torch.tensor(x[b, slots]), 0).numpy())
                assert np.array_equal(x[b, win[b, i], np.arange(3)], out[b, i]) and np.isin(win[b, i], slots).all()
        # the gradient: autograd's where no slot ties, all of it to the winner
        d_out = np.random.default_rng(1).standard_normal((2, N, 3)).astype(np.float32)
        d = GA.np_segment_max_backward(d_out, win, idx, NE, E_CAP)
        xt = torch.tensor(np.nan_to_num(x), dtype=torch.float64, requires_grad=True)
        g = GA.CpuAttnGraph(idx, idx, NE, N)
        ((g.segment_min if minimum else g.segment_max)(xt, "senders") * torch.tensor(d_out, dtype=torch.float64)).sum().backward()
        auto = xt.grad.numpy()
        tied = np.zeros(x.shape, bool)
        if idx is IDX:
            tied[0, :2, 0] = True
        assert np.array_equal(d[~tied], auto[~tied].astype(np.float32))
        assert (d[0, NE[0]:].view(np.uint32) == 0).all() and (d[1, NE[1]:].view(np.uint32) == 0).all()
    if idx is IDX:   # first wins: the tie's gradient goes to slot 0, whichever way the comparison runs
        for minimum in (False, True):
            xs = _inputs(3)
            xs[0, :2, 0] = 100.0 * (-1 if minimum else 1)
            out, win = GA.np_segment_max(xs, idx, NE, N, minimum)
            assert win[0, 0, 0] == 0
            d = GA.np_segment_max_backward(np.ones((2, N, 3), np.float32), win, idx, NE, E_CAP)
            assert d[0, 0, 0] == 1 and d[0, 1, 0] == 0
    # -0.0 then +0.0 stays -0.0; a NaN in a real slot wins and stays
    z = np.zeros((2, E_CAP, 1), np.float32)
    z[0, 0, 0], z[1, 1, 0] = -0.0, np.nan
    out, win = GA.np_segment_max(z, IDX, NE, N)
    assert np.signbit(out[0, 0, 0]) and win[0, 0, 0] == 0 and np.isnan(out[1, 1, 0]) and win[1, 1, 0] == 1
    mean = GA.np_segment_mean(x, idx, NE, N)
    want = GA.CpuAttnGraph(idx, idx, NE, N).segment_mean(torch.tensor(x, dtype=torch.float64), "senders").numpy()
    assert np.abs(mean - want).max() <= 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("idx", [IDX, IDX2], ids=["sorted", "scattered"])
def test_softmax_and_attend_restatements_against_torch(idx):
    H, D = 3, 2
    x = _inputs(H)
    x[:, :, 1] += 1e4                                     # overflows without the shift
    v = np.random.default_rng(2).standard_normal((2, E_CAP, H, D)).astype(np.float32)
    for b in range(2):
        v[b, NE[b]:] = np.nan
    y = GA.softmax64(x, idx, NE, N)
    out = GA.attend64(x, v, idx, NE, N)
    d_y = np.random.default_rng(3).standard_normal(y.shape)
    d_out = np.random.default_rng(4).standard_normal(out.shape)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    rows_y, rows_out = [], []
    for b in range(2):
        assert np.array_equal(y[b, NE[b]:], np.zeros_like(y[b, NE[b]:]))
        for i in range(N):
            slots = torch.tensor(np.flatnonzero(idx[b, :NE[b]] == i))
            if len(slots) == 0:
                assert not out[b, i].any()
                continue
            a = torch.softmax(xt[b, slots], 0)                      # torch's own, per node
            assert np.abs(y[b, slots.numpy()] - a.detach().numpy()).max() <= 1e-14
            o = (a[..., None] * vt[b, slots]).sum(0)
            assert np.abs(out[b, i] - o.detach().numpy()).max() <= 1e-13
            rows_y.append((a * torch.tensor(d_y[b, slots.numpy()])).sum())
            rows_out.append((o * torch.tensor(d_out[b, i])).sum())
    assert len(rows_y) == (6 if idx is IDX else 7) and np.isfinite(y).all() and np.isfinite(out).all()
    (g_soft,) = torch.autograd.grad(sum(rows_y), xt, retain_graph=True)
    g_l, g_v = torch.autograd.grad(sum(rows_out), (xt, vt))
    real = np.arange(E_CAP)[None, :] < NE[:, None]
    assert np.abs(GA.softmax_backward64(y, d_y, idx, NE, N)[real] - g_soft.numpy()[real]).max() <= 1e-13
    d_l, d_v, scale = GA.attend_backward64(x, v, d_out, idx, NE, N)
    assert np.abs(d_l[real] - g_l.numpy()[real]).max() <= 1e-13 and np.abs(d_v[real] - g_v.numpy()[real]).max() <= 1e-13
    assert not d_l[~real].any() and not d_v[~real].any() and scale > 0
    # the differentiable CPU graph the model tests use says the same, gradients included
    cg = GA.CpuAttnGraph(idx, idx, NE, N)
    x2, v2 = xt.detach().clone().requires_grad_(), vt.detach().clone().requires_grad_()
    o2 = cg.attend(x2, v2, "receivers")
    assert np.abs(o2.detach().numpy() - out).max() <= 1e-13
    assert np.abs(cg.segment_softmax(x2, "receivers").detach().numpy() - y).max() <= 1e-14
    (o2 * torch.tensor(d_out)).sum().backward()
    assert np.abs(x2.grad.numpy()[real] - d_l[real]).max() <= 1e-13 and np.abs(v2.grad.numpy()[real] - d_v[real]).max() <= 1e-13
    assert np.isfinite(x2.grad.numpy()).all() and np.isfinite(v2.grad.numpy()).all()
