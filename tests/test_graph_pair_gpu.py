"""graph.Graph's edge-message ops on the device (csrc/lb_graph.hip): conv, pair_mul and pair_add, forward and backward, against
the numpy loops of tests/_graph_pair.py - bit for bit: the order of every sum is part of the contract, so there is no
tolerance here - and, for conv, against this library's own segment_sum(gather * w), which it replaces.

Cases, columns and roles are those of tests/test_graph_ops_gpu.py (B = 2 behind pads, more than one workgroup of rows, N = 3
with rows shorter than a wave, the radix-sorted sender view of the asymmetric list; 1 and 5 columns on the scalar kernels, 64
on 16-byte units, 130 with several units per lane), with K in {1, 3}: K = 3 at C = 130 is the shape where a unit must not
cross a k boundary.  Every pad slot of w and of every edge-shaped cotangent holds NaN.

The composition's d_w at K > 1 is spelled out as gather * gather added k by k: autograd's own reduction of the broadcast w
has no stated order.  bfloat16: round_to_bf16(the float32 twin(upcast inputs)) bit for bit, with the rounding of
tests/_graph_bf16.py.  The model path (TinyConv in models.TorchModel) uses the two-step rule of tests/test_torch_model_gpu.py
unchanged.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_bf16 as BF  # noqa: E402
from tests import _graph_pair as GP  # noqa: E402
from tests.test_graph_ops_gpu import CASES, COLUMNS, ROLES, _build, _setup, np_gather, np_segment_sum  # noqa: E402

pytestmark = pytest.mark.gpu

KS = [1, 3]
# 8-element units need C % 8 == 0: 64 and 520 (65 units, past a row's 64 lanes) take them, the others the scalar path
BF16_COLUMNS = [5, 64, 130, 520]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _nan_pads(a, ne):
    a = a.copy()
    for b in range(a.shape[0]):
        a[b, ne[b]:] = np.nan
    return a


def _pads_are_zero(a, ne, view=np.uint32):
    return all((np.ascontiguousarray(a[b, ne[b]:]).view(view) == 0).all() for b in range(a.shape[0]))


def _edge(rng, B, E, C, ne):
    """(B, E_cap, C) float32 over seven decades, NaN in every pad slot."""
    return _nan_pads((rng.standard_normal((B, E, C)) * 10.0 ** rng.integers(-3, 4, (B, E, 1))).astype(np.float32), ne)


def _dev(a, eng, grad=False):
    return torch.tensor(a, device=eng.device, requires_grad=grad)


def _case(cid):
    """_setup(cid) of tests/test_graph_ops_gpu.py.  Its cache is shared by every test file that imports it, and a test of
    another file may have built a new list on a cached engine since: such features are stale, and the cases are built anew."""
    got = _setup(cid)
    if got[0].version != got[1].version:
        _setup.cache_clear()
        got = _setup(cid)
    return got


# ------------------------------------------------------------------------------------------------ conv, float32
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_conv_equals_numpy_and_the_composition_bit_for_bit(cid, C, K):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, pairs, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(1000 * C + 10 * K + len(cid))
    x = rng.standard_normal((B, N, K, C)).astype(np.float32)
    w = _edge(rng, B, E, C, ne)
    d = rng.standard_normal((B, N, K, C)).astype(np.float32)
    shape = (B, N, K, C) if K > 1 else (B, N, C)            # K = 1: the (B, N, C) form of the call
    for role in ROLES:
        other = GP.OTHER[role]
        xd, wd = _dev(x.reshape(shape), eng, True), _dev(w, eng, True)
        out = g.conv(xd, wd, role)
        assert out.shape == shape and out.dtype == torch.float32
        out.backward(_dev(d.reshape(shape), eng))
        got, got_dx, got_dw = _np(out).reshape(x.shape), _np(xd.grad).reshape(x.shape), _np(wd.grad)
        assert np.isfinite(got).all() and np.isfinite(got_dx).all() and np.isfinite(got_dw).all(), (cid, role, C, K)
        # ---- the numpy loops
        assert _same(got, GP.np_conv(x, w, idx[role], idx[other], ne, N)), (cid, role, C, K, "forward")
        assert _same(got_dx, GP.np_conv(d, w, idx[other], idx[role], ne, N)), (cid, role, C, K, "d_x")
        assert _same(got_dw, GP.np_pair_mul(x, d, idx[other], idx[role], ne, E)), (cid, role, C, K, "d_w")
        assert got_dw.shape == (B, E, C) and _pads_are_zero(got_dw, ne)
        # ---- this library's own segment_sum(gather * w): forward and d_x through autograd, d_w added k by k
        x2, w2 = _dev(x, eng, True), _dev(w, eng)
        comp = g.segment_sum(g.gather(x2, other) * w2[:, :, None, :], role)
        comp.backward(_dev(d, eng))
        assert _same(_np(comp), got) and _same(_np(x2.grad), got_dx), (cid, role, C, K, "composition")
        gx, gd = g.gather(_dev(x, eng), other), g.gather(_dev(d, eng), role)
        comp_dw = gx[:, :, 0] * gd[:, :, 0]
        for k in range(1, K):
            comp_dw = comp_dw + gx[:, :, k] * gd[:, :, k]
        assert _same(_np(comp_dw), got_dw), (cid, role, C, K, "composition d_w")
        # ---- a second call: the same bits
        x3, w3 = _dev(x.reshape(shape), eng, True), _dev(w, eng, True)
        again = g.conv(x3, w3, role)
        again.backward(_dev(d.reshape(shape), eng))
        assert _same(_np(again).reshape(x.shape), got) and _same(_np(x3.grad).reshape(x.shape), got_dx) and _same(_np(w3.grad), got_dw)
    if pairs is not None:
        assert eng.graph_sender_sorts() >= 1


def test_conv_skips_the_gradient_nobody_asked_for_and_folds_trailing_dimensions():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("rpf2d_b2")
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, N, 3, 4)).astype(np.float32)
    w = _edge(rng, B, E, 12, ne).reshape(B, E, 3, 4)
    calls = []
    conv, pair = eng.graph_conv, eng.graph_pair_mul
    eng.graph_conv = lambda *a: (calls.append("conv"), conv(*a))[1]
    eng.graph_pair_mul = lambda *a: (calls.append("pair_mul"), pair(*a))[1]
    try:
        xd, wd = _dev(x, eng, True), _dev(w, eng)
        out = g.conv(xd, wd, "senders")                      # equal trailing dimensions: K = 1, C = 12
        out.sum().backward()
        assert calls == ["conv", "conv"] and wd.grad is None
        calls.clear()
        xd, wd = _dev(x, eng), _dev(w, eng, True)
        g.conv(xd, wd, "senders").sum().backward()
        assert calls == ["conv", "pair_mul"] and xd.grad is None and wd.grad.shape == w.shape
    finally:
        del eng.graph_conv, eng.graph_pair_mul
    want = GP.np_conv(x.reshape(B, N, 1, 12), w.reshape(B, E, 12), idx["senders"], idx["receivers"], ne, N)
    assert out.shape == x.shape and _same(_np(out).reshape(want.shape), want)
    # (B, N, 1, C) with w (B, E_cap, C): K = 1 by the second rule
    x1 = rng.standard_normal((B, N, 1, 12)).astype(np.float32)
    got = g.conv(_dev(x1, eng), _dev(w.reshape(B, E, 12), eng), "receivers")
    assert got.shape == x1.shape
    assert _same(_np(got), GP.np_conv(x1, w.reshape(B, E, 12), idx["receivers"], idx["senders"], ne, N))


# ------------------------------------------------------------------------------------------------ pair_mul, pair_add, float32
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_pair_mul_and_pair_add_equal_numpy_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(77 * C + len(cid))
    a = (rng.standard_normal((B, N, C)) * 10.0 ** rng.integers(-3, 4, (B, N, 1))).astype(np.float32)
    b = rng.standard_normal((B, N, C)).astype(np.float32)
    d = _edge(rng, B, E, C, ne)
    s_idx, r_idx = idx["senders"], idx["receivers"]
    a4, b4 = a[:, :, None], b[:, :, None]
    want = {"pair_mul": (GP.np_pair_mul(a4, b4, s_idx, r_idx, ne, E),
                         GP.np_conv(b4, d, s_idx, r_idx, ne, N)[:, :, 0],           # d_a = conv(b, d, "senders")
                         GP.np_conv(a4, d, r_idx, s_idx, ne, N)[:, :, 0]),          # d_b = conv(a, d, "receivers")
            "pair_add": (GP.np_pair_add(a, b, s_idx, r_idx, ne, E),
                         np_segment_sum(d, s_idx, ne, N), np_segment_sum(d, r_idx, ne, N))}
    assert _same(want["pair_add"][0], np_gather(a, s_idx, ne) + np_gather(b, r_idx, ne))
    for name in ("pair_mul", "pair_add"):
        runs = []
        for _ in range(2):
            ad, bd = _dev(a, eng, True), _dev(b, eng, True)
            out = getattr(g, name)(ad, bd)
            assert out.shape == (B, E, C) and out.dtype == torch.float32
            out.backward(_dev(d, eng))
            runs.append((_np(out), _np(ad.grad), _np(bd.grad)))
        for got, exp, what in zip(runs[0], want[name], ("forward", "d_a", "d_b")):
            assert np.isfinite(got).all() and _same(got, exp), (cid, C, name, what)
        assert _pads_are_zero(runs[0][0], ne)
        assert all(_same(p, q) for p, q in zip(runs[0], runs[1])), (cid, C, name, "second call")
    # one operand without a gradient: the other's arrives alone
    ad, bd = _dev(a, eng), _dev(b, eng, True)
    g.pair_mul(ad, bd).backward(_dev(d, eng))
    assert ad.grad is None and _same(_np(bd.grad), want["pair_mul"][2])


# ------------------------------------------------------------------------------------------------ bfloat16
def _bf(a):
    """float32 -> (its bfloat16 bits, the float32 values they hold); a NaN stays a NaN."""
    bits = BF.round_bf16(a)
    return bits, BF.widen(bits)


def _rb(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return BF.round_bf16(a)


@pytest.mark.parametrize("C", BF16_COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_bfloat16_is_the_rounded_float32_op_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(31 * C + len(cid))
    s_idx, r_idx = idx["senders"], idx["receivers"]
    w_bits, w = _bf(_edge(rng, B, E, C, ne))
    for K in KS:
        x_bits, x = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        d_bits, d = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        shape = (B, N, K, C) if K > 1 else (B, N, C)
        for role in ROLES:
            other = GP.OTHER[role]
            xd = BF.from_bits(x_bits.reshape(shape), eng.device, True)
            wd = BF.from_bits(w_bits, eng.device, True)
            out = g.conv(xd, wd, role)
            assert out.dtype == torch.bfloat16 and out.shape == shape
            out.backward(BF.from_bits(d_bits.reshape(shape), eng.device))
            got, got_dx, got_dw = BF.torch_bits(out), BF.torch_bits(xd.grad), BF.torch_bits(wd.grad)
            assert xd.grad.dtype == torch.bfloat16 and wd.grad.dtype == torch.bfloat16
            assert BF.same_bits(got.reshape(x.shape), _rb(GP.np_conv(x, w, idx[role], idx[other], ne, N))), (cid, role, C, K)
            assert BF.same_bits(got_dx.reshape(x.shape), _rb(GP.np_conv(d, w, idx[other], idx[role], ne, N))), (cid, role, C, K)
            assert BF.same_bits(got_dw, _rb(GP.np_pair_mul(x, d, idx[other], idx[role], ne, E))), (cid, role, C, K)
            assert _pads_are_zero(got_dw, ne, np.uint16)
            for bits in (got, got_dx, got_dw):
                assert np.isfinite(BF.widen(bits)).all()
    # ---- pair_mul and pair_add: torch's bfloat16 arithmetic on the gathered rows
    a_bits, a = _bf(rng.standard_normal((B, N, C)).astype(np.float32))
    b_bits, b = _bf((3 * rng.standard_normal((B, N, C))).astype(np.float32))
    e_bits, e = w_bits, w                                    # the edge-shaped cotangent, NaN in the pads
    a4, b4 = a[:, :, None], b[:, :, None]
    want = {"pair_mul": (GP.np_pair_mul(a4, b4, s_idx, r_idx, ne, E), GP.np_conv(b4, e, s_idx, r_idx, ne, N)[:, :, 0],
                         GP.np_conv(a4, e, r_idx, s_idx, ne, N)[:, :, 0]),
            "pair_add": (GP.np_pair_add(a, b, s_idx, r_idx, ne, E), np_segment_sum(e, s_idx, ne, N), np_segment_sum(e, r_idx, ne, N))}
    for name in ("pair_mul", "pair_add"):
        ad, bd = BF.from_bits(a_bits, eng.device, True), BF.from_bits(b_bits, eng.device, True)
        out = getattr(g, name)(ad, bd)
        assert out.dtype == torch.bfloat16
        out.backward(BF.from_bits(e_bits, eng.device))
        for got, exp, what in zip((out, ad.grad, bd.grad), want[name], ("forward", "d_a", "d_b")):
            assert BF.same_bits(BF.torch_bits(got), _rb(exp)), (cid, C, name, what)
        assert _pads_are_zero(BF.torch_bits(out), ne, np.uint16)
        ga, gb = g.gather(BF.from_bits(a_bits, eng.device), "senders"), g.gather(BF.from_bits(b_bits, eng.device), "receivers")
        assert BF.same_bits(BF.torch_bits(out), BF.torch_bits(ga * gb if name == "pair_mul" else ga + gb)), (cid, C, name, "torch")


@pytest.mark.parametrize("C", [5, 64])
def test_bfloat16_conv_is_not_the_composition_of_the_bfloat16_ops(C):
    """One planted row: x = 1 and w = [256, 1, 1, 1, 1] on a node with at least five slots.  conv keeps the products in float32
    and rounds the ordered sum once: 260.  Held in bfloat16, the running sum stays 256 (256 + 1 is a tie that rounds back)."""
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("rpf2d_b1")
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    for role in ROLES:
        other = GP.OTHER[role]
        real = idx[role][0, :ne[0]]
        node = int(np.flatnonzero(np.bincount(real, minlength=N) >= 5)[0])
        slots = np.flatnonzero(real == node)
        w = np.zeros((B, E, C), np.float32)
        w[0, slots[:5]] = np.array(BF.PLANTED_ROWS[0], np.float32)[:, None]
        w = _nan_pads(w, ne)
        x = np.ones((B, N, C), np.float32)
        out = g.conv(BF.from_bits(BF.round_bf16(x), eng.device), BF.from_bits(BF.round_bf16(w), eng.device), role)
        assert (BF.widen(BF.torch_bits(out))[0, node] == BF.PLANTED_SUMS[0]).all(), (role, BF.widen(BF.torch_bits(out))[0, node])
        msg = BF.round_bf16(np_gather(x, idx[other], ne) * np.nan_to_num(w))     # the bfloat16 products (exact here)
        held = BF.widen(BF.np_segment_sum_bf16_acc(msg, idx[role], ne, N))
        assert (held[0, node] == 256.0).all() and (BF.widen(BF.np_segment_sum_bf16(msg, idx[role], ne, N))[0, node] == 260.0).all()


# ------------------------------------------------------------------------------------------------ memory
def test_conv_forward_allocates_nothing_edge_shaped():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("ldc3d")
    B, N, E, C = eng.B, eng.N, eng.e_cap, 64
    g = Graph(feats)
    x = torch.randn((B, N, C), device=eng.device, requires_grad=True)
    w = torch.randn((B, E, C), device=eng.device, requires_grad=True)
    bound, edge_tensor = B * N * C * 4 + 64 * 1024, B * E * C * 4
    print(f"[conv memory] bound {bound} bytes (the output plus 64 KiB); one edge-shaped tensor {edge_tensor} bytes")
    assert bound < edge_tensor
    for role in ROLES:
        g.conv(x, w, role)                                   # (the first sender call builds the engine's sender view)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = g.conv(x, w, role)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print(f"[conv memory] {role}: rise {rise} bytes")
        assert out.shape == (B, N, C) and rise <= bound, (role, rise, bound)
        del out


# ------------------------------------------------------------------------------------------------ staleness and refusals
def test_ops_after_the_list_moved_on_raise_and_wrong_arguments_are_refused():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _build("rpf2d_b1")
    N, E = eng.N, eng.e_cap
    g = Graph(feats)
    x = torch.randn((1, N, 4), device=eng.device, requires_grad=True)
    w = torch.randn((1, E, 4), device=eng.device, requires_grad=True)
    with pytest.raises(ValueError, match=r"\(1, %d, 3\).*\(1, %d, 4\)" % (N, E)):
        g.conv(torch.zeros((1, N, 3), device=eng.device), w, "senders")
    with pytest.raises(TypeError, match="one dtype"):
        g.conv(x, w.detach().to(torch.bfloat16), "senders")
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            g.pair_mul(x.detach().to(dt), x.detach().to(dt))
    with pytest.raises(TypeError, match="engine on"):
        g.pair_add(torch.zeros((1, N, 4)), torch.zeros((1, N, 4)))
    # the library's own refusals
    flat_x, flat_w = torch.zeros((N, 1, 4), device=eng.device), torch.zeros((E, 4), device=eng.device)
    out = torch.empty_like(flat_x)
    for args in ((2, flat_x.data_ptr(), flat_w.data_ptr(), out.data_ptr(), 1, 4, 0), (0, flat_x.data_ptr(), flat_w.data_ptr(), out.data_ptr(), 0, 4, 0),
                 (0, flat_x.data_ptr(), flat_w.data_ptr(), out.data_ptr(), 1, 0, 0), (0, flat_x.data_ptr(), flat_w.data_ptr(), out.data_ptr(), 1, 4, 2),
                 (0, flat_x.data_ptr(), None, out.data_ptr(), 1, 4, 0)):
        assert eng.lib.lb_graph_conv(eng._h, *args) == -1, args
    conv = g.conv(x, w, "senders")
    pm, pa = g.pair_mul(x, x), g.pair_add(x, x)
    eng.nl_update()
    for call in (lambda: g.conv(x, w, "receivers"), lambda: g.pair_mul(x, x), lambda: g.pair_add(x, x)):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    for made in (conv, pm, pa):                              # ... and so does a backward of a graph made before
        with pytest.raises(RuntimeError, match="stale"):
            made.sum().backward()
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    for call in (lambda: eng.graph_conv(1, flat_x, torch.zeros((eng.e_cap, 4), device=eng.device)),
                 lambda: eng.graph_pair_mul(1, flat_x, flat_x), lambda: eng.graph_pair_add(1, flat_x[:, 0], flat_x[:, 0])):
        with pytest.raises(LbHipError, match="-3.*overflowed"):
            call()
    eng.nl_allocate()
    assert eng.graph_pair_add(1, flat_x[:, 0].contiguous(), flat_x[:, 0].contiguous()).shape == (eng.e_cap, 4)


def test_unbatched_features():
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    _, _, _, _, _, hcase = _build("rpf2d_b1")               # (a case of its own: the new list must not stale a shared one)
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=6, scale=0.25)
    feats, _ = hcase.allocate_eval((ds[0][0][:, :6], ds[0][1]))
    assert not feats.batched
    eng = feats.engine
    g = Graph(feats)
    i, ne = eng.nl_idx()
    i, ne = _np(i), _np(ne)
    r_idx, s_idx = i[:, 0], i[:, 1]
    rng = np.random.default_rng(2)
    x, w = rng.standard_normal((eng.N, 3, 4)).astype(np.float32), _edge(rng, 1, eng.e_cap, 4, ne)[0]
    got = g.conv(_dev(x, eng), _dev(w, eng), "senders")
    assert got.shape == (eng.N, 3, 4)
    assert _same(_np(got), GP.np_conv(x[None], w[None], s_idx, r_idx, ne, eng.N)[0])
    a = rng.standard_normal((eng.N, 4)).astype(np.float32)
    pa = g.pair_add(_dev(a, eng), _dev(x[:, 0], eng))
    assert pa.shape == (eng.e_cap, 4) and _same(_np(pa), GP.np_pair_add(a[None], x[None, :, 0], s_idx, r_idx, ne, eng.e_cap)[0])


# ------------------------------------------------------------------------------------------------ through the model path
ISL = 6


def _conv_model(hcase, B, dim):
    from lagrangebench_amd.models import TorchModel
    from tests import _torch_models as TM
    model = TorchModel(GP.TinyConv(TM.node_in_of(hcase.engine(B)), dim, 32))
    params, state = model.init(np.array([7]), None)
    rng = np.random.default_rng(3)
    params["~"]["gain"] = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32)
    state["~"]["in_scale"] = (1.0 + 0.1 * rng.standard_normal(state["~"]["in_scale"].shape)).astype(np.float32)
    model.set_state(state)
    return model, params, state


def _cpu_run(model, params, state, feats, ne, pt, dtype, target):
    from tests import _torch_models as TM
    from tests.test_torch_model_gpu import _cpu_module
    mod = _cpu_module(model, params, state, dtype)
    fd = TM.cpu_features(feats, dtype)
    pred = mod(fd, torch.as_tensor(pt).long(), GP.CpuPairGraph(fd["senders"], fd["receivers"], ne, pt.shape[1]))
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach(), mod, float(mean.detach())


@pytest.mark.parametrize("cid", ["rpf2d_b2", "ldc3d"])
def test_tiny_conv_forward_and_gradients_match_the_float64_restatement(cid):
    _need_gpu()
    from tests._common import hip_case
    from tests.test_torch_model_gpu import CASES as MODEL_CASES, _dataset, _two_step
    B = MODEL_CASES[cid][3]
    ds = _dataset(cid)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    model, params, state = _conv_model(hcase, B, pos.shape[3])
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert out.shape == (B, eng.N, eng.dim) and _same(out, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    tg = torch.randn((B, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[tiny conv forward {cid}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}"
          f"{'' if ok else ' (held to the fp32 restatement)'}")
    assert ok or ok32, (cid, e, e32)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[tiny conv loss {cid}] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. {abs(l32 - l64) / abs(l64):.2e}"
          f"{'' if el <= 1e-5 else ' (held to the fp32 restatement)'}")
    assert el <= 1e-5 or abs(loss - l64) <= 3 * abs(l32 - l64), (loss, l64, l32)
    g_h = model.unflatten(g_flat)
    n64, n32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    worst, loose, bad = 0.0, [], []
    for name in n64:
        mod_name, _, leaf = name.rpartition(".")
        e, ok, ok32, e32 = _two_step(g_h[mod_name or "~"][leaf], n64[name].grad.numpy(), n32[name].grad.numpy(), 1e-4)
        if ok:
            worst = max(worst, e)
        elif ok32:
            loose.append(f"{name} ({e:.2e}, fp32 {e32:.2e})")
        else:
            bad.append((name, e, e32))
    print(f"[tiny conv grad {cid}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, (cid, bad)
    for name in ("edge_s", "edge_r", "gate_s", "gate_r", "filt", "vec"):     # every new op's gradient arrived
        assert np.abs(g_h[name]["weight"]).max() > 0, name


def test_tiny_conv_takes_a_trainer_step_and_round_trips_a_checkpoint(tmp_path):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
    from tests._common import hip_case
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _conv_model(case, 2, 2)
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 1}, input_seq_length=ISL, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt = trainer.train(step_max=1, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    print(f"[tiny conv trainer] losses {['%.5e' % l for l in losses]}")
    assert len(losses) == 2 and np.isfinite(losses).all() and opt["count"] == 2 and np.abs(opt["m"]).max() > 0
    loaded, _, lopt, step = load_haiku(ckp)
    assert step == 1 and set(loaded) == set(params) and set(lopt) >= {"m", "v", "count"}
    assert _same(model.flatten(model.params_from_haiku(loaded)), model.flatten(params))
