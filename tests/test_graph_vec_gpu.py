"""graph.Graph's vector-message ops on the device (csrc/lb_graph.hip): conv_vec, conv_dot and their shared edge gradients,
forward and backward, against the numpy loops of tests/_graph_vec.py - bit for bit: the order of every sum, the blocked sum
over the columns in d_u included, is part of the contract, so there is no tolerance here - and against this library's own
gather / segment_sum composition, which they replace.

Cases and roles are those of tests/test_graph_ops_gpu.py (B = 2 behind pads, more than one workgroup of rows, N = 3 with rows
shorter than a wave, the radix-sorted sender view of the asymmetric list).  Columns: 1 and 5 take the scalar path with one
short block of the d_u sum; 64 is four full blocks on 16-byte units; 130 is nine blocks, the last two columns wide, several
units per lane, and a unit must not cross a k boundary.  K in {1, 3, 5}: 5 is past one chunk of three and no multiple of it.
Every pad slot of w, of u and of every edge-shaped cotangent holds NaN.

bfloat16: round_to_bf16(the float32 twin(upcast inputs)) bit for bit, with the rounding of tests/_graph_bf16.py; 520 columns
are 33 blocks, past half a wave.  The model path (TinyVec in models.TorchModel) uses the two-step rule of
tests/test_torch_model_gpu.py, the window gradient the bars of tests/test_torch_window_grad_gpu.py, both unchanged.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_bf16 as BF  # noqa: E402
from tests import _graph_vec as GV  # noqa: E402
from tests.test_graph_ops_gpu import CASES, COLUMNS, ROLES, _build, _setup  # noqa: E402

pytestmark = pytest.mark.gpu

VEC_COLUMNS = [1, 5, 64, 130]
assert set(VEC_COLUMNS) <= set(COLUMNS)
KS = [1, 3, 5]
BF16_COLUMNS = [5, 64, 130, 520]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(_bits(a), _bits(b))


def _nan_pads(a, ne):
    a = a.copy()
    for b in range(a.shape[0]):
        a[b, ne[b]:] = np.nan
    return a


def _pads_are_zero(a, ne, view=np.uint32):
    return all((np.ascontiguousarray(a[b, ne[b]:]).view(view) == 0).all() for b in range(a.shape[0]))


def _edge(rng, B, E, C, ne, decades=True):
    """(B, E_cap, C) float32 (over seven decades), NaN in every pad slot."""
    scale = 10.0 ** rng.integers(-3, 4, (B, E, 1)) if decades else 1.0
    return _nan_pads((rng.standard_normal((B, E, C)) * scale).astype(np.float32), ne)


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


def _run(g, op, node, w, u, d, role, eng):
    """One forward and backward of g.conv_vec / g.conv_dot on fresh leaves -> (out, d_node, d_w, d_u) as numpy."""
    nd, wd, ud = _dev(node, eng, True), _dev(w, eng, True), _dev(u, eng, True)
    out = getattr(g, op)(nd, wd, ud, role)
    out.backward(_dev(d, eng))
    return _np(out), _np(nd.grad), _np(wd.grad), _np(ud.grad)


# ------------------------------------------------------------------------------------------------ float32
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", VEC_COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_conv_vec_and_conv_dot_equal_numpy_and_the_composition_bit_for_bit(cid, C, K):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, pairs, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(1000 * C + 10 * K + len(cid))
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    v = rng.standard_normal((B, N, K, C)).astype(np.float32)
    w = _edge(rng, B, E, C, ne)
    u = _edge(rng, B, E, K, ne, decades=False)
    dv = rng.standard_normal((B, N, K, C)).astype(np.float32)      # the cotangent of conv_vec
    ds = rng.standard_normal((B, N, C)).astype(np.float32)         # ... of conv_dot
    for role in ROLES:
        other = GV.OTHER[role]
        ir, io = idx[role], idx[other]
        # ================= conv_vec
        got = _run(g, "conv_vec", x, w, u, dv, role, eng)
        assert got[0].shape == (B, N, K, C) and got[2].shape == (B, E, C) and got[3].shape == (B, E, K)
        assert all(np.isfinite(a).all() for a in got), (cid, role, C, K, "conv_vec finite")
        want_dw, want_du = GV.np_vec_edge_grad(x, dv, w, u, io, ir, ne, E)
        assert _same(got[0], GV.np_conv_vec(x, w, u, ir, io, ne, N)), (cid, role, C, K, "conv_vec forward")
        assert _same(got[1], GV.np_conv_dot(dv, w, u, io, ir, ne, N)), (cid, role, C, K, "conv_vec d_x")
        assert _same(got[2], want_dw), (cid, role, C, K, "conv_vec d_w")
        assert _same(got[3], want_du), (cid, role, C, K, "conv_vec d_u", np.abs(got[3] - want_du).max())
        assert _pads_are_zero(got[2], ne) and _pads_are_zero(got[3], ne)
        # ---- this library's own composition: the forward as written in the issue; d_x and d_w with the contraction over k
        # spelled k by k (autograd's own reduction of the broadcast over k has no stated order): S = x at the other node,
        # V = the cotangent at the role's node
        w2, u2 = _dev(np.nan_to_num(w), eng), _dev(np.nan_to_num(u), eng)
        comp = g.segment_sum((g.gather(_dev(x, eng), other) * w2)[:, :, None, :] * u2[:, :, :, None], role)
        assert _same(_np(comp), got[0]), (cid, role, C, K, "conv_vec composition")
        gs, gv = g.gather(_dev(x, eng), other), g.gather(_dev(dv, eng), role)
        t = gv[:, :, 0] * u2[:, :, 0:1]
        for k in range(1, K):
            t = t + gv[:, :, k] * u2[:, :, k:k + 1]
        assert _same(_np(g.segment_sum(w2 * t, other)), got[1]), (cid, role, C, K, "conv_vec composition d_x")
        assert _same(_np(gs * t), got[2]), (cid, role, C, K, "conv_vec composition d_w")
        # ---- a second call: the same bits
        again = _run(g, "conv_vec", x, w, u, dv, role, eng)
        assert all(_same(p, q) for p, q in zip(got, again)), (cid, role, C, K, "conv_vec second call")

        # ================= conv_dot
        got = _run(g, "conv_dot", v, w, u, ds, role, eng)
        assert got[0].shape == (B, N, C) and got[1].shape == (B, N, K, C) and got[3].shape == (B, E, K)
        assert all(np.isfinite(a).all() for a in got), (cid, role, C, K, "conv_dot finite")
        want_dw, want_du = GV.np_vec_edge_grad(ds, v, w, u, ir, io, ne, E)
        assert _same(got[0], GV.np_conv_dot(v, w, u, ir, io, ne, N)), (cid, role, C, K, "conv_dot forward")
        assert _same(got[1], GV.np_conv_vec(ds, w, u, io, ir, ne, N)), (cid, role, C, K, "conv_dot d_v")
        assert _same(got[2], want_dw), (cid, role, C, K, "conv_dot d_w")
        assert _same(got[3], want_du), (cid, role, C, K, "conv_dot d_u", np.abs(got[3] - want_du).max())
        assert _pads_are_zero(got[2], ne) and _pads_are_zero(got[3], ne)
        # ---- the composition: t from gather(v, other) k by k, forward segment_sum(w * t); d_v through autograd of the
        # composition of conv_vec's forward (its adjoint): segment_sum over the other role of the cotangent's message
        gv = g.gather(_dev(v, eng), other)
        t = gv[:, :, 0] * u2[:, :, 0:1]
        for k in range(1, K):
            t = t + gv[:, :, k] * u2[:, :, k:k + 1]
        assert _same(_np(g.segment_sum(w2 * t, role)), got[0]), (cid, role, C, K, "conv_dot composition")
        comp_dv = g.segment_sum((g.gather(_dev(ds, eng), role) * w2)[:, :, None, :] * u2[:, :, :, None], other)
        assert _same(_np(comp_dv), got[1]), (cid, role, C, K, "conv_dot composition d_v")
        assert _same(_np(g.gather(_dev(ds, eng), role) * t), got[2]), (cid, role, C, K, "conv_dot composition d_w")
        again = _run(g, "conv_dot", v, w, u, ds, role, eng)
        assert all(_same(p, q) for p, q in zip(got, again)), (cid, role, C, K, "conv_dot second call")
    if pairs is not None:
        assert eng.graph_sender_sorts() >= 1


# ------------------------------------------------------------------------------------------------ bfloat16
def _bf(a):
    """float32 -> (its bfloat16 bits, the float32 values they hold); a NaN stays a NaN."""
    bits = BF.round_bf16(a)
    return bits, BF.widen(bits)


def _rb(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return BF.round_bf16(a)


def _run_bf16(g, op, node_bits, w_bits, u_bits, d_bits, role, eng):
    nd, wd, ud = (BF.from_bits(b, eng.device, True) for b in (node_bits, w_bits, u_bits))
    out = getattr(g, op)(nd, wd, ud, role)
    assert out.dtype == torch.bfloat16
    out.backward(BF.from_bits(d_bits, eng.device))
    assert nd.grad.dtype == wd.grad.dtype == ud.grad.dtype == torch.bfloat16
    return BF.torch_bits(out), BF.torch_bits(nd.grad), BF.torch_bits(wd.grad), BF.torch_bits(ud.grad)


@pytest.mark.parametrize("C", BF16_COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_bfloat16_is_the_rounded_float32_op_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(31 * C + len(cid))
    w_bits, w = _bf(_edge(rng, B, E, C, ne))
    x_bits, x = _bf(rng.standard_normal((B, N, C)).astype(np.float32))
    ds_bits, ds = _bf(rng.standard_normal((B, N, C)).astype(np.float32))
    for K in KS:
        u_bits, u = _bf(_edge(rng, B, E, K, ne, decades=False))
        v_bits, v = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        dv_bits, dv = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        for role in ROLES:
            other = GV.OTHER[role]
            ir, io = idx[role], idx[other]
            got = _run_bf16(g, "conv_vec", x_bits, w_bits, u_bits, dv_bits, role, eng)
            d_w, d_u = GV.np_vec_edge_grad(x, dv, w, u, io, ir, ne, E)
            want = (GV.np_conv_vec(x, w, u, ir, io, ne, N), GV.np_conv_dot(dv, w, u, io, ir, ne, N), d_w, d_u)
            for a, b, what in zip(got, want, ("forward", "d_x", "d_w", "d_u")):
                assert BF.same_bits(a, _rb(b)), (cid, role, C, K, "conv_vec", what)
                assert np.isfinite(BF.widen(a)).all()
            assert _pads_are_zero(got[2], ne, np.uint16) and _pads_are_zero(got[3], ne, np.uint16)
            got = _run_bf16(g, "conv_dot", v_bits, w_bits, u_bits, ds_bits, role, eng)
            d_w, d_u = GV.np_vec_edge_grad(ds, v, w, u, ir, io, ne, E)
            want = (GV.np_conv_dot(v, w, u, ir, io, ne, N), GV.np_conv_vec(ds, w, u, io, ir, ne, N), d_w, d_u)
            for a, b, what in zip(got, want, ("forward", "d_v", "d_w", "d_u")):
                assert BF.same_bits(a, _rb(b)), (cid, role, C, K, "conv_dot", what)
                assert np.isfinite(BF.widen(a)).all()
            assert _pads_are_zero(got[2], ne, np.uint16) and _pads_are_zero(got[3], ne, np.uint16)


@pytest.mark.parametrize("C", [5, 64])
def test_bfloat16_conv_vec_is_not_the_composition_of_the_bfloat16_ops(C):
    """One planted row: x = 1, u = 1 and w = [256, 1, 1, 1, 1] on a node with at least five slots.  conv_vec keeps the terms in
    float32 and rounds the ordered sum once: 260.  Held in bfloat16, the running sum stays 256 (256 + 1 is a tie that rounds
    back)."""
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    from tests.test_graph_ops_gpu import np_gather
    feats, eng, idx, ne, _, _ = _case("rpf2d_b1")
    B, N, E, K = eng.B, eng.N, eng.e_cap, 3
    g = Graph(feats)
    for role in ROLES:
        other = GV.OTHER[role]
        real = idx[role][0, :ne[0]]
        node = int(np.flatnonzero(np.bincount(real, minlength=N) >= 5)[0])
        slots = np.flatnonzero(real == node)
        w = np.zeros((B, E, C), np.float32)
        w[0, slots[:5]] = np.array(BF.PLANTED_ROWS[0], np.float32)[:, None]
        w = _nan_pads(w, ne)
        x, u = np.ones((B, N, C), np.float32), _nan_pads(np.ones((B, E, K), np.float32), ne)
        out = g.conv_vec(*(BF.from_bits(BF.round_bf16(a), eng.device) for a in (x, w, u)), role)
        assert (BF.widen(BF.torch_bits(out))[0, node] == BF.PLANTED_SUMS[0]).all(), (role, BF.widen(BF.torch_bits(out))[0, node])
        msg = BF.round_bf16(np_gather(x, idx[other], ne) * np.nan_to_num(w))     # the bfloat16 messages of one k (exact here)
        held = BF.widen(BF.np_segment_sum_bf16_acc(msg, idx[role], ne, N))
        assert (held[0, node] == 256.0).all() and (BF.widen(BF.np_segment_sum_bf16(msg, idx[role], ne, N))[0, node] == 260.0).all()


# ------------------------------------------------------------------------------------------------ memory
def test_forward_allocates_nothing_edge_shaped_and_a_gradient_not_required_is_not_allocated():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("ldc3d")
    B, N, E, C, K = eng.B, eng.N, eng.e_cap, 64, 3
    g = Graph(feats)
    x = torch.randn((B, N, C), device=eng.device, requires_grad=True)
    v = torch.randn((B, N, K, C), device=eng.device, requires_grad=True)
    w = torch.randn((B, E, C), device=eng.device, requires_grad=True)
    u = torch.randn((B, E, K), device=eng.device, requires_grad=True)
    slack, edge_tensor = 64 * 1024, B * E * C * 4
    bounds = {"conv_vec": B * N * K * C * 4 + slack, "conv_dot": B * N * C * 4 + slack}
    print(f"[vec memory] bounds {bounds} bytes (the output plus 64 KiB); one (E_cap, C) tensor {edge_tensor} bytes, the product "
          f"(E_cap, K, C) {K * edge_tensor}")
    assert max(bounds.values()) < edge_tensor
    for op, node in (("conv_vec", x), ("conv_dot", v)):
        for role in ROLES:
            getattr(g, op)(node, w, u, role)                  # (the first sender call builds the engine's sender view)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = getattr(g, op)(node, w, u, role)
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
            print(f"[vec memory] {op} {role}: rise {rise} bytes")
            assert rise <= bounds[op], (op, role, rise, bounds[op])
            del out
    # ---- the backward: what is not required is neither computed nor allocated
    calls = []
    grad = eng.graph_conv_vec_edge_grad
    eng.graph_conv_vec_edge_grad = lambda *a: (calls.append(tuple(bool(f) for f in a[-2:])), grad(*a))[1]
    try:
        for op, node in (("conv_vec", x), ("conv_dot", v)):
            for need_w, need_u in ((True, False), (False, True), (False, False), (True, True)):
                calls.clear()
                nd, wd, ud = node.detach().requires_grad_(True), w.detach().requires_grad_(need_w), u.detach().requires_grad_(need_u)
                out = getattr(g, op)(nd, wd, ud, "senders")
                cot = torch.ones_like(out)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                out.backward(cot)
                torch.cuda.synchronize()
                rise = torch.cuda.max_memory_allocated() - before
                assert calls == ([(need_w, need_u)] if need_w or need_u else []), (op, need_w, need_u, calls)
                assert (wd.grad is not None) == need_w and (ud.grad is not None) == need_u and nd.grad is not None
                bound = nd.numel() * 4 + need_w * edge_tensor + need_u * B * E * K * 4 + slack
                print(f"[vec memory] {op} backward, d_w {need_w}, d_u {need_u}: rise {rise} bytes, bound {bound}")
                assert rise <= bound, (op, need_w, need_u, rise, bound)
        calls.clear()                                         # no gradient to the node tensor: no node-shaped launch
        conv_vec, conv_dot = eng.graph_conv_vec, eng.graph_conv_dot
        eng.graph_conv_vec = lambda *a: (calls.append("conv_vec"), conv_vec(*a))[1]
        eng.graph_conv_dot = lambda *a: (calls.append("conv_dot"), conv_dot(*a))[1]
        wd = w.detach().requires_grad_(True)
        g.conv_vec(x.detach(), wd, u.detach(), "receivers").sum().backward()
        assert calls == ["conv_vec", (True, False)] and wd.grad.shape == w.shape
    finally:
        for name in ("graph_conv_vec_edge_grad", "graph_conv_vec", "graph_conv_dot"):
            eng.__dict__.pop(name, None)


# ------------------------------------------------------------------------------------------------ staleness and refusals
def test_ops_after_the_list_moved_on_raise_and_wrong_arguments_are_refused():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _build("rpf2d_b1")
    N, E = eng.N, eng.e_cap
    g = Graph(feats)
    x = torch.randn((1, N, 4), device=eng.device, requires_grad=True)
    v = torch.randn((1, N, 3, 4), device=eng.device, requires_grad=True)
    w = torch.randn((1, E, 4), device=eng.device, requires_grad=True)
    u = torch.randn((1, E, 3), device=eng.device, requires_grad=True)
    shapes = r"\(1, %d, 'C'\).*\(1, %d, 'C'\).*\(1, %d, 'K'\)" % (N, E, E)
    with pytest.raises(ValueError, match=shapes):
        g.conv_vec(torch.zeros((1, N, 3), device=eng.device), w, u, "senders")
    with pytest.raises(ValueError, match=r"\(1, %d, 'K', 'C'\)" % N):
        g.conv_dot(x, w, u, "senders")                       # a scalar tensor where the vector one belongs
    with pytest.raises(ValueError, match=r"\(1, %d, 'K', 'C'\)" % N):
        g.conv_dot(torch.zeros((1, N, 2, 4), device=eng.device), w, u, "senders")     # K of v is not K of u
    with pytest.raises(ValueError, match="1 <= K <= 9"):
        g.conv_vec(x, w, torch.zeros((1, E, 10), device=eng.device), "receivers")
    with pytest.raises(ValueError, match="role"):
        g.conv_vec(x, w, u, "both")
    for args in ((x, w.detach().to(torch.bfloat16), u), (x, w, u.detach().to(torch.bfloat16))):
        with pytest.raises(TypeError, match="one dtype"):
            g.conv_vec(*args, "senders")
    with pytest.raises(TypeError, match="one dtype"):
        g.conv_dot(v.detach().to(torch.bfloat16), w, u, "senders")
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        g.conv_vec(x.detach().double(), w.detach().double(), u.detach().double(), "senders")
    with pytest.raises(TypeError, match="engine on"):
        g.conv_vec(torch.zeros((1, N, 4)), torch.zeros((1, E, 4)), torch.zeros((1, E, 3)), "senders")
    # the library's own refusals: role, K < 1, K > 9, C < 1, dtype, a null pointer
    fx, fv = torch.zeros((N, 4), device=eng.device), torch.zeros((N, 3, 4), device=eng.device)
    fw, fu = torch.zeros((E, 4), device=eng.device), torch.zeros((E, 3), device=eng.device)
    px, pv, pw, pu = (t.data_ptr() for t in (fx, fv, fw, fu))
    for entry, node, out in ((eng.lib.lb_graph_conv_vec, px, pv), (eng.lib.lb_graph_conv_dot, pv, px)):
        for args in ((2, node, pw, pu, out, 3, 4, 0), (0, node, pw, pu, out, 0, 4, 0), (0, node, pw, pu, out, 10, 4, 0),
                     (0, node, pw, pu, out, 3, 0, 0), (0, node, pw, pu, out, 3, 4, 2), (0, node, pw, None, out, 3, 4, 0),
                     (0, node, pw, pu, None, 3, 4, 0)):
            assert entry(eng._h, *args) == -1, args
        assert entry(eng._h, 0, node, pw, pu, out, 3, 4, 0) == 0
    dw, du = torch.empty_like(fw), torch.empty_like(fu)
    grad = eng.lib.lb_graph_conv_vec_edge_grad
    for args in ((2, px, pv, pw, pu, dw.data_ptr(), du.data_ptr(), 3, 4, 0), (0, px, pv, pw, pu, dw.data_ptr(), du.data_ptr(), 10, 4, 0),
                 (0, px, pv, pw, pu, dw.data_ptr(), du.data_ptr(), 0, 4, 0), (0, px, pv, pw, pu, dw.data_ptr(), du.data_ptr(), 3, 0, 0),
                 (0, px, pv, pw, pu, None, None, 3, 4, 0), (0, None, pv, pw, pu, dw.data_ptr(), du.data_ptr(), 3, 4, 0)):
        assert grad(eng._h, *args) == -1, args
    assert grad(eng._h, 1, px, pv, pw, pu, None, du.data_ptr(), 3, 4, 0) == 0
    # a stale list, in the forward and in the backward of a graph made before
    made = (g.conv_vec(x, w, u, "senders"), g.conv_dot(v, w, u, "receivers"))
    eng.nl_update()
    for call in (lambda: g.conv_vec(x, w, u, "receivers"), lambda: g.conv_dot(v, w, u, "senders")):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    for out in made:
        with pytest.raises(RuntimeError, match="stale"):
            out.sum().backward()
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    cap_w, cap_u = torch.zeros((eng.e_cap, 4), device=eng.device), torch.zeros((eng.e_cap, 3), device=eng.device)
    for call in (lambda: eng.graph_conv_vec(1, fx, cap_w, cap_u), lambda: eng.graph_conv_dot(0, fv, cap_w, cap_u),
                 lambda: eng.graph_conv_vec_edge_grad(0, fx, fv, cap_w, cap_u)):
        with pytest.raises(LbHipError, match="-3.*overflowed"):
            call()


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
    N, E, C, K = eng.N, eng.e_cap, 8, 2
    rng = np.random.default_rng(2)
    x, v = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, K, C)).astype(np.float32)
    w, u = _edge(rng, 1, E, C, ne)[0], _edge(rng, 1, E, K, ne, decades=False)[0]
    dv = rng.standard_normal((N, K, C)).astype(np.float32)
    out, d_x, d_w, d_u = _run(g, "conv_vec", x, w, u, dv, "senders", eng)
    assert out.shape == (N, K, C) and d_x.shape == (N, C) and d_w.shape == (E, C) and d_u.shape == (E, K)
    assert _same(out, GV.np_conv_vec(x[None], w[None], u[None], s_idx, r_idx, ne, N)[0])
    want_dw, want_du = GV.np_vec_edge_grad(x[None], dv[None], w[None], u[None], r_idx, s_idx, ne, E)
    assert _same(d_w, want_dw[0]) and _same(d_u, want_du[0])
    got = g.conv_dot(_dev(v, eng), _dev(w, eng), _dev(u, eng), "receivers")
    assert got.shape == (N, C) and _same(_np(got), GV.np_conv_dot(v[None], w[None], u[None], r_idx, s_idx, ne, N)[0])
    # u may be the engine's own rel_disp
    r = feats["rel_disp"].to(torch.float32)
    got = g.conv_vec(_dev(x, eng), _dev(w, eng), r, "senders")
    assert got.shape == (N, eng.dim, C)
    assert _same(_np(got), GV.np_conv_vec(x[None], w[None], _np(r)[None], s_idx, r_idx, ne, N)[0])


# ------------------------------------------------------------------------------------------------ through the model path
ISL = 6


def _vec_model(eng):
    from lagrangebench_amd.models import TorchModel
    from tests import _torch_models as TM
    model = TorchModel(GV.TinyVec(TM.node_in_of(eng), eng.dim, 32))
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
    pred = mod(fd, torch.as_tensor(pt).long(), GV.CpuVecGraph(fd["senders"], fd["receivers"], ne, pt.shape[1]))
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach(), mod, float(mean.detach())


@pytest.mark.parametrize("cid", ["rpf2d_b2", "ldc3d"])
def test_tiny_vec_forward_and_gradients_match_the_float64_restatement(cid):
    """Measured on an MI355X (rpf2d B = 2 / ldc3d): forward 1.9e-7 / 1.7e-7 of the largest entry from float64, loss 3.3e-9 /
    9.7e-8, worst gradient leaf 1.6e-6 / 2.1e-6; no leaf held to the float32 restatement."""
    _need_gpu()
    from tests._common import hip_case
    from tests.test_torch_model_gpu import CASES as MODEL_CASES, _dataset, _two_step
    B = MODEL_CASES[cid][3]
    ds = _dataset(cid)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    model, params, state = _vec_model(hcase.engine(B))
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert out.shape == (B, eng.N, eng.dim) and _same(out, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    tg = torch.randn((B, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[tiny vec forward {cid}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}"
          f"{'' if ok else ' (held to the fp32 restatement)'}")
    assert ok or ok32, (cid, e, e32)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[tiny vec loss {cid}] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. {abs(l32 - l64) / abs(l64):.2e}"
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
    print(f"[tiny vec grad {cid}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, (cid, bad)
    for name in ("enc", "edge_s", "edge_r", "edge_e", "filt", "read", "dec"):     # every op's gradient arrived
        assert np.abs(g_h[name]["weight"]).max() > 0, name
    assert np.abs(g_h["~"]["gain"]).max() > 0


def test_tiny_vec_takes_a_trainer_step_and_round_trips_a_checkpoint(tmp_path):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
    from tests._common import hip_case
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _vec_model(case.engine(2))
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 1}, input_seq_length=ISL, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt = trainer.train(step_max=1, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    print(f"[tiny vec trainer] losses {['%.5e' % l for l in losses]}")
    assert len(losses) == 2 and np.isfinite(losses).all() and opt["count"] == 2 and np.abs(opt["m"]).max() > 0
    loaded, _, lopt, step = load_haiku(ckp)
    assert step == 1 and set(loaded) == set(params) and set(lopt) >= {"m", "v", "count"}
    assert _same(model.flatten(model.params_from_haiku(loaded)), model.flatten(params))


# ------------------------------------------------------------------------------------------------ the window gradient through d_u
@pytest.mark.parametrize("cid", ["rpf2d_b1", "asym_b2"])
def test_window_gradient_flows_through_d_u(cid):
    """TinyVec through autograd.TorchModule with a window that requires grad: rel_disp reaches the loss only as the u of conv_vec
    and conv_dot and through the edge encoder, so d loss / d window carries d_u on to lb_graph_features_backward.  Against
    float64 autograd of tests/_features_torch.py + CpuVecGraph on the engine's own list, with the bars of
    tests/test_torch_window_grad_gpu.py: forward and loss 1e-5, d loss / d window 1e-4 of its largest entry, a parameter leaf
    1e-4 or 3x the float32 restatement's own deviation.
    Measured on an MI355X (rpf2d B = 1 / one-directional B = 2): forward 1.8e-7 / 1.9e-7; loss 1.6e-8 / 4.5e-8; d loss / d window
    1.9e-7 / 1.1e-7; worst parameter leaf 1.8e-6 / 1.4e-6, none held to the float32 restatement; with u cut out of the
    restatement d loss / d window moves by 0.33 / 0.17 of its largest entry."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule
    from tests import test_torch_window_grad_gpu as WG
    from tests._features_torch import features_torch
    ds, hcase, pos, pt, consts = WG._setup(cid)
    feats, eng = WG._allocate(cid)
    B, N, dim = eng.B, eng.N, eng.dim
    model, params, state = _vec_model(eng)
    mod = TorchModule(model, hcase, params, B, state=state)
    window = torch.as_tensor(pos[:, :, :WG.ISL], device=eng.device).requires_grad_(True)
    target = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    pred = mod(window, pt)["acc"]
    loss = WG._mse(pred, target.to(eng.device).float(), WG._mask(pt, eng.device))
    loss.backward()
    idx, ne, edges = WG._list(eng)
    if WG.CASES[cid][5]:
        from tests._asym import one_directional_edges
        assert all(one_directional_edges(np.stack([_np(e[0]), _np(e[1])])) for e in edges)
        assert eng.graph_sender_sorts() >= 1
    force = WG._force(eng)
    got_w, got_p = _np(window.grad), WG._grads(mod.module)

    def restate(module, dtype, windows, graph=GV.CpuVecGraph):
        E_cap = idx.shape[2]
        per = [features_torch(windows[b], edges[b][0], edges[b][1], force=None if force is None else force[b], **consts)
               for b in range(B)]
        fd = {}
        for k in per[0]:
            if k in ("node", "edge"):
                continue
            rows = [torch.cat([p[k], p[k].new_zeros((E_cap - p[k].shape[0], p[k].shape[1]))]) if k in WG.EDGE_KEYS else p[k]
                    for p in per]
            fd[k] = torch.stack(rows).to(dtype)
        return module(fd, torch.as_tensor(pt).long(), graph(idx[:, 1], idx[:, 0], ne, N))

    refs = {}
    for dt in (torch.float64, torch.float32):
        m = model._device_module(WG._Cpu(), params, state).to(dt)
        ws = [torch.as_tensor(pos[b, :, :WG.ISL]).clone().requires_grad_(True) for b in range(B)]
        pr = restate(m, dt, ws)
        ls = WG._mse(pr, target.to(dt), WG._mask(pt))
        ls.backward()
        refs[dt] = (pr.detach().double().numpy(), float(ls.detach()), np.stack([w.grad.numpy() for w in ws]), WG._grads(m))
    p64, l64, w64, g64 = refs[torch.float64]
    e_fwd = np.abs(_np(pred).astype(np.float64) - p64).max() / np.abs(p64).max()
    e_loss = abs(float(loss.detach()) - l64) / abs(l64)
    e_win = np.abs(got_w - w64).max() / np.abs(w64).max()
    print(f"[vec window grad {cid}] forward {e_fwd:.2e}; loss {e_loss:.2e}; d loss / d window {e_win:.2e} (largest entry "
          f"{np.abs(w64).max():.3e}; the fp32 restatement {np.abs(refs[torch.float32][2] - w64).max() / np.abs(w64).max():.2e})")
    assert e_fwd <= 1e-5 and e_loss <= 1e-5, (e_fwd, e_loss)
    assert got_w.dtype == np.float64 and np.isfinite(got_w).all() and e_win < 1e-4, e_win
    WG._leaf_report(f"vec {cid}", got_p, g64, refs[torch.float32][3])
    # the part of it that came through u: with rel_disp detached in the restatement the window gradient is another one
    m = model._device_module(WG._Cpu(), params, state).to(torch.float64)
    ws = [torch.as_tensor(pos[b, :, :WG.ISL]).clone().requires_grad_(True) for b in range(B)]

    class _CutU(GV.CpuVecGraph):
        def conv_vec(self, x, w, u, role):
            return super().conv_vec(x, w, u.detach(), role)

        def conv_dot(self, v, w, u, role):
            return super().conv_dot(v, w, u.detach(), role)

    WG._mse(restate(m, torch.float64, ws, _CutU), target, WG._mask(pt)).backward()
    cut = np.stack([w.grad.numpy() for w in ws])
    share = np.abs(cut - w64).max() / np.abs(w64).max()
    print(f"[vec window grad {cid}] the share of d_u in d loss / d window: {share:.2e} of the largest entry")
    assert share > 100 * 1e-4                                  # (far above the bar: a missing d_u could not pass it)
