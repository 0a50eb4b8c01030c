"""graph.Graph's edge-pair ops on the device (csrc/lb_graph.hip: k_graph_reverse, k_graph_edge_pair): the reverse map, swap,
symmetrize and antisymmetrize, forward and backward, against the numpy twins of tests/_graph_reverse.py - bit for bit: one
float32 operation has one answer, so there is no tolerance in the op tests.

Cases and columns are those of tests/test_graph_ops_gpu.py: B = 2 behind pads (rpf2d_b2), more than one workgroup (ldc3d, whose
box is not periodic), rows shorter than a wave and nearly every slot a pad (lj), edges without a transpose (asym); C = 1 (the
scalar path), 5 (odd), 64 (16-byte units), 130 (a short tail), 260 (several units per lane).  msg and the cotangent hold NaN in
every pad slot.

The model tests run tests/_graph_reverse_models.MomentumMP in models.TorchModel: the exact antisymmetry of its edge field, the
momentum bound derived in test_momentum_is_conserved_to_the_rounding_of_the_row_sums, the two-step rule of
tests/test_torch_model_gpu.py and the window-gradient bars of tests/test_torch_window_grad_gpu.py, both unchanged.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_bf16 as GB  # noqa: E402
from tests import _graph_reverse as GR  # noqa: E402
from tests import _graph_reverse_models as GM  # noqa: E402
from tests.test_graph_ops_gpu import CASES, COLUMNS, ROLES, _build, _setup  # noqa: E402
from tests.test_graph_reverse import check_map, check_symmetry, check_zeros  # noqa: E402

pytestmark = pytest.mark.gpu

assert COLUMNS == [1, 5, 64, 130, 260] and ROLES == ("receivers", "senders")
BF = torch.bfloat16
BF16 = [(cid, 64) for cid in CASES] + [(cid, 260) for cid in ("rpf2d_b2", "lj", "asym")]
ISL = 6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


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


def _edge(rng, B, E, C, ne):
    """(B, E_cap, C) float32 over seven decades, NaN in every pad slot."""
    m = (rng.standard_normal((B, E, C)) * 10.0 ** rng.integers(-3, 4, (B, E, 1))).astype(np.float32)
    for b in range(B):
        m[b, ne[b]:] = np.nan
    return m


def _twin_map(idx, ne):
    return GR.np_reverse(idx["receivers"], idx["senders"], ne)


def _unpaired(rev, idx, ne):
    return {(b, int(idx["receivers"][b, j]), int(idx["senders"][b, j])) for b in range(len(ne)) for j in range(int(ne[b]))
            if rev[b, j] < 0}


def _run(g, mode, msg_t, d_t):
    """One forward and backward of the op on a fresh leaf -> (out, d_msg) as tensors."""
    leaf = msg_t.detach().clone().requires_grad_()
    out = getattr(g, mode)(leaf)
    out.backward(d_t)
    return out.detach(), leaf.grad


# ------------------------------------------------------------------------------------------------ the map
@pytest.mark.parametrize("cid", CASES)
def test_the_reverse_map_equals_the_twin_integer_for_integer(cid):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, pairs, _ = _case(cid)
    g = Graph(feats)
    rev = g.reverse
    assert rev.dtype == torch.int32 and tuple(rev.shape) == (eng.B, eng.e_cap) and rev.device == eng.device
    want = _twin_map(idx, ne)
    got = _np(rev)
    assert np.array_equal(got, want), cid
    assert g.reverse is rev and np.array_equal(_np(eng.graph_reverse()).reshape(eng.B, eng.e_cap), want)   # cached; a second read
    lone = _unpaired(want, idx, ne)
    check_map(got, idx["receivers"], idx["senders"], ne, lone)
    selfs = sum(int((idx["receivers"][b, :ne[b]] == idx["senders"][b, :ne[b]]).sum()) for b in range(eng.B))
    print(f"[reverse {cid}] slots {eng.B} x {eng.e_cap}, real {ne.tolist()}, self-edges {selfs}, without a transpose {len(lone)}")
    assert selfs > 0
    if pairs is not None:
        from tests._asym import check_premise, one_directional_edges
        for b in range(eng.B):
            edges = np.stack([idx["receivers"][b, :ne[b]], idx["senders"][b, :ne[b]]])
            assert check_premise(edges, pairs, b) == one_directional_edges(edges)
        assert lone == set(pairs)                              # exactly the crafted pairs, and no other real slot, are -1
    else:
        assert not lone


def test_a_second_read_after_a_new_list_build_gives_the_new_lists_map():
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    from tests._common import hip_case
    ds = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(2)])
    maps = []
    for order in ([0, 1], [1, 0]):                             # the second build: the two trajectories exchanged
        feats, _ = hcase.allocate_eval((pos[order][:, :, :ISL], pt[order]))
        eng = feats.engine
        i, ne = eng.nl_idx()
        i, ne = _np(i), _np(ne)
        g = Graph(feats)
        maps.append((eng, g, _np(g.reverse), GR.np_reverse(i[:, 0], i[:, 1], ne), ne))
    (eng0, g0, got0, want0, ne0), (eng1, _, got1, want1, ne1) = maps
    assert eng0 is eng1 and ne0[0] != ne0[1] and ne0.tolist() == ne1.tolist()[::-1]
    assert np.array_equal(got0, want0) and np.array_equal(got1, want1) and not np.array_equal(want0, want1)
    with pytest.raises(RuntimeError, match="stale"):           # the first graph's list is gone
        g0.reverse


# ------------------------------------------------------------------------------------------------ the ops, float32
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_ops_equal_the_twin_and_the_torch_composition_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, E = eng.B, eng.e_cap
    g = Graph(feats)
    rev = _twin_map(idx, ne)
    rng = np.random.default_rng(1000 * C + len(cid))
    msg, d = _edge(rng, B, E, C, ne), _edge(rng, B, E, C, ne)
    md, dd = _dev(msg, eng), _dev(d, eng)
    for mode in GR.MODES:
        out, d_msg = _run(g, mode, md, dd)
        assert out.shape == (B, E, C) and out.dtype == torch.float32 and d_msg.shape == (B, E, C)
        assert GR.same_bits(_np(out), GR.np_edge_pair(mode, msg, rev, ne)), (cid, C, mode)
        assert GR.same_bits(_np(d_msg), GR.np_edge_pair_grad(mode, d, rev, ne)), (cid, C, mode)
        for res in (_np(out), _np(d_msg)):                     # pads and unpaired slots: all bits zero, with NaN in the pads
            check_zeros(res, rev, ne)
        out2, d_msg2 = _run(g, mode, md, dd)                   # two calls, the same bits
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
        assert torch.equal(d_msg2.view(torch.int32), d_msg.view(torch.int32))
        # the same thing written in torch with Graph.reverse and take_along_dim: one float32 add has one answer
        comp = GR.torch_edge_pair(mode, md, g.reverse)
        assert torch.equal(comp.view(torch.int32), out.view(torch.int32)), (cid, C, mode)
    if C == 5:
        check_symmetry("symmetrize", _np(g.symmetrize(md)), msg, rev, ne)
        check_symmetry("antisymmetrize", _np(g.antisymmetrize(md)), msg, rev, ne)


def test_an_unaligned_view_takes_the_single_element_path_and_gives_the_same_bits():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("rpf2d_b2")
    B, E, C = eng.B, eng.e_cap, 64
    g = Graph(feats)
    rev = _twin_map(idx, ne)
    rng = np.random.default_rng(31)

    def shifted(t):
        """t one element off alignment: 2 bytes for bfloat16, 4 for float32."""
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=eng.device)
        out = buf[1:].view(t.shape)
        out.copy_(t.detach())
        assert out.is_contiguous() and out.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
        return out

    msg, d = _edge(rng, B, E, C, ne), _edge(rng, B, E, C, ne)
    for dtype in (torch.float32, BF):
        md, dd = _dev(msg, eng).to(dtype), _dev(d, eng).to(dtype)
        bits = (lambda t: _np(t.view(torch.int32))) if dtype == torch.float32 else GB.torch_bits
        for mode in GR.MODES:
            out, d_msg = _run(g, mode, md, dd)
            if dtype == torch.float32:
                assert GR.same_bits(_np(out), GR.np_edge_pair(mode, msg, rev, ne))
            for m2, d2 in ((shifted(md), dd), (md, shifted(dd))):
                leaf = m2.detach().requires_grad_()            # (the shifted storage itself: a clone would be aligned again)
                assert leaf.data_ptr() == m2.data_ptr()
                o2 = getattr(g, mode)(leaf)
                o2.backward(d2)
                o2, g2 = o2.detach(), leaf.grad
                assert np.array_equal(bits(o2), bits(out)) and np.array_equal(bits(g2), bits(d_msg)), (dtype, mode)


# ------------------------------------------------------------------------------------------------ bfloat16
@pytest.mark.parametrize("cid,C", BF16)
def test_bfloat16_is_the_rounded_float32_op_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, E = eng.B, eng.e_cap
    g = Graph(feats)
    rev = _twin_map(idx, ne)
    rng = np.random.default_rng(7 * C + len(cid))
    mb, db = GB.round_bf16(_edge(rng, B, E, C, ne)), GB.round_bf16(_edge(rng, B, E, C, ne))   # NaN stays NaN in the pads
    md, dd = GB.from_bits(mb, eng.device), GB.from_bits(db, eng.device)
    for mode in GR.MODES:
        out, d_msg = _run(g, mode, md, dd)
        assert out.dtype == BF and d_msg.dtype == BF
        assert GB.same_bits(GB.torch_bits(out), GR.np_edge_pair_bf16(mode, mb, rev, ne)), (cid, C, mode)
        assert GB.same_bits(GB.torch_bits(d_msg), GR.np_edge_pair_bf16(mode, db, rev, ne)), (cid, C, mode)
        for res in (GB.torch_bits(out), GB.torch_bits(d_msg)):
            assert all((res[b, ne[b]:] == 0).all() and (res[b, :ne[b]][rev[b, :ne[b]] < 0] == 0).all() for b in range(B))


# ------------------------------------------------------------------------------------------------ shapes and refusals
def test_unbatched_features_trailing_dimensions_and_refusals():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    from tests._common import hip_case
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    feats, _ = hip_case(ds).allocate_eval((ds[0][0][:, :ISL], ds[0][1]))
    assert not feats.batched
    eng = feats.engine
    dev = eng.device
    g = Graph(feats)
    i, ne = eng.nl_idx()
    i, ne = _np(i), _np(ne)
    N, E = eng.N, eng.e_cap
    rev = GR.np_reverse(i[:, 0], i[:, 1], ne)
    assert tuple(g.reverse.shape) == (E,) and np.array_equal(_np(g.reverse), rev[0])
    msg = _edge(np.random.default_rng(2), 1, E, 12, ne)
    leaf = _dev(msg[0].reshape(E, 3, 4), eng, True)
    out = g.antisymmetrize(leaf)                               # trailing dimensions fold into C
    assert out.shape == (E, 3, 4) and GR.same_bits(_np(out).reshape(1, E, 12), GR.np_edge_pair("antisymmetrize", msg, rev, ne))
    out.backward(torch.ones_like(out))
    assert leaf.grad.shape == (E, 3, 4)
    m = torch.randn((E, 4), device=dev)
    for op in (g.swap, g.symmetrize, g.antisymmetrize):
        with pytest.raises(TypeError, match="float32 or bfloat16"):        # float16
            op(m.half())
        with pytest.raises(TypeError, match="engine on"):                  # a CPU tensor
            op(m.cpu())
        with pytest.raises(ValueError, match="expected"):
            op(torch.zeros((E + 1, 4), device=dev))
        y = op(m.clone().requires_grad_())                                 # a cotangent of another dtype (the node called directly:
        with pytest.raises(TypeError, match="cotangent"):                  # autograd itself would cast one handed to .backward())
            y.grad_fn.apply(torch.zeros((E, 4), dtype=BF, device=dev))
        x = m.clone().requires_grad_()                                     # once differentiable
        (gx,) = torch.autograd.grad(op(x).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError):
            gx.sum().backward()
    # ---- the library's own refusals: a mode or dtype it does not know, C < 1, a null pointer, out == msg
    flat, res = torch.zeros((E, 4), device=dev), torch.empty((E, 4), device=dev)
    pair = eng.lib.lb_graph_edge_pair_t
    for args in ((3, flat.data_ptr(), res.data_ptr(), 4, 0), (-1, flat.data_ptr(), res.data_ptr(), 4, 0),
                 (0, flat.data_ptr(), res.data_ptr(), 4, 2), (0, flat.data_ptr(), res.data_ptr(), 0, 0),
                 (0, None, res.data_ptr(), 4, 0), (0, flat.data_ptr(), None, 4, 0), (1, flat.data_ptr(), flat.data_ptr(), 4, 0)):
        assert pair(eng._h, *args) == -1, args
    assert pair(eng._h, 2, flat.data_ptr(), res.data_ptr(), 4, 0) == 0
    assert eng.lib.lb_graph_reverse(eng._h, None) == -1
    with pytest.raises(ValueError, match="lb_graph_edge_pair"):            # the engine's own check, below graph.Graph
        eng.graph_edge_pair(1, torch.zeros((E, 4), dtype=torch.float16, device=dev))
    # ---- a stale list, in the forward and in the backward of a graph made before
    made = [op(m.clone().requires_grad_()) for op in (g.swap, g.symmetrize, g.antisymmetrize)]
    eng.nl_update()
    for op, y in zip((g.swap, g.symmetrize, g.antisymmetrize), made):
        with pytest.raises(RuntimeError, match="stale"):
            op(m)
        with pytest.raises(RuntimeError, match="stale"):
            y.sum().backward()
    with pytest.raises(RuntimeError, match="stale"):
        g.reverse
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    for call in (lambda: eng.graph_reverse(), lambda: eng.graph_edge_pair(0, torch.zeros((eng.e_cap, 4), device=dev))):
        with pytest.raises(LbHipError, match="-3.*overflowed"):
            call()


# ------------------------------------------------------------------------------------------------ the model
def _model_case(cid):
    """(features, engine, particle types, engine case) of rpf2d_b2 or asym, built for the caller alone."""
    from tests._common import hip_case
    if cid == "asym":
        from tests._asym import asym_case
        ds, pos, pt, _ = asym_case("tgv2d", B=2)
    else:
        from lagrangebench_amd.data import make_case
        ds = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
        pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
        pt = np.stack([ds[b][1] for b in range(2)])
    hcase = hip_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :ds.input_seq_length], pt))
    return feats, feats.engine, pt, hcase


def _momentum_model(eng, antisym=True, tap=False, autocast=None):
    from lagrangebench_amd.models import TorchModel
    from tests import _torch_models as TM
    model = TorchModel(GM.MomentumMP(TM.node_in_of(eng), eng.dim, 32, antisym=antisym, tap=tap), autocast=autocast)
    params, state = model.init(np.array([7]), None)
    rng = np.random.default_rng(3)
    params["~"]["gain"] = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32)
    state["~"]["in_scale"] = (1.0 + 0.1 * rng.standard_normal(state["~"]["in_scale"].shape)).astype(np.float32)
    model.set_state(state)
    return model, params, state


@pytest.mark.parametrize("cid", ["rpf2d_b2", "asym"])
def test_momentum_is_conserved_to_the_rounding_of_the_row_sums(cid):
    """MomentumMP in models.TorchModel.  Its edge field m = antisymmetrize(...) must satisfy m[rev] == -m, with +0.0 on the
    unpaired, self and pad slots; so the real slots of m are a multiset closed under negation and their exact sum
    (math.fsum), per trajectory and component, is exactly 0.0.

    The bound on the total momentum.  acc_i is the ordered float32 sum of the d_i terms of row i: acc_i = S_i + err_i with S_i
    the exact row sum and |err_i| <= gamma(d_i - 1) sum_{j in row i} |m_j|, gamma(k) = k u / (1 - k u), u = 2^-24 (the standard
    bound of recursive summation).  The rows partition the real slots, so sum_i S_i is the exact sum of m, which is 0, and

        |sum_i acc_i| = |sum_i err_i| <= gamma(d_max - 1) sum_j |m_j| <= 2^-24 d_max sum_j |m_j|

    (gamma(d - 1) <= d u for every d below 2^12).  The left side is formed in float64 from the float32 acc_i (exact to 2^-53
    relative, far below the bound).  Control: the same network, same weights, without antisymmetrize exceeds the bound on the
    same input - there sum_i acc_i is the sum of m_ij + m_ji over the pairs, which no symmetry cancels."""
    _need_gpu()
    feats, eng, pt, _ = _model_case(cid)
    B, dim = eng.B, eng.dim
    i, ne = eng.nl_idx()
    i, ne = _np(i), _np(ne)
    r_idx, s_idx = i[:, 0], i[:, 1]
    rev = GR.np_reverse(r_idx, s_idx, ne)
    lone = int((rev[np.arange(rev.shape[1])[None, :] < ne[:, None]] < 0).sum())
    assert lone == (6 if cid == "asym" else 0)
    totals = {}
    for antisym in (True, False):
        model, params, state = _momentum_model(eng, antisym=antisym, tap=True)
        GM.MomentumMP.last = None
        out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
        m, acc = (_np(t) for t in GM.MomentumMP.last)
        GM.MomentumMP.last = None
        assert m.shape == (B, eng.e_cap, dim) and m.dtype == np.float32 and np.array_equal(acc, out)
        for b in range(B):
            n = int(ne[b])
            deg = int(np.bincount(r_idx[b, :n]).max())
            for c in range(dim):
                col = m[b, :n, c].astype(np.float64)
                bound = 2.0 ** -24 * deg * float(np.abs(col).sum())
                total = abs(float(acc[b, :, c].astype(np.float64).sum()))
                totals[(antisym, b, c)] = (total, bound, math.fsum(col.tolist()), deg)
        if antisym:
            check_zeros(m, rev, ne)
            for b in range(B):
                n = int(ne[b])
                p = rev[b, :n]
                ok = p >= 0
                assert np.array_equal(m[b, :n][ok], -m[b, p[ok]])                      # m[rev] == -m
                own = r_idx[b, :n] == s_idx[b, :n]
                assert own.any() and not m[b, :n][own].any() and np.abs(m[b, :n]).max() > 0
    for (antisym, b, c), (total, bound, exact, deg) in totals.items():
        print(f"[momentum {cid} antisymmetrize={antisym} b={b} c={c}] |sum acc| {total:.3e}, bound {bound:.3e} (max degree {deg}), "
              f"fsum of m {exact!r}")
    for (antisym, b, c), (total, bound, exact, _) in totals.items():
        if antisym:
            assert exact == 0.0 and total <= bound, (b, c, total, bound, exact)
        else:
            assert total > bound, (b, c, total, bound)                                 # the control: the assertion bites


def _cpu_run(model, params, state, feats, ne, pt, dtype, target):
    from tests import _torch_models as TM
    from tests.test_torch_model_gpu import _cpu_module
    mod = _cpu_module(model, params, state, dtype)
    fd = TM.cpu_features(feats, dtype)
    pred = mod(fd, torch.as_tensor(pt).long(), GM.CpuReverseGraph(fd["senders"], fd["receivers"], ne, pt.shape[1]))
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach(), mod, float(mean.detach())


@pytest.mark.parametrize("cid", ["rpf2d_b2", "ldc3d"])
def test_momentum_model_forward_and_gradients_match_the_float64_restatement(cid):
    """The two-step rule of tests/test_torch_model_gpu.py: within the bar of the float64 restatement, or within 3x the float32
    restatement's own deviation from it."""
    _need_gpu()
    from tests._common import hip_case
    from tests.test_torch_model_gpu import CASES as MODEL_CASES, _dataset, _two_step
    B = MODEL_CASES[cid][3]
    ds = _dataset(cid)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    model, params, state = _momentum_model(hcase.engine(B))
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert out.shape == (B, eng.N, eng.dim) and GR.same_bits(out, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    tg = torch.randn((B, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[momentum forward {cid}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}"
          f"{'' if ok else ' (held to the fp32 restatement)'}")
    assert ok or ok32, (cid, e, e32)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[momentum loss {cid}] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. "
          f"{abs(l32 - l64) / abs(l64):.2e}{'' if el <= 1e-5 else ' (held to the fp32 restatement)'}")
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
    print(f"[momentum grad {cid}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, (cid, bad)
    for name in ("enc", "ws", "wr", "we", "dec"):              # the gradient passed through antisymmetrize to every layer
        assert np.abs(g_h[name]["weight"]).max() > 0, name
    assert np.abs(g_h["~"]["gain"]).max() > 0


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
def test_momentum_model_takes_a_trainer_step(autocast):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.train import Trainer
    from tests._common import hip_case
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _momentum_model(case.engine(2), autocast=autocast)
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 1}, input_seq_length=ISL, seed=0)
    params, state, opt = trainer.train(step_max=1)
    losses = [l for _, l in trainer.loss_log]
    print(f"[momentum trainer autocast={autocast}] losses {['%.5e' % l for l in losses]}")
    assert len(losses) == 2 and np.isfinite(losses).all() and opt["count"] == 2 and np.abs(opt["m"]).max() > 0
    assert all(v.dtype == np.float32 for mod in params.values() for v in mod.values())


# ------------------------------------------------------------------------------------------------ the window gradient
@pytest.mark.parametrize("cid", ["rpf2d_b1", "asym_b2"])
def test_window_gradient_flows_through_antisymmetrize(cid):
    """MomentumMP through autograd.TorchModule with a window that requires grad: rel_disp reaches the loss only through
    antisymmetrize, so its share of d loss / d window is the op's backward carried on to lb_graph_features_backward.  Against
    float64 autograd of tests/_features_torch.py + CpuReverseGraph on the engine's own list, with the bars of
    tests/test_torch_window_grad_gpu.py: forward and loss 1e-5, d loss / d window 1e-4 of its largest entry, a parameter leaf
    1e-4 or 3x the float32 restatement's own deviation."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule
    from tests import test_torch_window_grad_gpu as WG
    from tests._features_torch import features_torch
    ds, hcase, pos, pt, consts = WG._setup(cid)
    feats, eng = WG._allocate(cid)
    B, N, dim = eng.B, eng.N, eng.dim
    model, params, state = _momentum_model(eng)
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
    force = WG._force(eng)
    got_w, got_p = _np(window.grad), WG._grads(mod.module)

    def restate(module, dtype, windows, graph=GM.CpuReverseGraph):
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
    print(f"[momentum window grad {cid}] forward {e_fwd:.2e}; loss {e_loss:.2e}; d loss / d window {e_win:.2e} (largest entry "
          f"{np.abs(w64).max():.3e}; the fp32 restatement {np.abs(refs[torch.float32][2] - w64).max() / np.abs(w64).max():.2e})")
    assert e_fwd <= 1e-5 and e_loss <= 1e-5, (e_fwd, e_loss)
    assert got_w.dtype == np.float64 and np.isfinite(got_w).all() and e_win < 1e-4, e_win
    WG._leaf_report(f"momentum {cid}", got_p, g64, refs[torch.float32][3])
    # all of it passes through the op's backward: with that cut (the forward unchanged) nothing reaches the window
    m = model._device_module(WG._Cpu(), params, state).to(torch.float64)
    ws = [torch.as_tensor(pos[b, :, :WG.ISL]).clone().requires_grad_(True) for b in range(B)]

    class _Cut(GM.CpuReverseGraph):
        def antisymmetrize(self, msg):
            return super().antisymmetrize(msg.detach()) + 0.0 * msg

    WG._mse(restate(m, torch.float64, ws, _Cut), target, WG._mask(pt)).backward()
    cut = np.stack([(w.grad if w.grad is not None else torch.zeros_like(w)).numpy() for w in ws])
    share = np.abs(cut - w64).max() / np.abs(w64).max()
    print(f"[momentum window grad {cid}] the share of antisymmetrize's backward in d loss / d window: {share:.2e} of the largest entry")
    assert share > 100 * 1e-4                                  # (far above the bar: a missing backward could not pass it)
