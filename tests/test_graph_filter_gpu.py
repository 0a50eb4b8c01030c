"""graph.Graph's filter_conv on the device (csrc/lb_graph.hip): conv with its one-Linear filter formed in registers, forward and
backward, against the numpy loops of tests/_graph_filter.py - bit for bit: the r-loop of the filter, the slot order of the sum,
the blocked column order of d_f and the chunked slot order of d_weight are part of the contract, so there is no tolerance on
float32 - and against this library's own conv on an r-loop filter formed in torch, which it replaces.

Cases and roles are those of tests/test_graph_ops_gpu.py (B = 2 behind pads, more than one workgroup of rows, N = 3 with rows
shorter than a wave, the radix-sorted sender view of the asymmetric list).  (R, C): (1, 1) has no r-loop and takes the scalar
path; (3, 5) is odd everywhere with one short column block; (20, 64) is PaiNN's shape on 16-byte units; (32, 130) is the limit of
R, nine column blocks, the last two columns wide, two passes of the gradient kernels' 128 columns and several units per lane;
(20, 128) is the benchmark's shape.  K in {1, 3}.  Every pad slot of f - and of no other tensor - holds NaN; f spans seven decades.

bfloat16: round_to_bf16(the float32 twin(upcast inputs)) bit for bit, with the rounding of tests/_graph_bf16.py, at (20, 64) on
every case and at (32, 520) - 33 column blocks, five passes, a row wider than its lane group, so the forward reloads the weight
per unit - on the three small lists (the numpy twin of d_weight at 32 x 520 on ldc3d alone would take several seconds).  The
model path (TinyFilter in models.TorchModel) uses the two-step rule of tests/test_torch_model_gpu.py, the window gradient the
bars of tests/test_torch_window_grad_gpu.py, both unchanged.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_bf16 as BF  # noqa: E402
from tests import _graph_filter as GF  # noqa: E402
from tests.test_graph_ops_gpu import CASES, ROLES, _build, _setup  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (20, 64), (32, 130), (20, 128)]
KS = [1, 3]
BF16 = [(cid, 20, 64) for cid in CASES] + [(cid, 32, 520) for cid in ("rpf2d_b2", "lj", "asym")]


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


def _basis(rng, B, E, R, ne):
    """f (B, E_cap, R) float32 over seven decades, NaN in every pad slot."""
    return _nan_pads((rng.standard_normal((B, E, R)) * 10.0 ** rng.integers(-3, 4, (B, E, 1))).astype(np.float32), ne)


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


def _run(g, x, f, weight, d, role, eng):
    """One forward and backward of g.filter_conv on fresh leaves -> (out, d_x, d_f, d_weight) as numpy."""
    xd, fd, wd = _dev(x, eng, True), _dev(f, eng, True), _dev(weight, eng, True)
    out = g.filter_conv(xd, fd, wd, role)
    out.backward(_dev(d, eng))
    return _np(out), _np(xd.grad), _np(fd.grad), _np(wd.grad)


def _chunk_kinds(ne, E):
    """Which kinds of chunk the flat padded slots of a list have: (chunks with a real slot, a chunk with real and pad slots, a
    chunk of pads only)."""
    chunk = GF.filter_chunk()
    real = np.zeros(len(ne) * E, bool)
    for b, n in enumerate(ne):
        real[b * E:b * E + int(n)] = True
    pad = -len(real) % chunk
    counts = np.concatenate([real, np.zeros(pad, bool)]).reshape(-1, chunk).sum(1)
    sizes = np.full(len(counts), chunk)
    sizes[-1] -= pad
    return int((counts > 0).sum()), bool(((counts > 0) & (counts < sizes)).any()), bool((counts == 0).any())


def _padded_case():
    """rpf2d B = 2 with the capacity raised by three chunks, built with _build's own helpers: whatever LB_GRAPH_FILTER_CHUNK is,
    each trajectory's slots end in chunks of pads only."""
    from lagrangebench_amd.case_setup.features import NeighborList
    from lagrangebench_amd.data import make_case
    _, eng, _, _, _, hcase = _build("rpf2d_b2")
    ds = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=6, scale=0.25)
    pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(2)])
    eng.nl_set_capacity(eng.cell_capacity, eng.e_cap + 3 * GF.filter_chunk())
    feats, _ = hcase.preprocess_eval((pos[:, :, :6], pt), NeighborList(eng, True))      # (keeps the raised capacity)
    assert feats.engine is eng
    i, ne = eng.nl_idx()
    i, ne = _np(i), _np(ne)
    return feats, eng, {"receivers": i[:, 0], "senders": i[:, 1]}, ne


def test_the_cases_cover_every_kind_of_chunk():
    """Over the cases: at least two chunks with real slots, a chunk that holds real and pad slots (B = 2 behind pads), and a
    chunk of pads only - what the two-level order of d_weight has to get right."""
    _need_gpu()
    kinds = {cid: _chunk_kinds(_case(cid)[3], _case(cid)[1].e_cap) for cid in CASES}
    print(f"[graph filter chunks of {GF.filter_chunk()}] (chunks with real slots, mixed chunk, pads-only chunk): {kinds}")
    assert max(k[0] for k in kinds.values()) >= 2
    assert _chunk_kinds(_case("rpf2d_b2")[3], _case("rpf2d_b2")[1].e_cap)[1]
    assert any(k[2] for k in kinds.values()) or _chunk_kinds(_padded_case()[3], _padded_case()[1].e_cap)[2]


# ------------------------------------------------------------------------------------------------ float32
def _check_float32(cid, feats, eng, idx, ne, R, C, K):
    from lagrangebench_amd.graph import Graph
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(1000 * C + 10 * K + R + len(cid))
    x = rng.standard_normal((B, N, K, C)).astype(np.float32)
    d = rng.standard_normal((B, N, K, C)).astype(np.float32)
    f = _basis(rng, B, E, R, ne)
    weight = rng.standard_normal((R, C)).astype(np.float32)
    xs, ds = (x[:, :, 0], d[:, :, 0]) if K == 1 else (x, d)          # K = 1 goes in as (B, N, C)
    for role in ROLES:
        other = GF.OTHER[role]
        ir, io = idx[role], idx[other]
        got = _run(g, xs, f, weight, ds, role, eng)
        assert got[0].shape == xs.shape and got[1].shape == xs.shape and got[2].shape == (B, E, R) and got[3].shape == (R, C)
        assert all(np.isfinite(a).all() for a in got), (cid, role, R, C, K, "finite")
        want_df, want_dw = GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E)
        assert _same(got[0].reshape(x.shape), GF.np_filter_conv(x, f, weight, ir, io, ne, N)), (cid, role, R, C, K, "forward")
        assert _same(got[1].reshape(x.shape), GF.np_filter_conv(d, f, weight, io, ir, ne, N)), (cid, role, R, C, K, "d_x")
        assert _same(got[2], want_df), (cid, role, R, C, K, "d_f", np.abs(got[2] - want_df).max())
        assert _same(got[3], want_dw), (cid, role, R, C, K, "d_weight", np.abs(got[3] - want_dw).max())
        assert _pads_are_zero(got[2], ne)
        # ---- this library's own conv on the r-loop filter formed in torch (one rounded product, one add per further r)
        f2, wt = _dev(np.nan_to_num(f), eng), _dev(weight, eng)
        wf = f2[..., 0:1] * wt[0]
        for r in range(1, R):
            wf = wf + f2[..., r:r + 1] * wt[r]
        assert _same(_np(g.conv(_dev(xs, eng), wf, role)), got[0]), (cid, role, R, C, K, "conv on the torch filter")
        assert _same(_np(g.conv(_dev(ds, eng), wf, other)), got[1]), (cid, role, R, C, K, "conv on the torch filter, d_x")
        # ---- a second call: the same bits
        again = _run(g, xs, f, weight, ds, role, eng)
        assert all(_same(p, q) for p, q in zip(got, again)), (cid, role, R, C, K, "second call")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R,C", SHAPES)
@pytest.mark.parametrize("cid", CASES)
def test_filter_conv_equals_numpy_and_conv_on_the_loop_filter_bit_for_bit(cid, R, C, K):
    _need_gpu()
    feats, eng, idx, ne, pairs, _ = _case(cid)
    _check_float32(cid, feats, eng, idx, ne, R, C, K)
    if pairs is not None:
        assert eng.graph_sender_sorts() >= 1


def test_filter_conv_on_a_list_with_chunks_of_pads_only():
    _need_gpu()
    feats, eng, idx, ne = _padded_case()
    many, mixed, empty = _chunk_kinds(ne, eng.e_cap)
    assert many >= 2 and mixed and empty, (many, mixed, empty)
    _check_float32("padded", feats, eng, idx, ne, 20, 64, 3)


@pytest.mark.parametrize("cid", ["rpf2d_b2", "asym"])
def test_d_weight_starts_from_plus_zero(cid):
    """The input that tells "start from +0.0" from "start from the first term": x = 1, the cotangent -0.0, f = 1, so every term
    of d_weight is -0.0.  The contract's partials and total start at +0.0 and +0.0 + -0.0 = +0.0: every bit of d_weight is zero.
    A partials or a finish kernel that started from its first term would give -0.0."""
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, N, E, R, C = eng.B, eng.N, eng.e_cap, 20, 64
    g = Graph(feats)
    weight = np.random.default_rng(0).standard_normal((R, C)).astype(np.float32)
    for K in KS:
        x = np.ones((B, N, K, C), np.float32)
        d = -0.0 * x
        f = _nan_pads(np.ones((B, E, R), np.float32), ne)
        for role in ROLES:
            other = GF.OTHER[role]
            got = _run(g, x, f, weight, d, role, eng)
            assert (_bits(got[3]) == 0).all(), (cid, role, K, np.unique(_bits(got[3])))
            want_df, want_dw = GF.np_filter_edge_grad(x, d, f, weight, idx[role], idx[other], ne, E)
            _, first = GF.np_filter_edge_grad(x, d, f, weight, idx[role], idx[other], ne, E, from_first=True)
            assert _same(got[3], want_dw) and _same(got[2], want_df) and (_bits(first) == 0x80000000).all()


# ------------------------------------------------------------------------------------------------ bfloat16
def _bf(a):
    """float32 -> (its bfloat16 bits, the float32 values they hold); a NaN stays a NaN."""
    bits = BF.round_bf16(a)
    return bits, BF.widen(bits)


def _rb(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return BF.round_bf16(a)


@pytest.mark.parametrize("cid,R,C", BF16)
def test_bfloat16_is_the_rounded_float32_op_bit_for_bit(cid, R, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(31 * C + R + len(cid))
    f_bits, f = _bf(_basis(rng, B, E, R, ne))
    w_bits, weight = _bf(rng.standard_normal((R, C)).astype(np.float32))
    for K in KS:
        x_bits, x = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        d_bits, d = _bf(rng.standard_normal((B, N, K, C)).astype(np.float32))
        for role in ROLES:
            other = GF.OTHER[role]
            ir, io = idx[role], idx[other]
            xd, fd, wd = (BF.from_bits(b, eng.device, True) for b in (x_bits, f_bits, w_bits))
            out = g.filter_conv(xd, fd, wd, role)
            assert out.dtype == torch.bfloat16
            out.backward(BF.from_bits(d_bits, eng.device))
            assert xd.grad.dtype == fd.grad.dtype == wd.grad.dtype == torch.bfloat16
            got = tuple(BF.torch_bits(t) for t in (out, xd.grad, fd.grad, wd.grad))
            want = (GF.np_filter_conv(x, f, weight, ir, io, ne, N), GF.np_filter_conv(d, f, weight, io, ir, ne, N)) + \
                GF.np_filter_edge_grad(x, d, f, weight, ir, io, ne, E)
            for a, b, what in zip(got, want, ("forward", "d_x", "d_f", "d_weight")):
                assert BF.same_bits(a, _rb(b)), (cid, role, R, C, K, what)
                assert np.isfinite(BF.widen(a)).all()
            assert _pads_are_zero(got[2], ne, np.uint16)


def test_bfloat16_filter_conv_is_not_the_composition_and_takes_a_float32_weight():
    """One planted row: x = 1, f = [256, 1, 1, 1, 1] down five slots of one node in one column of the basis, weight = 1.
    filter_conv keeps wf and the terms in float32 and rounds the ordered sum once: 260.  Held in bfloat16, the running sum of the
    composition stays 256 (256 + 1 is a tie that rounds back).  Then a float32 weight beside bfloat16 x and f: the same bits,
    and a float32 gradient."""
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    from tests.test_graph_ops_gpu import np_gather
    feats, eng, idx, ne, _, _ = _case("rpf2d_b1")
    B, N, E, R, C = eng.B, eng.N, eng.e_cap, 3, 64
    g = Graph(feats)
    for role in ROLES:
        other = GF.OTHER[role]
        real = idx[role][0, :ne[0]]
        node = int(np.flatnonzero(np.bincount(real, minlength=N) >= 5)[0])
        slots = np.flatnonzero(real == node)
        f = np.zeros((B, E, R), np.float32)
        f[0, slots[:5], 1] = np.array(BF.PLANTED_ROWS[0], np.float32)
        f = _nan_pads(f, ne)
        x, weight = np.ones((B, N, C), np.float32), np.ones((R, C), np.float32)
        xb, fb, wb = (BF.from_bits(BF.round_bf16(a), eng.device) for a in (x, f, weight))
        out = g.filter_conv(xb, fb, wb, role)
        assert (BF.widen(BF.torch_bits(out))[0, node] == BF.PLANTED_SUMS[0]).all(), (role, BF.widen(BF.torch_bits(out))[0, node])
        wf = np.nan_to_num(f).sum(-1, keepdims=True) * np.ones((1, 1, C), np.float32)     # (exact: one non-zero column)
        msg = BF.round_bf16(np_gather(x, idx[other], ne) * wf)
        held = BF.widen(BF.np_segment_sum_bf16_acc(msg, idx[role], ne, N))
        assert (held[0, node] == 256.0).all()
        # ---- a float32 weight (a Parameter under autocast): cast inside, the gradient comes back float32
        w32 = torch.ones((R, C), device=eng.device, requires_grad=True)
        xg, fg = xb.detach().requires_grad_(True), fb.detach().requires_grad_(True)
        out32 = g.filter_conv(xg, fg, w32, role)
        assert out32.dtype == torch.bfloat16 and torch.equal(out32.view(torch.int16), out.view(torch.int16))
        out32.float().sum().backward()
        assert w32.grad.dtype == torch.float32 and w32.grad.shape == (R, C) and xg.grad.dtype == fg.grad.dtype == torch.bfloat16
        assert torch.isfinite(w32.grad).all() and float(w32.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ memory
def test_forward_allocates_its_output_and_the_backward_nothing_edge_by_channel():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _case("ldc3d")
    B, N, E, R, C, K = eng.B, eng.N, eng.e_cap, 20, 64, 3
    g = Graph(feats)
    x = torch.randn((B, N, K, C), device=eng.device, requires_grad=True)
    f = torch.randn((B, E, R), device=eng.device, requires_grad=True)
    weight = torch.randn((R, C), device=eng.device, requires_grad=True)
    slack, edge_tensor = 64 * 1024, B * E * C * 4
    out_bytes, f_bytes, w_bytes = B * N * K * C * 4, B * E * R * 4, R * C * 4
    partials = -(-B * E // GF.filter_chunk()) * R * C * 4
    print(f"[filter memory] output {out_bytes} bytes, d_f {f_bytes}, d_weight {w_bytes}, partials {partials}; one (E_cap, C) tensor "
          f"{edge_tensor} bytes")
    assert out_bytes + slack < edge_tensor and partials + w_bytes + slack < edge_tensor
    for role in ROLES:
        g.filter_conv(x, f, weight, role)                     # (the first sender call builds the engine's sender view)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = g.filter_conv(x, f, weight, role)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print(f"[filter memory] forward {role}: rise {rise} bytes")
        assert rise <= out_bytes + slack, (role, rise)
        del out
    # ---- the backward: the results and the partials, nothing of E_cap x C elements; what is not required is not allocated
    calls = []
    grad, conv = eng.graph_filter_conv_grad, eng.graph_filter_conv
    eng.graph_filter_conv_grad = lambda *a: (calls.append(tuple(bool(v) for v in a[-2:])), grad(*a))[1]
    eng.graph_filter_conv = lambda *a: (calls.append("conv"), conv(*a))[1]
    try:
        for need_x, need_f, need_w in ((True, True, True), (True, False, True), (False, False, True), (False, True, False),
                                       (True, False, False)):
            xd, fd, wd = x.detach().requires_grad_(need_x), f.detach().requires_grad_(need_f), weight.detach().requires_grad_(need_w)
            out = g.filter_conv(xd, fd, wd, "senders")
            cot = torch.ones_like(out)
            calls.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out.backward(cot)
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
            assert calls == ["conv"] * need_x + [(need_f, need_w)] * (need_f or need_w), (need_x, need_f, need_w, calls)
            assert (xd.grad is not None) == need_x and (fd.grad is not None) == need_f and (wd.grad is not None) == need_w
            bound = need_x * out_bytes + need_f * f_bytes + need_w * (w_bytes + partials) + slack
            print(f"[filter memory] backward, d_x {need_x}, d_f {need_f}, d_weight {need_w}: rise {rise} bytes, bound {bound}")
            assert rise <= bound and bound - need_x * out_bytes - need_f * f_bytes < edge_tensor, (need_x, need_f, need_w, rise, bound)
    finally:
        for name in ("graph_filter_conv_grad", "graph_filter_conv"):
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
    f = torch.randn((1, E, 5), device=eng.device, requires_grad=True)
    weight = torch.randn((5, 4), device=eng.device, requires_grad=True)
    shapes = r"\(1, %d, 'C'\).*\(1, %d, 'K', 'C'\).*\(1, %d, 'R'\).*\('R', 'C'\).*1 <= R <= 32.*got" % (N, N, E)
    zeros = lambda *s: torch.zeros(s, device=eng.device)
    for args in ((zeros(1, N, 3), f, weight), (x, f, zeros(4, 4)), (x, f, zeros(5, 3)), (x, f, zeros(5)), (x, zeros(1, E, 2, 5), weight),
                 (zeros(1, N, 2, 3, 4), f, weight), (x, zeros(1, E, 33), zeros(33, 4))):
        with pytest.raises(ValueError, match=shapes):
            g.filter_conv(*args, "senders")
    with pytest.raises(ValueError, match=shapes):             # a weight that is no tensor
        g.filter_conv(x, f, [[0.0] * 4] * 5, "senders")
    with pytest.raises(ValueError):                           # R = 0
        g.filter_conv(x, torch.zeros((1, E, 0), device=eng.device), torch.zeros((0, 4), device=eng.device), "senders")
    assert g.filter_conv(x, zeros(1, E, 32), zeros(32, 4), "senders").shape == x.shape      # the limit itself
    with pytest.raises(ValueError, match="role"):
        g.filter_conv(x, f, weight, "both")
    bf = lambda t: t.detach().to(torch.bfloat16)
    for args in ((x, bf(f), weight), (bf(x), f, weight), (x, f, bf(weight)), (bf(x), f, bf(weight)), (x, bf(f), bf(weight))):
        with pytest.raises(TypeError, match="one dtype"):
            g.filter_conv(*args, "senders")
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        g.filter_conv(x.detach().double(), f.detach().double(), weight.detach().double(), "senders")
    with pytest.raises(TypeError, match="one dtype"):
        g.filter_conv(x, f, weight.detach().half(), "senders")
    with pytest.raises(TypeError, match="engine on"):
        g.filter_conv(torch.zeros((1, N, 4)), torch.zeros((1, E, 5)), torch.zeros((5, 4)), "senders")
    with pytest.raises(TypeError, match="engine on"):
        g.filter_conv(x, f, torch.zeros((5, 4)), "senders")
    # double backward raises
    out = g.filter_conv(v, f, weight, "senders")
    (gx,) = torch.autograd.grad(out.sum(), v, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # the library's own refusals: role, K < 1, R < 1, R > 32, C < 1, dtype, a null pointer, partials too short
    fx, ff, fw = zeros(N, 3, 4), zeros(E, 5), zeros(5, 4)
    px, pf, pw = (t.data_ptr() for t in (fx, ff, fw))
    out, d_f, d_w = torch.empty_like(fx), torch.empty_like(ff), torch.empty_like(fw)
    conv = eng.lib.lb_graph_filter_conv
    for args in ((2, px, pf, pw, out.data_ptr(), 3, 5, 4, 0), (0, px, pf, pw, out.data_ptr(), 0, 5, 4, 0),
                 (0, px, pf, pw, out.data_ptr(), 3, 0, 4, 0), (0, px, pf, pw, out.data_ptr(), 3, 33, 4, 0),
                 (0, px, pf, pw, out.data_ptr(), 3, 5, 0, 0), (0, px, pf, pw, out.data_ptr(), 3, 5, 4, 2),
                 (0, px, None, pw, out.data_ptr(), 3, 5, 4, 0), (0, px, pf, pw, None, 3, 5, 4, 0)):
        assert conv(eng._h, *args) == -1, args
    assert conv(eng._h, 0, px, pf, pw, out.data_ptr(), 3, 5, 4, 0) == 0
    n = int(eng.lib.lb_graph_filter_partials(eng._h, 5, 4))
    assert n == -(-E // GF.filter_chunk()) * 5 * 4
    part = torch.empty(n, device=eng.device)
    grad = eng.lib.lb_graph_filter_conv_grad
    ok = (0, px, px, pf, pw, d_f.data_ptr(), d_w.data_ptr(), part.data_ptr(), n, 3, 5, 4, 0)
    for k, bad in ((0, 2), (8, n - 1), (9, 0), (10, 0), (10, 33), (11, 0), (12, 2), (1, None), (7, None)):
        assert grad(eng._h, *(ok[:k] + (bad,) + ok[k + 1:])) == -1, (k, bad)
    assert grad(eng._h, *(ok[:5] + (None, None) + ok[7:])) == -1
    assert grad(eng._h, *ok) == 0 and grad(eng._h, *(ok[:6] + (None, None, 0) + ok[9:])) == 0
    # a stale list, in the forward and in the backward of a graph made before
    made = g.filter_conv(x, f, weight, "senders")
    eng.nl_update()
    with pytest.raises(RuntimeError, match="stale"):
        g.filter_conv(x, f, weight, "receivers")
    with pytest.raises(RuntimeError, match="stale"):
        made.sum().backward()
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    cap_f = torch.zeros((eng.e_cap, 5), device=eng.device)
    for call in (lambda: eng.graph_filter_conv(1, fx, cap_f, fw), lambda: eng.graph_filter_conv_grad(0, fx, fx, cap_f, fw)):
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
    N, E, C, K, R = eng.N, eng.e_cap, 8, 2, 6
    rng = np.random.default_rng(2)
    x, d = (rng.standard_normal((N, K, C)).astype(np.float32) for _ in range(2))
    f, weight = _basis(rng, 1, E, R, ne)[0], rng.standard_normal((R, C)).astype(np.float32)
    out, d_x, d_f, d_w = _run(g, x, f, weight, d, "senders", eng)
    assert out.shape == (N, K, C) and d_x.shape == (N, K, C) and d_f.shape == (E, R) and d_w.shape == (R, C)
    assert _same(out, GF.np_filter_conv(x[None], f[None], weight, s_idx, r_idx, ne, N)[0])
    want_df, want_dw = GF.np_filter_edge_grad(x[None], d[None], f[None], weight, s_idx, r_idx, ne, E)
    assert _same(d_f, want_df[0]) and _same(d_w, want_dw)
    got = g.filter_conv(_dev(x[:, 0], eng), _dev(f, eng), _dev(weight, eng), "receivers")
    assert got.shape == (N, C)
    assert _same(_np(got), GF.np_filter_conv(x[None, :, :1], f[None], weight, r_idx, s_idx, ne, N)[0, :, 0])


# ------------------------------------------------------------------------------------------------ through the model path
ISL = 6


def _filter_model(eng, autocast=None):
    from lagrangebench_amd.models import TorchModel
    from tests import _torch_models as TM
    model = TorchModel(GF.TinyFilter(TM.node_in_of(eng), eng.dim, 32), autocast=autocast)
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
    pred = mod(fd, torch.as_tensor(pt).long(), GF.CpuFilterGraph(fd["senders"], fd["receivers"], ne, pt.shape[1]))
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach(), mod, float(mean.detach())


@pytest.mark.parametrize("cid", ["rpf2d_b2", "ldc3d"])
def test_tiny_filter_forward_and_gradients_match_the_float64_restatement(cid):
    _need_gpu()
    from tests._common import hip_case
    from tests.test_torch_model_gpu import CASES as MODEL_CASES, _dataset, _two_step
    B = MODEL_CASES[cid][3]
    ds = _dataset(cid)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    model, params, state = _filter_model(hcase.engine(B))
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert out.shape == (B, eng.N, eng.dim) and _same(out, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    tg = torch.randn((B, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[tiny filter forward {cid}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}"
          f"{'' if ok else ' (held to the fp32 restatement)'}")
    assert ok or ok32, (cid, e, e32)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[tiny filter loss {cid}] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. "
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
    print(f"[tiny filter grad {cid}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, (cid, bad)
    for name in ("enc", "vec", "dec"):                        # every op's gradient arrived
        assert np.abs(g_h[name]["weight"]).max() > 0, name
    for leaf in ("gain", "w_s", "w_v"):
        assert np.abs(g_h["~"][leaf]).max() > 0, leaf


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
def test_tiny_filter_takes_a_trainer_step_and_round_trips_a_checkpoint(tmp_path, autocast):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
    from tests._common import hip_case
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _filter_model(case.engine(2), autocast)
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 1}, input_seq_length=ISL, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt = trainer.train(step_max=1, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    print(f"[tiny filter trainer autocast={autocast}] losses {['%.5e' % l for l in losses]}")
    assert len(losses) == 2 and np.isfinite(losses).all() and opt["count"] == 2 and np.abs(opt["m"]).max() > 0
    assert all(v.dtype == np.float32 for mod in params.values() for v in mod.values())
    loaded, _, lopt, step = load_haiku(ckp)
    assert step == 1 and set(loaded) == set(params) and set(lopt) >= {"m", "v", "count"}
    assert _same(model.flatten(model.params_from_haiku(loaded)), model.flatten(params))


# ------------------------------------------------------------------------------------------------ the window gradient through d_f
@pytest.mark.parametrize("cid", ["rpf2d_b1", "asym_b2"])
def test_window_gradient_flows_through_d_f(cid):
    """TinyFilter through autograd.TorchModule with a window that requires grad: rel_dist reaches the loss only as the basis f of
    the two filter_conv, so its share of d loss / d window is d_f carried on to lb_graph_features_backward.  Against float64
    autograd of tests/_features_torch.py + CpuFilterGraph on the engine's own list, with the bars of
    tests/test_torch_window_grad_gpu.py: forward and loss 1e-5, d loss / d window 1e-4 of its largest entry, a parameter leaf
    1e-4 or 3x the float32 restatement's own deviation."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule
    from tests import test_torch_window_grad_gpu as WG
    from tests._features_torch import features_torch
    ds, hcase, pos, pt, consts = WG._setup(cid)
    feats, eng = WG._allocate(cid)
    B, N, dim = eng.B, eng.N, eng.dim
    model, params, state = _filter_model(eng)
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

    def restate(module, dtype, windows, graph=GF.CpuFilterGraph):
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
    print(f"[filter window grad {cid}] forward {e_fwd:.2e}; loss {e_loss:.2e}; d loss / d window {e_win:.2e} (largest entry "
          f"{np.abs(w64).max():.3e}; the fp32 restatement {np.abs(refs[torch.float32][2] - w64).max() / np.abs(w64).max():.2e})")
    assert e_fwd <= 1e-5 and e_loss <= 1e-5, (e_fwd, e_loss)
    assert got_w.dtype == np.float64 and np.isfinite(got_w).all() and e_win < 1e-4, e_win
    WG._leaf_report(f"filter {cid}", got_p, g64, refs[torch.float32][3])
    # the part of it that came through f: with f detached in the restatement the window gradient is another one
    m = model._device_module(WG._Cpu(), params, state).to(torch.float64)
    ws = [torch.as_tensor(pos[b, :, :WG.ISL]).clone().requires_grad_(True) for b in range(B)]

    class _CutF(GF.CpuFilterGraph):
        def filter_conv(self, x, f, weight, role):
            return super().filter_conv(x, f.detach(), weight, role)

    WG._mse(restate(m, torch.float64, ws, _CutF), target, WG._mask(pt)).backward()
    cut = np.stack([w.grad.numpy() for w in ws])
    share = np.abs(cut - w64).max() / np.abs(w64).max()
    print(f"[filter window grad {cid}] the share of d_f in d loss / d window: {share:.2e} of the largest entry")
    assert share > 100 * 1e-4                                  # (far above the bar: a missing d_f could not pass it)
