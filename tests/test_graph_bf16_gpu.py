"""graph.Graph on bfloat16 tensors on the device (csrc/lb_graph.hip, the lb_graph_*_t entries) and
models.TorchModel(autocast=torch.bfloat16).  The contract, for every op and every backward:

    the bfloat16 op  ==  round_to_bf16( the float32 op( upcast(inputs) ) )        bit for bit (view(uint16); a NaN matches a NaN)

Cases and roles are those of tests/test_graph_ops_gpu.py.  Columns: 1; 5; 12 (a multiple of 4 but not of 8: float32 would take
16-byte units, bfloat16 must not); 64 (8 lanes of 16 bytes); 136 (past 128, a multiple of 8: a lane owns two units); 520 (65
units of 16 bytes: one more than a row's 64 lanes).  Attend shapes (H, D): (1, 1), (1, 5) elements; (3, 4) 8-byte units; (2,
8), (8, 16) 16-byte units; (2, 65) a head boundary inside a lane's stride; (5, 52) and (5, 104): 65 units of 8 and of 16
bytes, one more than a row's 64 lanes.  Inputs are float32 random values times 10^k, k in -2 .. 2, rounded to bfloat16; every
pad slot holds NaN.

  1  gather / segment_sum, forward and backward, against the numpy twin (tests/_graph_bf16.py), with planted rows: the three
     rows that tell a bfloat16 accumulator and another order from the contract, two exact ties and an overflow to inf
  2  every op and backward against this library's own float32 ops on the widened tensors, rounded once (those are pinned by
     tests/test_graph_ops_gpu.py and tests/test_graph_attention_gpu.py)
  3  segment_softmax and attend against the float64 restatements on the same inputs: today's bound (1e-5 of the scale
     tests/test_graph_attention_gpu.py uses) plus one bfloat16 rounding, 2^-8 |reference| per element; softmax rows sum to 1
     within (deg + 8) 2^-24 + deg 2^-9 (deg roundings of at most 2^-9 each)
  4  a tensor whose storage starts one element (2 bytes; for float32 4 bytes) off alignment gives the aligned call's bits
  5  TorchModel(autocast=torch.bfloat16): per output and gradient leaf the deviation from the float64 CPU restatement is at
     most 3x that of the CPU restatement under torch.autocast("cpu", bfloat16) on CpuGraphBf16; Trainer, checkpoint, infer,
     autograd.TorchModule
  6  refusals on the device
"""
import functools
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_attention as GA  # noqa: E402
from tests import _graph_bf16 as GB  # noqa: E402
from tests import _torch_models as TM  # noqa: E402
from tests.test_graph_ops_gpu import CASES, ROLES, _build, _np, np_gather  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = [1, 5, 12, 64, 136, 520]
SHAPES = [(1, 1), (1, 5), (3, 4), (2, 8), (8, 16), (2, 65), (5, 52), (5, 104)]
NAN = 0x7FC0
BF = torch.bfloat16
TIE_DOWN, TIE_UP, OVERFLOW = [1.0, 2.0 ** -8], [1.0 + 2.0 ** -7, 2.0 ** -8], [GB.widen([0x7F7F])[0], 2.0 ** 119]
PLANTED = list(GB.PLANTED_ROWS) + [TIE_DOWN, TIE_UP, OVERFLOW]
PLANTED_BITS = [GB.round_bf16(np.float32(v)) for v in GB.PLANTED_SUMS] + [0x3F80, 0x3F82, 0x7F80]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _setup(cid):
    """The cases of tests/test_graph_ops_gpu.py, built once for this file: the copies that module caches have moved on by the
    time this file runs (the last test of tests/test_graph_attention_gpu.py allocates another sample on rpf2d_b1's engine)."""
    return _build(cid)


def _rand_bits(rng, shape):
    x = rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3, shape[:-1] + (1,))
    return GB.round_bf16(x.astype(np.float32))


def _pad_nan(bits, ne):
    bits = bits.copy()
    for b in range(bits.shape[0]):
        bits[b, ne[b]:] = NAN
    return bits


def _pads_zero(bits, ne):
    return all((bits[b, ne[b]:] == 0).all() for b in range(bits.shape[0]))


def _dev(bits, eng, grad=False):
    return GB.from_bits(bits, eng.device, grad)


def _b(t):
    return GB.torch_bits(t)


@functools.lru_cache(maxsize=None)
def _slots(cid, role):
    _, eng, idx, ne, _, _ = _setup(cid)
    return GA.node_slots(idx[role], ne, eng.N)


def _plant(bits, cid, role):
    """Overwrite, per trajectory, the slots of one node per planted row (every column alike; the row padded with zeros to the
    node's degree) -> [(b, node, expected bits)]."""
    done = []
    for b, row in enumerate(_slots(cid, role)):
        used = set()
        for terms, want in zip(PLANTED, PLANTED_BITS):
            node = next((i for i, s in enumerate(row) if len(s) >= max(5, len(terms)) and i not in used), None)
            if node is None:
                continue
            used.add(node)
            vals = np.zeros(len(row[node]), np.float32)
            vals[:len(terms)] = terms
            bits[b, row[node]] = GB.round_bf16(vals)[:, None]
            done.append((b, node, want))
    return done


# ------------------------------------------------------------------------------------------------ 1: the numpy twin
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_gather_and_segment_sum_equal_the_numpy_twin(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(100 * C + len(cid))
    xb, wb = _rand_bits(rng, (B, N, C)), _rand_bits(rng, (B, N, C))
    for role in ROLES:
        mb = _rand_bits(rng, (B, E, C))
        planted = _plant(mb, cid, role)
        assert len(planted) == len(PLANTED) * B or cid == "lj"
        xd = _dev(xb, eng, True)
        got = g.gather(xd, role)
        assert got.dtype == BF and got.shape == (B, E, C)
        want_g = GB.round_bf16(np_gather(GB.widen(xb), idx[role], ne))
        assert np.array_equal(_b(got), want_g) and _pads_zero(_b(got), ne), (cid, role, C)
        got_s = _b(g.segment_sum(_dev(_pad_nan(mb, ne), eng), role))
        want_s = GB.np_segment_sum_bf16(mb, idx[role], ne, N)
        assert np.array_equal(got_s, want_s), (cid, role, C, int((got_s != want_s).sum()))
        for b, node, want in planted:
            assert (got_s[b, node] == want).all(), (cid, role, C, b, node, hex(int(got_s[b, node, 0])), hex(int(want)))
        # backward of (segment_sum(gather(x)) * w).sum(): the two adjoints, each rounded once
        y = g.segment_sum(g.gather(xd, role), role)
        (y * _dev(wb, eng)).sum().backward()
        assert xd.grad.dtype == BF
        mid = GB.round_bf16(np_gather(GB.widen(wb), idx[role], ne))
        assert np.array_equal(_b(xd.grad), GB.np_segment_sum_bf16(mid, idx[role], ne, N)), (cid, role, C)
        assert np.array_equal(_b(y), GB.np_segment_sum_bf16(want_g, idx[role], ne, N))
        assert np.array_equal(_b(g.segment_sum(_dev(_pad_nan(mb, ne), eng), role)), got_s)       # two calls: the same bits
        assert np.array_equal(_b(g.gather(_dev(xb, eng), role)), want_g)


# ------------------------------------------------------------------------------------------------ 2: the library's float32 ops
def _r(t):
    """float32 result -> bfloat16 bits, rounded once."""
    return _b(t.to(BF))


@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_column_ops_equal_the_rounded_float32_ops(cid, C):
    _need_gpu()
    feats, eng, idx, ne, _, _ = _setup(cid)
    from lagrangebench_amd.graph import Graph
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(7 * C + len(cid))
    for r, role in enumerate(ROLES):
        mb = _rand_bits(rng, (B, E, C))
        _plant(mb, cid, role)
        slots = _slots(cid, role)
        rich = [s for s in slots[0] if len(s) >= 2]
        if len(rich) >= 2:                                        # a tie at the top; -0.0 then +0.0 among -1s
            mb[0, rich[-1][:2], 0] = GB.round_bf16(np.float32(1e4))
            mb[0, rich[-2], 0] = GB.round_bf16(np.float32(-1.0))
            mb[0, rich[-2][0], 0], mb[0, rich[-2][1], 0] = 0x8000, 0x0000
        mb[0, int(ne[0]) // 2, C // 2] = NAN                      # a NaN in a real slot: it wins its column and stays
        m = _dev(_pad_nan(mb, ne), eng).reshape(B * E, C)
        m32 = m.float()
        dn = _dev(_rand_bits(rng, (B, N, C)), eng).reshape(B * N, C)
        de = _dev(_pad_nan(_rand_bits(rng, (B, E, C)), ne), eng).reshape(B * E, C)
        # ---- sum, mean
        assert GB.same_bits(_b(eng.graph_segment_sum(r, m)), _r(eng.graph_segment_sum(r, m32))), (cid, role, C)
        # (the mean is DEFINED on the rounded sum - the float32 sum rounded once, one float32 division, one rounding - so it is
        # held to that, not to the float32 mean rounded once)
        deg = g.degree(role).clamp(min=1).float().reshape(B * N, 1)
        want_mean = (eng.graph_segment_sum(r, m32).to(BF).float() / deg).to(BF)
        assert GB.same_bits(_b(g.segment_mean(m.reshape(B, E, C), role)).reshape(B * N, C), _b(want_mean)), (cid, role, C)
        assert GB.same_bits(_b(eng.graph_gather(r, dn)), _r(eng.graph_gather(r, dn.float())))
        # ---- max / min: the value, the winning slot, the backward
        for minimum in (False, True):
            out, win = eng.graph_segment_max(r, m, minimum)
            out32, win32 = eng.graph_segment_max(r, m32, minimum)
            assert out.dtype == BF and win.dtype == torch.int32
            assert GB.same_bits(_b(out), _r(out32)) and torch.equal(win, win32), (cid, role, C, minimum)
            d = eng.graph_segment_max_backward(r, dn, win)
            assert np.array_equal(_b(d), _r(eng.graph_segment_max_backward(r, dn.float(), win32))), (cid, role, C, minimum)
            assert _pads_zero(_b(d).reshape(B, E, C), ne)
        assert np.isnan(GB.widen(_b(out))).any(0).sum() == 1      # the NaN reached its column, and only that one
        # ---- softmax and its backward on the saved (rounded) y
        clean = _dev(_pad_nan(_rand_bits(rng, (B, E, C)), ne), eng).reshape(B * E, C)
        y = eng.graph_segment_softmax(r, clean)
        assert GB.same_bits(_b(y), _r(eng.graph_segment_softmax(r, clean.float()))), (cid, role, C)
        assert _pads_zero(_b(y).reshape(B, E, C), ne)
        dx = eng.graph_segment_softmax_backward(r, y, de)
        assert GB.same_bits(_b(dx), _r(eng.graph_segment_softmax_backward(r, y.float(), de.float()))), (cid, role, C)
        assert _pads_zero(_b(dx).reshape(B, E, C), ne)
        assert np.array_equal(_b(eng.graph_segment_softmax(r, clean)), _b(y))


@pytest.mark.parametrize("hd", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cid", CASES)
def test_attend_equals_the_rounded_float32_attend(cid, hd):
    _need_gpu()
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    H, D = hd
    rng = np.random.default_rng(13 * H + D + len(cid))
    for r, role in enumerate(ROLES):
        l = _dev(_pad_nan(_rand_bits(rng, (B, E, H)), ne), eng).reshape(B * E, H)
        v = _dev(_pad_nan(_rand_bits(rng, (B, E, H, D)), ne), eng).reshape(B * E, H, D)
        w = _dev(_rand_bits(rng, (B, N, H, D)), eng).reshape(B * N, H, D)
        out, m, s = eng.graph_attend(r, l, v)
        out32, m32, s32 = eng.graph_attend(r, l.float(), v.float())
        assert out.dtype == BF and m.dtype == torch.float32 and s.dtype == torch.float32
        assert torch.equal(m, m32) and torch.equal(s, s32), (cid, role, hd)       # formed in float32 from the widened logits
        assert GB.same_bits(_b(out), _r(out32)), (cid, role, hd)
        d_l, d_v = eng.graph_attend_backward(r, l, v, m, s, w)
        d_l32, d_v32 = eng.graph_attend_backward(r, l.float(), v.float(), m32, s32, w.float())
        assert GB.same_bits(_b(d_l), _r(d_l32)) and GB.same_bits(_b(d_v), _r(d_v32)), (cid, role, hd)
        assert _pads_zero(_b(d_l).reshape(B, E, H), ne) and _pads_zero(_b(d_v).reshape(B, E, H * D), ne)
        again = eng.graph_attend_backward(r, l, v, m, s, w)
        assert np.array_equal(_b(again[0]), _b(d_l)) and np.array_equal(_b(again[1]), _b(d_v))


# ------------------------------------------------------------------------------------------------ 3: float64
@pytest.mark.parametrize("cid", CASES)
def test_softmax_and_attend_against_float64(cid):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(11 + len(cid))
    R = 2.0 ** -8
    worst = {}

    def hold(name, got, ref, scale):
        over = (np.abs(got - ref) - R * np.abs(ref)) / scale
        worst[name] = max(worst.get(name, 0.0), float(over.max()))
        assert over.max() <= 1e-5, (cid, name, float(over.max()))

    for role in ROLES:
        deg = GA.np_degree(idx[role], ne, N)
        for C in (5, 64):
            shift = GB.to_bf16_values(rng.choice(np.array([0.0, 1e4, -1e4, 88.0], np.float32), (B, N, 1)))
            x = GB.to_bf16_values(3 * rng.standard_normal((B, E, C)).astype(np.float32) + np_gather(shift, idx[role], ne))
            d_y = GB.to_bf16_values(rng.standard_normal((B, E, C)).astype(np.float32))
            xd = _dev(_pad_nan(GB.round_bf16(x), ne), eng, True)
            y = g.segment_softmax(xd, role)
            y.backward(_dev(_pad_nan(GB.round_bf16(d_y), ne), eng))
            yh, dx = GB.widen(_b(y)).astype(np.float64), GB.widen(_b(xd.grad)).astype(np.float64)
            assert np.isfinite(yh).all() and _pads_zero(_b(y), ne) and _pads_zero(_b(xd.grad), ne)
            hold("softmax", yh, GA.softmax64(x, idx[role], ne, N), 1.0)
            hold("softmax backward", dx, GA.softmax_backward64(yh, d_y, idx[role], ne, N), np.abs(d_y).max())
            sums = np.stack([np.stack([yh[b, s].sum(0) if len(s) else np.ones(C) for s in row])
                             for b, row in enumerate(_slots(cid, role))])
            off = np.abs(sums - 1.0) / ((deg[..., None] + 8) * 2.0 ** -24 + deg[..., None] * 2.0 ** -9)
            worst["row sums / bound"] = max(worst.get("row sums / bound", 0.0), float(off.max()))
            assert off.max() <= 1.0, (cid, role, C, float(off.max()))
        for H, D in ((3, 4), (8, 16)):
            shift = GB.to_bf16_values(rng.choice(np.array([0.0, 1e4, -1e4, 88.0], np.float32), (B, N, 1)))
            l = GB.to_bf16_values(3 * rng.standard_normal((B, E, H)).astype(np.float32) + np_gather(shift, idx[role], ne))
            v = GB.to_bf16_values(rng.standard_normal((B, E, H, D)).astype(np.float32))
            w = GB.to_bf16_values(rng.standard_normal((B, N, H, D)).astype(np.float32))
            ld, vd = _dev(_pad_nan(GB.round_bf16(l), ne), eng, True), _dev(_pad_nan(GB.round_bf16(v), ne), eng, True)
            out = g.attend(ld, vd, role)
            out.backward(_dev(GB.round_bf16(w), eng))
            assert out.dtype == BF and ld.grad.dtype == BF and vd.grad.dtype == BF
            hold("attend", GB.widen(_b(out)).astype(np.float64), GA.attend64(l, v, idx[role], ne, N), np.abs(v).max())
            d_l64, d_v64, scale = GA.attend_backward64(l, v, w, idx[role], ne, N)
            hold("attend d_logits", GB.widen(_b(ld.grad)).astype(np.float64), d_l64, scale)
            hold("attend d_values", GB.widen(_b(vd.grad)).astype(np.float64), d_v64, np.abs(w).max())
    print(f"[graph bf16 {cid}] largest (error - 2^-8 |ref|) / scale (bar 1e-5) and row sums: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ 4: alignment
def test_a_tensor_two_bytes_off_alignment_gives_the_same_bits():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup("rpf2d_b2")
    B, N, E, C = eng.B, eng.N, eng.e_cap, 64
    g = Graph(feats)
    rng = np.random.default_rng(5)

    def shifted(t):
        """t one element off alignment: 2 bytes for bfloat16, 4 for float32."""
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=eng.device)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
        return out

    def bits32(t):
        return t.contiguous().view(torch.int32)

    x, msg = _dev(_rand_bits(rng, (B, N, C)), eng), _dev(_pad_nan(_rand_bits(rng, (B, E, C)), ne), eng)
    x2 = _dev(_rand_bits(rng, (B, N, C)), eng)
    clean = _dev(_pad_nan(_rand_bits(rng, (B, E, C)), ne), eng)
    for role in ROLES:
        for op, t in ((g.gather, x), (g.segment_sum, msg), (g.segment_max, msg), (g.segment_softmax, clean)):
            assert GB.same_bits(_b(op(shifted(t), role)), _b(op(t, role))), (role, op.__name__)
        l, v = clean[..., :8].contiguous(), msg.reshape(B, E, 8, 8)
        assert GB.same_bits(_b(g.attend(l, shifted(v), role)), _b(g.attend(l, v, role)))
        want = _b(g.conv(x, clean, role))                                    # (the pad slots of w are never read)
        assert GB.same_bits(_b(g.conv(shifted(x), clean, role)), want) and GB.same_bits(_b(g.conv(x, shifted(clean), role)), want)
    for op in (g.pair_mul, g.pair_add):
        want = _b(op(x, x2))
        assert GB.same_bits(_b(op(shifted(x), x2)), want) and GB.same_bits(_b(op(x, shifted(x2))), want), op.__name__
    # float32, 4 bytes off (data_ptr() % 16 == 4): no 16-byte units either
    x32, msg32, w32 = x.float(), msg.float(), clean.float()
    assert shifted(x32).data_ptr() % 16 == 4
    for role in ROLES:
        assert torch.equal(bits32(g.gather(shifted(x32), role)), bits32(g.gather(x32, role))), role
        assert torch.equal(bits32(g.segment_sum(shifted(msg32), role)), bits32(g.segment_sum(msg32, role))), role
        want = bits32(g.conv(x32, w32, role))
        assert torch.equal(bits32(g.conv(shifted(x32), w32, role)), want), role
        assert torch.equal(bits32(g.conv(x32, shifted(w32), role)), want), role


# ------------------------------------------------------------------------------------------------ 5: TorchModel(autocast)
ISL = 6


def _model(kind, hcase, dim, autocast=BF):
    from lagrangebench_amd.models import TorchModel
    node_in = TM.node_in_of(hcase.engine(1))
    net = TM.TinyMP(node_in, dim, 32) if kind == "mp" else GA.TinyAttn(node_in, dim, 32, 4)
    model = TorchModel(net, autocast=autocast)
    params, state = model.init(np.array([7]), None)
    rng = np.random.default_rng(3)
    params["~"]["gain"] = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32)
    state["~"]["in_scale"] = (1.0 + 0.1 * rng.standard_normal(state["~"]["in_scale"].shape)).astype(np.float32)
    model.set_state(state)
    return model, params, state


def _cpu_run(model, params, state, feats, ne, pt, dtype, target, autocast):
    from tests.test_torch_model_gpu import _cpu_module
    mod = _cpu_module(model, params, state, dtype)
    fd = TM.cpu_features(feats, dtype)
    graph = GB.CpuGraphBf16(fd["senders"], fd["receivers"], ne, pt.shape[1])
    if autocast:
        with torch.autocast("cpu", dtype=BF):
            pred = mod(fd, torch.as_tensor(pt).long(), graph)
        assert pred.dtype == BF
    else:
        pred = mod(fd, torch.as_tensor(pt).long(), graph)
    pred = pred.to(dtype)
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach().numpy(), dict((n, p.grad.numpy()) for n, p in mod.named_parameters()), float(mean.detach())


@pytest.mark.parametrize("kind", ["mp", "attn"])
def test_autocast_model_is_as_close_to_float64_as_the_cpu_autocast_restatement(kind):
    _need_gpu()
    from tests._common import hip_case
    from tests.test_torch_model_gpu import _dataset
    ds = _dataset("rpf2d_b2")
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(2)])
    model, params, state = _model(kind, hcase, pos.shape[3])
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    assert eng.N == 200 and eng.B == 2
    ne = _np(eng.nl_idx()[1])
    out = model.apply(params, state, (feats, pt))[0]["acc"]
    assert out.dtype == torch.float32
    out = _np(out)
    tg = torch.randn((2, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, g64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg, False)
    pbf, gbf, lbf = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg, True)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    weights = th.read("weights")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0 and np.isfinite(loss)
    assert np.array_equal(weights.view(np.uint32), model.flatten(params).view(np.uint32))     # the blob stays float32
    g_h = model.unflatten(g_flat)
    rows = [("forward", out, p64, pbf)]
    for name in g64:
        mod_name, _, leaf = name.rpartition(".")
        rows.append((name, g_h[mod_name or "~"][leaf], g64[name], gbf[name]))
    bad = []
    for name, dev, r64, rbf in rows:
        scale = max(np.abs(r64).max(), 1e-30)
        d, dbf = np.abs(dev - r64).max() / scale, np.abs(rbf - r64).max() / scale
        print(f"[autocast {kind}] {name}: device vs float64 {d:.2e}, cpu bfloat16 autocast vs float64 {dbf:.2e}")
        if not d <= 3 * dbf:
            bad.append((name, d, dbf))
    print(f"[autocast {kind}] loss: device {loss:.6e} float64 {l64:.6e} cpu bfloat16 autocast {lbf:.6e}")
    assert not bad, bad


def test_without_autocast_nothing_changes():
    _need_gpu()
    from lagrangebench_amd.models import TorchModel
    from tests._common import hip_case
    from tests.test_torch_model_gpu import _dataset
    ds = _dataset("rpf2d_b2")
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(2)])
    seen = []

    class Probe(TM.TinyMP):
        def forward(self, features, particle_type, graph):
            h = self.enc(torch.cat([features[k] for k in TM.NODE_KEYS if k in features] + [particle_type[..., None].float()], -1))
            seen.append((torch.is_autocast_enabled(), h.dtype, graph.gather(h, "senders").dtype))
            return super().forward(features, particle_type, graph)

    net = Probe(TM.node_in_of(hcase.engine(2)), 2, 32)
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    outs = []
    for model in (TorchModel(net), TorchModel(net, autocast=None), TorchModel(net, autocast=BF)):
        params, state = model.init(np.array([7]), None)
        outs.append(_np(model.apply(params, state, (feats, pt))[0]["acc"]))
    assert seen == [(False, torch.float32, torch.float32)] * 2 + [(True, BF, BF)]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert not np.array_equal(outs[0], outs[2]) and np.isfinite(outs[2]).all()

    class Half(TM.TinyMP):
        def forward(self, features, particle_type, graph):
            return super().forward(features, particle_type, graph).to(BF)

    model = TorchModel(Half(TM.node_in_of(hcase.engine(2)), 2, 32))
    params, state = model.init(np.array([7]), None)
    with pytest.raises(ValueError, match="float32 tensor"):     # the float32-only output check holds without the flag
        model.apply(params, state, (feats, pt))


def test_autocast_model_trains_round_trips_a_checkpoint_and_differentiates_the_window(tmp_path):
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.evaluate import infer
    from lagrangebench_amd.train import Trainer
    from tests._common import hip_case
    import lagrangebench_amd.train.trainer as T
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=3, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _model("attn", case, 2)
    cfg_train = {"batch_size": 2, "noise_std": 3e-4, "pushforward": {"steps": [-1], "unrolls": [1], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 3}, input_seq_length=ISL, seed=0)
    drawn = []
    sample_steps = T.push_forward_sample_steps

    def recording(key, step, pushforward):
        key, n = sample_steps(key, step, pushforward)
        drawn.append(n)
        return key, n
    T.push_forward_sample_steps = recording
    try:
        ckp = str(tmp_path / "ckp")
        params, state, opt = trainer.train(step_max=3, store_ckp=ckp)
    finally:
        T.push_forward_sample_steps = sample_steps
    losses = [l for _, l in trainer.loss_log]
    print(f"[autocast trainer] unrolls {drawn} losses {['%.5e' % l for l in losses]}")
    assert len(losses) >= 3 and np.isfinite(losses).all() and any(n == 1 for n in drawn)
    assert all(v.dtype == np.float32 for mod in params.values() for v in mod.values())
    cfg = {"batch_size": 2, "metrics": ["mse"], "out_type": "pkl", "n_trajs": 2}
    infer(model, case, data_valid, params=params, state=state, cfg_eval_infer=cfg, n_rollout_steps=4, rollout_dir=str(tmp_path / "mem"))
    infer(model, case, data_valid, load_ckp=ckp, cfg_eval_infer=cfg, n_rollout_steps=4, rollout_dir=str(tmp_path / "ckp_roll"))
    for i in range(2):
        a = pickle.load(open(tmp_path / "mem" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        b = pickle.load(open(tmp_path / "ckp_roll" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        assert a.shape == (ISL + 4, 200, 2) and np.isfinite(a).all() and np.array_equal(a, b)
    # ---- autograd.TorchModule: the same context, a gradient to the window
    pos = np.stack([data_valid[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([data_valid[b][1] for b in range(2)])
    case.allocate_eval((pos[:, :, :ISL], pt))
    mod = TorchModule(model, case, params, 2, state=state)
    window = torch.as_tensor(pos[:, :, :ISL], device=mod.engine.device).requires_grad_(True)
    pred = mod(window, pt)["acc"]
    assert pred.dtype == torch.float32 and pred.requires_grad
    pred.pow(2).sum().backward()
    assert window.grad.dtype == torch.float64 and bool(torch.isfinite(window.grad).all()) and float(window.grad.abs().max()) > 0
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()) for p in mod.parameters())


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_on_the_device():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _build("rpf2d_b1")
    g = Graph(feats)
    N, E, dev = eng.N, eng.e_cap, eng.device
    edge = lambda *s, dt=BF: torch.randn((1, E) + s, device=dev).to(dt)   # noqa: E731
    with pytest.raises(TypeError, match="one dtype"):
        g.attend(edge(4, dt=torch.float32), edge(4, 2), "receivers")
    with pytest.raises(TypeError, match="one dtype"):
        g.attend(edge(4), edge(4, 2, dt=torch.float32), "receivers")
    with pytest.raises(TypeError, match="float32"):
        g.segment_sum(edge(4, dt=torch.float16), "receivers")
    with pytest.raises(ValueError, match="bfloat16"):             # ... and the engine's own check, below graph.Graph
        eng.graph_segment_sum(0, torch.zeros((E, 4), dtype=torch.float16, device=dev))
    with pytest.raises(ValueError, match="lb_graph_attend"):
        eng.graph_attend(0, torch.zeros((E, 4), device=dev), torch.zeros((E, 4, 2), dtype=BF, device=dev))
    # ---- a cotangent in another dtype than the forward's (autograd itself would cast one handed to .backward(): the nodes
    # are called directly)
    x32 = torch.randn((1, N, 4), device=dev, requires_grad=True)
    e32 = edge(4, dt=torch.float32).requires_grad_()
    for y, d in ((g.gather(x32, "senders"), edge(4)), (g.segment_sum(e32, "senders"), torch.zeros((1, N, 4), dtype=BF, device=dev)),
                 (g.segment_max(e32, "receivers"), torch.zeros((1, N, 4), dtype=BF, device=dev)),
                 (g.segment_softmax(e32, "receivers"), edge(4)),
                 (g.attend(e32, edge(4, 2, dt=torch.float32), "receivers"), torch.zeros((1, N, 4, 2), dtype=BF, device=dev))):
        with pytest.raises(TypeError, match="cotangent"):
            y.grad_fn.apply(d)
    xb = x32.detach().to(BF).requires_grad_()
    with pytest.raises(TypeError, match="cotangent"):
        g.gather(xb, "senders").grad_fn.apply(edge(4, dt=torch.float32))
    # ---- a stale list in a bfloat16 backward
    leaves = [edge(4).requires_grad_() for _ in range(4)]
    results = [g.segment_sum(leaves[0], "senders"), g.segment_max(leaves[1], "senders"), g.segment_softmax(leaves[2], "receivers"),
               g.attend(leaves[3], edge(4, 2), "receivers")]
    eng.nl_update()
    for y in results:
        with pytest.raises(RuntimeError, match="stale"):
            y.float().sum().backward()
    with pytest.raises(RuntimeError, match="stale"):
        g.gather(xb.detach(), "senders")
