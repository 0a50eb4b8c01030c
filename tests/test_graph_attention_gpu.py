"""graph.Graph's attention ops on the device (csrc/lb_graph.hip): degree, segment_mean, segment_max / segment_min, segment_softmax
and the fused attend, over receivers and senders, forward and backward.

Cases and columns are those of tests/test_graph_ops_gpu.py (its docstring says which path each reaches); the attend shapes
(H, D): (1, 1); (1, 5) scalars; (3, 4) 16-byte units, H no power of two; (8, 16) C = 128; (2, 65) a head boundary inside a
lane's stride, no multiple of 4; (5, 52) 65 units of 16 bytes, one more than a row's 64 lanes.  Every pad slot of every edge
input holds NaN.

What is held to the bit (view(uint32)): degree, segment_mean, the extrema with their gradient (numpy float32 loops that state
the order contract), attend against the composition of this library's own segment_softmax and segment_sum, its d_values, and
a second call of everything.  What has a tolerance, against float64 restatements on the same float32 inputs:
  segment_softmax forward  1e-5 absolute, the project's per-layer bar; the derived bound is (deg + 8) 2^-24 relative (expf to
                           1 ulp, deg ordered adds, one division; x - m is exact), under 1e-5 while deg <= 150 - asserted;
                           every non-empty row sums to 1 within (deg + 8) 2^-24
  segment_softmax backward 1e-5 max|d_y| in the max norm
  attend forward           1e-5 max|v| (it equals the composition to the bit; this catches an error the two share)
  attend d_logits          1e-5 max over the slots of sum_d |d_out v|; bound (D + deg + 10) 2^-24, D + deg <= 150 asserted
The model path (TinyAttn in models.TorchModel) uses the two-step rule of tests/test_torch_model_gpu.py unchanged.
"""
import functools
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_attention as GA  # noqa: E402
from tests.test_graph_ops_gpu import CASES, COLUMNS, ROLES, _bits, _build, _np, _setup, np_gather  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (3, 4), (8, 16), (2, 65), (5, 52)]
ULP = 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(a, eng, grad=False):
    return torch.tensor(a, device=eng.device, requires_grad=grad)


def _pad_nan(a, ne):
    a = a.copy()
    for b in range(a.shape[0]):
        a[b, ne[b]:] = np.nan
    return a


def _pads_are_plus_zero(a, ne):
    return all((_bits(a[b, ne[b]:]) == 0).all() for b in range(a.shape[0]))


@functools.lru_cache(maxsize=None)
def _degrees(cid):
    _, eng, idx, ne, _, _ = _setup(cid)
    return {role: GA.np_degree(idx[role], ne, eng.N) for role in ROLES}


def test_degrees_stay_inside_the_derived_bounds():
    _need_gpu()
    for cid in CASES:
        deg = _degrees(cid)
        top = max(int(d.max()) for d in deg.values())
        print(f"[graph attention] {cid}: max degree {top}")
        assert top <= 150 and top + max(D for _, D in SHAPES) <= 150


# ------------------------------------------------------------------------------------------------ degree, mean, max, min
def _extrema_input(rng, idx, ne, N, E, C):
    """random values; per trajectory one row whose first two slots tie at the top (even columns) or the bottom (odd columns),
    and one row that reads -0.0, +0.0, -1, -1, ... in column 0."""
    B = idx.shape[0]
    msg = (rng.standard_normal((B, E, C)) * 10.0 ** rng.integers(-2, 3, (B, E, 1))).astype(np.float32)
    planted = 0
    for b, row in enumerate(GA.node_slots(idx, ne, N)):
        rich = [s for s in row if len(s) >= 2]
        if rich:
            s = rich[0]
            msg[b, s[:2], 0::2], msg[b, s[:2], 1::2] = 1e4, -1e4
            planted += 1
        if len(rich) >= 2:
            s = rich[-1]
            msg[b, s, 0] = -1.0
            msg[b, s[0], 0], msg[b, s[1], 0] = -0.0, 0.0
    return msg, planted


@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_degree_mean_and_extrema_equal_numpy_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(7 * C + len(cid))
    w = rng.standard_normal((B, N, C)).astype(np.float32)
    for role in ROLES:
        deg = g.degree(role)
        assert deg.dtype == torch.int32 and deg.shape == (B, N)
        assert np.array_equal(_np(deg), _degrees(cid)[role])
        msg, planted = _extrema_input(rng, idx[role], ne, N, E, C)
        assert planted or cid == "lj"
        # ---- mean: the ordered sum, one division
        md = _dev(_pad_nan(msg, ne), eng, True)
        mean = g.segment_mean(md, role)
        assert np.array_equal(_bits(_np(mean)), _bits(GA.np_segment_mean(msg, idx[role], ne, N))), (cid, role, C)
        (mean * _dev(w, eng)).sum().backward()
        inv = (w / np.maximum(_degrees(cid)[role], 1).astype(np.float32)[..., None]).astype(np.float32)
        assert np.array_equal(_bits(_np(md.grad)), _bits(np_gather(inv, idx[role], ne)))
        # ---- max / min, forward and backward
        for minimum in (False, True):
            op = g.segment_min if minimum else g.segment_max
            md = _dev(_pad_nan(msg, ne), eng, True)
            got = op(md, role)
            want, win = GA.np_segment_max(msg, idx[role], ne, N, minimum)
            assert got.shape == (B, N, C) and np.isfinite(_np(got)).all()
            assert np.array_equal(_bits(_np(got)), _bits(want)), (cid, role, C, minimum)
            (got * _dev(w, eng)).sum().backward()
            d = _np(md.grad)
            assert np.array_equal(_bits(d), _bits(GA.np_segment_max_backward(w, win, idx[role], ne, E))), (cid, role, C, minimum)
            assert _pads_are_plus_zero(d, ne)
            again = op(_dev(_pad_nan(msg, ne), eng), role)
            assert np.array_equal(_bits(_np(again)), _bits(_np(got)))
        # ---- forward only: a NaN in a real slot wins and stays
        nan = msg.copy()
        nan[0, int(ne[0]) // 2] = np.nan
        want, _ = GA.np_segment_max(nan, idx[role], ne, N)
        got = _np(g.segment_max(_dev(_pad_nan(nan, ne), eng), role))
        assert np.isnan(want).sum() == C and np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ segment_softmax
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_segment_softmax_against_float64(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(11 * C + len(cid))
    for role in ROLES:
        shift = rng.choice(np.array([0.0, 1e4, -1e4, 88.0], np.float32), (B, N, 1))
        x = (3 * rng.standard_normal((B, E, C)).astype(np.float32) + np_gather(shift, idx[role], ne)).astype(np.float32)
        d_y = rng.standard_normal((B, E, C)).astype(np.float32)
        xd = _dev(_pad_nan(x, ne), eng, True)
        y = g.segment_softmax(xd, role)
        y.backward(_dev(_pad_nan(d_y, ne), eng))
        yh, dx = _np(y), _np(xd.grad)
        y64 = GA.softmax64(x, idx[role], ne, N)
        err = np.abs(yh - y64).max()
        assert y.shape == (B, E, C) and np.isfinite(yh).all() and _pads_are_plus_zero(yh, ne)
        deg = _degrees(cid)[role]
        sums = np.stack([np.stack([yh[b, s].astype(np.float64).sum(0) if len(s) else np.ones(C) for s in row])
                         for b, row in enumerate(GA.node_slots(idx[role], ne, N))])
        off = np.abs(sums - 1.0) / ((deg[..., None] + 8) * ULP)
        dx64 = GA.softmax_backward64(y64, d_y, idx[role], ne, N)
        berr = np.abs(dx - dx64).max() / np.abs(d_y).max()
        print(f"[segment_softmax {cid} {role} C={C}] forward {err:.2e}; row sums off by {off.max():.2f} of (deg + 8) ulp; "
              f"backward {berr:.2e} of max|d_y|")
        assert err <= 1e-5, (cid, role, C, err)
        assert off.max() <= 1.0, (cid, role, C, off.max())
        assert berr <= 1e-5 and _pads_are_plus_zero(dx, ne), (cid, role, C, berr)
        # ---- two calls: identical bits, forward and backward
        xd2 = _dev(_pad_nan(x, ne), eng, True)
        y2 = g.segment_softmax(xd2, role)
        y2.backward(_dev(_pad_nan(d_y, ne), eng))
        assert np.array_equal(_bits(_np(y2)), _bits(yh)) and np.array_equal(_bits(_np(xd2.grad)), _bits(dx))


# ------------------------------------------------------------------------------------------------ attend
@pytest.mark.parametrize("hd", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cid", CASES)
def test_attend_equals_the_composition_and_float64(cid, hd):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    H, D = hd
    g = Graph(feats)
    rng = np.random.default_rng(13 * H + D + len(cid))
    for role in ROLES:
        assert int(_degrees(cid)[role].max()) + D <= 150
        shift = rng.choice(np.array([0.0, 1e4, -1e4, 88.0], np.float32), (B, N, 1))
        l = (3 * rng.standard_normal((B, E, H)).astype(np.float32) + np_gather(shift, idx[role], ne)).astype(np.float32)
        v = rng.standard_normal((B, E, H, D)).astype(np.float32)
        w = rng.standard_normal((B, N, H, D)).astype(np.float32)

        def fused():
            ld, vd = _dev(_pad_nan(l, ne), eng, True), _dev(_pad_nan(v, ne), eng, True)
            out = g.attend(ld, vd, role)
            out.backward(_dev(w, eng))
            return _np(out), _np(ld.grad), _np(vd.grad)

        out, d_l, d_v = fused()
        assert out.shape == (B, N, H, D) and d_l.shape == (B, E, H) and d_v.shape == (B, E, H, D)
        # ---- the composition of this library's own ops: forward and d_values to the bit
        ld, vd = _dev(_pad_nan(l, ne), eng, True), _dev(_pad_nan(v, ne), eng, True)
        comp = g.segment_sum(g.segment_softmax(ld, role)[..., None] * vd, role)
        comp.backward(_dev(w, eng))
        assert np.array_equal(_bits(out), _bits(_np(comp))), (cid, role, hd, np.abs(out - _np(comp)).max())
        assert np.array_equal(_bits(d_v), _bits(_np(vd.grad))), (cid, role, hd)
        assert _pads_are_plus_zero(d_v, ne) and _pads_are_plus_zero(d_l, ne)
        # ---- float64
        err = np.abs(out - GA.attend64(l, v, idx[role], ne, N)).max() / np.abs(v).max()
        d_l64, d_v64, scale = GA.attend_backward64(l, v, w, idx[role], ne, N)
        lerr = np.abs(d_l - d_l64).max() / scale
        cerr = np.abs(_np(ld.grad) - d_l64).max() / scale
        print(f"[attend {cid} {role} H={H} D={D}] forward {err:.2e} of max|v|; d_logits {lerr:.2e} of the scale (the "
              f"composition's: {cerr:.2e}); d_values {np.abs(d_v - d_v64).max():.2e}")
        assert np.isfinite(out).all() and err <= 1e-5, (cid, role, hd, err)
        assert lerr <= 1e-5, (cid, role, hd, lerr)
        # ---- a second call: identical bits
        out2, d_l2, d_v2 = fused()
        assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(d_l2), _bits(d_l))
        assert np.array_equal(_bits(d_v2), _bits(d_v))


def test_unbatched_features_and_trailing_dimensions():
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    _, _, _, _, _, hcase = _setup("rpf2d_b1")
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=6, scale=0.25)
    feats, _ = hcase.allocate_eval((ds[0][0][:, :6], ds[0][1]))
    assert not feats.batched
    eng = feats.engine
    g = Graph(feats)
    idx, ne = eng.nl_idx()
    idx, ne = _np(idx), _np(ne)
    N, E = eng.N, eng.e_cap
    rng = np.random.default_rng(2)
    msg = rng.standard_normal((E, 3, 4)).astype(np.float32)
    md = _dev(msg, eng)
    assert g.degree("senders").shape == (N,)
    want, _ = GA.np_segment_max(msg.reshape(1, E, 12), idx[:, 1], ne, N)
    got = g.segment_max(md, "senders")
    assert got.shape == (N, 3, 4) and np.array_equal(_bits(_np(got)), _bits(want.reshape(N, 3, 4)))
    assert g.segment_mean(md, "senders").shape == (N, 3, 4) and g.segment_softmax(md, "receivers").shape == (E, 3, 4)
    out = g.attend(md[..., 0], md, "receivers")
    assert out.shape == (N, 3, 4)
    comp = g.segment_sum(g.segment_softmax(md[..., 0], "receivers")[..., None] * md, "receivers")
    assert np.array_equal(_bits(_np(out)), _bits(_np(comp)))


# ------------------------------------------------------------------------------------------------ staleness and refusals
def test_stale_lists_and_wrong_arguments_are_refused():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, hcase = _build("rpf2d_b1")
    g = Graph(feats)
    N, E, dev = eng.N, eng.e_cap, eng.device
    edge = lambda *s: torch.randn((1, E) + s, device=dev)   # noqa: E731
    ops = {"segment_mean": lambda t: g.segment_mean(t, "senders"), "segment_max": lambda t: g.segment_max(t, "senders"),
           "segment_min": lambda t: g.segment_min(t, "receivers"), "segment_softmax": lambda t: g.segment_softmax(t, "senders"),
           "attend": lambda t: g.attend(t, edge(4, 2), "receivers")}
    # ---- CPU tensors and wrong shapes
    for name, op in ops.items():
        with pytest.raises(TypeError, match="engine on"):
            op(torch.zeros((1, E, 4)))
        with pytest.raises(TypeError, match="float32"):
            op(edge(4).double())
        with pytest.raises(ValueError, match="expected"):
            op(torch.zeros((1, E + 1, 4), device=dev))
    with pytest.raises(TypeError, match="engine on"):
        g.attend(edge(4), torch.zeros((1, E, 4, 2)), "receivers")
    for bad in (edge(3, 2), edge(4), edge(4, 2, 2)):         # another H, no D, one dimension too many
        with pytest.raises(ValueError, match="expected"):
            g.attend(edge(4), bad, "receivers")
    with pytest.raises(ValueError, match="expected"):
        g.attend(edge(4, 2), edge(4, 2), "receivers")
    with pytest.raises(ValueError, match="role"):
        g.degree("nodes")
    # ---- graphs made on the fresh list; then the list moves on
    leaves = {name: edge(4).requires_grad_() for name in ops}
    results = {name: op(leaves[name]) for name, op in ops.items()}
    eng.nl_update()
    with pytest.raises(RuntimeError, match="stale"):
        g.degree("senders")
    for name, op in ops.items():
        with pytest.raises(RuntimeError, match="stale"):
            op(edge(4))
        with pytest.raises(RuntimeError, match="stale"):
            results[name].sum().backward()
    # ---- the library's own refusal of an overflowed list, for every entry
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    E = eng.e_cap
    e2, n2 = torch.zeros((E, 4), device=dev), torch.zeros((N, 4), device=dev)
    e3, n3 = torch.zeros((E, 4, 2), device=dev), torch.zeros((N, 4, 2), device=dev)
    calls = [lambda: eng.graph_degree(1), lambda: eng.graph_segment_max(1, e2), lambda: eng.graph_segment_max(0, e2, True),
             lambda: eng.graph_segment_max_backward(1, n2, torch.zeros((N, 4), dtype=torch.int32, device=dev)),
             lambda: eng.graph_segment_softmax(1, e2), lambda: eng.graph_segment_softmax_backward(1, e2, e2),
             lambda: eng.graph_attend(1, e2, e3), lambda: eng.graph_attend_backward(1, e2, e3, n2, n2, n3)]
    for call in calls:
        with pytest.raises(LbHipError, match="-3.*overflowed"):
            call()
    eng.nl_allocate()
    assert eng.graph_degree(1).shape == (N,)


# ------------------------------------------------------------------------------------------------ through the model path
ISL = 6


def _attn_model(hcase, dim):
    from lagrangebench_amd.models import TorchModel
    from tests import _torch_models as TM
    model = TorchModel(GA.TinyAttn(TM.node_in_of(hcase.engine(1)), dim, 32, 4))
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
    pred = mod(fd, torch.as_tensor(pt).long(), GA.CpuAttnGraph(fd["senders"], fd["receivers"], ne, pt.shape[1]))
    total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
    total.backward()
    return pred.detach(), mod, float(mean.detach())


def test_tiny_attn_forward_and_gradients_match_the_float64_restatement():
    _need_gpu()
    from tests.test_torch_model_gpu import _dataset, _two_step
    from tests._common import hip_case
    ds = _dataset("rpf2d_b1")
    hcase = hip_case(ds)
    pos, pt = ds[0][0][None].astype(np.float64), ds[0][1][None]
    model, params, state = _attn_model(hcase, pos.shape[3])
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert np.array_equal(_bits(out), _bits(_np(model.apply(params, state, (feats, pt))[0]["acc"])))
    tg = torch.randn((1, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[tiny attn forward] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}")
    assert ok or ok32, (e, e32)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    th.close()
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[tiny attn loss] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. {abs(l32 - l64) / abs(l64):.2e}")
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
    print(f"[tiny attn grad] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, bad
    assert np.abs(g_h["edge"]["weight"][:4]).max() > 0      # the logits' rows of the edge Linear: d_logits arrived


def test_tiny_attn_trains_and_round_trips_a_checkpoint(tmp_path):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.evaluate import infer
    from lagrangebench_amd.train import Trainer
    from tests._common import hip_case
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model, _, _ = _attn_model(case, 2)
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 2}, input_seq_length=ISL, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt = trainer.train(step_max=2, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    print(f"[tiny attn trainer] losses {['%.5e' % l for l in losses]}")
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[2] < losses[1] < losses[0]
    cfg = {"batch_size": 2, "metrics": ["mse"], "out_type": "pkl", "n_trajs": 2}
    infer(model, case, data_valid, params=params, state=state, cfg_eval_infer=cfg, n_rollout_steps=4, rollout_dir=str(tmp_path / "mem"))
    infer(model, case, data_valid, load_ckp=ckp, cfg_eval_infer=cfg, n_rollout_steps=4, rollout_dir=str(tmp_path / "ckp_roll"))
    for i in range(2):
        a = pickle.load(open(tmp_path / "mem" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        b = pickle.load(open(tmp_path / "ckp_roll" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        assert a.shape == (ISL + 4, 200, 2) and np.isfinite(a).all() and np.array_equal(a, b)
