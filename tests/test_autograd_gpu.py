"""Differentiable model step on the device (lb_train_forward / lb_train_backward, lagrangebench_amd/autograd.py).

The seam between forward and backward is invisible to the fused step; weight gradients under a Huber loss written in torch
against float64 autograd of the restatements (oracle/gns_torch.py, oracle/segnn_torch.py, tests/_egnn_oracle.py) on the
engine's own edge list; the position gradient of GNS against autograd through tests/_features_torch.py; pads; a two-step
unroll with the integrator in torch; determinism; a torch optimiser on the aliased weights; the refusals.
Bars: every leaf (and d loss / d window) within 1e-4 of its largest entry - the bar of tests/test_train.py and
tests/test_segnn_train.py; EGNN leaves past it are held to 3x the float32 restatement's own deviation, as in
tests/test_egnn_train.py.
"""
import numpy as np
import pytest
import torch

from tests._common import hip_case, make_params
from tests._features_torch import case_constants, displacement_torch, features_torch

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ set-up
def _gns_setup(name, scale, B, L=2, latent=128, free=False, mag=False, extra=3):
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    ds = make_case(name, n_trajs=B, extra_seq_length=extra, scale=scale)
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    if mag:
        ds.magnitude_features = True
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0, latent_size=latent)
    model = GNS(dim, latent, 2, L, 16)
    hcase = hip_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    return ds, hcase, pos, pt, params, model, feats


def _edges(eng):
    """The engine's current edge list per trajectory: [(receivers, senders)] int64 on the host, padding dropped."""
    idx, _ = eng.nl_idx()
    idx = idx.cpu().long()
    out = []
    for b in range(eng.B):
        real = idx[b, 0] < eng.N
        out.append((idx[b, 0][real], idx[b, 1][real]))
    return out


def _force(eng):
    f = eng.node_features().get("force")
    return None if f is None else f.cpu()


def _huber_sum(res, delta):
    """Huber loss (torch.nn.functional.huber_loss) of the residuals, summed."""
    a = res.abs()
    return torch.where(a <= delta, 0.5 * res * res, delta * (a - 0.5 * delta)).sum()


def _huber_setup(pred, target, mask):
    """delta = the median absolute residual over the masked entries; each branch of the loss holds >= 20 % of them."""
    res = (pred.detach().double().cpu() - target)[mask]
    delta = float(res.abs().median())
    quad = float((res.abs() <= delta).double().mean())
    assert 0.2 <= quad <= 0.8, quad
    return delta


def _p64(params):
    from oracle.gns_torch import params_to_torch
    return {m: {k: v.double().requires_grad_(True) for k, v in lv.items()} for m, lv in params_to_torch(params).items()}


def _gns_ref_pred(p64, window_b, edges_b, force_b, pt_b, consts, L):
    """float64 restatement of one trajectory: features (tests/_features_torch.py) then the network (oracle/gns_torch.py)."""
    from oracle.gns_torch import gns_apply_torch
    rcv, snd = edges_b
    f = features_torch(window_b, rcv, snd, force=force_b, **consts)
    return gns_apply_torch(p64, f["node"], f["edge"], snd, rcv, torch.as_tensor(pt_b), L, 2)


def _leaf_check(g_h, ref64, tag, ref32=None):
    worst, loose = 0.0, []
    for mod, lv in ref64.items():
        for leaf, v in lv.items():
            if v.numel() == 0:
                continue
            ref = _np(v.grad)
            dev = np.abs(g_h[mod][leaf] - ref).max()
            err = dev / max(np.abs(ref).max(), 1e-30)
            if err >= 1e-4 and ref32 is not None:   # fp32 positions: the float32 restatement's own deviation
                dev32 = np.abs(_np(ref32[mod][leaf].grad) - ref).max()
                assert dev <= 3 * dev32, (tag, mod, leaf, err, dev, dev32)
                loose.append(f"{mod}/{leaf}")
                continue
            worst = max(worst, err)
            assert err < 1e-4, (tag, mod, leaf, err)
    print(f"[autograd {tag}] worst relative weight-gradient error over the leaves {worst:.2e}; held to fp32: {loose or 'none'}")


# ------------------------------------------------------------------------------------------------ 1. the seam
def _seam_check(th, fused, apply_pred=None):
    th.zero_grad()
    loss1, pred1 = fused()
    g1 = th.read("grads")
    pred = th.forward()
    assert torch.equal(pred, pred1)
    if apply_pred is not None:
        assert np.array_equal(_np(pred).astype(np.float64), apply_pred)
    th.backward(torch.randn(pred.shape, generator=torch.Generator().manual_seed(1)).to(pred.device))
    assert np.abs(th.read("grads") - g1).max() > 0
    th.zero_grad()
    loss2, pred2 = fused()
    assert loss2 == loss1 and torch.equal(pred2, pred1) and np.array_equal(th.read("grads"), g1)


def test_seam_is_invisible_gns():
    _need_gpu()
    ds, hcase, pos, pt, params, model, feats = _gns_setup("rpf2d", 0.5, 1)
    th = model.train_handle(feats.engine, params)
    target = torch.randn((1, pos.shape[1], 2), generator=torch.Generator().manual_seed(5))
    _seam_check(th, lambda: th.loss_grad(target, 1.0, want_pred=True))
    th.close()


def _segnn_setup():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps
    from oracle import segnn_oracle as S
    B, L = 2, 2
    ds = make_case("small2d", n_trajs=B, extra_seq_length=3, scale=1.0)
    ds.magnitude_features = True
    isl = ds.input_seq_length
    homog = bool(np.all(ds[0][1] == 0))
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=homog,
                  blocks_per_step=2)
    params = S.segnn_init(np.random.default_rng(11), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=L,
                          blocks_per_step=2, random_bias=True)
    params = {k: v for k, v in params.items() if isinstance(v, dict)}
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    hcase = hip_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    return ds, hcase, pos, pt, params, model, feats, homog, L


def test_seam_is_invisible_segnn():
    _need_gpu()
    ds, hcase, pos, pt, params, model, feats, homog, L = _segnn_setup()
    th = model.train_handle(feats.engine, params)
    target = torch.randn((2, pos.shape[1], 2), generator=torch.Generator().manual_seed(5))
    _seam_check(th, lambda: th.loss_grad(target, 1.0, want_pred=True))
    th.close()


def _egnn_setup():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN
    from tests._egnn_oracle import random_biases
    isl, L = 6, 3
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=3, input_seq_length=isl, scale=0.5)
    pos = np.stack([ds[0][0]])
    pt = np.stack([ds[0][1]])
    model = EGNN(64, 1, 0.01, isl - 1, num_mp_steps=L)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    hcase = hip_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    apply_pos = _np(model.apply(params, {}, (feats, pt))[0]["pos"])
    r_c = float(ds.metadata["default_connectivity_radius"])
    g = torch.Generator().manual_seed(3)
    target = torch.as_tensor(apply_pos) + 1e-2 * r_c * torch.randn(apply_pos.shape, generator=g, dtype=torch.float64)
    return ds, hcase, pos, pt, params, model, feats, apply_pos, target, L


def test_seam_is_invisible_egnn():
    _need_gpu()
    ds, hcase, pos, pt, params, model, feats, apply_pos, target, L = _egnn_setup()
    th = model.train_handle(feats.engine, params)
    _seam_check(th, lambda: th.loss_grad({"pos": target}, {"pos": 1.0}, want_pred=True), apply_pos)
    th.close()


# ------------------------------------------------------------------------------------------------ 2. / 3. / 5. GNS
_GNS_CASES = {
    # id: name, scale, B, latent, free space, magnitude features, position gradient too
    "rpf2d_b1_dpos": ("rpf2d", 0.5, 1, 128, False, False, True),
    "rpf2d_b2": ("rpf2d", 0.5, 2, 128, False, False, False),
    "ldc3d_free_dpos": ("ldc3d", 0.5, 1, 128, True, False, True),
    "rpf2d_latent32": ("rpf2d", 0.5, 1, 32, False, False, False),
    "rpf2d_magnitude_dpos": ("rpf2d", 0.5, 1, 128, False, True, True),
}


@pytest.mark.parametrize("cid", list(_GNS_CASES))
def test_gns_gradients_under_a_huber_loss_match_float64_autograd(cid):
    """Huber loss in torch on the non-kinematic particles: d loss / d weights (every case) and d loss / d window (the
    `dpos` cases) of DeviceModule against float64 autograd of features + network on the engine's edge list, each within
    1e-4 of its largest entry; a second forward + backward gives the same bits.

    Measured on an MI355X.  d loss / d window: 8.2e-07 (rpf2d), 8.3e-07 (ldc3d in free space), 1.1e-06 (magnitude
    features); worst weight-gradient leaf 5.9e-07 in those steps (exact products throughout), 2.5e-07 (rpf2d B = 2) and
    6.8e-07 (latent 32) in the weight-only steps (DeviceModule's rule for GNS: exact forward, f16x2 backward).
    rpf2d_b2 is the case that needs the exact forward: with an f16x2 forward its leaf embed/embeddings is 1.95e-04 off
    (the fused lb_gns_train_loss_grad with _mse on the same batch: 1.48e-04).  Every particle of rpf2d has type 0, so the
    leaf is one row: the sum of d xnode over all 1600 particles with both signs; the f16x2 forward leaves a few ReLU units
    on the other side of their kink than float64 and their rows, off by per cent, do not average out of a sum that cancels."""
    _need_gpu()
    from lagrangebench_amd.autograd import DeviceModule, non_kinematic_mask
    name, scale, B, latent, free, mag, want_dpos = _GNS_CASES[cid]
    L = 2
    ds, hcase, pos, pt, params, model, feats = _gns_setup(name, scale, B, L, latent, free, mag)
    eng = feats.engine
    isl, dim, N = ds.input_seq_length, len(ds.box), pos.shape[1]
    if name == "ldc3d":
        assert set(np.unique(pt)) >= {0, 1, 2} and eng.has_bound
    mod = DeviceModule(model, hcase, params, B)
    assert mod.engine is eng
    window = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device).requires_grad_(want_dpos)
    mask = non_kinematic_mask(torch.as_tensor(pt))                          # (B, N) host
    target = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(5), dtype=torch.float64)

    def run():
        mod.zero_grad()
        if window.grad is not None:
            window.grad = None
        pred = mod(window, pt)["acc"]
        assert pred.dtype == torch.float32 and pred.grad_fn is not None and tuple(pred.shape) == (B, N, dim)
        delta = _huber_setup(pred, target, mask)
        res = (pred.double() - target.to(pred.device))[mask.to(pred.device)]
        (_huber_sum(res, delta) / float(mask.sum())).backward()
        return pred.detach(), delta

    pred_h, delta = run()
    edges, force = _edges(eng), _force(eng)
    g_dev = mod.weights.grad.clone()
    g_flat = mod.handle.read("grads")
    if latent == 128:
        assert np.array_equal(_np(g_dev), g_flat)                          # the parameter's gradient IS the handle's blob
    else:
        assert g_dev.numel() > g_flat.size and float(g_dev.abs().sum()) == pytest.approx(float(np.abs(g_flat).sum()), rel=1e-5)
    dpos_h = window.grad.clone() if want_dpos else None
    # determinism: the same bits again
    pred_2, delta_2 = run()
    assert torch.equal(pred_2, pred_h) and delta_2 == delta and torch.equal(mod.weights.grad, g_dev)
    if want_dpos:
        assert torch.equal(window.grad, dpos_h)
    assert mod.recomputed == 0

    # reference: float64, host
    consts = case_constants(ds)
    p64 = _p64(params)
    w64 = torch.as_tensor(pos[:, :, :isl].astype(np.float64)).requires_grad_(want_dpos)
    tot = 0.0
    for b in range(B):
        pr = _gns_ref_pred(p64, w64[b], edges[b], None if force is None else force[b], pt[b], consts, L)
        assert float((pr.detach() - pred_h[b].cpu().double()).abs().max() / pr.detach().abs().max()) < 1e-5
        tot = tot + _huber_sum((pr - target[b])[mask[b]], delta)
    (tot / float(mask.sum())).backward()
    _leaf_check(model.unflatten(g_flat, params), p64, cid)
    if want_dpos:
        ref = w64.grad.numpy()
        got = _np(dpos_h)
        assert got.dtype == np.float64 and got.shape == ref.shape
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"[autograd {cid}] d loss / d window: largest entry {np.abs(ref).max():.3e}, relative error {err:.2e}")
        assert np.abs(ref[:, :, :-1]).max() > 0 and np.abs(ref[:, :, -1]).max() > 0
        assert err < 1e-4, err
    mod.handle.close()


def test_other_models_weight_gradients_under_a_huber_loss_segnn():
    _need_gpu()
    from lagrangebench_amd.autograd import DeviceModule
    from oracle import segnn_torch as ST
    ds, hcase, pos, pt, params, model, feats, homog, L = _segnn_setup()
    eng = feats.engine
    B, N, dim, isl = 2, pos.shape[1], 2, ds.input_seq_length
    mod = DeviceModule(model, hcase, params, B)
    window = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device)
    target = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    mask = torch.ones((B, N), dtype=torch.bool)
    pred = mod(window, pt)["acc"]
    delta = _huber_setup(pred, target, mask)
    (_huber_sum((pred.double() - target.to(pred.device)).reshape(-1), delta) / (B * N)).backward()
    g_h = model.unflatten(mod.handle.read("grads"))
    fe = eng_features_numpy(eng, pos[:, :, :isl])
    tp = ST.params_to_torch(params, requires_grad=True)
    tot = 0.0
    for b in range(B):
        node, nattr, eattr, msg, snd, rcv, d3 = ST.inputs_from_features(fe[b], pt[b], isl - 1, homog)
        pr = ST.segnn_apply_torch(tp, node, nattr, eattr, msg, snd, rcv, d3, 2, L)
        assert float((pr.detach() - pred[b].detach().cpu().double()).abs().max() / pr.detach().abs().max()) < 1e-5
        tot = tot + _huber_sum((pr - target[b]).reshape(-1), delta)
    (tot / (B * N)).backward()
    _leaf_check(g_h, tp, "segnn small2d")
    with pytest.raises(NotImplementedError, match="GNS only"):
        mod(window.clone().requires_grad_(True), pt)
    mod.handle.close()


def eng_features_numpy(eng, window):
    """The engine's current features and edge list as one plain dict of host arrays per trajectory (feature_transform's
    keys), for the restatements that take a feature dict."""
    out = []
    nf, ef = eng.node_features(), eng.edge_features()
    idx, _ = eng.nl_idx()
    for b in range(eng.B):
        d = {k: _np(v[b]) for k, v in nf.items()}
        d.update({k: _np(v[b]) for k, v in ef.items()})
        d["receivers"], d["senders"] = _np(idx[b, 0]), _np(idx[b, 1])
        d["abs_pos"] = np.asarray(window[b], np.float64)
        out.append(d)
    return out


def test_other_models_weight_gradients_under_a_huber_loss_egnn():
    _need_gpu()
    from lagrangebench_amd.autograd import DeviceModule
    from tests._egnn_oracle import case_kwargs
    from tests.test_egnn_train import _tparams, egnn_loss
    ds, hcase, pos, pt, params, model, feats, apply_pos, target, L = _egnn_setup()
    eng = feats.engine
    isl, N, dim = 6, pos.shape[1], 2
    mod = DeviceModule(model, hcase, params, 1)
    window = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device)
    pred = mod(window, pt)["pos"]
    assert np.array_equal(_np(pred).astype(np.float64), apply_pos)
    mask = torch.ones((1, N), dtype=torch.bool)
    delta = _huber_setup(pred, target, mask)
    (_huber_sum((pred.double() - target.to(pred.device)).reshape(-1), delta) / N).backward()
    g_h = model.unflatten(mod.handle.read("grads"), like=params)
    fe = eng_features_numpy(eng, pos[:, :, :isl])[0]
    kw = dict(case_kwargs(ds), num_mp_steps=L, n_vels=isl - 1, homogeneous=True, residual=True, tanh=False)
    refs = {}
    for dt in (torch.float64, torch.float32):
        tp = _tparams(params)
        _, pr = egnn_loss(tp, fe, pt[0], {"pos": _np(target[0])}, {"pos": 1.0}, dtype=dt, **kw)
        (_huber_sum((pr["pos"].double() - target[0]).reshape(-1), delta) / N).backward()
        refs[dt] = tp
    _leaf_check(g_h, refs[torch.float64], "egnn rpf2d", refs[torch.float32])
    mod.handle.close()


# ------------------------------------------------------------------------------------------------ 3. pads
def test_pad_rows_do_not_train_and_get_no_position_gradient():
    _need_gpu()
    from lagrangebench_amd.data import make_padded_case
    from lagrangebench_amd.models import GNS
    L = 2
    ds = make_padded_case("small2d", (256, 160), extra_seq_length=4)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(2)])
    pt = np.stack([ds[b][1] for b in range(2)])
    pads = torch.as_tensor(pt == -1)
    assert int(pads.sum()) == 96
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(dim, 128, 2, L, 16)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    th = model.train_handle(eng, params)
    dpred = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(2)).to(eng.device)   # pads included
    assert float(dpred[pads.to(eng.device)].abs().min()) > 0
    out = {}
    for tag, d in (("with", dpred), ("zeroed", torch.where(pads.to(eng.device)[..., None], torch.zeros_like(dpred), dpred))):
        th.zero_grad()
        th.forward()
        dpos = th.backward(d, want_dpos=True)
        out[tag] = (th.read("grads"), dpos.clone())
    assert np.abs(out["with"][0]).max() > 0
    assert np.array_equal(out["with"][0], out["zeroed"][0])
    assert torch.equal(out["with"][1], out["zeroed"][1])
    assert float(out["with"][1][pads.to(eng.device)].abs().max()) == 0.0
    assert float(out["with"][1][~pads.to(eng.device)].abs().max()) > 0.0
    th.close()


# ------------------------------------------------------------------------------------------------ 4. two-step unroll
def test_two_step_unroll_is_differentiable_end_to_end():
    """rpf2d 0.25, GNS L = 2: predict, integrate and shift the window in torch (case.integrate: case.py:230-259), predict
    again; the loss reads both predictions.  Gradients with respect to the weights and the FIRST window against the float64
    restatement on the engine's two edge lists; the first step's backward recomputes its forward (the handle's live
    forward is the second step's)."""
    _need_gpu()
    from lagrangebench_amd.autograd import DeviceModule
    L = 2
    ds, hcase, pos, pt, params, model, feats = _gns_setup("rpf2d", 0.25, 1, L)
    eng = feats.engine
    isl, dim, N = ds.input_seq_length, len(ds.box), pos.shape[1]
    consts = case_constants(ds)
    assert not np.any((pt == 1) | (pt == 2))          # no kinematic particle: the integrator moves every one
    g = torch.Generator().manual_seed(7)
    t1 = torch.randn((1, N, dim), generator=g, dtype=torch.float64)
    t2 = torch.randn((1, N, dim), generator=g, dtype=torch.float64)

    def step_window(w, pred):
        """integrate_fn for "acc" + the window shift, in torch float64"""
        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=w.device)
        acc = pred.double() * t(consts["acc_std"]) + t(consts["acc_mean"])
        vel = displacement_torch(w[..., -1, :], w[..., -2, :], consts["box"], consts["periodic"])
        new = torch.remainder(w[..., -1, :] + vel + acc, t(consts["box"])) if consts["periodic"] else w[..., -1, :] + vel + acc
        return torch.cat([w[..., 1:, :], new[..., None, :]], dim=-2)

    mod = DeviceModule(model, hcase, params, 1)
    w1 = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device).requires_grad_(True)
    p1 = mod(w1, pt)["acc"]
    e1, force1 = _edges(eng)[0], _force(eng)[0]
    w2 = step_window(w1, p1)
    p2 = mod(w2)["acc"]
    e2, force2 = _edges(eng)[0], _force(eng)[0]
    loss = ((p1.double() - t1.to(eng.device)) ** 2).sum() / N + ((p2.double() - t2.to(eng.device)) ** 2).sum() / N
    assert mod.recomputed == 0
    loss.backward()
    assert mod.recomputed == 1
    g_last = mod.handle.read("grads")                         # (the blob holds the LAST backward only ...)
    g_total = _np(mod.weights.grad)                           # ... the parameter's gradient the sum of both)
    dpos_h = _np(w1.grad)

    p64 = _p64(params)
    r1 = torch.as_tensor(pos[0, :, :isl].astype(np.float64)).requires_grad_(True)
    q1 = _gns_ref_pred(p64, r1, e1, force1, pt[0], consts, L)
    r2 = step_window(r1, q1)
    q2 = _gns_ref_pred(p64, r2, e2, force2, pt[0], consts, L)
    assert float((q1.detach() - p1.detach().cpu()[0]).abs().max() / q1.detach().abs().max()) < 1e-5
    assert float((q2.detach() - p2.detach().cpu()[0]).abs().max() / q2.detach().abs().max()) < 1e-4
    (((q1 - t1[0]) ** 2).sum() / N + ((q2 - t2[0]) ** 2).sum() / N).backward()
    assert g_total.shape == g_last.shape and np.abs(g_total - g_last).max() > 0
    _leaf_check(model.unflatten(g_total, params), p64, "unroll weights")
    ref = r1.grad.numpy()
    err = np.abs(dpos_h[0] - ref).max() / np.abs(ref).max()
    print(f"[autograd unroll] d loss / d first window: relative error {err:.2e}")
    assert err < 1e-4, err
    mod.handle.close()


# ------------------------------------------------------------------------------------------------ 6. aliasing
def test_a_torch_optimiser_on_the_aliased_weights_trains_the_handle():
    _need_gpu()
    from lagrangebench_amd.autograd import DeviceModule
    ds, hcase, pos, pt, params, model, feats = _gns_setup("rpf2d", 0.5, 1, 2, latent=32)
    eng = feats.engine
    isl, dim, N = ds.input_seq_length, len(ds.box), pos.shape[1]
    mod = DeviceModule(model, hcase, params, 1)
    th = mod.handle
    blob0 = th.device_blob("weights").clone()
    padded = blob0 == 0           # the padded slots (and nothing else: random_affine leaves no exact zero)
    assert int(padded.sum()) == blob0.numel() - th.n_floats
    opt = torch.optim.AdamW([mod.weights], lr=1e-3, weight_decay=1e-2)
    window = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device)
    target = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(5)).to(eng.device)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.huber_loss(mod(window, pt)["acc"], target, delta=0.5)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    w = th.read("weights")
    assert np.abs(w - model.flatten(params)).max() > 1e-4            # it trained
    assert np.array_equal(w, model.flatten(mod.params()))
    assert float(th.device_blob("weights")[padded].abs().max()) == 0.0   # every padded slot is still exactly 0
    th.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_refusals():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.autograd import DeviceModule
    ds, hcase, pos, pt, params, model, feats = _gns_setup("rpf2d", 0.5, 1)
    eng = feats.engine
    isl, N, dim = ds.input_seq_length, pos.shape[1], 2
    th = model.train_handle(eng, params)
    d = torch.zeros((1, N, dim), device=eng.device)
    with pytest.raises(LbHipError, match="lb_train_forward"):
        th.backward(d)
    th.forward()
    th.adamw_step(1e-3)                                # any other call ends the live forward ...
    with pytest.raises(LbHipError, match="lb_train_forward"):
        th.backward(d)
    th.forward()
    th.zero_grad()                                     # ... but zero_grad
    th.backward(d)
    with pytest.raises(LbHipError, match="lb_train_forward"):
        th.backward(d)                                 # the backward consumed it
    th.close()
    # stale features
    mod = DeviceModule(model, hcase, params, 1)
    window = torch.as_tensor(pos[:, :, :isl].astype(np.float64), device=eng.device)
    feats2, _ = hcase.preprocess_eval((pos[:, :, :isl], pt), hcase.allocate_eval((pos[:, :, :isl], pt))[1])
    assert mod(window, pt, features=feats2)["acc"].grad_fn is not None
    eng.nl_update()
    with pytest.raises(RuntimeError, match="stale"):
        mod(window, pt, features=feats2)
    mod.handle.close()


@pytest.mark.parametrize("which", ["segnn", "egnn"])
def test_position_gradient_is_refused_for_other_handles(which):
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    s = _segnn_setup() if which == "segnn" else _egnn_setup()
    pos, params, model, feats = s[2], s[4], s[5], s[6]
    th = model.train_handle(feats.engine, params)
    pred = th.forward()
    with pytest.raises(LbHipError, match="-5.*GNS only"):
        th.backward(torch.zeros_like(pred), want_dpos=True)
    assert th.backward(torch.zeros_like(pred)) is None   # the refusal left the forward live
    th.close()
