"""PaiNN training on the device (csrc/lb_train_painn.h) against float64 torch autograd of tests/_painn_oracle.py on
engine-built graphs: the gradient table, AdamW, the frozen radial basis, optimisation against a float64 replay, the
Trainer (checkpoint, resume, train.device_unroll) and autograd.DeviceModule."""
import json
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._common import hip_case, oracle_case  # noqa: E402
from tests._painn_oracle import random_biases  # noqa: E402
from tests._painn_train import (_TorchPass, batch_autograd, compare_leaves, kinematic, oracle_kw,  # noqa: E402
                                painn_forward_graph, painn_grad_check, tparams)

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


def _dataset(name, B, scale, isl=6, free=False):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=B, extra_seq_length=3, input_seq_length=isl, scale=scale)
    ds.magnitude_features = True
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    return ds, pos, pt


def _model(ds, radius, H=128, L=3, isl=6, trainable=True, cutoff=True, **kw):
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    r = 1.5 * ds.metadata["default_connectivity_radius"] if radius == "runner" else float(radius)
    return PaiNN(H, 1, L, gaussian_rbf(20, r, trainable=trainable), cosine_cutoff(r) if cutoff else None, isl - 1, **kw)


def _params(model, ds, free=False):
    p, s = model.init_params(7, ds.external_force_fn is not None, free)
    return random_biases(p, 8), s


def _targets(B, N, dim):
    return torch.randn((B, N, dim), generator=torch.Generator().manual_seed(3), dtype=torch.float32)


# id -> (case, scale, B, radius, L, isl, free space, model switches)
_GRAD_CASES = {
    "all_live": ("rpf2d", 0.25, 1, 1.5, 3, 6, False, {}),
    "all_live_b2": ("rpf2d", 0.25, 2, 1.5, 3, 6, False, {}),
    "self_only": ("rpf2d", 0.25, 1, "runner", 3, 6, False, {}),
    "partly_live": ("tgv3d", 0.5, 1, "runner", 3, 6, False, {}),
    "clips": ("ldc3d", 0.5, 1, "runner", 2, 6, True, {"homogeneous_particles": False}),
    "h64_nocut": ("rpf2d", 0.25, 1, 1.5, 3, 6, False, {"H": 64, "cutoff": False}),
    "shared_filters": ("rpf2d", 0.25, 1, 1.5, 3, 6, False, {"shared_filters": True}),
    "shared_interactions": ("rpf2d", 0.25, 1, 1.5, 3, 6, False, {"shared_interactions": True}),
    "rbf_state": ("rpf2d", 0.25, 1, 1.5, 3, 6, False, {"trainable": False}),
    "n_vels3": ("rpf2d", 0.25, 1, 1.5, 3, 4, False, {}),
}


class _ClampSpy(_TorchPass):
    """The restatement's torch with clamp recording its argument: the pre-clip values of every clip site, in call order
    (per layer: message-s, message-v, update-s, update-v)."""

    def __init__(self):
        self.seen = []

    def clamp(self, x, lo, hi):
        self.seen.append(x.detach().numpy().copy())
        return torch.clamp(x, lo, hi)


def clip_premise(model, params, state, ocase, pos, pt):
    """On the float64 oracle: at least three of the clip sites clip >= 0.1 % of their entries, and no pre-clip value lies
    within 0.1 of +-100 (the device's fp32 forward could take the other side).  Returns the clipped shares."""
    import tests._painn_oracle as PO
    import tests._painn_train as PT
    spy = _ClampSpy()
    old = PT._TorchPass
    PT._TorchPass = lambda: spy
    try:
        tp = tparams(params)
        of, _ = ocase.allocate_eval((pos[0, :, :model._n_vels + 1].astype(np.float64), pt[0]))
        painn_forward_graph(tp, of, pt[0], **oracle_kw(model, tp, state))
    finally:
        PT._TorchPass = old
    assert PO.torch is torch
    assert len(spy.seen) == 4 * model._num_mp_steps
    shares = [float((np.abs(x) >= 100.0).mean()) for x in spy.seen]
    near = sum(int((np.abs(np.abs(x) - 100.0) < 0.1).sum()) for x in spy.seen)
    assert sum(s >= 1e-3 for s in shares) >= 3, shares
    assert near == 0, near
    return shares


def _adamw_reference(tp64, g_h):
    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            v.grad = torch.as_tensor(np.asarray(g_h[mod][leaf], np.float64).reshape(v.shape))
    leaves = [v for mod in sorted(tp64) for _, v in sorted(tp64[mod].items())]
    torch.optim.AdamW(leaves, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2).step()


@pytest.mark.parametrize("cid", list(_GRAD_CASES))
def test_gradients_match_float64_autograd(cid):
    """One loss_grad per case against float64 autograd: prediction = PaiNN.apply's bits, loss within 1e-5, every leaf
    within 1e-4 of its largest entry (or 3x the float32 restatement's deviation), identical bits on repeats, read =
    flatten; then one AdamW step against torch.optim.AdamW on the device's own gradients (2e-6 max(|w|, 1) + 1e-7)."""
    _need_gpu()
    name, scale, B, radius, L, isl, free, sw = _GRAD_CASES[cid]
    sw = dict(sw)
    ds, pos, pt = _dataset(name, B, scale, isl, free)
    model = _model(ds, radius, H=sw.pop("H", 128), L=L, isl=isl, **sw)
    params, state = _params(model, ds, free)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    if cid == "clips":
        assert kinematic(pt).sum() > 0
        print("[painn grad clips] clipped shares", clip_premise(model, params, state, ocase, pos, pt))
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    N, dim = pos.shape[1], len(ds.box)
    apply_acc = _np(model.apply(params, state, (feats, pt))[0]["acc"]).reshape(B, N, dim)
    target = _targets(B, N, dim)
    th = model.train_handle(eng, params, state)
    _, g_h, g_flat, tp64 = painn_grad_check(th, model, params, state, ocase, pos, pt, target, apply_acc, cid)
    R = model.radial_basis_fn.n_rbf
    w0 = th.read("weights")
    if cid == "rbf_state":
        assert "~" not in g_h and np.all(g_flat[-2 * R:] == 0)
    else:
        assert np.abs(g_h["~"]["widths"]).max() > 0 and np.abs(g_h["~"]["offset"]).max() > 0
    _adamw_reference(tp64, g_h)
    th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    w_h = model.unflatten(th.read("weights"), like=params)
    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            ref = v.detach().numpy()
            assert np.abs(w_h[mod][leaf].reshape(ref.shape) - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1.0) + 1e-7, (mod, leaf)
    assert th.step_count() == 1
    if cid == "rbf_state":
        # the frozen basis: bit-identical after three steps, and after the gathered step with world 1; gradient exactly 0
        for _ in range(2):
            th.zero_grad()
            th.loss_grad(target, 1.0)
            th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-2)
        assert th.step_count() == 3
        w3 = th.read("weights")
        assert np.array_equal(w3[-2 * R:].view(np.uint32), w0[-2 * R:].view(np.uint32))
        assert not np.array_equal(w3[:-2 * R], w0[:-2 * R])
        th.zero_grad()
        th.loss_grad(target, 1.0)
        assert np.all(th.read("grads")[-2 * R:] == 0)
        th.adamw_step_gathered(th.device_blob("grads").reshape(1, -1).clone(), 1e-3, 0.9, 0.999, 1e-8, 1e-2)
        w4 = th.read("weights")
        assert np.array_equal(w4[-2 * R:].view(np.uint32), w0[-2 * R:].view(np.uint32))
        assert not np.array_equal(w4[:-2 * R], w3[:-2 * R]) and np.all(th.read("grads")[-2 * R:] == 0)
    th.close()


def test_one_directional_edges_are_counted_once():
    """tests/_asym.asym_case: lists that hold some edges in one direction only (premise asserted on the oracle's list)."""
    _need_gpu()
    from tests._asym import asym_case, check_premise, oracle_edges
    ds, pos, pt, pairs = asym_case("rpf2d", B=2, scale=0.5)
    ds.magnitude_features = True
    isl, B = ds.input_seq_length, 2
    for b in range(B):
        check_premise(oracle_edges(ds, pos[b], pt[b], isl), pairs, b)
    model = _model(ds, 1.5, L=2)
    params, state = _params(model, ds)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    idx, ne = _np(nbrs.idx), _np(nbrs.n_edges)
    for b in range(B):   # the engine's list is the oracle's: it holds the one-directional edges too
        want = oracle_edges(ds, pos[b], pt[b], isl)
        assert int(ne[b]) == want.shape[1] and np.array_equal(idx[b][:, :want.shape[1]], want)
    N, dim = pos.shape[1], len(ds.box)
    apply_acc = _np(model.apply(params, state, (feats, pt))[0]["acc"]).reshape(B, N, dim)
    th = model.train_handle(feats.engine, params, state)
    painn_grad_check(th, model, params, state, ocase, pos, pt, _targets(B, N, dim), apply_acc, "one_directional")
    th.close()


def replay(model, params, state, ocase, pos, pt, target, dtype, lr, steps):
    """`steps` AdamW steps on a fixed window with the restatement's autograd in `dtype` + torch.optim.AdamW: the losses."""
    tp = tparams(params)
    if dtype == torch.float32:
        tp = {m: {k: v.detach().float().requires_grad_(True) for k, v in lv.items()} for m, lv in tp.items()}
    leaves = [v for mod in sorted(tp) for _, v in sorted(tp[mod].items())]
    opt = torch.optim.AdamW(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8)
    isl = model._n_vels + 1
    of, _ = ocase.allocate_eval((pos[0, :, :isl].astype(np.float64), pt[0]))
    from tests._painn_train import painn_loss
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss, _ = painn_loss(tp, of, pt[0], np.asarray(target[0]), dtype=dtype, **oracle_kw(model, tp, state))
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    return losses


REPLAY_LR, REPLAY_STEPS = 3e-4, 6   # (at 1e-3 the float64 replay's loss rises at its second step)


def test_optimisation_follows_the_float64_replay():
    """Six AdamW steps on a fixed window: at every step the device loss deviates from the float64 replay by no more than
    max(1e-5 relative, 3x the float32 replay's deviation); the replay's own loss falls at every step."""
    _need_gpu()
    ds, pos, pt = _dataset("rpf2d", 1, 0.25)
    model = _model(ds, 1.5, L=2)
    params, state = _params(model, ds)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    N, dim = pos.shape[1], len(ds.box)
    target = _targets(1, N, dim)
    l64 = replay(model, params, state, ocase, pos, pt, target, torch.float64, REPLAY_LR, REPLAY_STEPS)
    l32 = replay(model, params, state, ocase, pos, pt, target, torch.float32, REPLAY_LR, REPLAY_STEPS)
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    feats, _ = hcase.allocate_eval((pos[:, :, :6], pt))
    th = model.train_handle(feats.engine, params, state)
    worst = 0.0
    for k in range(REPLAY_STEPS):
        th.zero_grad()
        loss = th.loss_grad(target, 1.0)
        th.adamw_step(REPLAY_LR, 0.9, 0.999, 1e-8, 1e-8)
        dev, dev32 = abs(loss - l64[k]) / l64[k], abs(l32[k] - l64[k]) / l64[k]
        worst = max(worst, dev)
        assert dev <= max(1e-5, 3 * dev32), (k, loss, l64[k], l32[k])
    print(f"[painn replay] losses {l64[0]:.6f} -> {l64[-1]:.6f}; largest relative deviation of the device loss {worst:.2e}")
    th.close()


def test_trainer_trains_painn_checkpoints_and_resumes(tmp_path, capsys):
    """PaiNN-2-64 on the LJ dataset with magnitude features, push-forward unrolls [0, 1]: finite losses, a checkpoint under
    the Haiku names plus the AdamW moments, a resumed run with the step count restored, and train.device_unroll on / off
    giving the same loss bits without the "has no device route" message."""
    _need_gpu()
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku, painn_params_to_haiku
    root = os.path.dirname(os.path.abspath(__file__))
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(os.path.join(root, "golden", "3D_LJ_3_1214every1"), ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    md.setdefault("write_every", 1)
    json.dump(md, open(ds_dir / "metadata.json", "w"))
    isl, L = 6, 2
    data_train = H5Dataset("train", str(ds_dir), name="lj3d", input_seq_length=isl, extra_seq_length=1)
    data_valid = H5Dataset("valid", str(ds_dir), name="lj3d", input_seq_length=isl, extra_seq_length=10)
    bounds = np.array(md["bounds"])

    def run(device_unroll, step_max, seed=0, load_ckp=None, store_ckp=None):
        case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=3e-4, cfg_model={"magnitude_features": True})
        model = PaiNN(64, 1, L, gaussian_rbf(20, 1.5, trainable=True), cosine_cutoff(1.5), isl - 1)
        cfg_train = {"batch_size": 2, "noise_std": 3e-4, "device_unroll": device_unroll,
                     "optimizer": {"lr_start": 5e-4, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 500},
                     "pushforward": {"steps": [-1, 4], "unrolls": [0, 1], "probs": [1, 1]}}
        trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                          cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                          cfg_logging={"log_steps": 1, "eval_steps": 12}, input_seq_length=isl, seed=seed)
        out = trainer.train(step_max=step_max, store_ckp=store_ckp, load_ckp=load_ckp)
        return model, trainer, out

    ckp = str(tmp_path / "ckp")
    model, trainer, (params, state, opt_state) = run(False, 12, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    assert len(losses) == 13 and np.isfinite(losses).all()
    loaded, _, opt_loaded, step = load_haiku(ckp)
    assert step == 12 and set(opt_loaded) >= {"m", "v", "step", "count"} and np.abs(opt_loaded["v"]).max() > 0
    assert set(loaded) == set(painn_params_to_haiku(params, model))
    capsys.readouterr()
    _, trainer_dev, _ = run(True, 12)
    assert "has no device route" not in capsys.readouterr().out
    assert [l for _, l in trainer_dev.loss_log] == losses   # same bits, weights never left the device for the unroll
    _, trainer2, (p2, _, opt2) = run(False, step + 3, seed=1, load_ckp=ckp)
    assert set(p2) == set(params)
    assert opt2["count"] >= opt_loaded["count"] + 1 and trainer2.loss_log[0][0] == step


def test_device_module_weight_gradient_under_a_huber_loss():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.autograd import DeviceModule
    ds, pos, pt = _dataset("rpf2d", 1, 0.25)
    model = _model(ds, 1.5, L=2)
    params, state = _params(model, ds)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :6], pt))
    eng = feats.engine
    N, dim = pos.shape[1], len(ds.box)
    apply_acc = _np(model.apply(params, state, (feats, pt))[0]["acc"]).reshape(1, N, dim)
    mod = DeviceModule(model, hcase, params, 1)
    window = torch.as_tensor(pos[:, :, :6].astype(np.float64), device=eng.device)
    target = _targets(1, N, dim).double()
    pred = mod(window, pt)["acc"]
    assert np.array_equal(_np(pred), apply_acc)
    res = (pred.detach().double().cpu() - target).reshape(-1)
    delta = float(res.abs().median())

    def huber(acc, b=0):
        r = (acc.double() - target[b].to(acc.device)).reshape(-1)
        a = r.abs()
        return torch.where(a <= delta, 0.5 * r * r, delta * (a - 0.5 * delta)).sum() / N

    huber(pred[0]).backward()
    g_h = model.unflatten(mod.handle.read("grads"), like=params)
    tp64, _ = batch_autograd(model, params, state, ocase, pos, pt, target, torch.float64, loss_fn=huber)
    tp32, _ = batch_autograd(model, params, state, ocase, pos, pt, target, torch.float32, loss_fn=huber)
    compare_leaves(g_h, tp64, tp32, "device module, huber")
    assert set(mod.params()) == set(params)
    with pytest.raises(NotImplementedError, match="GNS only"):
        mod(window.clone().requires_grad_(True), pt)
    th = mod.handle
    p2 = th.forward()
    with pytest.raises(LbHipError, match="-5.*GNS only"):
        th.backward(torch.zeros_like(p2), want_dpos=True)
    th.zero_grad()
    th.backward(torch.zeros_like(p2))   # the refusal left the forward live
    assert np.all(th.read("grads") == 0)
    th.close()


def test_egnn_loss_grad_refuses_a_painn_handle():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.engine import EgnnTrainHandle
    ds, pos, pt = _dataset("rpf2d", 1, 0.25)
    model = _model(ds, 1.5, L=2, H=64)
    params, state = _params(model, ds)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :6], pt))
    th = model.train_handle(feats.engine, params, state)
    tg = {"pos": torch.zeros((1, pos.shape[1], 2), dtype=torch.float64)}
    with pytest.raises(LbHipError, match=r"\(-1:"):
        EgnnTrainHandle.loss_grad(th, tg, {"pos": 1.0})
    th.close()
