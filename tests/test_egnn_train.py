"""EGNN training (csrc/lb_train_egnn.h, EGNN.train_handle, Trainer).

CPU: the float64 torch restatement of the reference (tests/_egnn_oracle.py) plus the three-term loss of _mse
(train/trainer.py:35-60 over EGNN's pos / vel / acc outputs, models/egnn.py:361-369) is differentiated by autograd and
checked against central finite differences - the yardstick the device gradients are then held to; with normalize=True
the same autograd is not finite on a graph with self-edges, which is why training refuses it.
GPU: the device step against that autograd on engine-built graphs, bit-identical predictions and gradients, AdamW, the
Trainer and the runner's `mode: all` route."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import tests._egnn_oracle as EO
from tests._egnn_oracle import case_kwargs, random_biases, space


class _NpPass:
    """numpy with an asarray that passes torch tensors through (the restatement then keeps the autograd graph)."""

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def asarray(a, *args, **kw):
        return a if isinstance(a, torch.Tensor) else np.asarray(a, *args, **kw)


class _TorchPass:
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def as_tensor(a, dtype=None, device=None):
        return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=dtype, device=device)


def _kinematic(pt):
    pt = np.asarray(pt)
    return (pt == 1) | (pt == 2) | (pt == -1)   # utils.py:28-35


def egnn_loss(tparams, features, particle_type, targets, loss_weight, *, dtype=torch.float64, **kw):
    """_mse of one trajectory through tests/_egnn_oracle.egnn_forward: pos = x^L, vel = displacement(x^L, x^0),
    acc = vel - the normalised last velocity feature (in `dtype`); residuals against the targets in float64."""
    old_np, old_torch = EO.np, EO.torch
    EO.np, EO.torch = _NpPass(), _TorchPass()
    try:
        _, xs = EO.egnn_forward(tparams, features, particle_type, dtype=dtype, **kw)
    finally:
        EO.np, EO.torch = old_np, old_torch
    disp, _ = space(kw["box"], kw["periodic"], dtype)
    N = xs[0].shape[0]
    vel = disp(xs[-1], xs[0])
    vh = torch.as_tensor(np.asarray(features["vel_hist"]), dtype=dtype).reshape(N, kw["n_vels"], -1)[:, -1]
    pred = {"pos": xs[-1], "vel": vel, "acc": vel - vh}
    tot = torch.zeros(N, dtype=torch.float64)
    for k, p in pred.items():
        w = float(loss_weight.get(k, 0.0))
        if w:
            tot = tot + w * ((p.double() - torch.as_tensor(np.asarray(targets[k]), dtype=torch.float64)) ** 2).sum(-1)
    nk = torch.as_tensor(~_kinematic(particle_type))
    return torch.where(nk, tot, torch.zeros_like(tot)).sum() / nk.sum(), pred


def _tparams(params):
    return {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in lv.items()}
            for m, lv in params.items()}


# ----------------------------------------------------------------------------------------------------------------- CPU
def _wrap_sample(rng, N=10, n_vels=3, box=1.0):
    """A small periodic 2D sample (self-edges included, as in every radius graph here) with a |force| attribute."""
    dim = 2
    base = rng.uniform(0.1, 0.9, size=(N, 1, dim))
    steps = rng.normal(0, 0.004, size=(N, n_vels + 1, dim)).cumsum(1)
    pos = base + steps
    pos[0, :, 0] = box - 0.004 + 0.0015 * np.arange(n_vels + 1) - 0.0015 * n_vels   # newest at box - 0.004, moving +x
    pos = np.mod(pos, box)
    vel = pos[:, 1:] - pos[:, :-1]
    vel = vel - box * np.round(vel / box)
    s, r = np.nonzero(np.ones((N, N)))
    d = pos[s, -1] - pos[r, -1]
    d = np.linalg.norm(d - box * np.round(d / box), axis=-1)
    keep = d < 0.45
    f = {"abs_pos": pos, "vel_hist": (vel / 0.004).reshape(N, -1), "senders": s[keep], "receivers": r[keep],
         "rel_dist": d[keep][:, None] / 0.45, "force": rng.standard_normal((N, dim))}
    return f, np.zeros(N, np.int64)


def test_restatement_loss_gradients_match_finite_differences():
    from lagrangebench_amd.models import EGNN
    rng = np.random.default_rng(0)
    f, pt = _wrap_sample(rng)
    n_vels, L, H = 3, 2, 16
    m = EGNN(H, 1, 0.04, n_vels, num_mp_steps=L, tanh=True)
    params = random_biases(m.init_params(4, True), 5)
    kw = dict(box=np.array([1.0, 1.0]), periodic=True, vel_mean=np.zeros(2), vel_std=np.full(2, 0.004), num_mp_steps=L,
              n_vels=n_vels, tanh=True)
    tp = _tparams(params)
    # translate the whole box (the model is invariant to it) so that particle 0's shift in x carries it across the edge
    _, pred = egnn_loss(tp, f, pt, {}, {}, **kw)
    x0 = np.asarray(f["abs_pos"])[0, -1, 0]
    delta = float(pred["pos"][0, 0].detach()) - x0
    delta -= np.round(delta)
    assert abs(delta) > 1e-4
    c = (1.0 - 0.5 * delta - x0) if delta > 0 else (-0.5 * delta - x0)
    f["abs_pos"] = np.mod(np.asarray(f["abs_pos"]) + np.array([c, 0.0]), 1.0)
    _, pred = egnn_loss(tp, f, pt, {}, {}, **kw)
    x0, xl = np.asarray(f["abs_pos"])[0, -1, 0], float(pred["pos"][0, 0].detach())
    assert abs(xl - x0) > 0.5, "particle 0 must wrap across the periodic edge"
    tg = {k: v.detach().numpy() + rng.normal(0, 0.05, v.shape) for k, v in pred.items()}
    lw = {"pos": 1.0, "vel": 0.5, "acc": 0.25}
    loss, _ = egnn_loss(tp, f, pt, tg, lw, **kw)
    loss.backward()
    checked = 0
    for mod, leaf in [("scalar_emb", "w"), ("layer_0/edge_0", "w"), ("layer_0/edge_0", "b"), ("layer_0/node_0", "w"),
                      ("layer_1/edge_1", "w"), ("layer_0/pos_1", "w"), ("layer_1/vel_0", "w"), ("layer_1/vel_1", "w"),
                      ("layer_0/pos_0", "b")]:
        g = tp[mod][leaf].grad.numpy().ravel()
        v = tp[mod][leaf].detach().numpy().ravel()
        for j in rng.choice(v.size, size=min(4, v.size), replace=False):
            vals = []
            for sgn in (1, -1):
                p2 = {a: {b: x.detach().clone() for b, x in lv.items()} for a, lv in tp.items()}
                p2[mod][leaf].view(-1)[j] += sgn * 1e-6
                vals.append(float(egnn_loss(p2, f, pt, tg, lw, **kw)[0]))
            fd = (vals[0] - vals[1]) / 2e-6
            assert abs(fd - g[j]) <= 1e-5 * max(1.0, abs(g).max()), (mod, leaf, j, fd, g[j])
            checked += 1
    assert checked >= 30


def test_restatement_gradient_not_finite_with_normalize():
    from lagrangebench_amd.models import EGNN
    rng = np.random.default_rng(1)
    f, pt = _wrap_sample(rng)
    assert (np.asarray(f["senders"]) == np.asarray(f["receivers"])).any()   # self-edges, as every radius graph here
    m = EGNN(16, 1, 0.04, 3, num_mp_steps=2, normalize=True)
    params = random_biases(m.init_params(4, True), 5)
    kw = dict(box=np.array([1.0, 1.0]), periodic=True, vel_mean=np.zeros(2), vel_std=np.full(2, 0.004), num_mp_steps=2,
              n_vels=3, normalize=True)
    tp = _tparams(params)
    loss, pred = egnn_loss(tp, f, pt, {"pos": np.zeros((10, 2))}, {"pos": 1.0}, **kw)
    assert torch.isfinite(loss) and torch.isfinite(pred["pos"]).all()   # the forward is fine ...
    loss.backward()
    assert not all(torch.isfinite(v.grad).all() for lv in tp.values() for v in lv.values())   # ... its gradient is not


def test_trainer_refuses_egnn_normalize():
    from lagrangebench_amd.models import EGNN
    from lagrangebench_amd.train import Trainer
    model = EGNN(32, 1, 0.01, 5, num_mp_steps=2, normalize=True)
    with pytest.raises(NotImplementedError, match="normalize"):
        Trainer(model, None, None, None)
    with pytest.raises(NotImplementedError, match="normalize"):
        model.train_handle(None, None)


# ----------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


_GRAD_CASES = [
    # id, case, B, scale, free space, model kwargs, loss weights
    ("rpf2d_b1", "rpf2d", 1, 0.5, False, {}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("rpf2d_b2", "rpf2d", 2, 0.5, False, {}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("ldc3d_free_types", "ldc3d", 1, 0.5, True, {"homogeneous_particles": False}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("tgv3d", "tgv3d", 1, 1.0, False, {}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("residual_off", "rpf2d", 1, 0.5, False, {"residual": False}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("tanh", "rpf2d", 1, 0.5, False, {"tanh": True}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("h64", "rpf2d", 1, 0.5, False, {"H": 64}, {"pos": 1.0, "vel": 0.0, "acc": 0.0}),
    ("vel_only", "rpf2d", 1, 0.5, False, {}, {"pos": 0.0, "vel": 1.0, "acc": 0.0}),
    ("acc_only", "rpf2d", 1, 0.5, False, {}, {"pos": 0.0, "vel": 0.0, "acc": 1.0}),
    ("all_three", "rpf2d", 1, 0.5, False, {}, {"pos": 1.0, "vel": 0.5, "acc": 0.25}),
]


def _egnn_grad_check(th, model, params, ocase, pos, pt, tg, lw, kw, apply_pos, cid):
    """One lb_egnn_train_loss_grad on the engine's current window / list against float64 autograd of the restatement on
    the oracle's graph: the prediction is EGNN.apply's (apply_pos) bit for bit, the loss within 1e-5, every leaf within
    1e-4 of its largest entry (or 3x the float32 restatement's own deviation); two more calls give the same bits.  Returns
    (loss, gradients, the float64 torch leaves)."""
    Bn, isl = pos.shape[0], kw["n_vels"] + 1
    box = kw["box"]
    th.zero_grad()
    loss_h, pred_h = th.loss_grad(tg, lw, want_pred=True)
    pred_h = pred_h.cpu().numpy()
    assert np.array_equal(pred_h.astype(np.float64), apply_pos)   # the inference forward, bit for bit
    g_flat = th.read("grads")
    for _ in range(2):   # no floating-point atomics anywhere in the step
        th.zero_grad()
        assert th.loss_grad(tg, lw) == loss_h and np.array_equal(th.read("grads"), g_flat)
    assert np.array_equal(th.read("weights"), model.flatten(params))   # blob <-> padded device layout
    g_h = model.unflatten(g_flat, like=params)
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0

    tp64, tp32 = _tparams(params), _tparams(params)
    losses = []
    for b in range(Bn):
        of, _ = ocase.allocate_eval((pos[b, :, :isl].astype(np.float64), pt[b]))
        tgb = {k: v[b].numpy() for k, v in tg.items()}
        lb, pr = egnn_loss(tp64, of, pt[b], tgb, lw, dtype=torch.float64, **kw)
        lb.backward()
        losses.append(float(lb))
        l32, _ = egnn_loss(tp32, of, pt[b], tgb, lw, dtype=torch.float32, **kw)
        l32.backward()
        # no particle on different sides of a periodic wrap in the two predictions
        d = np.abs(pred_h[b].astype(np.float64) - pr["pos"].detach().numpy())
        assert d.max() < 0.25 * np.min(box), (b, d.max())
    assert abs(loss_h - np.mean(losses)) <= 1e-5 * abs(np.mean(losses)), (loss_h, losses)
    worst, loose = 0.0, []
    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            ref = v.grad.numpy()
            dev = np.abs(g_h[mod][leaf] - ref).max()
            err = dev / max(np.abs(ref).max(), 1e-30)
            if err >= 1e-4:   # fp32 positions: hold the leaf to the float32 restatement's own deviation
                dev32 = np.abs(tp32[mod][leaf].grad.numpy() - ref).max()
                assert dev <= 3 * dev32, (mod, leaf, err, dev, dev32)
                loose.append(f"{mod}/{leaf}")
            else:
                worst = max(worst, err)
    print(f"[egnn grad {cid}] loss {loss_h:.6e}; worst relative gradient error {worst:.2e}; leaves held to the fp32 "
          f"restatement: {loose or 'none'}")
    return loss_h, g_h, tp64


@pytest.mark.gpu
@pytest.mark.parametrize("cid,name,B,scale,free,mkw,lw", _GRAD_CASES, ids=[c[0] for c in _GRAD_CASES])
def test_hip_egnn_gradients_match_torch_autograd(cid, name, B, scale, free, mkw, lw):
    """lb_egnn_train_loss_grad against float64 autograd of the restatement on engine-built graphs: the prediction is
    EGNN.apply's bit for bit, the loss within 1e-5, every leaf's gradient within 1e-4 of its largest entry (or, where fp32
    positions dominate, within 3x the float32 restatement's own deviation); two calls give identical bits; one AdamW step
    matches torch.optim.AdamW."""
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN
    from tests._common import hip_case, oracle_case
    isl, L = 6, 3
    mkw = dict(mkw)
    H = mkw.pop("H", 128)
    ds = make_case(name, n_trajs=B, extra_seq_length=3, input_seq_length=isl, scale=scale)
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    Bn, N, dim = pos.shape[0], pos.shape[1], len(ds.box)
    model = EGNN(H, 1, 0.01, isl - 1, num_mp_steps=L, **mkw)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    apply_pos = model.apply(params, {}, (feats, pt))[0]["pos"].detach().cpu().numpy()   # (B, N, dim) fp64 of fp32
    kw = dict(case_kwargs(ds), num_mp_steps=L, n_vels=isl - 1, homogeneous=mkw.get("homogeneous_particles", True),
              residual=mkw.get("residual", True), tanh=mkw.get("tanh", False))
    box, periodic = kw["box"], kw["periodic"]
    r_c = float(ds.metadata["default_connectivity_radius"])
    g = torch.Generator().manual_seed(3)
    tg = {"pos": torch.as_tensor(apply_pos) + 1e-2 * r_c * torch.randn((Bn, N, dim), generator=g, dtype=torch.float64),
          "vel": torch.randn((Bn, N, dim), generator=g, dtype=torch.float64),
          "acc": torch.randn((Bn, N, dim), generator=g, dtype=torch.float64)}
    th = model.train_handle(eng, params)
    loss_h, g_h, tp64 = _egnn_grad_check(th, model, params, ocase, pos, pt, tg, lw, kw, apply_pos, cid)

    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            v.grad = torch.as_tensor(g_h[mod][leaf]).double()
    leaves = [v for mod in sorted(tp64) for _, v in sorted(tp64[mod].items())]
    opt = torch.optim.AdamW(leaves, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    opt.step()
    th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    w_h = model.unflatten(th.read("weights"), like=params)
    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            ref = v.detach().numpy()
            assert np.abs(w_h[mod][leaf] - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1.0) + 1e-7, (mod, leaf)
    assert th.step_count() == 1
    th.close()


@pytest.mark.gpu
def test_gns_loss_grad_refuses_egnn_handle():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN
    from tests._common import hip_case
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=6, scale=0.5)
    pos, pt = ds[0]
    feats, _ = hip_case(ds).allocate_eval((pos[None, :, :6], pt[None]))
    model = EGNN(32, 1, 0.01, 5, num_mp_steps=2)
    th = model.train_handle(feats.engine, model.init_params(0, True))
    from lagrangebench_amd.engine import GnsTrainHandle
    with pytest.raises(LbHipError):
        GnsTrainHandle.loss_grad(th, torch.zeros((1, pos.shape[0], 2)))
    th.close()


@pytest.mark.gpu
def test_trainer_trains_egnn_and_runner_mode_all(tmp_path):
    """The Trainer lowers an EGNN's loss (loss_weight {pos: 1, vel: 0, acc: 0}, configs/rpf_*/egnn.yaml) on the LJ dataset,
    writes a checkpoint with Haiku EGNN names plus the AdamW moments, resumes from it with the step count restored, and
    `mode: all` of the runner with model.name egnn returns 0.
    The loss check covers the first 30 steps: the `pos` target is not minimum-imaged (case.py:141-153, kept as the
    reference has it), so a particle of this 3-particle periodic box that crosses the edge during a step contributes a
    box-sized residual - with this seed at step 45 (loss ~4 instead of ~1e-4), after which AdamW needs many steps to
    recover; no mean over a window that holds such a step shows the trend."""
    _need_gpu()
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import EGNN
    from lagrangebench_amd.runner import train_or_infer
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
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
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=3e-4)
    model = EGNN(64, 1, md["dt"] * md["write_every"], isl - 1, normalization_stats=case.normalization_stats,
                 num_mp_steps=L)
    lw = {"pos": 1.0, "vel": 0.0, "acc": 0.0}
    cfg_train = {"batch_size": 2, "noise_std": 3e-4, "loss_weight": lw,
                 "optimizer": {"lr_start": 5e-4, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 500},
                 "pushforward": {"steps": [-1, 20], "unrolls": [0, 1], "probs": [1, 1]}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 5, "eval_steps": 30}, input_seq_length=isl, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt_state = trainer.train(step_max=30, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    assert np.isfinite(losses).all() and np.mean(losses[-4:]) < 0.8 * np.mean(losses[:3]), losses
    loaded, _, opt_loaded, step = load_haiku(ckp)
    assert step == 30 and set(opt_loaded) >= {"m", "v", "step", "count"} and np.abs(opt_loaded["v"]).max() > 0
    assert "egnn/~/scalar_emb" in loaded and "egnn/~/layer_1/~/mlp_xav_1/~/linear_0" in loaded
    trainer2 = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                       cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                       cfg_logging={"log_steps": 1, "eval_steps": 1000}, input_seq_length=isl, seed=1)
    p2, _, opt2 = trainer2.train(step_max=step + 3, load_ckp=ckp)
    assert set(p2) == set(params)
    assert opt2["count"] >= opt_loaded["count"] + 1 and trainer2.loss_log[0][0] == step   # resumed, step count restored
    cfg = {"mode": "all", "dataset": {"src": str(ds_dir), "name": "lj3d"},
           "model": {"name": "egnn", "num_mp_steps": 2, "input_seq_length": isl, "latent_dim": 64},
           "train": {"step_max": 12, "batch_size": 1, "loss_weight": lw,
                     "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]}},
           "logging": {"log_steps": 5, "eval_steps": 5, "ckp_dir": str(tmp_path / "ckp2"), "run_name": "r"},
           "eval": {"n_rollout_steps": 5, "train": {"n_trajs": 1, "metrics": ["mse"]},
                    "infer": {"n_trajs": 1, "batch_size": 1, "metrics": ["mse"], "out_type": "none"}}}
    assert train_or_infer(cfg) == 0
