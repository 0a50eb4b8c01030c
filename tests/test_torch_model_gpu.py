"""models.TorchModel on the device: a user's torch network (tests/_torch_models.TinyMP) on the engine's features and graph
ops, trained by the Trainer through engine.BlobTrainHandle.

Cases: rpf2d scale 0.25 at B = 1 and B = 2 (N = 200, periodic, external force, one type) and ldc3d scale 0.5 in free space
(N = 1020, dim 3, types 0 / 1 / 2: the kinematic mask of the loss, the bound columns).

Tolerances - the project's two-step rule (tests/test_egnn_train.py): a figure is held to the project's bar (forward and loss
1e-5 of the largest entry, gradients 1e-4 of the leaf's largest entry) against the float64 CPU restatement; where it misses
that bar, to 3x the float32 CPU restatement's own deviation from float64 - the same network in the same precision, with
torch's CPU kernels and index_add_ in place of the device's.  The leaves that needed the second step are printed.
The graph ops and the optimiser are pinned to the bit (no tolerance); the dense layers are torch's.
"""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _torch_models as TM  # noqa: E402
from tests._common import hip_case  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"rpf2d_b1": ("rpf2d", 0.25, False, 1), "rpf2d_b2": ("rpf2d", 0.25, False, 2), "ldc3d": ("ldc3d", 0.5, True, 1)}
ISL = 6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _dataset(cid, n_trajs=None, extra=6):
    from lagrangebench_amd.data import make_case
    name, scale, free, B = CASES[cid]
    ds = make_case(name, n_trajs=n_trajs or B, extra_seq_length=extra, input_seq_length=ISL, scale=scale)
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    return ds


def _setup(cid):
    """(pos (B, N, T, dim), particle types (B, N), engine case, model, params, state)."""
    from lagrangebench_amd.models import TorchModel
    B = CASES[cid][3]
    ds = _dataset(cid)
    hcase = hip_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    model = TorchModel(TM.TinyMP(TM.node_in_of(hcase.engine(B)), pos.shape[3], 32))
    params, state = model.init(np.array([7]), None)
    rng = np.random.default_rng(3)   # the defaults (gain 1, in_scale 1) would leave those two paths unseen
    params["~"]["gain"] = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32)
    state["~"]["in_scale"] = (1.0 + 0.1 * rng.standard_normal(state["~"]["in_scale"].shape)).astype(np.float32)
    model.set_state(state)
    return pos, pt, hcase, model, params, state


class _Cpu:
    device = torch.device("cpu")


def _cpu_module(model, params, state, dtype):
    """The module on the CPU in `dtype`, holding (params, state)."""
    return model._device_module(_Cpu(), params, state).to(dtype)


def _cpu_eval(mod, feats, ne, pt, dtype, target=None):
    """`mod` on the exported features with CpuGraph: (prediction, mean loss) - after a backward of the batch-summed _mse
    when a target is given."""
    fd = TM.cpu_features(feats, dtype)
    g = TM.CpuGraph(fd["senders"], fd["receivers"], ne, pt.shape[1])
    pred = mod(fd, torch.as_tensor(pt).long(), g)
    loss = None
    if target is not None:
        total, mean = TM.mse_loss(pred, torch.as_tensor(target).to(dtype), pt)
        total.backward()
        loss = float(mean.detach())
    return pred.detach(), loss


def _cpu_run(model, params, state, feats, ne, pt, dtype, target=None):
    mod = _cpu_module(model, params, state, dtype)
    pred, loss = _cpu_eval(mod, feats, ne, pt, dtype, target)
    return pred, mod, loss


def _two_step(dev, r64, r32, bar):
    """(deviation / scale, passes the bar, passes 3x the float32 restatement's deviation)."""
    r64 = np.asarray(r64, np.float64)
    scale = max(np.abs(r64).max(), 1e-30)
    d = np.abs(np.asarray(dev, np.float64) - r64).max()
    d32 = np.abs(np.asarray(r32, np.float64) - r64).max()
    return d / scale, d / scale <= bar, d <= 3 * d32, d32 / scale


# ------------------------------------------------------------------------------------------------ forward and gradients
@pytest.mark.parametrize("cid", list(CASES))
def test_forward_and_gradients_match_the_float64_restatement(cid):
    _need_gpu()
    pos, pt, hcase, model, params, state = _setup(cid)
    B, N, dim = pos.shape[0], pos.shape[1], pos.shape[3]
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert out.shape == (B, N, dim) and out.dtype == np.float32
    assert np.array_equal(_bits(out), _bits(_np(model.apply(params, state, (feats, pt))[0]["acc"])))   # two calls: the same bits
    tg = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    p64, m64, l64 = _cpu_run(model, params, state, feats, ne, pt, torch.float64, tg)
    p32, m32, l32 = _cpu_run(model, params, state, feats, ne, pt, torch.float32, tg)
    e, ok, ok32, e32 = _two_step(out, p64.numpy(), p32.numpy(), 1e-5)
    print(f"[torch model forward {cid}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}"
          f"{'' if ok else ' (held to the fp32 restatement)'}")
    assert ok or ok32, (cid, e, e32)
    if cid == "ldc3d":
        assert set(np.unique(pt)) == {0, 1, 2}
    # ---- loss and gradients of the batch-summed _mse
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    g_flat = th.read("grads")
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    el = abs(loss - l64) / abs(l64)
    print(f"[torch model loss {cid}] device {loss:.9e} fp64 {l64:.9e} (rel. {el:.2e}); fp32 restatement rel. {abs(l32 - l64) / abs(l64):.2e}")
    assert el <= 1e-5 or abs(loss - l64) <= 3 * abs(l32 - l64), (loss, l64, l32)
    g_h = model.unflatten(g_flat)
    worst, loose, bad = 0.0, [], []
    n64, n32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    for name in n64:
        mod_name, _, leaf = name.rpartition(".")
        e, ok, ok32, e32 = _two_step(g_h[mod_name or "~"][leaf], n64[name].grad.numpy(), n32[name].grad.numpy(), 1e-4)
        if ok:
            worst = max(worst, e)
        elif ok32:
            loose.append(f"{name} ({e:.2e}, fp32 {e32:.2e})")
        else:
            bad.append((name, e, e32))
    print(f"[torch model grad {cid}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: {loose or 'none'}")
    assert not bad, (cid, bad)
    # gradients accumulate until zero_grad; a second evaluation gives the same loss
    loss2 = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 1.0})
    assert abs(loss2 - loss) <= 1e-6 * abs(loss)
    assert np.abs(th.read("grads") - 2 * g_flat).max() <= 1e-5 * np.abs(g_flat).max()
    # the loss weight scales loss and gradients
    th.zero_grad()
    loss_w = model.loss_grad(th, {"acc": torch.as_tensor(tg)}, {"acc": 0.5})
    assert abs(loss_w - 0.5 * loss) <= 1e-6 * abs(loss)
    assert np.abs(th.read("grads") - 0.5 * g_flat).max() <= 1e-5 * np.abs(g_flat).max()
    th.close()


# ------------------------------------------------------------------------------------------------ the blob handle
def test_blob_handle_steps_like_a_model_handle_and_refuses_the_model_entries():
    _need_gpu()
    import ctypes as C
    from lagrangebench_amd._lib import LbHipError, check
    from lagrangebench_amd.engine import BlobTrainHandle, GnsTrainHandle
    from lagrangebench_amd.models import Linear
    pos, pt, hcase, _, _, _ = _setup("rpf2d_b1")
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    lin = Linear(2)
    lp = lin.init_params(1, eng.node_in + 1)
    w0 = lin.flatten(lp)
    n = w0.size
    rng = np.random.default_rng(5)
    g0 = rng.standard_normal(n).astype(np.float32)
    m0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v0 = (0.01 * rng.random(n)).astype(np.float32)
    ref = lin.train_handle(eng, lp)
    blob, blob2 = eng.blob_train_handle(w0), eng.blob_train_handle(w0)
    assert isinstance(blob, BlobTrainHandle) and isinstance(blob, GnsTrainHandle) and blob.n_floats == n
    assert blob.device_floats() == n and blob.step_count() == 0   # no padding
    assert np.array_equal(blob.read("weights"), w0) and not blob.read("m").any() and not blob.read("grads").any()
    for th in (ref, blob, blob2):
        th.write("grads", g0)
        th.write("m", m0)
        th.write("v", v0, step=4)
    hyper = (3e-3, 0.9, 0.999, 1e-8, 1e-2)
    ref.adamw_step(*hyper)
    blob.adamw_step(*hyper)
    blob2.adamw_step_gathered(blob2.device_blob("grads").clone()[None], *hyper)   # its own single gradient row
    for th in (blob, blob2):
        assert th.step_count() == ref.step_count() == 5
        for which in ("weights", "m", "v", "grads"):
            assert np.array_equal(_bits(th.read(which)), _bits(ref.read(which))), which
    assert not np.array_equal(blob.read("weights"), w0)
    # two ranks' rows: summed in rank order by the same kernel, on both kinds of handle
    ref2, blob3 = lin.train_handle(eng, lp), eng.blob_train_handle(w0)
    rows = torch.tensor(np.stack([g0, rng.standard_normal(n).astype(np.float32)]), device=eng.device)
    for th in (ref2, blob3):
        th.write("m", m0)
        th.write("v", v0, step=4)
        th.adamw_step_gathered(rows, *hyper)
    for which in ("weights", "m", "v", "grads"):
        assert np.array_equal(_bits(blob3.read(which)), _bits(ref2.read(which))), which
    assert np.array_equal(_bits(blob3.read("grads")), _bits(_np(rows[0] + rows[1])))
    ref2.close(), blob3.close()
    blob.zero_grad()
    assert not blob.read("grads").any()
    # every entry that runs a model refuses the handle and names it
    tgt = torch.zeros((1, eng.N, eng.dim), device=eng.device)
    for call in (lambda: blob.loss_grad(tgt), blob.forward, lambda: blob.backward(tgt)):
        with pytest.raises(LbHipError, match="-5.*blob training handle"):
            call()
    loss = C.c_double()
    with pytest.raises(LbHipError, match="-5.*blob training handle"):
        check(eng.lib.lb_segnn_train_loss_grad(blob._h, tgt.data_ptr(), C.c_float(1.0), C.byref(loss), None))
    with pytest.raises(LbHipError, match="-5.*blob training handle"):
        check(eng.lib.lb_egnn_train_loss_grad(blob._h, None, None, None, C.c_float(0), C.c_float(0), C.c_float(0), C.byref(loss), None))
    for th in (ref, blob, blob2):
        th.close()


def test_parameters_and_gradients_are_the_blobs():
    _need_gpu()
    pos, pt, hcase, model, params, state = _setup("rpf2d_b2")
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    th = model.train_handle(eng, params)
    assert np.array_equal(_bits(th.read("weights")), _bits(model.flatten(params)))
    tg = torch.randn((2, eng.N, eng.dim), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    th.zero_grad()
    model.loss_grad(th, {"acc": tg}, {"acc": 1.0})
    gblob, wblob = th.device_blob("grads"), th.device_blob("weights")
    lo, hi = gblob.data_ptr(), gblob.data_ptr() + 4 * gblob.numel()
    off = 0
    for p in th.module.parameters():
        assert lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi      # autograd accumulated in place
        assert p.grad.data_ptr() == lo + 4 * off and p.data_ptr() == wblob.data_ptr() + 4 * off
        off += p.numel()
    assert off == gblob.numel() == th.n_floats
    assert np.array_equal(_bits(th.read("grads")), _bits(model.flatten(model._tree(model._names, {n: p.grad for n, p in th.module.named_parameters()}))))
    before = model.flatten(model.params_of(th.module))
    th.adamw_step(1e-3)
    after = model.flatten(model.params_of(th.module))
    assert np.array_equal(_bits(after), _bits(th.read("weights"))) and not np.array_equal(before, after)
    # the unroll handle is the live module: apply_handle on it follows the optimiser without a copy
    view = model.unroll_handle(eng, th, params)
    a = _np(model.apply_handle(view, state, (feats, pt))[0]["acc"])
    fresh = _np(model.apply(model.unflatten(th.read("weights")), state, (feats, pt))[0]["acc"])
    assert np.array_equal(_bits(a), _bits(fresh))
    assert not np.array_equal(a, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    mod = th.module
    th.close()
    assert all(p.numel() == 0 for p in mod.parameters())   # nothing aliases the freed blobs


# ------------------------------------------------------------------------------------------------ six AdamW steps
def _replay(model, params, state, feats, ne, pt, tg, dtype, steps=6, lr=1e-3):
    """Six noise-free steps on the CPU in `dtype` (weights, gradients and moments all in `dtype`): autograd of _mse +
    optax.adamw restated (tests/_torch_models.adamw_replay_step).  Returns the loss of every step."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    mod = _cpu_module(model, params, state, dtype)
    leaves = list(mod.parameters())
    w = np.concatenate([p.detach().numpy().ravel() for p in leaves])
    m, v = np.zeros_like(w), np.zeros_like(w)
    hp = [npd(x) for x in (lr, 0.9, 0.999, 1e-8, 1e-8)]
    losses = []
    for k in range(steps):
        mod.zero_grad()
        losses.append(_cpu_eval(mod, feats, ne, pt, dtype, tg)[1])
        g = np.concatenate([p.grad.numpy().ravel() for p in leaves])
        w, m, v = (a.astype(npd) for a in TM.adamw_replay_step(w, g, m, v, k + 1, *hp))
        off = 0
        with torch.no_grad():
            for p in leaves:
                p.copy_(torch.from_numpy(w[off:off + p.numel()].reshape(tuple(p.shape))))
                off += p.numel()
    return losses


@pytest.mark.parametrize("cid", ["rpf2d_b1", "ldc3d"])
def test_six_adamw_steps_follow_the_float64_replay(cid):
    _need_gpu()
    pos, pt, hcase, model, params, state = _setup(cid)
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    ne = _np(eng.nl_idx()[1])
    tg = torch.randn((1, eng.N, eng.dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    th = model.train_handle(eng, params)
    dev = []
    for _ in range(6):
        th.zero_grad()
        dev.append(model.loss_grad(th, {"acc": tg}, {"acc": 1.0}))
        th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-8)
    assert th.step_count() == 6
    th.close()
    ref = _replay(model, params, state, feats, ne, pt, tg.numpy(), torch.float64)
    r32 = _replay(model, params, state, feats, ne, pt, tg.numpy(), torch.float32)
    devi = [abs(d - r) / abs(r) for d, r in zip(dev, ref)]
    d32 = [abs(a - r) / abs(r) for a, r in zip(r32, ref)]
    print(f"[torch model six steps {cid}] device {['%.6e' % x for x in dev]}; deviation from the fp64 replay "
          f"{['%.2e' % x for x in devi]}; fp32 replay {['%.2e' % x for x in d32]}")
    assert ref[-1] < ref[0]
    for k in range(6):
        assert devi[k] <= 1e-5 or devi[k] <= 3 * d32[k], (k, devi, d32)


# ------------------------------------------------------------------------------------------------ Trainer end to end
def _train12(tmp_path, device_unroll, store=None, device_data=False):
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import TorchModel
    from lagrangebench_amd.train import Trainer
    data_train = make_case("rpf2d", n_trajs=4, extra_seq_length=2, input_seq_length=ISL, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=ISL, scale=0.25)
    case = hip_case(data_train)
    model = TorchModel(TM.TinyMP(TM.node_in_of(case.engine(2)), 2, 32))
    cfg_train = {"batch_size": 2, "noise_std": 3e-4, "device_unroll": device_unroll, "device_data": device_data,
                 "pushforward": {"steps": [-1, -1], "unrolls": [0, 1], "probs": [1, 1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 11}, input_seq_length=ISL, seed=0)
    import lagrangebench_amd.train.trainer as T
    drawn = []
    sample_steps = T.push_forward_sample_steps

    def recording(key, step, pushforward):
        key, n = sample_steps(key, step, pushforward)
        drawn.append(n)
        return key, n
    T.push_forward_sample_steps = recording
    try:
        params, state, opt = trainer.train(step_max=11, store_ckp=store)
    finally:
        T.push_forward_sample_steps = sample_steps
    return trainer.loss_log, params, state, opt, drawn, model, case, data_valid


def test_trainer_end_to_end(tmp_path):
    _need_gpu()
    from lagrangebench_amd.evaluate import infer
    from lagrangebench_amd.utils import load_haiku
    ckp = str(tmp_path / "ckp")
    off = _train12(tmp_path, False, ckp)
    on = _train12(tmp_path, True)
    log, params, state, opt, drawn, model, case, data_valid = off
    losses = [l for _, l in log]
    print(f"[torch model trainer] unrolls {drawn[:12]} losses {['%.5e' % l for l in losses]}")
    assert len(log) == 12 and opt["count"] == 12 and np.isfinite(losses).all()
    assert drawn == on[4] and 0 < sum(n > 0 for n in drawn[:12]) < 12   # both routes of the step were taken
    assert log == on[0], (log, on[0])                                   # device_unroll on: the same losses to the bit
    assert np.array_equal(_bits(model.flatten(params)), _bits(on[5].flatten(on[1])))
    assert opt["m"].shape == (model.flatten(params).size,) and np.abs(opt["v"]).max() > 0
    # the checkpoint of the evaluation at step 11 holds the weights the run returned; infer from it = infer from memory
    loaded, lstate, lopt, step = load_haiku(ckp)
    assert step == 11 and set(loaded) == set(params) and set(lopt) >= {"m", "v", "count"}
    assert np.array_equal(_bits(model.flatten(model.params_from_haiku(loaded))), _bits(model.flatten(params)))
    cfg = {"batch_size": 2, "metrics": ["mse"], "out_type": "pkl", "n_trajs": 2}
    out_m = infer(model, case, data_valid, params=params, state=state, cfg_eval_infer=cfg, n_rollout_steps=4,
                  rollout_dir=str(tmp_path / "mem"))
    out_c = infer(model, case, data_valid, load_ckp=ckp, cfg_eval_infer=cfg, n_rollout_steps=4, rollout_dir=str(tmp_path / "ckp_roll"))
    for i in range(2):
        a = pickle.load(open(tmp_path / "mem" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        b = pickle.load(open(tmp_path / "ckp_roll" / f"rollout_{i}.pkl", "rb"))["predicted_rollout"]
        assert a.shape == (ISL + 4, 200, 2) and np.isfinite(a).all() and np.array_equal(a, b)
        assert not np.array_equal(a[ISL:], np.transpose(data_valid[i][0], (1, 0, 2))[ISL:ISL + 4])
        assert torch.equal(out_m[f"rollout_{i}"]["mse"].cpu(), out_c[f"rollout_{i}"]["mse"].cpu())


def test_trainer_with_the_sample_made_on_the_device(tmp_path):
    """train.device_data: the sample comes from case.preprocess_device / engine.train_batch, which hands the particle types
    to the engine through set_particle_type_device - where TorchModel.loss_grad reads them.  The noise stream differs
    from the host route's, so the losses are compared between the two unroll routes, not with the run above."""
    _need_gpu()
    off = _train12(tmp_path, False, device_data=True)
    on = _train12(tmp_path, True, device_data=True)
    log, params, state, opt, drawn, model = off[:6]
    losses = [l for _, l in log]
    print(f"[torch model trainer, device_data] unrolls {drawn[:12]} losses {['%.5e' % l for l in losses]}")
    assert len(log) == 12 and opt["count"] == 12 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert 0 < sum(n > 0 for n in drawn[:12]) < 12 and drawn == on[4]
    assert log == on[0], (log, on[0])
    assert np.array_equal(_bits(model.flatten(params)), _bits(on[5].flatten(on[1])))
    eng = off[6].engine(2)
    assert eng.particle_type is not None and eng.particle_type.dtype == torch.int32 and tuple(eng.particle_type.shape) == (2, 200)


def test_a_state_other_than_the_training_copys_is_refused():
    _need_gpu()
    pos, pt, hcase, model, params, state = _setup("rpf2d_b1")
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    other = {"~": {"in_scale": (state["~"]["in_scale"] * np.float32(1.5))}}
    ref = _np(model.apply(params, other, (feats, pt))[0]["acc"])          # no training handle: any state is fine
    assert not np.array_equal(ref, _np(model.apply(params, state, (feats, pt))[0]["acc"]))
    th = model.train_handle(eng, params)
    model.apply(params, state, (feats, pt))                                # the training copy's buffers
    model.apply(params, {}, (feats, pt))                                   # no state: the wrapped module's, the same
    for call in (lambda: model.apply(params, other, (feats, pt)),
                 lambda: model.apply_handle(model.unroll_handle(eng, th, params), other, (feats, pt))):
        with pytest.raises(RuntimeError, match="set_state"):
            call()
    th.close()
    assert np.array_equal(_bits(_np(model.apply(params, other, (feats, pt))[0]["acc"])), _bits(ref))
    # set_state first: the training copy is made from it, and loss_grad, unroll and apply agree
    model.set_state(other)
    th = model.train_handle(eng, params)
    a = _np(model.apply_handle(model.unroll_handle(eng, th, params), other, (feats, pt))[0]["acc"])
    assert np.array_equal(_bits(a), _bits(ref))
    # dropping the last reference frees the handle at once (no reference cycle through the aliased parameters)
    import weakref
    mod, wr = th.module, weakref.ref(th)
    del th
    assert wr() is None and all(p.numel() == 0 for p in mod.parameters())


def test_double_backward_through_the_graph_ops_raises():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    pos, pt, hcase, _, _, _ = _setup("rpf2d_b1")
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    g = Graph(feats)
    x = torch.randn((1, eng.N, 4), device=eng.device, requires_grad=True)
    y = (g.segment_sum(g.gather(x, "senders"), "receivers") ** 2).sum()
    (gx,) = torch.autograd.grad(y, x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated"):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------ eval_rollout
def test_eval_rollout_takes_the_generic_loop(tmp_path, monkeypatch):
    _need_gpu()
    from lagrangebench_amd.evaluate import MetricsComputer, eval_rollout
    from lagrangebench_amd.evaluate.rollout import _Loader
    from lagrangebench_amd.utils import get_kinematic_mask
    n_steps = 4
    pos, pt, hcase, model, params, state = _setup("ldc3d")
    params["dec"]["weight"] *= np.float32(0.05)   # a calm rollout
    params["dec"]["bias"] *= np.float32(0.05)
    ds = _dataset("ldc3d")
    eng = hcase.engine(1)
    monkeypatch.setattr(eng, "rollout", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused device loop ran")))
    _, nbrs = hcase.allocate_eval((pos[0, :, :ISL], pt[0]))
    mc = MetricsComputer(["mse"], dist_fn=hcase.displacement, metadata=ds.metadata, input_seq_length=ISL, stride=1, case=hcase)
    out = eval_rollout(model.apply, hcase, params, state, _Loader(ds, 1), nbrs, mc, n_steps, 1, str(tmp_path), out_type="pkl")
    pred = pickle.load(open(tmp_path / "rollout_0.pkl", "rb"))["predicted_rollout"][ISL:]
    assert pred.shape == (n_steps, pos.shape[1], 3) and out["rollout_0"]["mse"].shape[0] == n_steps
    # the same four steps by hand: preprocess_eval -> apply -> case.integrate -> kinematic particles from the data
    cur = torch.as_tensor(pos[:, :, :ISL], device=eng.device)
    ptd = torch.as_tensor(pt, device=eng.device)
    kin = get_kinematic_mask(ptd)
    _, nb = hcase.allocate_eval((cur, ptd))
    for k in range(n_steps):
        feats, nb = hcase.preprocess_eval((cur, ptd), nb)
        assert not bool(nb.did_buffer_overflow.any())
        p, _ = model.apply(params, state, (feats, ptd))
        nxt = hcase.integrate(p, cur)
        nxt = torch.where(kin[..., None], torch.as_tensor(pos[:, :, ISL + k], device=eng.device), nxt)
        cur = torch.cat([cur[:, :, 1:], nxt[:, :, None]], dim=2)
        assert np.array_equal(_np(nxt[0]), pred[k]), k
    assert kin.any() and not kin.all()
    assert not np.array_equal(pred[-1], pos[0, :, ISL + n_steps - 1])
