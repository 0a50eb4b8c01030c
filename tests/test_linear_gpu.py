"""models.Linear on the device (csrc/lb_linear.hip, csrc/lb_train_linear.h) against the float64 restatement
tests/_linear_oracle.py on the oracle case's features: forward, determinism and batching, the fused rollout without a
neighbor search, the training step (closed-form gradient, AdamW), six optimiser steps against a float64 replay, the
autograd module and the device unroll route, and the reference's own end-to-end test (tests/runner_test.py) replayed.

Cases - the smallest that reach every path of the kernels:
  rpf2d   scale 0.25, magnitude features: N = 200 (the last wave pass of k_ln_forward holds 8 rows, two of its four
          16-lane groups are masked), F = 17 (the feature row ends inside a float4), external force, periodic, one type;
          B = 1 and B = 2 (N = 400)
  ldc3d   scale 0.5 in free space, magnitudes on and off: N = 1020 (more than one workgroup, a tail of 12 rows; 16 chunks of
          k_ln_dw, the last one short), F = 26 / 21, bound columns, types 0 / 1 / 2 (a non-zero type column, the kinematic
          mask), dim 3
  lj      the LJ fixture with input_seq_length 3: N = 3 (one partial wave pass), F = 6
"""
import json
import os
import shutil
from functools import partial

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lb_oracle as O  # noqa: E402
from tests import _linear_oracle as LO  # noqa: E402
from tests._common import hip_case, oracle_case, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
LJ = os.path.join(ROOT, "golden", "3D_LJ_3_1214every1")
CASES = {   # id: (name, scale, magnitude features, free space, B)
    "rpf2d_b1": ("rpf2d", 0.25, True, False, 1),
    "rpf2d_b2": ("rpf2d", 0.25, True, False, 2),
    "ldc3d_mag": ("ldc3d", 0.5, True, True, 1),
    "ldc3d": ("ldc3d", 0.5, False, True, 1),
    "lj": ("lj", None, False, False, 1),
}
N_IN = {"rpf2d_b1": 18, "rpf2d_b2": 18, "ldc3d_mag": 27, "ldc3d": 22, "lj": 7}
SINGLE = ["rpf2d_b1", "ldc3d_mag", "lj"]   # the three cases of the six-step test (B = 1)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _setup(cid, extra=6):
    """(pos (B, N, T, dim), particle types (B, N), engine case, oracle case, isl)."""
    name, scale, mag, free, B = CASES[cid]
    if name == "lj":
        from lagrangebench_amd.case_setup import case_builder
        from lagrangebench_amd.data import H5Dataset
        isl = 3
        ds = H5Dataset("valid", LJ, name="lj3d", input_seq_length=isl, extra_seq_length=extra)
        md = ds.metadata
        bounds = np.array(md["bounds"])
        box = bounds[:, 1] - bounds[:, 0]
        hcase, ocase = case_builder(box, md, isl, noise_std=0.0), O.case_builder(box, md, isl, noise_std=0.0)
    else:
        from lagrangebench_amd.data import make_case
        isl = 6
        ds = make_case(name, n_trajs=B, extra_seq_length=extra, input_seq_length=isl, scale=scale)
        ds.magnitude_features = mag
        if free:
            ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
        hcase, ocase = hip_case(ds), oracle_case(ds)
    pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(B)])
    return pos, pt, hcase, ocase, isl


def _params(cid, dim, seed=7):
    """hk.Linear's initialiser with a random bias on top (b = 0 would leave the bias path unseen)."""
    from lagrangebench_amd.models import Linear
    model = Linear(dim)
    params = model.init_params(seed, N_IN[cid])
    params["linear"]["b"] = (0.1 * np.random.default_rng(seed + 1).standard_normal(dim)).astype(np.float32)
    return model, params


def _oracle_features(ocase, pos, pt, isl):
    return [ocase.allocate_eval((pos[b, :, :isl], pt[b]))[0] for b in range(pos.shape[0])]


# ------------------------------------------------------------------------------------------------ 1, 2: forward
@pytest.mark.parametrize("cid", list(CASES))
def test_forward_matches_the_float64_restatement(cid):
    _need_gpu()
    pos, pt, hcase, ocase, isl = _setup(cid)
    B, N, dim = pos.shape[0], pos.shape[1], pos.shape[3]
    model, params = _params(cid, dim)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    assert feats.engine.node_in + 1 == N_IN[cid]
    out = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    assert out.dtype == np.float32 and out.shape == (B, N, dim)
    w, b = params["linear"]["w"], params["linear"]["b"]
    for i, of in enumerate(_oracle_features(ocase, pos, pt, isl)):
        assert LO.concat(of, pt[i]).shape == (N, N_IN[cid])
        r64 = LO.linear_forward(w, b, of, pt[i], torch.float64).numpy()
        r32 = LO.linear_forward(w, b, of, pt[i], torch.float32).numpy()
        e, e32 = rel_err(out[i], r64), rel_err(r32, r64)
        print(f"[linear forward {cid} b={i}] device vs fp64 {e:.2e}; fp32 restatement vs fp64 {e32:.2e}")
        assert e <= 1e-5, (cid, i, e, e32)
    if cid.startswith("ldc3d"):
        assert set(np.unique(pt)) == {0, 1, 2}   # the type column is not all zero
    # two calls: identical bits
    again = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    assert np.array_equal(_bits(out), _bits(again))


def test_a_batch_equals_its_trajectories_one_by_one():
    _need_gpu()
    pos, pt, hcase, _, isl = _setup("rpf2d_b2")
    model, params = _params("rpf2d_b2", 2)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    both = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    assert not np.array_equal(pos[0], pos[1])
    for b in range(2):
        f1, _ = hcase.allocate_eval((pos[b:b + 1, :, :isl], pt[b:b + 1]))
        assert f1.engine is not feats.engine and f1.engine.B == 1
        one = _np(model.apply(params, {}, (f1, pt[b:b + 1]))[0]["acc"])
        assert np.array_equal(_bits(both[b]), _bits(one[0]))


def test_create_checks_the_description_against_the_engine():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    pos, pt, hcase, _, isl = _setup("rpf2d_b1")
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    model, params = _params("ldc3d", 2)   # 22 inputs on an 18-input case
    with pytest.raises(LbHipError, match="-1.*does not match the case"):
        model.apply(params, {}, (feats, pt))
    with pytest.raises(LbHipError, match="does not match the case"):
        model.train_handle(feats.engine, params)


def test_forward_reports_an_overflowed_list_and_needs_none():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    pos, pt, hcase, _, isl = _setup("rpf2d_b1")
    model, params = _params("rpf2d_b1", 2)
    eng = hcase.engine(1)
    eng.set_particle_type(pt)
    eng.load_window(pos, 0, 0)
    h = model._create(eng, params, None)
    assert eng.e_cap == 0
    no_list = _np(eng.linear_forward(h))          # the model reads no edges: no list has been allocated yet
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    ref = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    assert np.array_equal(_bits(no_list), _bits(ref))
    eng.nl_set_capacity(eng.cell_capacity, eng.stats()["n_edges_total"] - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    with pytest.raises(LbHipError, match="-3.*overflowed"):   # the step kernels are no-ops now: say so, write nothing
        eng.linear_forward(h)
    eng.nl_allocate()
    assert np.array_equal(_bits(_np(eng.linear_forward(h))), _bits(ref))


# ------------------------------------------------------------------------------------------------ 3: rollout
def _rollouts(hcase, pos, pt, model, params, n_steps, isl):
    """(fused lb_linear_rollout, generic Python loop driving Linear.apply + case.integrate) through evaluate.rollout, and
    the neighbor-list builds each of the two made."""
    from lagrangebench_amd.evaluate.rollout import _eval_batched_rollout, _forward_eval
    out, builds = [], []
    for fused in (True, False):
        fe = partial(_forward_eval, model_apply=model.apply, case_integrate=hcase.integrate)
        if fused:
            fe._lb_gns = model
        _, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
        eng = hcase.engine(pos.shape[0])
        eng.edge_accounting(reset=True)
        preds, _, _ = _eval_batched_rollout(fe, hcase.preprocess_eval, hcase, params, {}, (pos, pt), nbrs,
                                            lambda a, b: {}, n_steps, isl)
        builds.append(eng.edge_accounting()["builds"])
        out.append(_np(preds))
    return out, builds


@pytest.mark.parametrize("cid", ["ldc3d_mag", "rpf2d_b2"])
def test_fused_rollout_equals_the_generic_loop_without_a_search(cid):
    _need_gpu()
    n_steps = 5
    pos, pt, hcase, _, isl = _setup(cid, extra=n_steps)
    model, params = _params(cid, pos.shape[3])
    params["linear"]["w"] *= np.float32(0.05)   # a calm rollout
    (fused, generic), builds = _rollouts(hcase, pos, pt, model, params, n_steps, isl)
    assert np.isfinite(fused).all() and np.array_equal(fused, generic)
    # the generic loop searches once per step; the fused loop not at all (the one build is evaluate.rollout's own
    # nl_update on the state it leaves behind)
    assert builds[1] >= n_steps and builds[0] == 1, builds
    if cid == "ldc3d_mag":
        kin = (pt[0] == 1) | (pt[0] == 2)
        assert kin.any() and not kin.all()
        for k in range(n_steps):
            assert np.array_equal(fused[0, k][kin], pos[0, kin, isl + k])   # kinematic particles follow the data
    assert not np.array_equal(fused[:, -1], pos[:, :, isl + n_steps - 1])   # the others do not
    # the handle's own entry point: no re-allocation reported, and again the same bits
    eng = hcase.engine(pos.shape[0])
    eng.edge_accounting(reset=True)
    pred, n_realloc = eng.rollout(model.handle(eng, params), pos, n_steps)
    assert eng.edge_accounting()["builds"] == 0   # the fused loop itself: not one list build
    assert n_realloc == 0 and np.array_equal(_np(pred), fused)


# ------------------------------------------------------------------------------------------------ 4: training step
def _closed_form_batch(params, feats_o, pt, tg):
    """(mean loss, summed dW, summed db) over the trajectories of a batch (trainer.py:63-89), float64."""
    w, b = params["linear"]["w"], params["linear"]["b"]
    ls, dws, dbs = zip(*[LO.closed_form(w, b, of, pt[i], tg[i]) for i, of in enumerate(feats_o)])
    return float(np.mean([float(v) for v in ls])), sum(dws).numpy(), sum(dbs).numpy()


@pytest.mark.parametrize("cid", list(CASES))
def test_training_step(cid):
    _need_gpu()
    pos, pt, hcase, ocase, isl = _setup(cid)
    B, N, dim = pos.shape[0], pos.shape[1], pos.shape[3]
    model, params = _params(cid, dim)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    apply_acc = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    tg = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss_h, pred_h = th.loss_grad(tg, 1.0, want_pred=True)
    assert np.array_equal(_bits(_np(pred_h)), _bits(apply_acc))   # the inference forward, bit for bit
    g_flat = th.read("grads")
    for _ in range(2):   # three calls in all: identical bits
        th.zero_grad()
        assert th.loss_grad(tg, 1.0) == loss_h and np.array_equal(_bits(th.read("grads")), _bits(g_flat))
    assert np.array_equal(th.read("weights"), model.flatten(params))
    l_ref, dw_ref, db_ref = _closed_form_batch(params, _oracle_features(ocase, pos, pt, isl), pt, tg.numpy())
    g_h = model.unflatten(g_flat, params)["linear"]
    e_l = abs(loss_h - l_ref) / abs(l_ref)
    e_w = np.abs(g_h["w"] - dw_ref).max() / np.abs(dw_ref).max()
    e_b = np.abs(g_h["b"] - db_ref).max() / np.abs(db_ref).max()
    print(f"[linear train {cid}] loss {loss_h:.6e} (rel. error {e_l:.2e}); dW {e_w:.2e}, db {e_b:.2e} of the leaf's largest entry")
    assert e_l <= 1e-5 and e_w <= 1e-4 and e_b <= 1e-4, (e_l, e_w, e_b)
    # (the loss leaves the type row of dW at zero here: the only non-zero types, 1 and 2, are kinematic and masked; the
    # type column of the backward is checked with a caller's d pred in test_device_module_...)
    # gradients accumulate until zero_grad
    th.loss_grad(tg, 1.0)
    assert np.abs(th.read("grads") - 2 * g_flat).max() <= 1e-6 * np.abs(g_flat).max()
    th.zero_grad()
    th.loss_grad(tg, 1.0)
    # one AdamW step against torch.optim.AdamW on the device gradients
    leaves = {k: torch.tensor(np.asarray(params["linear"][k], np.float64), requires_grad=True) for k in ("w", "b")}
    for k, v in leaves.items():
        v.grad = torch.as_tensor(g_h[k]).double()
    torch.optim.AdamW(list(leaves.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2).step()
    th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    w_h = model.unflatten(th.read("weights"), params)["linear"]
    for k, v in leaves.items():
        ref = v.detach().numpy()
        assert np.abs(w_h[k] - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1.0) + 1e-7, k
    assert th.step_count() == 1
    th.close()


# ------------------------------------------------------------------------------------------------ 5: six steps
@pytest.mark.parametrize("cid", SINGLE)
def test_six_steps_lower_the_loss_like_the_float64_replay(cid):
    """Six AdamW steps (lr 1e-3, weight decay 1e-8) on one fixed window with random targets (seed 7).  The float64 replay -
    closed-form gradient + torch.optim.AdamW - must lower its loss by at least 0.49 % at every step on all three cases: three
    orders above the 1e-5 the device loss is held to, so rounding cannot flip the sign and the device loss must fall
    strictly.  The initial weights are hk.Linear's initialiser with seed 0 (plus the random bias): with them the replay falls
    by 0.66 - 0.68 % (rpf2d), 0.52 - 0.54 % (ldc3d) and 0.500 - 0.505 % (lj) a step (computed on the CPU; with seed 7, the
    weights of the other tests, lj falls by 0.458 % only).  Step 0 is held to 1e-5; the deviation of steps 1 - 5 is printed
    (DESIGN.md section 4.6d keeps the largest value)."""
    _need_gpu()
    pos, pt, hcase, ocase, isl = _setup(cid)
    N, dim = pos.shape[1], pos.shape[3]
    model, params = _params(cid, dim, seed=0)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    tg = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    th = model.train_handle(feats.engine, params)
    dev = []
    for _ in range(6):
        th.zero_grad()
        dev.append(th.loss_grad(tg, 1.0))
        th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-8)
    th.close()
    ref = replay_losses(params, _oracle_features(ocase, pos, pt, isl)[0], pt[0], tg[0].numpy())
    drop = [(ref[k] - ref[k + 1]) / ref[k] for k in range(5)]
    devi = [abs(d - r) / r for d, r in zip(dev, ref)]
    print(f"[linear six steps {cid}] device {['%.6e' % v for v in dev]}; replay drop per step {['%.3e' % v for v in drop]}; "
          f"deviation from the replay {['%.2e' % v for v in devi]} (largest of steps 1-5: {max(devi[1:]):.2e})")
    assert min(drop) >= 4.9e-3, drop
    assert devi[0] <= 1e-5, devi
    assert all(dev[k + 1] < dev[k] for k in range(5)), dev


def replay_losses(params, of, pt, tg, steps=6, lr=1e-3):
    """The losses of `steps` AdamW steps in float64: closed-form gradient, torch.optim.AdamW(weight_decay 1e-8)."""
    w = torch.tensor(np.asarray(params["linear"]["w"], np.float64), requires_grad=True)
    b = torch.tensor(np.asarray(params["linear"]["b"], np.float64), requires_grad=True)
    opt = torch.optim.AdamW([w, b], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8)
    out = []
    for _ in range(steps):
        loss, dw, db = LO.closed_form(w.detach().numpy(), b.detach().numpy(), of, pt, tg)
        w.grad, b.grad = dw, db
        opt.step()
        out.append(float(loss))
    return out


# ------------------------------------------------------------------------------------------------ 6: handle and unroll
def test_device_module_gives_the_fused_steps_gradient_and_refuses_the_window():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.autograd import DeviceModule
    cid = "ldc3d_mag"
    pos, pt, hcase, ocase, isl = _setup(cid)
    N, dim = pos.shape[1], pos.shape[3]
    model, params = _params(cid, dim)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    tg = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    th = model.train_handle(eng, params)
    th.zero_grad()
    th.loss_grad(tg, 1.0)
    g_fused = th.read("grads")
    # the same d loss / d pred through forward / backward: the kinematic rows are zero, the others 2 (pred - target) / n_nk
    pred = th.forward()
    nk = LO.non_kinematic(pt[0]).to(pred.device)
    dpred = torch.zeros_like(pred)
    dpred[0] = torch.where(nk[:, None], 2.0 * (pred[0] - tg[0].to(pred.device).float()) / nk.sum().float(), torch.zeros_like(pred[0]))
    with pytest.raises(LbHipError, match="-5.*GNS only"):
        th.backward(dpred, want_dpos=True)
    th.zero_grad()
    assert th.backward(dpred) is None   # the refusal left the forward live
    g_split = th.read("grads")
    # the view between forward and backward (the unroll route): it has rows of its own, the saved activations stay
    th.forward()
    other = np.roll(pos, 1, axis=1)[:, :, 1:isl + 1]
    eng.load_window(np.ascontiguousarray(other), 0, 0)
    assert not torch.equal(eng.linear_forward(th.model_handle()), pred)
    th.zero_grad()
    th.backward(dpred)
    assert np.array_equal(_bits(th.read("grads")), _bits(g_split))
    eng.load_window(pos[:, :, :isl], 0, 0)
    # a d pred that is non-zero on the kinematic rows too: the type column (types 1 and 2) of [X | type | 1]^T dY
    dall = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).to(pred.device)
    th.forward()
    th.zero_grad()
    th.backward(dall)
    g_all = model.unflatten(th.read("grads"), params)["linear"]
    x = LO.concat(ocase.allocate_eval((pos[0, :, :isl], pt[0]))[0], pt[0]).numpy()
    dw_ref, db_ref = x.T @ _np(dall[0]).astype(np.float64), _np(dall[0]).astype(np.float64).sum(0)
    assert np.abs(dw_ref[-1]).max() > 0
    assert np.abs(g_all["w"] - dw_ref).max() <= 1e-4 * np.abs(dw_ref).max(), np.abs(g_all["w"] - dw_ref).max(0)
    assert np.abs(g_all["w"][-1] - dw_ref[-1]).max() <= 1e-4 * np.abs(dw_ref[-1]).max()   # the type row by itself
    assert np.abs(g_all["b"] - db_ref).max() <= 1e-4 * np.abs(db_ref).max()
    th.close()
    mod = DeviceModule(model, hcase, params, 1)
    window = torch.as_tensor(pos[:, :, :isl], device=eng.device)
    out = mod(window, pt)["acc"]
    assert torch.equal(out, pred) and out.grad_fn is not None
    out.backward(dpred)
    g_mod = _np(mod.weights.grad)
    assert np.array_equal(_bits(g_mod), _bits(g_split))   # the module is the handle's forward / backward
    # k_mse_grad forms 2 lw w_i diff with w_i = 1 / n_nk in one rounding order, the lines above in another: each d pred differs by
    # a few ulp (2^-22 relative), and a sum of N = 1020 such terms with cancellation by up to sqrt(N) times that: 1e-5
    assert np.abs(g_split - g_fused).max() <= 1e-5 * np.abs(g_fused).max()
    with pytest.raises(NotImplementedError, match="GNS only"):
        mod(window.clone().requires_grad_(True), pt)
    mod.handle.close()


def test_unroll_handle_follows_the_optimiser_without_a_host_copy():
    _need_gpu()
    cid = "rpf2d_b1"
    pos, pt, hcase, _, isl = _setup(cid)
    N, dim = pos.shape[1], pos.shape[3]
    model, params = _params(cid, dim)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    th = model.train_handle(eng, params)
    view = model.unroll_handle(eng, th, params)
    assert view is th.model_handle() and view is model.unroll_handle(eng, th, params)
    before = _np(eng.linear_forward(view))
    assert np.array_equal(_bits(before), _bits(_np(model.apply(params, {}, (feats, pt))[0]["acc"])))
    tg = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    th.zero_grad()
    th.loss_grad(tg, 1.0)
    th.adamw_step(1e-2)
    after = _np(eng.linear_forward(view))
    assert not np.array_equal(before, after)
    fresh = model._create(eng, model.unflatten(th.read("weights"), params), None)
    assert np.array_equal(_bits(after), _bits(_np(eng.linear_forward(fresh))))
    # the push-forward route of the Trainer on the view
    out, _ = model.apply_handle(view, {}, (feats, pt))
    assert np.array_equal(_bits(_np(out["acc"])), _bits(after))
    ra, rb = _np(eng.rollout(view, pos, 3)[0]), _np(eng.rollout(fresh, pos, 3)[0])
    assert np.isfinite(ra).all() and np.array_equal(ra, rb)
    view.close()          # borrowed: closing it frees nothing
    assert _np(eng.linear_forward(th.model_handle())).shape == after.shape
    th.close()


# ------------------------------------------------------------------------------------------------ 7: the reference's test
def test_the_references_runner_test_replayed(tmp_path):
    """lagrangebench's tests/runner_test.py: Linear on the LJ set, input_seq_length 3, mode all, 10 steps - its config dict
    verbatim, merged onto the full defaults as it does."""
    _need_gpu()
    pytest.importorskip("yaml")
    from lagrangebench_amd import config as C
    from lagrangebench_amd.runner import train_or_infer
    from lagrangebench_amd.utils import load_haiku
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(LJ, ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    md.setdefault("write_every", 1)
    json.dump(md, open(ds_dir / "metadata.json", "w"))
    cfg = {
        "mode": "all",
        "dataset": {"src": "tests/3D_LJ_3_1214every1"},
        "model": {"name": "linear", "input_seq_length": 3},
        "train": {"step_max": 10, "noise_std": 0.0},
        "eval": {
            "n_rollout_steps": 5,
            "train": {"n_trajs": 2, "metrics_stride": 5, "metrics": ["mse"], "out_type": "none"},
            "infer": {"n_trajs": 2, "metrics_stride": 1, "metrics": ["mse"], "out_type": "none"},
        },
        "logging": {"log_steps": 1, "eval_steps": 5, "wandb": False, "ckp_dir": "/tmp/ckp"},
    }
    cfg["dataset"]["src"] = str(ds_dir)               # the two paths of the reference's checkout
    cfg["logging"]["ckp_dir"] = str(tmp_path / "ckp")
    cfg = C.merge(C.reference_defaults(), cfg)
    C.check_cfg(cfg)
    assert train_or_infer(cfg) == 0
    runs = os.listdir(tmp_path / "ckp")
    assert len(runs) == 1 and runs[0].startswith("linear_")
    run = tmp_path / "ckp" / runs[0]
    for d in (run, run / "best"):
        loaded, _, opt, step = load_haiku(str(d))
        assert set(loaded) == {"linear/~/linear"} and loaded["linear/~/linear"]["w"].shape == (7, 3) and step in (5, 10)
        assert set(opt) >= {"m", "v", "count"}
        saved = C.load(str(d / "config.yaml"))
        assert saved.model.name == "linear" and saved.train.step_max == 10 and saved.dataset.src == str(ds_dir)
        assert saved.logging.run_name == runs[0] and saved.mode == "all"
