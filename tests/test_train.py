"""Training step: lagrangebench_amd/train mirrors lagrangebench/train.

CPU: the training tricks against the reference's own tests (tests/case_test.py:165-187 noise
consistency, tests/pushforward_test.py:24-42 unroll sampling), the differentiable torch GNS against
the NumPy oracle, its gradients against finite differences, the learning-rate schedule.
GPU: the torch forward on engine-built graphs equals the HIP forward; the Trainer lowers the loss on
the LJ dataset, writes reference-format checkpoints, and `train_or_infer(mode="all")` returns 0
(tests/runner_test.py:14-57).
"""
import json
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lb_oracle as O  # noqa: E402
from tests._common import feature_widths, make_params, oracle_case  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
LJ = os.path.join(ROOT, "golden", "3D_LJ_3_1214every1")


def test_random_walk_noise_statistics_and_consistency():
    """strats.py:12-83: kinematic particles stay clean, the noise of the last input frame is carried
    onto the targets (so the target velocity is unchanged), and the velocity noise of the last input
    step has standard deviation noise_std."""
    from lagrangebench_amd.case_setup.case import make_displacement
    from lagrangebench_amd.train import add_gns_noise
    disp, shift = make_displacement(np.array([1.0, 1.0]), True)
    n, isl, T = 4000, 6, 9
    rng = np.random.default_rng(0)
    pos = torch.from_numpy(rng.random((n, T, 2)))
    pt = torch.zeros(n, dtype=torch.int64)
    pt[:100] = 1
    g = torch.Generator().manual_seed(3)
    g2, noisy = add_gns_noise(g, pos, pt, isl, 3e-4, shift)
    assert g2 is g and noisy.shape == pos.shape
    d = disp(noisy, pos)
    assert float(d[:100].abs().max()) == 0.0                       # kinematic: no noise
    assert float(d[100:, 0].abs().max()) == 0.0                    # frame 0 is never perturbed
    assert torch.allclose(d[:, isl:], d[:, isl - 1:isl].expand(-1, T - isl, -1), atol=1e-15)
    vel_noise_last = (d[100:, isl - 1] - d[100:, isl - 2]).numpy() # noise of the last input velocity
    assert abs(vel_noise_last.std() / 3e-4 - 1.0) < 0.05
    # target velocity (frame isl -> isl+1) is untouched by the noise
    v_clean = disp(pos[:, isl + 1], pos[:, isl])
    v_noisy = disp(noisy[:, isl + 1], noisy[:, isl])
    assert torch.allclose(v_clean, v_noisy, atol=1e-12)


def test_push_forward_sampling_frequencies():
    """tests/pushforward_test.py:24-42: before the first threshold only unroll 0; afterwards the
    unlocked unroll lengths appear with the configured probability ratios."""
    from lagrangebench_amd.train import push_forward_sample_steps
    pf = {"steps": [-1, 20000, 50000, 100000], "unrolls": [0, 1, 3, 20], "probs": [4.05, 4.88, 1.25, 0.32]}
    g = torch.Generator().manual_seed(1)
    for step, n_open in [(1, 1), (30000, 2), (60000, 3), (150000, 4)]:
        draws = []
        for _ in range(4000):
            g, u = push_forward_sample_steps(g, step, pf)
            draws.append(u)
        draws = np.array(draws)
        assert set(np.unique(draws)) <= set(pf["unrolls"][:n_open])
        p = np.array(pf["probs"][:n_open])
        p = p / p.sum()
        for u, pu in zip(pf["unrolls"][:n_open], p):
            assert abs((draws == u).mean() - pu) < 0.03


def test_learning_rate_schedule():
    from lagrangebench_amd.train.trainer import exponential_decay
    assert exponential_decay(0, 1e-4, 1e5, 0.1, 1e-6) == pytest.approx(1e-4)
    assert exponential_decay(100000, 1e-4, 1e5, 0.1, 1e-6) == pytest.approx(1e-5)
    assert exponential_decay(50000, 1e-4, 1e5, 0.1, 1e-6) == pytest.approx(1e-4 * 0.1 ** 0.5)
    assert exponential_decay(10**7, 1e-4, 1e5, 0.1, 1e-6) == pytest.approx(1e-6)   # end_value


def _oracle_inputs(name="small2d", L=2):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=1, extra_seq_length=3)
    case = oracle_case(ds)
    pos, pt = ds[0]
    feats, _ = case.allocate_eval((pos[:, :ds.input_seq_length].astype(np.float64), pt))
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    return ds, feats, pt, params


def test_torch_gns_matches_the_oracle_and_its_gradients_match_finite_differences():
    from oracle.gns_torch import gns_apply_torch, gns_inputs_from_features, params_to_torch
    L = 2
    ds, feats, pt, params = _oracle_inputs(L=L)
    ref = O.gns_apply(params, feats, pt, num_mp_steps=L, skip_padding=True)["acc"]
    node, edge, snd, rcv, ptt = gns_inputs_from_features(feats, pt)
    p32 = params_to_torch(params)
    acc = gns_apply_torch(p32, node, edge, snd, rcv, ptt, L).numpy()
    assert np.abs(acc - ref).max() <= 1e-5 * np.abs(ref).max()
    # gradients in float64: autograd vs central differences of the same function
    p64 = {m: {k: v.double().requires_grad_(True) for k, v in leaves.items()} for m, leaves in p32.items()}
    target = torch.from_numpy(np.random.default_rng(0).standard_normal(ref.shape))

    def loss_of(p):
        out = gns_apply_torch(p, node.double(), edge.double(), snd, rcv, ptt, L)
        return ((out - target) ** 2).sum(-1).mean()
    loss = loss_of(p64)
    loss.backward()
    rng = np.random.default_rng(1)
    for mod, leaf in [("enc_node/linear_0", "w"), ("proc1_edge/linear_1", "w"), ("proc0_node/layer_norm", "scale"),
                      ("decoder/linear_1", "b"), ("embed", "embeddings"), ("proc0_edge/linear_0", "b")]:
        t = p64[mod][leaf]
        flat = t.detach().reshape(-1)
        for idx in rng.integers(0, flat.numel(), size=3):
            old = float(flat[idx])
            h = 1e-6 * max(1.0, abs(old))
            with torch.no_grad():
                t.reshape(-1)[idx] = old + h
                lp = float(loss_of(p64))
                t.reshape(-1)[idx] = old - h
                lm = float(loss_of(p64))
                t.reshape(-1)[idx] = old
            fd = (lp - lm) / (2 * h)
            an = float(t.grad.reshape(-1)[idx])
            assert abs(fd - an) <= 1e-6 + 1e-4 * abs(fd), (mod, leaf, idx, fd, an)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_torch_forward_on_engine_graph_equals_hip_forward():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from oracle.gns_torch import gns_apply_torch, gns_inputs_from_features, params_to_torch
    from tests._common import hip_case
    L = 3
    ds = make_case("small3d", n_trajs=2, extra_seq_length=3)
    hcase = hip_case(ds)
    isl = ds.input_seq_length
    pos = np.stack([ds[0][0], ds[1][0]])
    pt = np.stack([ds[0][1], ds[1][1]])
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(3, 128, 2, L, 16)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    acc_hip = model.apply(params, {}, (feats, pt))[0]["acc"]
    feats.materialize()
    pt_t = params_to_torch(params, device=acc_hip.device)
    for b in range(2):
        node, edge, snd, rcv, ptt = gns_inputs_from_features(feats, torch.as_tensor(pt), b)
        acc_t = gns_apply_torch(pt_t, node, edge, snd, rcv, ptt, L)
        err = float((acc_t - acc_hip[b]).abs().max() / acc_hip[b].abs().max())
        assert err < 1e-5, err


def _gns_grad_check(model, th, feats, params, target, pt, L, depth, name):
    """One lb_gns_train_loss_grad on the engine's current window / list against torch autograd in float64 on the same
    graph (gns_inputs_from_features): loss, and every gradient leaf within 1e-4 relative; three more calls give the same
    bits.  Returns (loss, gradients by module / leaf, the torch leaves)."""
    from oracle.gns_torch import gns_apply_torch, gns_inputs_from_features, params_to_torch
    from lagrangebench_amd.utils import get_kinematic_mask
    eng = feats.engine
    B = target.shape[0]
    th.zero_grad()
    loss_h, pred_h = th.loss_grad(target, 1.0, want_pred=True)
    g_flat = th.read("grads")
    g_h = model.unflatten(g_flat, params)
    # round 4: no floating-point atomics in the training step (sender-sorted gather transpose, ordered loss / embedding
    # sums): loss and every gradient are bit-reproducible
    for _ in range(3):
        th.zero_grad()
        loss_2, _ = th.loss_grad(target, 1.0, want_pred=True)
        assert loss_2 == loss_h and np.array_equal(th.read("grads"), g_flat)

    feats.materialize()
    dev = eng.device
    # the reference gradients come from a float64 evaluation (round 4): a float32 torch run on the GPU sums its
    # index_add / matmul terms in an order that changes from run to run (atomics), and with both sides in float32 the
    # largest leaf error of the TGV2D L = 10 case scattered around the 1e-4 bar (0.9e-4 .. 1.04e-4: 2 failures in 120
    # runs); against float64 the engine's own error is what is measured
    pt_t = {mod: {k: v.double().requires_grad_(True) for k, v in leaves.items()}
            for mod, leaves in params_to_torch(params, device=dev).items()}
    losses = []
    for b in range(B):
        node, edge, snd, rcv, ptt = gns_inputs_from_features(feats, torch.as_tensor(pt), b)
        pred = gns_apply_torch(pt_t, node.double(), edge.double(), snd, rcv, ptt, L, depth)
        assert float((pred.detach() - pred_h[b]).abs().max() / pred.detach().abs().max()) < 1e-5
        nk = ~get_kinematic_mask(ptt)
        tot = ((pred - target[b].to(dev)) ** 2).sum(dim=-1)
        lb = torch.where(nk, tot, torch.zeros_like(tot)).sum() / nk.sum()
        lb.backward()
        losses.append(float(lb))
    assert abs(loss_h - np.mean(losses)) <= 1e-5 * abs(np.mean(losses)), (loss_h, losses)
    worst = 0.0
    for mod, leaves in pt_t.items():
        for leaf, v in leaves.items():
            ref = v.grad.detach().cpu().numpy()
            err = np.abs(g_h[mod][leaf] - ref).max() / max(np.abs(ref).max(), 1e-30)
            worst = max(worst, err)
            assert err < 1e-4, (mod, leaf, err)
    print(f"[grad {name}] loss {loss_h:.6f}, worst relative gradient error over the leaves {worst:.2e}")
    return loss_h, g_h, pt_t


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale,L,B,latent,depth", [("small2d", 1.0, 3, 2, 128, 2), ("small3d", 1.0, 2, 1, 128, 2),
                                                         ("tgv2d", 0.6, 10, 2, 128, 2), ("ldc3d", 0.4, 2, 2, 128, 2),
                                                         ("small2d", 1.0, 5, 2, 64, 2), ("small3d", 1.0, 2, 2, 40, 2),
                                                         ("small3d", 1.0, 2, 2, 128, 3), ("small2d", 1.0, 3, 2, 48, 4)])
def test_hip_gradients_match_torch_autograd(name, scale, L, B, latent, depth):
    """the hand-written backward (csrc/lb_train.hip: lb_gns_train_loss_grad) against torch
    autograd of the checker network (oracle/gns_torch.py, itself checked against the oracle and finite differences
    above) on engine-built graphs: loss and every parameter gradient of _mse (trainer.py:35-60), gradients summed and
    loss averaged over the batch (trainer.py:63-89), within 1e-4 relative per leaf; then one AdamW step against
    torch.optim.AdamW.  depth = num_mlp_layers (Linears per MLP, models/utils.py:100-115): 2 in every shipped config; 3 and 4
    exercise the middle Linears of the training step (round 6)."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case
    ds = make_case(name, n_trajs=B, extra_seq_length=3, scale=scale)
    hcase = hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    # latent < 128 (round 4: GNS-5-64 of the reference's baselines): the device step runs 128-wide with zero padding
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0, latent_size=latent, blocks_per_step=depth)
    model = GNS(dim, latent, depth, L, 16)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    target = torch.randn((B, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    th = model.train_handle(eng, params)
    loss_h, g_h, pt_t = _gns_grad_check(model, th, feats, params, target, pt, L, depth, name)
    assert th.sort_fallbacks() == 0   # a symmetric list: the sender view by transposition, never the radix sort
    dev = eng.device

    # one optimiser step: optax.adamw == torch AdamW (decoupled decay).  Both get the SAME gradients (the engine's):
    # the first Adam step is sign(g) * lr for |g| >> eps, so rounding-level differences of near-zero gradients
    # (dead ReLU units) would otherwise show up as 1e-5-sized differences of the update
    for mod, lv in pt_t.items():
        for leaf, v in lv.items():
            v.grad = torch.as_tensor(g_h[mod][leaf], device=dev).double()
    leaves = [v for mod in sorted(pt_t) for _, v in sorted(pt_t[mod].items())]
    opt = torch.optim.AdamW(leaves, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    opt.step()
    th.adamw_step(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    w_h = model.unflatten(th.read("weights"), params)
    for mod, lv in pt_t.items():
        for leaf, v in lv.items():
            ref = v.detach().cpu().numpy()
            assert np.abs(w_h[mod][leaf] - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1.0) + 1e-7, (mod, leaf)
    th.close()


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["f16x2", "f32"])
def test_hip_gradients_are_equivariant_under_power_of_two_loss_weights(math, monkeypatch):
    """The training step's products run in f16x2 arithmetic (csrc/lb_lin32.h: k_lin32h, csrc/lb_train.hip: k_dw_part_h) whose
    fp16 range is MADE safe by power-of-two scaling of every row chunk / matrix / row block - not by a guard.  A loss weight of
    2^-30 scales every gradient of the backward pass by 2^-30 (values around 1e-12 .. 1e-15, far below fp16's range): all
    scale factors are exponent arithmetic, so every gradient must come out as EXACTLY 2^-30 times the unweighted one -
    any dependence of the split arithmetic on magnitude would show as a different bit pattern.  LB_TRAIN_MATH=f32 (the exact
    kernels) has the property trivially and runs as the control."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case
    monkeypatch.setenv("LB_TRAIN_MATH", math)
    ds = make_case("small3d", n_trajs=1, extra_seq_length=3)
    hcase = hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos, pt = ds[0]
    params = make_params(ds, num_mp_steps=2, decoder_scale=1.0)
    model = GNS(dim, 128, 2, 2, 16)
    feats, _ = hcase.allocate_eval((pos[None, :, :isl], pt[None]))
    target = torch.randn((1, pos.shape[0], dim), generator=torch.Generator().manual_seed(5))
    th = model.train_handle(feats.engine, params)
    grads = {}
    for w in (1.0, 2.0 ** -30, 2.0 ** 20):
        th.zero_grad()
        th.loss_grad(target, w)
        grads[w] = th.read("grads").astype(np.float64)
    assert np.abs(grads[1.0]).max() > 1e-6
    for w in (2.0 ** -30, 2.0 ** 20):
        assert np.array_equal(grads[w], grads[1.0] * w), (math, w, np.abs(grads[w] / w - grads[1.0]).max())
    th.close()


@pytest.mark.gpu
def test_hip_gradients_agree_between_the_two_arithmetics(monkeypatch):
    """LB_TRAIN_MATH=f32 (exact-fp32 MFMA products: k_lin32f, k_dw_part) against the default scaled f16x2 products (k_lin32h,
    k_dw_part_h) on the same step: loss equal to 1e-6, every gradient leaf within 2e-5 of the leaf's largest entry (the
    autograd test above holds the default arithmetic to 1e-4 against float64; this keeps the exact kernels exercised)."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case
    ds = make_case("small3d", n_trajs=2, extra_seq_length=3)
    hcase = hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(2)])
    pt = np.stack([ds[b][1] for b in range(2)])
    params = make_params(ds, num_mp_steps=3, decoder_scale=1.0)
    model = GNS(dim, 128, 2, 3, 16)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    target = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    out = {}
    for math in ("f32", "f16x2"):
        monkeypatch.setenv("LB_TRAIN_MATH", math)
        th = model.train_handle(feats.engine, params)
        th.zero_grad()
        loss = th.loss_grad(target, 1.0)
        out[math] = (loss, model.unflatten(th.read("grads"), params))
        th.close()
    assert abs(out["f32"][0] - out["f16x2"][0]) <= 1e-6 * abs(out["f32"][0])
    for mod, leaves in out["f32"][1].items():
        for leaf, ref in leaves.items():
            got = out["f16x2"][1][mod][leaf]
            assert np.abs(got - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-30), (mod, leaf)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [18, -14])
def test_activation_range_guard_of_the_weight_gradient_kernel(shift, monkeypatch):
    """k_dw_part_h splits its X operand - saved activations - into fp16 hi / lo "as it is".  Put the
    hidden activations of the node encoder and of the first processor node block out of range without changing the network
    function (first Linear x 2^shift, second Linear x 2^-shift: exact in fp32): 2^18 pushes |a| past fp16's 65504 (NaN weight
    gradients before round 6), 2^-14 pushes every lo half into fp16 subnormals.  The kernel's range guard must catch it: the
    step is repeated with the site's X scale re-centred, or scaled per chunk, in f16x2 (no gradient of the first attempt is
    added), the handle reports one repeated step, and the gradients agree with an LB_TRAIN_MATH=f32 handle like those of an in-range network do (2e-5 per leaf)."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case
    ds = make_case("small3d", n_trajs=1, extra_seq_length=3)
    hcase = hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos, pt = ds[0]
    params = make_params(ds, num_mp_steps=2, decoder_scale=1.0)
    f = np.float32(2.0 ** shift)
    for blk in ("enc_node", "proc0_node"):
        params[f"{blk}/linear_0"]["w"] = params[f"{blk}/linear_0"]["w"] * f
        params[f"{blk}/linear_0"]["b"] = params[f"{blk}/linear_0"]["b"] * f
        params[f"{blk}/linear_1"]["w"] = params[f"{blk}/linear_1"]["w"] / f
    model = GNS(dim, 128, 2, 2, 16)
    feats, _ = hcase.allocate_eval((pos[None, :, :isl], pt[None]))
    target = torch.randn((1, pos.shape[0], dim), generator=torch.Generator().manual_seed(5))
    out = {}
    for math in ("f32", "f16x2"):
        monkeypatch.setenv("LB_TRAIN_MATH", math)
        th = model.train_handle(feats.engine, params)
        th.zero_grad()
        loss = th.loss_grad(target, 1.0)
        out[math] = (loss, th.read("grads"), th.math_fallbacks())
        th.close()
    assert out["f32"][2] == 0 and out["f16x2"][2] == 1, (out["f32"][2], out["f16x2"][2])
    assert np.isfinite(out["f16x2"][1]).all() and np.abs(out["f16x2"][1]).max() > 0
    assert abs(out["f16x2"][0] - out["f32"][0]) <= 1e-6 * abs(out["f32"][0])
    gf, gh = model.unflatten(out["f32"][1], params), model.unflatten(out["f16x2"][1], params)
    for mod, leaves in gf.items():
        for leaf, ref in leaves.items():
            assert np.abs(gh[mod][leaf] - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-30), (mod, leaf)


@pytest.mark.gpu
def test_sender_view_by_transposition_equals_the_radix_sort():
    """Round 6: the sender-sorted view of the edge list (the transpose of the [n_s | n_r | e] gather) comes from the symmetry
    of the neighbor relation - k_sender_transpose, one bisection per edge - instead of hipcub's radix sort, which stays as
    the fall-back for a list that is not symmetric (LB_TRAIN_SORT=cub forces it).  Both must give the same gradients bit
    for bit, on a periodic 3D case with two trajectories in the batch; the subprocess keeps the env switch out of this
    process (it is read once)."""
    import subprocess
    import sys
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, ".")
from lagrangebench_amd.data import make_case
from lagrangebench_amd.models import GNS
from tests._common import hip_case, make_params
ds = make_case("small3d", n_trajs=2, extra_seq_length=3)
hcase = hip_case(ds)
isl, dim = ds.input_seq_length, len(ds.box)
pos = np.stack([ds[b][0] for b in range(2)]); pt = np.stack([ds[b][1] for b in range(2)])
params = make_params(ds, num_mp_steps=2, decoder_scale=1.0)
model = GNS(dim, 128, 2, 2, 16)
feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
target = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
th = model.train_handle(feats.engine, params)
th.zero_grad(); loss = th.loss_grad(target, 1.0)
np.save(sys.argv[1], th.read("grads")); print("LOSS", repr(loss), th.math_fallbacks())
'''
    import tempfile
    outs = {}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("transpose", "cub"):
            env = dict(os.environ)
            env.pop("LB_TRAIN_SORT", None)
            if mode == "cub":
                env["LB_TRAIN_SORT"] = "cub"
            f = os.path.join(d, mode + ".npy")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=os.path.dirname(ROOT), env=env, capture_output=True, text=True,
                               timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[mode] = (np.load(f), [ln for ln in r.stdout.splitlines() if ln.startswith("LOSS")][-1])
    assert outs["transpose"][1] == outs["cub"][1], (outs["transpose"][1], outs["cub"][1])
    assert np.abs(outs["cub"][0]).max() > 0 and np.array_equal(outs["transpose"][0], outs["cub"][0])


@pytest.mark.gpu
def test_trainer_lowers_the_loss_and_runner_mode_all(tmp_path):
    """tests/runner_test.py:14-57 runs train_or_infer end to end on the LJ dataset and expects 0."""
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.runner import train_or_infer
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(LJ, ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    md.setdefault("write_every", 1)
    json.dump(md, open(ds_dir / "metadata.json", "w"))
    isl, L = 6, 2
    data_train = H5Dataset("train", str(ds_dir), name="lj3d", input_seq_length=isl, extra_seq_length=1)
    data_valid = H5Dataset("valid", str(ds_dir), name="lj3d", input_seq_length=isl, extra_seq_length=10)
    bounds = np.array(md["bounds"])
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=3e-4)
    model = GNS(3, 128, 2, L, 16)
    cfg_train = {"batch_size": 2, "noise_std": 3e-4,
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200},
                 "pushforward": {"steps": [-1, 20], "unrolls": [0, 1], "probs": [1, 1]}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 5, "eval_steps": 30}, input_seq_length=isl, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt_state = trainer.train(step_max=60, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    assert np.isfinite(losses).all() and np.mean(losses[-4:]) < 0.7 * np.mean(losses[:3]), losses
    assert os.path.exists(os.path.join(ckp, "params_tree.pkl")) and os.path.exists(os.path.join(ckp, "best", "params_array.npy"))
    loaded, _, opt_loaded, step = load_haiku(ckp)
    assert step in (30, 60) and any("MLP" in k for k in loaded)
    # the optimiser state travels with the checkpoint (opt_state.pkl: both AdamW moments + the step counter)
    assert os.path.exists(os.path.join(ckp, "opt_state.pkl")) and set(opt_loaded) >= {"m", "v", "step"}
    assert opt_loaded["m"].shape == opt_loaded["v"].shape and np.abs(opt_loaded["v"]).max() > 0
    # resume from the checkpoint for a few more steps (trainer.py:267-269)
    p2, _, _ = trainer.train(step_max=step + 3, load_ckp=ckp)
    assert set(p2) == set(params)
    # the runner route of the reference's runner_test
    cfg = {"mode": "all", "dataset": {"src": str(ds_dir), "name": "lj3d"},
           "model": {"name": "gns", "num_mp_steps": 1, "input_seq_length": isl, "latent_dim": 64},  # (a narrow latent: round 4)
           "train": {"step_max": 12, "batch_size": 1, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]}},
           "logging": {"log_steps": 5, "eval_steps": 5, "ckp_dir": str(tmp_path / "ckp2"), "run_name": "r"},
           "eval": {"n_rollout_steps": 5, "train": {"n_trajs": 1, "metrics": ["mse"]},
                    "infer": {"n_trajs": 1, "batch_size": 1, "metrics": ["mse"], "out_type": "none"}}}
    assert train_or_infer(cfg) == 0
