"""Data-parallel training on the device: the rank-ordered gradient sum fused into AdamW (csrc/lb_train.hip:
k_adamw_gathered behind lb_adamw_step_gathered, lb_gns_train_device_blob) and the Trainer / runner on top of it.

One process: world 1 gives lb_adamw_step's bits for GNS, SEGNN and EGNN handles; three rows are summed in rank order, bit
for bit, and stepped like torch.optim.AdamW; two B = 1 gradients summed by the kernel are the correctly rounded sum, and
their distance to the single-process B = 2 gradient is reported.
Two ranks (fresh child processes, each under its own `timeout -k 10`, sharing the device over gloo as
tests/test_dist_gpu.py's shared-device route does): six Trainer steps end with identical weight bits and loss logs on both
ranks and one checkpoint tree; one noise-free step logs exactly the mean of the two B = 1 losses; `mode: all` of the
runner returns 0 on both ranks."""
import json
import os
import shutil
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ = os.path.join(ROOT, "tests", "golden", "3D_LJ_3_1214every1")
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, weight_decay=1e-2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ handles of the 3 models
def _gns_handle(latent=64):
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case, make_params
    L = 2
    ds = make_case("small3d", n_trajs=2, extra_seq_length=3)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(2)])
    pt = np.stack([ds[b][1] for b in range(2)])
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0, latent_size=latent)
    model = GNS(dim, latent, 2, L, 16)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :isl], pt))
    target = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    make = lambda: model.train_handle(feats.engine, params)
    step = lambda th: model.loss_grad(th, {"acc": target}, {"acc": 1.0})
    return make, step, feats


def _segnn_handle():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps
    from oracle import segnn_oracle as S
    from tests._common import hip_case
    L = 2
    ds = make_case("small2d", n_trajs=2, extra_seq_length=3)
    ds.magnitude_features = True
    isl, dim = ds.input_seq_length, len(ds.box)
    homog = bool(np.all(ds[0][1] == 0))
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=homog,
                  blocks_per_step=2)
    params = S.segnn_init(np.random.default_rng(11), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=L,
                          blocks_per_step=2, random_bias=True)
    params = {k: v for k, v in params.items() if isinstance(v, dict)}
    pos = np.stack([ds[b][0] for b in range(2)])
    pt = np.stack([ds[b][1] for b in range(2)])
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :isl], pt))
    target = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    make = lambda: model.train_handle(feats.engine, params)
    step = lambda th: model.loss_grad(th, {"acc": target}, {"acc": 1.0})
    return make, step, feats


def _egnn_handle():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN
    from tests._common import hip_case
    from tests._egnn_oracle import random_biases
    isl, L = 6, 2
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=3, input_seq_length=isl, scale=0.5)
    pos, pt = ds[0][0][None], ds[0][1][None]
    N, dim = pos.shape[1], len(ds.box)
    model = EGNN(64, 1, 0.01, isl - 1, num_mp_steps=L)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :isl], pt))
    apply_pos = model.apply(params, {}, (feats, pt))[0]["pos"].detach().cpu()
    g = torch.Generator().manual_seed(3)
    r_c = float(ds.metadata["default_connectivity_radius"])
    tg = {"pos": apply_pos + 1e-2 * r_c * torch.randn((1, N, dim), generator=g, dtype=torch.float64),
          "vel": torch.randn((1, N, dim), generator=g, dtype=torch.float64),
          "acc": torch.randn((1, N, dim), generator=g, dtype=torch.float64)}
    lw = {"pos": 1.0, "vel": 0.5, "acc": 0.25}
    make = lambda: model.train_handle(feats.engine, params)
    step = lambda th: model.loss_grad(th, tg, lw)
    return make, step, feats


@pytest.mark.parametrize("kind", ["gns", "segnn", "egnn"])
def test_world_one_gives_the_bits_of_adamw_step(kind):
    """loss_grad, then on one handle adamw_step_gathered(its gradients as ONE row), on a second handle made from the same
    parameters, with the same gradients written, adamw_step: weights and both moments equal bit for bit, one step each."""
    make, step, _keep = {"gns": _gns_handle, "segnn": _segnn_handle, "egnn": _egnn_handle}[kind]()
    a = make()
    a.zero_grad()
    step(a)
    grads = a.read("grads")
    assert np.isfinite(grads).all() and np.abs(grads).max() > 0
    view = a.device_blob("grads")
    assert view.dtype == torch.float32 and view.dim() == 1 and view.numel() == a.device_floats() >= grads.size
    assert view.data_ptr() == a.device_blob("grads").data_ptr()            # a view on the handle's memory, not a copy
    b = make()
    b.write("grads", grads)
    assert np.array_equal(_bits(b.device_blob("grads").cpu().numpy()), _bits(view.cpu().numpy()))
    a.adamw_step_gathered(view.clone().view(1, -1), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["weight_decay"])
    b.adamw_step(ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["weight_decay"])
    for which in ("weights", "m", "v", "grads"):
        assert np.array_equal(_bits(a.read(which)), _bits(b.read(which))), which
        assert np.array_equal(_bits(a.device_blob(which).cpu().numpy()), _bits(b.device_blob(which).cpu().numpy())), which
    assert a.step_count() == 1 and b.step_count() == 1
    # a second step, this time on the gradient blob ITSELF as the one row (the view all_gather_rows returns on one rank)
    a.adamw_step_gathered(a.device_blob("grads").view(1, -1), **{k: ADAM[k] for k in ("lr", "b1", "b2", "eps", "weight_decay")})
    b.adamw_step(ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["weight_decay"])
    for which in ("weights", "m", "v", "grads"):
        assert np.array_equal(_bits(a.read(which)), _bits(b.read(which))), which
    assert a.step_count() == 2 and b.step_count() == 2
    # the padding of the device layout is still exactly zero
    pad = b.device_blob("weights").cpu().numpy().size - b.read("weights").size
    assert int((a.device_blob("weights").cpu().numpy() == 0).sum()) >= pad
    a.close()
    b.close()


def test_gathered_step_refuses_bad_rows():
    make, _, _keep = _gns_handle()
    th = make()
    n = th.device_floats()
    dev = th.engine.device
    with pytest.raises(ValueError):
        th.adamw_step_gathered(torch.zeros((2, n + 1), device=dev), 1e-3)
    with pytest.raises(ValueError):
        th.adamw_step_gathered(torch.zeros((17, n), device=dev), 1e-3)
    with pytest.raises(ValueError):
        th.adamw_step_gathered(torch.zeros((2, n), dtype=torch.float64, device=dev), 1e-3)
    with pytest.raises(ValueError):
        th.adamw_step_gathered(torch.zeros((2, n)), 1e-3)                    # host memory
    rc = th.engine.lib.lb_adamw_step_gathered(th._h, th.device_blob("grads").data_ptr(), 0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert rc == -1 and b"world" in th.engine.lib.lb_last_error()
    rc = th.engine.lib.lb_adamw_step_gathered(th._h, th.device_blob("grads").data_ptr(), 17, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert rc == -1
    assert th.step_count() == 0
    th.close()


@pytest.mark.parametrize("latent", [64, 128])
def test_three_rows_are_summed_in_rank_order(latent):
    """Three rows of fp32 data spanning six decades, in the device layout: the gradient blob after the call is numpy's
    ((r0 + r1) + r2) in float32 bit for bit - which for this seed is neither r0 + (r1 + r2) nor ((r2 + r1) + r0) - and the
    weights follow torch.optim.AdamW fed that sum within 2e-6 * max(|ref|, 1) + 1e-7 (tests/test_egnn_train.py's bound)."""
    # latent 64: the device layout is padded, the rows respect the padding; latent 128: no padding, and a length that is
    # not a multiple of four floats, so rows 1 and 2 start off the 16-byte grid and the last parameters go one by one
    make, _, _keep = _gns_handle(latent=latent)
    th = make()
    n, dev = th.device_floats(), th.engine.device
    th.write("grads", np.ones(th.read("grads").size, np.float32))
    real = th.device_blob("grads").cpu().numpy() != 0                      # the entries of the layout that are parameters
    assert real.sum() == th.read("grads").size and (real.sum() < n if latent == 64 else n % 4 != 0), (n, real.sum())
    rng = np.random.default_rng(2024)
    rows = (rng.standard_normal((3, n)) * 10.0 ** rng.uniform(-3, 3, size=(3, n))).astype(np.float32) * real
    r0, r1, r2 = rows
    want = (r0 + r1) + r2
    assert want.dtype == np.float32
    other = r0 + (r1 + r2)
    rev = (r2 + r1) + r0
    n_assoc, n_rev = int((_bits(want) != _bits(other)).sum()), int((_bits(want) != _bits(rev)).sum())
    print(f"[ddp order] {real.sum()} parameters in {n} floats: (a+b)+c != a+(b+c) in {n_assoc}, != (c+b)+a in {n_rev}")
    assert n_assoc > 1000 and n_rev > 1000
    w0 = th.device_blob("weights").cpu().numpy().copy()
    th.adamw_step_gathered(torch.from_numpy(rows).to(dev), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["weight_decay"])
    got = th.device_blob("grads").cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(rev)) and not np.array_equal(_bits(got), _bits(other))
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    p.grad = torch.from_numpy(want).double()
    torch.optim.AdamW([p], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"], weight_decay=ADAM["weight_decay"]).step()
    ref = p.detach().numpy()
    w1 = th.device_blob("weights").cpu().numpy()
    err = np.abs(w1 - ref)
    print(f"[ddp order] largest weight deviation from torch.optim.AdamW {err.max():.3e}")
    assert (err <= 2e-6 * np.maximum(np.abs(ref), 1.0) + 1e-7).all()
    assert (w1[~real] == 0).all() and th.step_count() == 1                  # the padding stays exactly zero
    # grad_scale multiplies the ordered sum
    th.adamw_step_gathered(torch.from_numpy(rows).to(dev), ADAM["lr"], grad_scale=0.5)
    assert np.array_equal(_bits(th.device_blob("grads").cpu().numpy()), _bits(want * np.float32(0.5)))
    th.close()


def test_two_shards_sum_to_the_global_batch_gradient():
    """g0, g1 from two B = 1 engines on the two trajectories of rpf2d, gathered and summed by the kernel: the correctly
    rounded fp32 sum, exactly.  Its distance to the single-process B = 2 gradient (the previous result, which sums the same
    terms in another order) is reported next to that gradient's own distance to the fp64 sum."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from tests._common import hip_case, make_params
    L = 2
    ds = make_case("rpf2d", n_trajs=2, extra_seq_length=3, scale=0.5)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos = np.stack([ds[b][0] for b in range(2)])
    pt = np.stack([ds[b][1] for b in range(2)])
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(dim, 128, 2, L, 16)
    target = torch.randn((2, pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    shards, keep, compact = [], [], []
    for b in range(2):
        case = hip_case(ds)                                                 # an engine of its own per shard
        feats, _ = case.allocate_eval((pos[b:b + 1, :, :isl], pt[b:b + 1]))
        th = model.train_handle(feats.engine, params)
        th.zero_grad()
        th.loss_grad(target[b:b + 1], 1.0)
        shards.append(th)
        compact.append(th.read("grads"))
        keep.append((case, feats))
    assert shards[0].engine is not shards[1].engine
    g0, g1 = (th.device_blob("grads").cpu().numpy().copy() for th in shards)
    assert np.abs(g0).max() > 0 and np.abs(g1).max() > 0 and not np.array_equal(g0, g1)
    gathered = torch.stack([th.device_blob("grads") for th in shards])
    shards[0].adamw_step_gathered(gathered, 1e-3)
    got = shards[0].device_blob("grads").cpu().numpy()
    exact = g0.astype(np.float64) + g1.astype(np.float64)
    assert np.array_equal(_bits(got), _bits(exact.astype(np.float32)))      # a two-term fp32 add is correctly rounded
    summed = shards[0].read("grads")
    sum64 = compact[0].astype(np.float64) + compact[1].astype(np.float64)
    assert np.array_equal(_bits(summed), _bits(sum64.astype(np.float32)))   # the same through read()
    case2 = hip_case(ds)
    feats2, _ = case2.allocate_eval((pos[:, :, :isl], pt))
    th2 = model.train_handle(feats2.engine, params)
    th2.zero_grad()
    th2.loss_grad(target, 1.0)
    g2 = th2.read("grads")
    scale = np.abs(g2).max()
    d_kernel = np.abs(summed.astype(np.float64) - g2.astype(np.float64)).max() / scale
    d_b2 = np.abs(g2.astype(np.float64) - sum64).max() / scale
    print(f"[ddp global batch] rpf2d x 2, GNS-{L}-128: kernel sum of two B = 1 gradients vs the B = 2 gradient "
          f"{d_kernel:.3e} of the largest entry; the B = 2 gradient vs the fp64 sum of the two {d_b2:.3e}")
    for th in shards + [th2]:
        th.close()


def test_world_one_trainer_is_unchanged_by_the_environment(tmp_path, monkeypatch):
    """WORLD_SIZE unset and WORLD_SIZE=1 take the same (previous) code path: equal loss logs and weights."""
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.train import Trainer
    ds_dir = _lj_copy(tmp_path)
    md = json.load(open(os.path.join(ds_dir, "metadata.json")))
    isl = 6
    logs, weights = [], []
    for world in (None, "1"):
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            monkeypatch.delenv(k, raising=False)
        if world:
            monkeypatch.setenv("WORLD_SIZE", world)
            monkeypatch.setenv("RANK", "0")
            monkeypatch.setenv("LOCAL_RANK", "0")
        data_train = H5Dataset("train", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=1)
        data_valid = H5Dataset("valid", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=10)
        bounds = np.array(md["bounds"])
        case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=3e-4)
        model = GNS(3, 128, 2, 2, 16)
        cfg_train = {"batch_size": 2, "noise_std": 3e-4,
                     "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200},
                     "pushforward": {"steps": [-1, 3], "unrolls": [0, 1], "probs": [1, 1]}}
        trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                          cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                          cfg_logging={"log_steps": 1, "eval_steps": 4}, input_seq_length=isl, seed=0)
        assert trainer.world == 1 and trainer.shard == slice(0, 2)
        params, _, opt = trainer.train(step_max=7)
        logs.append(trainer.loss_log)
        weights.append(model.flatten(params))
        assert opt["count"] == 8
    assert len(logs[0]) == 8 and logs[0] == logs[1] and np.isfinite([l for _, l in logs[0]]).all()
    assert np.array_equal(_bits(weights[0]), _bits(weights[1]))


# ------------------------------------------------------------------------------------------------ two ranks
WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["LB_ROOT"])
import numpy as np, torch
from lagrangebench_amd import dist as lbdist
from lagrangebench_amd.case_setup import case_builder
from lagrangebench_amd.data import H5Dataset
from lagrangebench_amd.models import GNS
from lagrangebench_amd.train import Trainer
from lagrangebench_amd.train.trainer import _ShuffledLoader

mode, out, ds_dir = sys.argv[1], os.environ["LB_OUT"], os.environ["LB_DATA"]
rank, local_rank, world = lbdist.env_world()
assert world == 2
torch.cuda.set_device(lbdist.local_device(local_rank))
isl, seed = 6, 0
md = json.load(open(os.path.join(ds_dir, "metadata.json")))
bounds = np.array(md["bounds"])


def setup(noise_std):
    data_train = H5Dataset("train", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=1)
    data_valid = H5Dataset("valid", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=10)
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=noise_std)
    return data_train, data_valid, case, GNS(3, 64, 2, 2, 16)


opt_cfg = {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}
if mode == "six":
    data_train, data_valid, case, model = setup(3e-4)
    cfg_train = {"batch_size": 2, "noise_std": 3e-4, "optimizer": opt_cfg,
                 "pushforward": {"steps": [-1, 2], "unrolls": [0, 1], "probs": [1, 1]}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 4}, input_seq_length=isl, seed=seed)
    assert trainer.world == 2 and trainer.shard == slice(rank, rank + 1)
    params, _, opt = trainer.train(step_max=5, store_ckp=os.path.join(out, "ckp"))
    assert torch.distributed.is_initialized() and torch.distributed.get_backend() == "gloo"
    np.save(os.path.join(out, f"weights_{rank}.npy"), model.flatten(params))
    np.save(os.path.join(out, f"m_{rank}.npy"), np.asarray(opt["m"]))
    json.dump({"loss_log": trainer.loss_log, "count": int(opt["count"]), "step": int(opt["step"])},
              open(os.path.join(out, f"log_{rank}.json"), "w"))
elif mode == "one":
    data_train, data_valid, case, model = setup(0.0)
    off = {"steps": [-1], "unrolls": [0], "probs": [1]}
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "optimizer": opt_cfg, "pushforward": off}
    kw = dict(cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
              cfg_logging={"log_steps": 1, "eval_steps": 100}, input_seq_length=isl, seed=seed)
    # the batch of step 0: train() draws one permutation for the sample it sizes the lists on, then one per epoch
    gen = torch.Generator()
    gen.manual_seed(seed)
    loader = _ShuffledLoader(data_train, 2, gen)
    first = next(iter(loader))
    batch = next(iter(loader))
    _, feats0, _, nbrs = case.allocate(None, (first[0][0], first[1][0]))
    params0, _ = model.init(np.array([7]), (feats0, first[1][0]))
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train, **kw)
    trainer.train(step_max=0, params=params0)
    assert len(trainer.loss_log) == 1 and trainer.loss_log[0][0] == 0
    logged = trainer.loss_log[0][1]
    # the two B = 1 losses, in this process, the way a rank computes its own
    losses = []
    for b in range(2):
        _, _, _, nbrs = case.allocate(None, (first[0][b], first[1][b]))   # rank b sizes its list on its own first sample
        _, feats, target, nb = case.preprocess(None, (batch[0][b:b + 1], batch[1][b:b + 1]), 0.0, nbrs, 0)
        assert not bool(nb.did_buffer_overflow.sum() > 0)
        th = model.train_handle(case.engine(1), params0)
        th.zero_grad()
        losses.append(model.loss_grad(th, target, trainer.loss_weight))
        th.close()
    mean = (losses[0] + losses[1]) / 2
    _, feats, target, nb2 = case.allocate(None, (batch[0], batch[1]))
    th = model.train_handle(case.engine(2), params0)
    th.zero_grad()
    loss2 = model.loss_grad(th, target, trainer.loss_weight)
    th.close()
    json.dump({"logged": logged, "losses": losses, "mean": mean, "loss_b2": loss2},
              open(os.path.join(out, f"one_{rank}.json"), "w"))
    assert np.isfinite(logged) and abs(logged - mean) <= 1e-12 * abs(mean), (logged, losses)
elif mode == "all":
    from lagrangebench_amd.runner import train_or_infer
    cfg = {"mode": "all", "dataset": {"src": ds_dir, "name": "lj3d"},
           "model": {"name": "gns", "num_mp_steps": 1, "input_seq_length": isl, "latent_dim": 64},
           "train": {"step_max": 6, "batch_size": 2, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]}},
           "logging": {"log_steps": 2, "eval_steps": 3, "ckp_dir": os.path.join(out, "ckp_all"), "run_name": None},
           "eval": {"n_rollout_steps": 5, "train": {"n_trajs": 2, "metrics": ["mse"]},
                    "infer": {"n_trajs": 2, "batch_size": 1, "metrics": ["mse"], "out_type": "none"}}}
    rc = train_or_infer(cfg)
    json.dump({"rc": rc}, open(os.path.join(out, f"all_{rank}.json"), "w"))
    assert rc == 0
if torch.distributed.is_initialized():
    torch.distributed.destroy_process_group()
print("DDP_WORKER_OK", mode, rank)
'''


def _lj_copy(tmp_path):
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    if not ds_dir.exists():
        shutil.copytree(LJ, ds_dir)
        md = json.load(open(ds_dir / "metadata.json"))
        md.setdefault("write_every", 1)
        json.dump(md, open(ds_dir / "metadata.json", "w"))
    return str(ds_dir)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_two_ranks(tmp_path, mode, limit=420):
    """Two fresh children, rank 0 and 1, each under its own `timeout -k 10`; both share the visible device(s) round-robin
    and talk over gloo.  Stops at the first non-zero status (the other child is ended) and fails with that child's output."""
    script = tmp_path / "ddp_worker.py"
    script.write_text(WORKER)
    out = tmp_path / f"out_{mode}"
    out.mkdir()
    port = str(_free_port())
    procs, logs = [], []
    for rank in range(2):
        env = dict(os.environ, LB_ROOT=ROOT, LB_OUT=str(out), LB_DATA=_lj_copy(tmp_path), LB_DIST_BACKEND="gloo",
                   RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, OMP_NUM_THREADS="1")
        log = open(tmp_path / f"{mode}_rank{rank}.log", "w")
        logs.append(log)
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, str(script), mode], env=env,
                                      stdout=log, stderr=subprocess.STDOUT, cwd=str(tmp_path)))
    status = [None, None]
    try:
        while any(s is None for s in status):
            for r, p in enumerate(procs):
                if status[r] is None:
                    status[r] = p.poll()
            if any(s not in (None, 0) for s in status):
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
        for log in logs:
            log.close()
    texts = [open(tmp_path / f"{mode}_rank{r}.log").read() for r in range(2)]
    for r in range(2):
        assert status[r] == 0, f"rank {r} ended with {status[r]} (mode {mode}):\n{texts[r][-6000:]}"
        assert f"DDP_WORKER_OK {mode} {r}" in texts[r]
    return out, texts


def test_two_ranks_six_trainer_steps_end_with_identical_weights(tmp_path):
    out, texts = _run_two_ranks(tmp_path, "six")
    w = [np.load(out / f"weights_{r}.npy") for r in range(2)]
    m = [np.load(out / f"m_{r}.npy") for r in range(2)]
    logs = [json.load(open(out / f"log_{r}.json")) for r in range(2)]
    assert w[0].size > 0 and np.isfinite(w[0]).all()
    assert np.array_equal(_bits(w[0]), _bits(w[1])) and np.array_equal(_bits(m[0]), _bits(m[1]))
    assert logs[0]["loss_log"] == logs[1]["loss_log"] and len(logs[0]["loss_log"]) == 6
    assert np.isfinite([l for _, l in logs[0]["loss_log"]]).all()
    assert [s for s, _ in logs[0]["loss_log"]] == list(range(6))
    # steps 0 .. 5 ran (a skipped step is repeated, not counted): six AdamW steps on every rank
    assert logs[0]["count"] == logs[1]["count"] == 6 and logs[0]["step"] == 6
    # one checkpoint tree, written by rank 0 at the one evaluation (step 4)
    assert sorted(os.listdir(out)) == ["ckp", "log_0.json", "log_1.json", "m_0.npy", "m_1.npy", "weights_0.npy", "weights_1.npy"]
    from lagrangebench_amd.utils import load_haiku
    _, _, opt, step = load_haiku(str(out / "ckp"))
    assert step == 4 and opt["count"] == 5 and os.path.exists(out / "ckp" / "best" / "params_array.npy")
    assert "train/loss" in texts[0] and "train/loss" not in texts[1]          # rank 0 alone prints


def test_two_ranks_one_step_logs_the_mean_of_the_two_shard_losses(tmp_path):
    out, _ = _run_two_ranks(tmp_path, "one")
    res = [json.load(open(out / f"one_{r}.json")) for r in range(2)]
    assert res[0] == res[1]
    r = res[0]
    assert np.isfinite(r["logged"]) and abs(r["logged"] - r["mean"]) <= 1e-12 * abs(r["mean"]), r
    print(f"[ddp loss] logged {r['logged']!r} = mean of {r['losses']!r}; the single-process B = 2 loss {r['loss_b2']!r} "
          f"differs by {abs(r['loss_b2'] - r['mean']) / abs(r['mean']):.3e} relative")


def test_two_ranks_runner_mode_all_returns_zero(tmp_path):
    out, _ = _run_two_ranks(tmp_path, "all")
    assert [json.load(open(out / f"all_{r}.json"))["rc"] for r in range(2)] == [0, 0]
    runs = os.listdir(out / "ckp_all")
    assert len(runs) == 1 and os.path.exists(out / "ckp_all" / runs[0] / "best" / "params_array.npy")   # ONE tree
