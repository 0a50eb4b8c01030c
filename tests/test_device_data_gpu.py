"""Device-resident training input on the device: lb_train_batch (csrc/lb_train_input.hip) behind case.preprocess_device /
allocate_device, against the host route (H5Dataset window -> add_gns_noise on the CPU -> prepare_traj -> _compute_target),
and the Trainer / runner / two-rank run with train.device_data on.

Without noise the two routes must agree bit for bit (window, edge list, targets, loss, gradient blob).  With noise the
device's draws are those of the numpy restatement in tests/test_device_data.py, and the trajectory and targets are those a
host rebuilds in fp64 from these draws with the oracle's shift."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_device_data import normals_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ = os.path.join(ROOT, "tests", "golden", "3D_LJ_3_1214every1")
ISL = 6


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


class _Setup:
    """A dataset, its host samples and its DeviceDataset; cases per dtype."""

    def __init__(self, name):
        from lagrangebench_amd.case_setup import case_builder
        from lagrangebench_amd.data import DeviceDataset, H5Dataset, make_case, make_padded_case
        from tests._common import hip_case
        self.name = name
        if name == "lj":
            self.ds = H5Dataset("train", LJ, name="lj3d", input_seq_length=ISL, extra_seq_length=2)
            md = self.ds.metadata
            b = np.array(md["bounds"])
            self.box = b[:, 1] - b[:, 0]
            self.case = lambda dtype: case_builder(self.box, md, ISL, noise_std=3e-4, dtype=dtype)
            self.idx = [3, len(self.ds) - 1, len(self.ds) // 2]
        else:
            if name == "rpf2d":
                self.ds = make_case("rpf2d", n_trajs=3, extra_seq_length=3, input_seq_length=ISL, scale=0.5)
            elif name == "ldc3d":
                self.ds = make_case("ldc3d", n_trajs=3, extra_seq_length=3, input_seq_length=ISL, scale=0.5)
            else:
                self.ds = make_padded_case("waterdrop2d", [500, 625, 431], extra_seq_length=3, input_seq_length=ISL)
            self.box = self.ds.box
            self.case = lambda dtype: hip_case(self.ds, dtype=dtype)
            self.idx = [2, 0, 1]
        self.periodic = bool(np.any(self.ds.metadata["periodic_boundary_conditions"]))
        self.dim = len(self.box)
        self.dd = DeviceDataset(self.ds)
        self.T = self.dd.subseq_length

    def host_sample(self, idx):
        items = [self.ds[i] for i in idx]
        return np.stack([it[0] for it in items]), np.stack([it[1] for it in items])

    def gns(self):
        from lagrangebench_amd.models import GNS
        return GNS(self.dim, 64, 2, 2, 16)


_SETUPS = {}


def _setup(name):
    if name not in _SETUPS:
        _SETUPS[name] = _Setup(name)
    return _SETUPS[name]


CASES = ["rpf2d", "ldc3d", "lj", "padded"]


# ------------------------------------------------------------------------------------------------ 1. no noise: bit for bit
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_without_noise_the_routes_agree_bit_for_bit(name, dtype):
    s = _setup(name)
    case = s.case(dtype)
    model = s.gns()
    n_checked = 0
    for B in (1, 3):
        idx = s.idx[:B]
        pos, pt = s.host_sample(idx)
        if name == "ldc3d":
            assert set(np.unique(pt)) == {0, 1, 2}
        _, feats0, _, _ = case.allocate(None, (pos[0], pt[0]))
        params, _ = model.init(np.array([3]), (feats0, pt[0]))
        case.allocate(None, (pos, pt), 0.0, 0)
        th = model.train_handle(case.engine(B), params)
        for unroll in (0, 2):
            _, feats, tgt_h, nb_h = case.allocate(None, (pos, pt), 0.0, unroll)
            eng = case.engine(B)
            win_h, idx_h, ne_h, pads_h = eng.read_window(), nb_h.idx.clone(), nb_h.n_edges.clone(), eng.has_pads
            th.zero_grad()
            loss_h = model.loss_grad(th, tgt_h, {"acc": 1.0})
            grad_h = th.device_blob("grads").clone()
            feats_d, tgt_d, nb_d = case.allocate_device(s.dd, idx, list(range(B)), 11, 5, 0.0, unroll)
            assert eng.has_pads == pads_h
            assert np.array_equal(_bits(eng.read_window()), _bits(win_h))
            assert np.array_equal(_bits(feats_d["abs_pos"]), _bits(feats["abs_pos"]))
            assert np.array_equal(nb_d.idx.cpu().numpy(), idx_h.cpu().numpy())
            assert np.array_equal(nb_d.n_edges.cpu().numpy(), ne_h.cpu().numpy())
            assert (nb_d.max_occupancy, nb_d.cell_capacity) == (nb_h.max_occupancy, nb_h.cell_capacity)
            for k in ("acc", "vel", "pos"):
                assert tgt_d[k].dtype == tgt_h[k].dtype and tgt_d[k].shape == tgt_h[k].shape, k
                assert np.array_equal(_bits(tgt_d[k]), _bits(tgt_h[k])), (name, dtype, B, unroll, k)
            th.zero_grad()
            loss_d = model.loss_grad(th, tgt_d, {"acc": 1.0})
            assert np.isfinite(loss_h) and loss_d == loss_h
            assert np.array_equal(_bits(th.device_blob("grads")), _bits(grad_h))
            assert float(grad_h.abs().max()) > 0
            # preprocess_device on the list just sized: the same edges again
            _, tgt_p, nb_p = case.preprocess_device(s.dd, idx, list(range(B)), 11, 5, 0.0, nb_d, unroll)
            assert np.array_equal(nb_p.idx.cpu().numpy(), idx_h.cpu().numpy())
            assert np.array_equal(_bits(tgt_p["acc"]), _bits(tgt_h["acc"]))
            n_checked += 1
        th.close()
    assert n_checked == 4
    # an un-batched sample (an int) gives un-batched results, as allocate does
    feats1, tgt1, nb1 = case.allocate_device(s.dd, s.idx[0], [0], 0, 0, 0.0)
    assert tgt1["acc"].dim() == 2 and nb1.idx.dim() == 2 and feats1["abs_pos"].dim() == 3


# ------------------------------------------------------------------------------------------------ 2. noise
def _rebuild(s, dtype, idx, normals, noise_std):
    """strats.py:12-83 on the host in fp64 from the device's draws, with the oracle's shift."""
    from lagrangebench_amd.utils import get_kinematic_mask
    from oracle import lb_oracle as O
    pos, pt = s.host_sample(idx)
    raw = pos.astype(np.float32).astype(np.float64) if dtype == "float32" else pos.astype(np.float64)
    K = ISL - 1
    vel = np.cumsum(normals * (noise_std / K ** 0.5), axis=2)
    walk = np.concatenate([np.zeros_like(vel[:, :, :1]), np.cumsum(vel, axis=2)], axis=2)          # (B, N, isl, dim)
    walk = np.where(get_kinematic_mask(pt)[:, :, None, None], 0.0, walk)
    noise = np.concatenate([walk, np.repeat(walk[:, :, -1:], s.T - ISL, axis=2)], axis=2)
    shift = O.space_periodic(np.asarray(s.box, np.float64))[1] if s.periodic else O.space_free()[1]
    out = shift(raw, noise)
    return raw, pt, noise, (out.astype(np.float32).astype(np.float64) if dtype == "float32" else out)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_noise_is_the_restated_random_walk(name, dtype):
    from lagrangebench_amd.utils import get_kinematic_mask
    s = _setup(name)
    case = s.case(dtype)
    noise_std, seed, step, B, unroll = 3e-4, 0x0123456789ABCDEF, 41, 3, 2
    idx, slots = s.idx[:B], [4, 0, 9]
    feats, tgt, nbrs, (traj, normals) = case.allocate_device(s.dd, idx, slots, seed, step, noise_std, unroll, want_normals=True)
    N, K, L = s.dd.N, ISL - 1, float(np.max(s.box))
    trajs, t0s = s.dd.locate_batch(idx)
    types_dev = case.engine(B).train_batch(s.dd, trajs, t0s, slots, seed, step, noise_std, unroll)[1]
    assert np.array_equal(types_dev.cpu().numpy(), s.host_sample(idx)[1])
    normals, dev = normals.cpu().numpy(), traj.cpu().numpy()
    assert dev.shape == (B, N, s.T, s.dim) and normals.shape == (B, N, K, s.dim)
    want = np.stack([normals_for(seed, step, slots[b], N, K, s.dim) for b in range(B)])
    err_n = np.abs(normals - want).max()
    raw, pt, noise, ref = _rebuild(s, dtype, idx, normals, noise_std)
    err_t = np.abs(dev - ref).max()
    kin = np.asarray(get_kinematic_mask(pt))
    print(f"[device data] {name} {dtype}: draws vs numpy {err_n:.3e}; trajectory vs the fp64 rebuild {err_t:.3e} "
          f"(box {L:.4g}); {int(kin.sum())} kinematic of {kin.size}")
    assert err_n <= 1e-12
    # the fp64 rebuild; a float32 case stores the rounded value: one fp32 spacing of the box where the rounding flips
    assert err_t <= (1e-13 * L if dtype == "float64" else float(np.spacing(np.float32(L))))
    # frame 0, kinematic and pad particles carry no noise: the rebuilt values exactly (shift(r, 0)), the data where in the box
    assert np.array_equal(_bits(dev[:, :, 0]), _bits(ref[:, :, 0]))
    assert np.array_equal(_bits(dev[kin]), _bits(ref[kin]))
    inside = (raw >= 0) & (raw < np.asarray(s.box)) if s.periodic else np.ones(raw.shape, bool)
    assert np.array_equal(dev[:, :, 0][inside[:, :, 0]], raw[:, :, 0][inside[:, :, 0]])
    assert np.array_equal(dev[kin][inside[kin]], raw[kin][inside[kin]])
    if name == "padded":
        pad = pt == -1
        assert pad.any() and (dev[pad] == 0).all()
        e = nbrs.idx.cpu().numpy()
        for b in range(B):
            n_real = s.ds.n_real[idx[b]]
            real_edges = e[b][:, : int(nbrs.n_edges[b])]
            assert real_edges.size and real_edges.max() < n_real             # the pads are the trailing rows: in no edge
    # what the device added, minimum-imaged: frames past the window carry the last input frame's noise; its spread
    box = np.asarray(s.box, np.float64)
    added = dev - raw
    if s.periodic:
        added = added - box * np.round(added / box)
    tol = 1e-13 * L if dtype == "float64" else 2 * float(np.spacing(np.float32(L)))
    for f in range(ISL, s.T):
        assert np.abs(added[:, :, f] - added[:, :, ISL - 1]).max() <= tol
    assert np.abs(added - noise).max() <= tol
    last = added[:, :, ISL - 1][~kin]
    assert last.size >= 1500 * s.dim or name == "lj"
    if last.size >= 1500 * s.dim:
        # strats.py:61-83 scales the draws so that the last step of the VELOCITY walk has standard deviation noise_std
        # ("noise_std_last_step"); the position noise is the running sum of that walk, so on the last input frame its
        # standard deviation is noise_std * sqrt(sum_{j=1..K} j^2 / K) (3.32 noise_std at K = 5), not noise_std.  Both are
        # held to 3 % (estimator sigma < 1.3 % at >= 1500 particles x dim).
        last_vel = (added[:, :, ISL - 1] - added[:, :, ISL - 2])[~kin]
        walk_std = noise_std * (sum(j * j for j in range(1, K + 1)) / K) ** 0.5
        print(f"[device data] {name} {dtype}: last velocity step std {last_vel.std():.4e} (noise_std {noise_std:.1e}), "
              f"last frame position std {last.std():.4e} (expected {walk_std:.4e})")
        assert abs(last_vel.std() / noise_std - 1.0) < 0.03, last_vel.std()
        assert abs(last.std() / walk_std - 1.0) < 0.03, last.std()
    # targets: _compute_target of the rebuilt trajectory
    b0 = ISL - 2 + unroll
    want_t = case._compute_target(torch.from_numpy(ref[:, :, b0:b0 + 3]).to(traj.device), True)
    stats = case.normalization_stats
    for k, scale in (("acc", 1.0 / np.min(stats["acceleration"]["std"])), ("vel", 1.0 / np.min(stats["velocity"]["std"])),
                     ("pos", 1.0)):
        got, ref_t = tgt[k].cpu().numpy().astype(np.float64), want_t[k].cpu().numpy().astype(np.float64)
        assert tgt[k].dtype == want_t[k].dtype
        err = np.abs(got - ref_t)
        if dtype == "float64":
            assert err.max() <= 1e-13 * L * scale, (k, err.max())
        else:
            assert (err <= 2 * np.spacing(np.abs(ref_t).astype(np.float32)).astype(np.float64)).all(), (k, err.max())


# ------------------------------------------------------------------------------------------------ 3. keying
def test_draws_depend_on_seed_step_and_global_slot_only():
    s = _setup("rpf2d")
    case = s.case("float64")
    idx = s.idx
    run = lambda ix, slots, seed=7, step=3: case.allocate_device(s.dd, ix, slots, seed, step, 3e-4, 0, want_normals=True)[3]
    t3, n3 = run(idx, [0, 1, 2])
    t3b, n3b = run(idx, [0, 1, 2])
    assert np.array_equal(_bits(t3), _bits(t3b)) and np.array_equal(_bits(n3), _bits(n3b))
    t1, n1 = run(idx[1:2], [1])                                  # slot 1 alone, B = 1: another engine, place 0 of the batch
    assert np.array_equal(_bits(t1[0]), _bits(t3[1])) and np.array_equal(_bits(n1[0]), _bits(n3[1]))
    for other in (run(idx, [0, 1, 2], step=4), run(idx, [0, 1, 2], seed=8), run(idx, [0, 1, 2], seed=7 + (1 << 32)),
                  run(idx, [0, 5, 2])):
        assert not np.array_equal(_bits(other[1][1]), _bits(n3[1]))
    moved = run(idx, [0, 5, 2])[1]
    assert np.array_equal(_bits(moved[0]), _bits(n3[0])) and np.array_equal(_bits(moved[2]), _bits(n3[2]))


def test_entry_point_refuses_bad_samples():
    from lagrangebench_amd._lib import LbHipError
    s = _setup("rpf2d")
    eng = s.case("float64").engine(1)
    with pytest.raises(LbHipError, match="outside"):
        eng.train_batch(s.dd, [s.dd.n_traj], [0], [0], 0, 0, 0.0)
    with pytest.raises(LbHipError, match="outside"):
        eng.train_batch(s.dd, [0], [1], [0], 0, 0, 0.0)
    with pytest.raises(LbHipError, match="unroll_steps"):
        eng.train_batch(s.dd, [0], [0], [0], 0, 0, 0.0, unroll_steps=3)
    with pytest.raises(ValueError):
        eng.train_batch(s.dd, [0, 1], [0, 0], [0, 1], 0, 0, 0.0)


# ------------------------------------------------------------------------------------------------ 4. padded batch + loss
def test_padded_batch_loss_counts_the_real_particles():
    """A batch mixing 500, 625 and 431 real particles among 625 rows: without noise the device route's loss (denominator:
    the non-kinematic real particles of each trajectory) and gradients are the host route's, bit for bit; with noise the
    pads stay at 0 with type -1 and the loss stays finite."""
    s = _setup("padded")
    case, model, B = s.case("float64"), s.gns(), 3
    pos, pt = s.host_sample(s.idx)
    _, feats0, _, _ = case.allocate(None, (pos[0], pt[0]))
    params, _ = model.init(np.array([3]), (feats0, pt[0]))
    _, feats, tgt_h, _ = case.allocate(None, (pos, pt), 0.0, 0)
    assert case.engine(B).has_pads
    th = model.train_handle(case.engine(B), params)
    th.zero_grad()
    loss_h = model.loss_grad(th, tgt_h, {"acc": 1.0})
    grad_h = th.device_blob("grads").clone()
    _, tgt_d, nb = case.allocate_device(s.dd, s.idx, [0, 1, 2], 1, 0, 0.0)
    assert case.engine(B).has_pads
    th.zero_grad()
    assert model.loss_grad(th, tgt_d, {"acc": 1.0}) == loss_h
    assert np.array_equal(_bits(th.device_blob("grads")), _bits(grad_h))
    _, tgt_n, nb = case.preprocess_device(s.dd, s.idx, [0, 1, 2], 1, 0, 3e-4, nb)
    win = case.engine(B).read_window().cpu().numpy()
    assert (win[pt == -1] == 0).all() and not (win[pt != -1] == 0).all()
    th.zero_grad()
    loss_n = model.loss_grad(th, tgt_n, {"acc": 1.0})
    assert np.isfinite(loss_n) and loss_n != loss_h
    th.close()


# ------------------------------------------------------------------------------------------------ 5. Trainer / runner
def _lj_copy(tmp_path):
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    if not ds_dir.exists():
        shutil.copytree(LJ, ds_dir)
        md = json.load(open(ds_dir / "metadata.json"))
        md.setdefault("write_every", 1)
        json.dump(md, open(ds_dir / "metadata.json", "w"))
    return str(ds_dir)


def _lj_trainer(ds_dir, kind, device_data, noise_std, log_steps, eval_steps, seed=0, pushforward=None):
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import EGNN, GNS
    from lagrangebench_amd.train import Trainer
    md = json.load(open(os.path.join(ds_dir, "metadata.json")))
    data_train = H5Dataset("train", ds_dir, name="lj3d", input_seq_length=ISL, extra_seq_length=1)
    data_valid = H5Dataset("valid", ds_dir, name="lj3d", input_seq_length=ISL, extra_seq_length=10)
    bounds = np.array(md["bounds"])
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, ISL, noise_std=noise_std)
    cfg_train = {"batch_size": 2, "noise_std": noise_std, "device_data": device_data,
                 "pushforward": pushforward or {"steps": [-1, 20], "unrolls": [0, 1], "probs": [1, 1]}}
    if kind == "egnn":   # the settings of tests/test_egnn_train.py
        model = EGNN(64, 1, md["dt"] * md["write_every"], ISL - 1, normalization_stats=case.normalization_stats, num_mp_steps=2)
        cfg_train.update(loss_weight={"pos": 1.0, "vel": 0.0, "acc": 0.0},
                         optimizer={"lr_start": 5e-4, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 500})
    else:
        model = GNS(3, 64, 2, 2, 16)
        cfg_train.update(optimizer={"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200})
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": log_steps, "eval_steps": eval_steps}, input_seq_length=ISL, seed=seed)
    return trainer, model


@pytest.mark.parametrize("kind", ["gns", "egnn"])
def test_trainer_trains_from_the_device_dataset(tmp_path, kind):
    from lagrangebench_amd.utils import load_haiku
    ds_dir = _lj_copy(tmp_path)
    trainer, model = _lj_trainer(ds_dir, kind, True, 3e-4, 5, 30)
    assert trainer.device_data
    ckp = str(tmp_path / "ckp")
    params, _, opt = trainer.train(step_max=30, store_ckp=ckp)
    assert trainer._dd is not None and trainer._dd.pos.is_cuda and trainer._dd.num_samples == len(trainer.loader_train.dataset)
    losses = [l for _, l in trainer.loss_log]
    print(f"[device data] {kind} losses {losses}")
    assert np.isfinite(losses).all() and np.mean(losses[-4:]) < 0.8 * np.mean(losses[:3]), losses
    _, _, opt_loaded, step = load_haiku(ckp)
    assert step == 30 and set(opt_loaded) >= {"m", "v", "step", "count"} and np.abs(opt_loaded["v"]).max() > 0
    trainer2, _ = _lj_trainer(ds_dir, kind, True, 3e-4, 1, 1000, seed=1)
    p2, _, opt2 = trainer2.train(step_max=step + 3, load_ckp=ckp)
    assert set(p2) == set(params)
    assert opt2["count"] >= opt_loaded["count"] + 1 and trainer2.loss_log[0][0] == step


def test_without_noise_the_trainer_logs_are_the_host_routes(tmp_path):
    ds_dir = _lj_copy(tmp_path)
    logs, weights = [], []
    for device_data in (False, True):
        trainer, model = _lj_trainer(ds_dir, "gns", device_data, 0.0, 1, 4,
                                     pushforward={"steps": [-1, 3], "unrolls": [0, 1], "probs": [1, 1]})
        params, _, opt = trainer.train(step_max=7)
        logs.append(trainer.loss_log)
        weights.append(model.flatten(params))
        assert opt["count"] == 8
    assert len(logs[0]) == 8 and logs[0] == logs[1], logs
    assert np.array_equal(_bits(weights[0]), _bits(weights[1]))


def test_runner_mode_all_with_device_data(tmp_path):
    from lagrangebench_amd.runner import train_or_infer
    ds_dir = _lj_copy(tmp_path)
    cfg = {"mode": "all", "dataset": {"src": ds_dir, "name": "lj3d"},
           "model": {"name": "gns", "num_mp_steps": 1, "input_seq_length": ISL, "latent_dim": 64},
           "train": {"step_max": 8, "batch_size": 1, "device_data": True,
                     "pushforward": {"steps": [-1, 2], "unrolls": [0, 1], "probs": [1, 1]}},
           "logging": {"log_steps": 2, "eval_steps": 4, "ckp_dir": str(tmp_path / "ckp_all"), "run_name": "r"},
           "eval": {"n_rollout_steps": 5, "train": {"n_trajs": 1, "metrics": ["mse"]},
                    "infer": {"n_trajs": 1, "batch_size": 1, "metrics": ["mse"], "out_type": "none"}}}
    assert train_or_infer(cfg) == 0
    assert os.path.exists(tmp_path / "ckp_all" / "r" / "best" / "params_array.npy")


# ------------------------------------------------------------------------------------------------ 6. two ranks
WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["LB_ROOT"])
import numpy as np, torch
from lagrangebench_amd import dist as lbdist
from lagrangebench_amd.case_setup import case_builder
from lagrangebench_amd.data import H5Dataset
from lagrangebench_amd.models import GNS
from lagrangebench_amd.train import Trainer

mode, out, ds_dir = sys.argv[1], os.environ["LB_OUT"], os.environ["LB_DATA"]
rank, local_rank, world = lbdist.env_world()
assert world == 2
torch.cuda.set_device(lbdist.local_device(local_rank))
isl = 6
noise_std = 3e-4 if mode == "dev" else 0.0
md = json.load(open(os.path.join(ds_dir, "metadata.json")))
bounds = np.array(md["bounds"])
data_train = H5Dataset("train", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=1)
data_valid = H5Dataset("valid", ds_dir, name="lj3d", input_seq_length=isl, extra_seq_length=10)
case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=noise_std)
model = GNS(3, 64, 2, 2, 16)
cfg_train = {"batch_size": 2, "noise_std": noise_std, "device_data": mode != "host0",
             "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200},
             "pushforward": {"steps": [-1, 1], "unrolls": [0, 1], "probs": [1, 1]}}
trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                  cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                  cfg_logging={"log_steps": 1, "eval_steps": 100}, input_seq_length=isl, seed=0)
assert trainer.world == 2 and trainer.shard == slice(rank, rank + 1)
params, _, opt = trainer.train(step_max=2)
assert opt["count"] == 3
np.save(os.path.join(out, f"weights_{rank}.npy"), model.flatten(params))
json.dump({"loss_log": trainer.loss_log}, open(os.path.join(out, f"log_{rank}.json"), "w"))
if torch.distributed.is_initialized():
    torch.distributed.destroy_process_group()
print("DDP_WORKER_OK", mode, rank)
'''


def _two_ranks(tmp_path, mode):
    from tests.test_train_ddp_gpu import _run_two_ranks
    import tests.test_train_ddp_gpu as ddp
    saved = ddp.WORKER
    ddp.WORKER = WORKER   # the same launcher: fresh children, each under its own `timeout -k 10`, first failure ends both
    try:
        out, _ = _run_two_ranks(tmp_path, mode, limit=300)
    finally:
        ddp.WORKER = saved
    return ([np.load(out / f"weights_{r}.npy") for r in range(2)],
            [json.load(open(out / f"log_{r}.json"))["loss_log"] for r in range(2)])


def test_two_ranks_device_data_identical_weights(tmp_path):
    w, logs = _two_ranks(tmp_path, "dev")
    assert w[0].size > 0 and np.isfinite(w[0]).all() and np.array_equal(_bits(w[0]), _bits(w[1]))
    assert logs[0] == logs[1] and [s for s, _ in logs[0]] == [0, 1, 2]


def test_two_ranks_without_noise_equal_the_host_route(tmp_path):
    wd, logs_d = _two_ranks(tmp_path, "dev0")
    wh, logs_h = _two_ranks(tmp_path, "host0")
    assert np.array_equal(_bits(wd[0]), _bits(wd[1])) and np.array_equal(_bits(wh[0]), _bits(wh[1]))
    assert np.array_equal(_bits(wd[0]), _bits(wh[0])) and logs_d[0] == logs_h[0]
