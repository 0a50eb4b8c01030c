"""Padded trajectories on the engine (the reference's `matscipy` backend: variable particle counts, every sample padded to
num_particles_max with particles of type -1 at position 0).  Expected values: the fp64 oracle on the COMPACT trajectory
(only the n_b real particles; pads trail, so real indices are the same in both).  Pad rows are the only rows left out of a
comparison, and every test asserts the pad share of its input."""
import copy
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import lb_oracle as O
from tests._common import hip_case, make_params, oracle_case, oracle_model_apply, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _batch(ds):
    pos = np.stack([ds[b][0] for b in range(len(ds))])
    pt = np.stack([ds[b][1] for b in range(len(ds))])
    N = pos.shape[1]
    counts = list(ds.n_real)
    assert min(counts) <= 0.7 * N, "needs a trajectory with >= 30 % pads"
    assert len(counts) == 1 or len(set(counts)) >= 2, "a batch needs two different particle counts"
    for b, n in enumerate(counts):
        assert (pt[b, :n] != -1).all() and (pt[b, n:] == -1).all() and (pos[b, n:] == 0).all()
    return pos, pt, counts, N


def _compact_ds(ds, n):
    """The same case with num_particles_max = n: what the engine needs to run one trajectory unpadded."""
    c = copy.copy(ds)
    c.metadata = copy.deepcopy(ds.metadata)
    c.metadata["num_particles_max"] = int(n)
    return c


def _check_lists(nbrs, feats, want_idx, want_feats, counts, N, cast=lambda x: x, what=""):
    """Edge list, edge count, self-edges, edge and node features of every trajectory of a padded batch against the oracle's on
    the compact trajectory."""
    idx_all, ne_all = _np(nbrs.idx), _np(nbrs.n_edges)
    for b, n in enumerate(counts):
        want = O.canonical_edges(want_idx[b], n)
        ne = want.shape[1]
        idx = idx_all[b]
        assert int(ne_all[b]) == ne, (what, b, int(ne_all[b]), ne)
        # exact: both are sorted by (receiver, sender) and real indices coincide, so equal arrays <=> equal edge sets
        assert np.array_equal(idx[:, :ne], want), (what, b)
        assert (idx[:, :ne] < n).all() and (idx[:, ne:] == N).all(), (what, b)
        assert int((idx[0, :ne] == idx[1, :ne]).sum()) == n, (what, b)     # every real particle keeps its self-edge
        if feats is None:
            continue
        of = want_feats[b]
        real = want_idx[b][0] < n
        order = np.lexsort((want_idx[b][1][real], want_idx[b][0][real]))
        assert np.array_equal(cast(_np(feats["rel_disp"])[b][:ne]), of["rel_disp"][real][order]), (what, b)
        assert np.array_equal(cast(_np(feats["rel_dist"])[b][:ne]), of["rel_dist"][real][order]), (what, b)
        for k in ("vel_hist", "vel_mag", "bound", "force"):
            if k in of:
                got = _np(feats[k])[b]
                assert np.array_equal(cast(got[:n]), of[k]), (what, b, k)
                assert np.isfinite(got).all(), (what, b, k)


# The search routes (csrc/lb_neighbor.hip: lbk_nl_build), picked by the input alone as in tests/test_gpu_parity.py:
#   wd2d_batch        waterdrop2d B=2 fp64: allocate = counting sort (CSR) + k_nl count / fill; update = fixed-stride bins + k_nl
#   wd2d_single       waterdrop2d B=1: update = the single launch k_nl_small
#   wd2d_f32          float32 geometry: k_nlc<F32, 2> (wave per cell), fixed-stride bins
#   small2d_batch     allocate = one-launch binning k_cells_small (<= 4096 particles and cells)
#   tgv3d_batch       k_nlc<fp64, 3>, fixed-stride bins
#   tgv3d_single_mid  update = the single launch k_nl_mid (8000 slots, 5000 real)
#   tgv3d_dense       > 256 neighbors: the dense fall-back k_nlw over the one-launch per-trajectory binning k_cells_traj
#   many_pads         5000 pads next to 1000 / 700 real particles: binned at the origin they would be LB_ERR_DENSITY
ROUTES = {"wd2d_batch": ("waterdrop2d", (300, 190), None, 1.0, 1.0, "float64"),
          "wd2d_single": ("waterdrop2d", (190,), 300, 1.0, 1.0, "float64"),
          "wd2d_f32": ("waterdrop2d", (300, 190), None, 1.0, 1.0, "float32"),
          "small2d_batch": ("small2d", (256, 160), None, 1.0, 1.0, "float64"),
          "tgv3d_batch": ("tgv3d", (1728, 1100), None, 0.6, 1.0, "float64"),
          "tgv3d_single_mid": ("tgv3d", (5000,), 8000, 1.0, 1.0, "float64"),
          "tgv3d_dense": ("tgv3d", (2197, 1500), None, 0.65, 2.8, "float64"),
          "many_pads": ("waterdrop2d", (1000, 700), 6000, 1.0, 1.0, "float64")}


def _make(name, counts, n_max, scale, rc_factor, extra=4):
    from lagrangebench_amd.data import make_padded_case
    ds = make_padded_case(name, counts, n_max=n_max, extra_seq_length=extra, scale=scale)
    if rc_factor != 1.0:
        ds.metadata["default_connectivity_radius"] = float(ds.metadata["default_connectivity_radius"]) * rc_factor
    return ds


@pytest.mark.parametrize("route", list(ROUTES))
def test_padded_neighbor_list_and_features_match_compact_oracle(route):
    """Edge sets, edge counts, self-edges, capacities and fp64 features on every search route: after allocate, after updates on
    later frames, and after a forced overflow re-allocation."""
    name, counts, n_max, scale, rc_factor, dtype = ROUTES[route]
    ds = _make(name, counts, n_max, scale, rc_factor)
    f32 = dtype == "float32"
    odt = np.float32 if f32 else np.float64
    cast = (lambda x: x.astype(np.float32)) if f32 else (lambda x: x)
    ocase, hcase = oracle_case(ds, dtype=odt), hip_case(ds, dtype=dtype)
    isl = ds.input_seq_length
    pos, pt, counts, N = _batch(ds)
    if route == "many_pads":
        assert N - max(counts) > 4096   # more pads than LB_MAX_ROW_DENSE neighbors: one cell, one row if they were binned
    B = len(counts)

    def oracle_alloc(t0):
        oo = [ocase.allocate_eval((pos[b][:n, t0:t0 + isl].astype(odt), pt[b][:n])) for b, n in enumerate(counts)]
        return [o[0] for o in oo], [o[1] for o in oo]

    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    ofs, ons = oracle_alloc(0)
    _check_lists(nbrs, feats, [o.idx for o in ons], ofs, counts, N, cast, "allocate")
    if rc_factor > 1.0:
        assert max(O.canonical_edges(on.idx, n).shape[1] / n for on, n in zip(ons, counts)) > 256
    # the capacity counts real edges only: int(max_b occupancy_b * multiplier) (the existing rule, tests/test_gpu_parity.py)
    assert nbrs.max_occupancy == int(max(O.canonical_edges(on.idx, n).shape[1] for on, n in zip(ons, counts)) * ds.multiplier)
    for shift in (1, 3):
        feats, nbrs = hcase.preprocess_eval((pos[:, :, shift:shift + isl], pt), nbrs)
        assert not bool(nbrs.did_buffer_overflow.any())
        ofs, ons = oracle_alloc(shift)
        _check_lists(nbrs, feats, [o.idx for o in ons], ofs, counts, N, cast, f"update {shift}")
    # forced overflow: capacity below the largest real edge count -> flag -> re-allocation on that frame
    eng = hcase.engine(B)
    ne_b = _np(nbrs.n_edges).astype(np.int64)
    cap = int(ne_b.max()) - 5
    eng.nl_set_capacity(eng.cell_capacity, cap)
    eng.nl_update()
    flags = _np(eng.nl_flags())
    assert [int(f) for f in flags] == [int(e > cap) for e in ne_b] and flags.any()
    feats, nbrs = hcase.allocate_eval((pos[:, :, 3:3 + isl], pt))
    _check_lists(nbrs, feats, [o.idx for o in ons], ofs, counts, N, cast, "re-allocation")
    feats, nbrs = hcase.preprocess_eval((pos[:, :, 4:4 + isl], pt), nbrs)
    ofs, ons = oracle_alloc(4)
    assert not bool(nbrs.did_buffer_overflow.any())
    _check_lists(nbrs, feats, [o.idx for o in ons], ofs, counts, N, cast, "update after re-allocation")


def test_padded_lists_on_the_multi_launch_paths():
    """LB_SMALL_FUSED=0 (read once per process): the counting-sort (CSR) binning and the separate scan / finish / compaction
    launches on the update path too - the same checks in a fresh process."""
    sel = "test_padded_neighbor_list_and_features_match_compact_oracle and (wd2d or small2d or tgv3d_batch)"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_padded_gpu.py", "-m", "gpu", "-q", "-x", "-k", sel,
                        "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, LB_SMALL_FUSED="0"), capture_output=True,
                       text=True, timeout=900)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-15:])
    assert r.returncode == 0, tail
    assert "5 passed" in r.stdout and "failed" not in r.stdout, tail


CASES = [("waterdrop2d", (300, 190), None, 1.0), ("small3d", (512, 330), None, 1.0)]


@pytest.mark.parametrize("name,counts,n_max,scale", CASES, ids=["waterdrop2d", "small3d"])
def test_padded_gns_forward_matches_compact_oracle_and_compact_device_run(name, counts, n_max, scale):
    """acc on the real rows within 1e-5 (max norm) of the oracle on the compact trajectory, pad rows
    finite; trajectory b alone, unpadded (N = n_b), on the device: the same edge set, acc within 1e-5."""
    from lagrangebench_amd.models import GNS
    L = 3
    ds = _make(name, counts, n_max, scale, 1.0)
    ocase, hcase = oracle_case(ds), hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos, pt, counts, N = _batch(ds)
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(dim, 128, 2, L, 16)
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    acc = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    assert acc.shape == (len(counts), N, dim) and np.isfinite(acc).all()
    idx_all, ne_all = _np(nbrs.idx), _np(nbrs.n_edges)
    for b, n in enumerate(counts):
        of, on = ocase.allocate_eval((pos[b][:n, :isl].astype(np.float64), pt[b][:n]))
        ref = O.gns_apply(params, of, pt[b][:n], num_mp_steps=L, skip_padding=True)["acc"]
        err = rel_err(acc[b][:n], ref)
        print(f"[padded forward {name} b={b} n={n}/{N}] rel err vs compact oracle {err:.2e}")
        assert err < 1e-5
        # the same trajectory alone and unpadded on the device
        ccase = hip_case(_compact_ds(ds, n))
        cf, cn = ccase.allocate_eval((pos[b][None, :n, :isl], pt[b][None, :n]))
        ne = int(_np(cn.n_edges)[0])
        assert ne == int(ne_all[b]) and np.array_equal(_np(cn.idx)[0][:, :ne], idx_all[b][:, :ne])
        cacc = _np(model.apply(params, {}, (cf, pt[b][None, :n]))[0]["acc"])[0]
        err_c = rel_err(acc[b][:n], cacc)
        print(f"[padded forward {name} b={b}] rel err vs compact device run {err_c:.2e}")
        assert err_c < 1e-5


def _oracle_compact_rollout(ds, params, L, n_steps, pos, pt, counts):
    ocase = oracle_case(ds)
    isl = ds.input_seq_length
    out = []
    for b, n in enumerate(counts):
        p = pos[b][None, :n].astype(np.float64)
        _, nb = ocase.allocate_eval((p[0][:, :isl], pt[b][:n]))
        preds, _, _ = O.eval_batched_rollout(oracle_model_apply(L), ocase, params, {}, (p, pt[b][None, :n]), nb,
                                             n_rollout_steps=n_steps, t_window=isl)
        out.append(preds[0])
    return out


@pytest.mark.parametrize("name,counts,n_max,scale", CASES, ids=["waterdrop2d", "small3d"])
def test_padded_fused_rollout_equals_loop_and_compact_oracle(name, counts, n_max, scale):
    """lb_rollout == the Python loop over GNS.apply + case.integrate bit for bit on the padded batch; pads stay exactly
    0 at every step, also across an overflow re-allocation; real positions within 1e-6 dx of the oracle's compact rollout."""
    from lagrangebench_amd.evaluate.metrics import MetricsComputer
    from lagrangebench_amd.evaluate.rollout import _eval_batched_rollout, _forward_eval
    from lagrangebench_amd.models import GNS
    L, n_steps = 3, 10
    ds = _make(name, counts, n_max, scale, 1.0, extra=n_steps)
    dim = len(ds.box)
    params = make_params(ds, num_mp_steps=L)
    model = GNS(dim, 128, 2, L, 16)
    hcase = hip_case(ds)
    isl = ds.input_seq_length
    pos, pt, counts, N = _batch(ds)
    _, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    mc = MetricsComputer(["mse"], hcase.displacement, ds.metadata, isl, case=hcase)
    fwd = partial(_forward_eval, model_apply=model.apply, case_integrate=hcase.integrate)
    p_gen, m_gen, _ = _eval_batched_rollout(fwd, hcase.preprocess_eval, hcase, params, {}, (pos, pt), nbrs, mc, n_steps, isl)
    fwd._lb_gns = model
    p_fused, m_fused, _ = _eval_batched_rollout(fwd, hcase.preprocess_eval, hcase, params, {}, (pos, pt), nbrs, mc, n_steps, isl)
    pg, pf = _np(p_gen), _np(p_fused)
    assert np.array_equal(pg, pf) and np.array_equal(_np(m_gen["mse"]), _np(m_fused["mse"]))
    want = _oracle_compact_rollout(ds, params, L, n_steps, pos, pt, counts)
    dx = float(ds.metadata["dx"])
    for b, n in enumerate(counts):
        assert (pf[b][:, n:] == 0).all()                      # (B, T, N, dim): pads stay at the origin
        err = np.abs(pf[b][:, :n] - want[b]).max()
        print(f"[padded rollout {name} b={b} n={n}/{N}] max |pos - compact oracle| = {err:.3e} ({err / dx:.2e} dx)")
        assert err < 1e-6 * dx
    # across an overflow re-allocation inside lb_rollout
    eng = hcase.engine(len(counts))
    eng.set_particle_type(pt)
    eng.load_window(pos.astype(np.float64), 0, 0)
    eng.nl_allocate()
    eng.nl_set_capacity(eng.cell_capacity, eng.stats()["n_edges_total"] // len(counts) - 5)
    pred, n_realloc = eng.rollout(model.handle(eng, params), pos.astype(np.float64), n_steps)
    assert n_realloc >= 1 and np.array_equal(_np(pred), pf)


@pytest.mark.parametrize("name,counts,n_max,scale", CASES, ids=["waterdrop2d", "small3d"])
def test_padded_training_gradients_match_autograd_on_compact_trajectories(name, counts, n_max, scale):
    """lb_gns_train_loss_grad on the padded batch against float64 torch autograd of oracle/gns_torch.py on the COMPACT
    trajectories (the oracle's own features and lists), gradients summed and loss averaged over the batch as the Trainer does:
    the bars of tests/test_train.py::test_hip_gradients_match_torch_autograd (predictions 1e-5, loss 1e-5, every leaf 1e-4
    relative); repeated calls give the same bits."""
    from oracle.gns_torch import gns_apply_torch, gns_inputs_from_features, params_to_torch
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.utils import get_kinematic_mask
    L, depth = 3, 2
    ds = _make(name, counts, n_max, scale, 1.0)
    ocase, hcase = oracle_case(ds), hip_case(ds)
    isl, dim = ds.input_seq_length, len(ds.box)
    pos, pt, counts, N = _batch(ds)
    B = len(counts)
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(dim, 128, depth, L, 16)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    target = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(5))
    th = model.train_handle(eng, params)
    th.zero_grad()
    loss_h, pred_h = th.loss_grad(target, 1.0, want_pred=True)
    g_flat = th.read("grads")
    g_h = model.unflatten(g_flat, params)
    for _ in range(2):
        th.zero_grad()
        loss_2, _ = th.loss_grad(target, 1.0, want_pred=True)
        assert loss_2 == loss_h and np.array_equal(th.read("grads"), g_flat)
    assert torch.isfinite(pred_h).all()
    dev = eng.device
    pt_t = {mod: {k: v.double().requires_grad_(True) for k, v in leaves.items()}
            for mod, leaves in params_to_torch(params, device=dev).items()}
    losses = []
    for b, n in enumerate(counts):
        of, _ = ocase.allocate_eval((pos[b][:n, :isl].astype(np.float64), pt[b][:n]))
        node, edge, snd, rcv, ptt = (x.to(dev) for x in gns_inputs_from_features(of, torch.as_tensor(pt[b][:n])))
        pred = gns_apply_torch(pt_t, node.double(), edge.double(), snd, rcv, ptt, L, depth)
        assert float((pred.detach() - pred_h[b][:n]).abs().max() / pred.detach().abs().max()) < 1e-5
        nk = ~get_kinematic_mask(ptt)
        assert int(nk.sum()) == n                                   # the denominator: the non-kinematic REAL particles
        tot = ((pred - target[b][:n].to(dev)) ** 2).sum(dim=-1)
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
    print(f"[padded grad {name}] loss {loss_h:.6f}, worst relative gradient error over the leaves {worst:.2e}")
    th.close()


def test_padded_trainer_and_runner_mode_all_on_h5(tmp_path):
    """End to end: a padded H5 dataset (variable particle counts on disk) through H5Dataset(nl_backend="matscipy"),
    the Trainer (shuffled batches mix particle counts) and train_or_infer(mode="all"): finite losses and metrics, a checkpoint
    that loads again.  The noise leaves the pads at the origin."""
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset, make_padded_case, write_padded_h5
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.runner import train_or_infer
    from lagrangebench_amd.train import Trainer
    from lagrangebench_amd.utils import load_haiku
    ds = make_padded_case("waterdrop2d", (300, 190, 240), extra_seq_length=8)
    root = write_padded_h5(ds, str(tmp_path / "WaterDropLike"))
    isl, L = 6, 2
    kw = dict(dataset_path=root, name="waterdroplike", input_seq_length=isl, nl_backend="matscipy")
    data_train = H5Dataset("train", extra_seq_length=1, **kw)
    data_valid = H5Dataset("valid", extra_seq_length=8, **kw)
    md = data_train.metadata
    assert data_train[0][0].shape[0] == 300 and (data_valid[1][1] == -1).sum() == 110
    bounds = np.array(md["bounds"])
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, cfg_neighbors={"backend": "matscipy"}, noise_std=3e-4)
    # noise: kinematic particles (pads) untouched by case.preprocess
    p0, t0 = data_train[len(data_train) - 1]
    case.allocate(torch.Generator().manual_seed(1), (p0, t0), noise_std=3e-4)
    win = _np(case.engine(1).read_window())[0]
    n0 = int((t0 != -1).sum())
    assert n0 < 300 and (win[n0:] == 0).all() and np.abs(win[:n0] - p0[:n0, :isl]).max() > 0
    model = GNS(2, 64, 2, L, 16)
    cfg_train = {"batch_size": 2, "noise_std": 3e-4,
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200},
                 "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 8, "train": {"n_trajs": 2, "metrics": ["mse", "e_kin", "sinkhorn"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 4}, input_seq_length=isl, seed=0)
    ckp = str(tmp_path / "ckp")
    params, state, opt_state = trainer.train(step_max=6, store_ckp=ckp)
    losses = [l for _, l in trainer.loss_log]
    assert len(losses) >= 6 and np.isfinite(losses).all(), losses
    loaded, _, opt_loaded, step = load_haiku(ckp)
    assert step == 4 and set(opt_loaded) >= {"m", "v", "step"}
    back = model.params_from_haiku(loaded)
    assert set(back) == set(params) and all(np.isfinite(v).all() for m in back.values() for v in m.values())
    cfg = {"mode": "all", "dataset": {"src": root, "name": "waterdroplike"}, "neighbors": {"backend": "matscipy"},
           "model": {"name": "gns", "num_mp_steps": 1, "input_seq_length": isl, "latent_dim": 64},
           "train": {"step_max": 6, "batch_size": 2, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]}},
           "logging": {"log_steps": 2, "eval_steps": 3, "ckp_dir": str(tmp_path / "ckp2"), "run_name": "r"},
           "eval": {"n_rollout_steps": 8, "train": {"n_trajs": 2, "metrics": ["mse"]},
                    "infer": {"n_trajs": 3, "batch_size": 2, "metrics": ["mse", "e_kin", "sinkhorn"], "out_type": "none"}}}
    assert train_or_infer(cfg) == 0
    assert os.path.exists(os.path.join(str(tmp_path / "ckp2"), "r", "best", "params_array.npy"))
    cfg_i = dict(cfg, mode="infer", load_ckp=os.path.join(str(tmp_path / "ckp2"), "r", "best"))
    assert train_or_infer(cfg_i) == 0


def test_other_models_refuse_padded_batches_before_running():
    """SEGNN / EGNN / PaiNN on an engine that holds pads: NotImplementedError naming padded trajectories, with the GNS forward
    on the same state still fine; an unpadded sample clears the flag."""
    from lagrangebench_amd.models import EGNN, GNS
    ds = _make("waterdrop2d", (300, 190), None, 1.0, 1.0)
    hcase = hip_case(ds)
    isl = ds.input_seq_length
    pos, pt, counts, N = _batch(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    assert feats.engine.has_pads
    egnn = EGNN(hidden_size=32, output_size=1, dt=1.0, n_vels=isl - 1, normalization_stats=hcase.normalization_stats,
                num_mp_steps=1)
    with pytest.raises(NotImplementedError, match="padded trajectories"):
        egnn.apply({}, {}, (feats, pt))
    params = make_params(ds, num_mp_steps=1)
    acc = _np(GNS(2, 128, 2, 1, 16).apply(params, {}, (feats, pt))[0]["acc"])
    assert np.isfinite(acc).all()
    hcase.allocate_eval((pos[:1, :, :isl], np.zeros_like(pt[:1])))
    assert not hcase.engine(1).has_pads
