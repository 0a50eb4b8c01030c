"""Push-forward from device weights (train.device_unroll) on the GPU: lb_gns_train_sync_model makes the images lb_gns_create
makes - byte for byte - so forwards, rollouts, Trainer losses and weights of the two routes are EQUAL, not close; the EGNN
training handle lends its inference view; the Trainer reads no weights back for an unroll.

Shapes: make_case("rpf2d", scale=0.5) and, for particle types and the embedding, make_case("ldc3d", scale=0.5); the Trainer
runs on the 3D Lennard-Jones fixture every Trainer test here uses (the Trainer needs an H5 dataset)."""
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests._common import feature_widths, hip_case  # noqa: E402
from tests.test_device_unroll import _model_and_blob  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ = os.path.join(ROOT, "tests", "golden", "3D_LJ_3_1214every1")
ISL = 6


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _engine(name):
    if not torch.cuda.is_available():
        pytest.fail("these tests need a HIP device (they are selected with -m gpu)")
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=1, extra_seq_length=4, input_seq_length=ISL, scale=0.5)
    pos, pt = ds[0][0][None], ds[0][1][None]
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :ISL], pt))
    return ds, pos, pt, feats


def _gns(ds, latent, depth, L, seed, **kw):
    """(model, params): random everything, the decoder head small enough for a calm 3-step rollout."""
    node_in, _ = feature_widths(ds)
    types = 9 if ds.name.startswith("ldc") else 1     # rpf2d: one particle type, no embedding
    return _model_and_blob(latent, depth, L, types, node_in, len(ds.box), seed=seed, **{"head_scale": 0.01, **kw})


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. images
@pytest.mark.parametrize("name,latent,depth", [("rpf2d", 128, 2), ("rpf2d", 64, 2), ("rpf2d", 32, 3), ("ldc3d", 128, 2)])
def test_synced_images_are_those_of_lb_gns_create(name, latent, depth):
    ds, pos, pt, feats = _engine(name)
    eng = feats.engine
    model, pB = _gns(ds, latent, depth, 2, seed=11)
    _, pA = _gns(ds, latent, depth, 2, seed=3)
    th = model.train_handle(eng, pB)
    hA = model._create(eng, pA, None)
    before = hA.image()
    th.sync_model(hA)
    hB = model._create(eng, pB, None)
    synced, direct = hA.image(), hB.image()
    assert synced.size == direct.size > 100_000 and not np.array_equal(before, direct)
    assert np.array_equal(synced, direct), int((synced != direct).sum())
    fa, fb = _np(eng.gns_forward(hA)), _np(eng.gns_forward(hB))
    assert np.isfinite(fb).all() and np.abs(fb).max() > 0 and np.array_equal(_bits(fa), _bits(fb))
    ra, rb = _np(eng.rollout(hA, pos, 3)[0]), _np(eng.rollout(hB, pos, 3)[0])
    assert np.isfinite(rb).all() and np.array_equal(ra, rb)
    th.close()


# ------------------------------------------------------------------------------------------------ 2. after optimiser steps
def test_sync_after_adamw_steps_and_twice():
    ds, pos, pt, feats = _engine("rpf2d")
    eng = feats.engine
    model, p0 = _gns(ds, 64, 2, 2, seed=5)
    th = model.train_handle(eng, p0)
    h = model._create(eng, p0, None)
    target = torch.randn((1, pos.shape[1], len(ds.box)), generator=torch.Generator().manual_seed(5))
    for _ in range(2):
        th.zero_grad()
        assert np.isfinite(th.loss_grad(target))
        th.adamw_step(1e-3)
    assert th.step_count() == 2
    th.sync_model(h)
    trained = model.unflatten(th.read("weights"), p0)
    assert not np.array_equal(model.flatten(trained), model.flatten(p0))
    direct = model._create(eng, trained, None).image()
    once = h.image()
    assert np.array_equal(once, direct), int((once != direct).sum())
    th.sync_model(h)
    assert np.array_equal(h.image(), once)
    th.close()


# ------------------------------------------------------------------------------------------------ 3. head scale, rms guard
def test_scaled_head_gives_the_host_routes_forward():
    outs = []
    for route in ("device", "host"):
        ds, pos, pt, feats = _engine("rpf2d")       # a fresh engine per route
        eng = feats.engine
        model, pB = _gns(ds, 128, 2, 2, seed=11, head_scale=2.0 ** -20)
        if route == "device":
            _, pA = _gns(ds, 128, 2, 2, seed=3)
            th = model.train_handle(eng, pB)
            h = model._create(eng, pA, None)
            th.sync_model(h)
        else:
            h = model._create(eng, pB, None)
        outs.append(_np(eng.gns_forward(h)))
        assert eng.math_mode()[0] == 1
    assert np.abs(outs[1]).max() > 0 and np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_rms_guard_fires_on_both_routes(capfd):
    if "LB_MATH" in os.environ:
        pytest.skip("LB_MATH fixes the arithmetic mode")
    outs = []
    for route in ("device", "host"):
        ds, pos, pt, feats = _engine("rpf2d")
        eng = feats.engine
        model, pB = _gns(ds, 128, 2, 2, seed=11)
        w = pB["proc1_node/linear_0"]["w"]
        rms = np.sqrt(np.mean(w[w != 0].astype(np.float64) ** 2))
        pB["proc1_node/linear_0"]["w"] = (w * np.float32(2.0 ** -9 / rms)).astype(np.float32)   # rms ~ 2^-9
        assert eng.math_mode()[0] == 1
        capfd.readouterr()
        if route == "device":
            _, pA = _gns(ds, 128, 2, 2, seed=3)
            th = model.train_handle(eng, pB)
            h = model._create(eng, pA, None)
            assert eng.math_mode()[0] == 1 and "rms" not in capfd.readouterr().err   # A's matrices are ordinary
            th.sync_model(h)
        else:
            h = model._create(eng, pB, None)
        assert "a weight matrix has rms" in capfd.readouterr().err
        assert eng.math_mode()[0] == 0                                                   # exact fp32 from here on
        outs.append(_np(eng.gns_forward(h)))
    assert np.isfinite(outs[1]).all() and np.array_equal(_bits(outs[0]), _bits(outs[1]))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_sync_refuses_another_engine_and_another_latent():
    from lagrangebench_amd._lib import LbHipError
    ds, pos, pt, feats = _engine("rpf2d")
    _, _, _, feats2 = _engine("rpf2d")
    eng = feats.engine
    model, p = _gns(ds, 64, 2, 1, seed=5)
    narrow, pn = _gns(ds, 32, 2, 1, seed=5)
    th = model.train_handle(eng, p)
    for h in (model._create(feats2.engine, p, None), narrow._create(eng, pn, None)):
        before = h.image()
        with pytest.raises(LbHipError):
            th.sync_model(h)
        assert np.array_equal(h.image(), before)
    th.close()


# ------------------------------------------------------------------------------------------------ 5. EGNN
def test_egnn_training_handle_lends_its_view():
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import EGNN
    from tests._egnn_oracle import random_biases
    if not torch.cuda.is_available():
        pytest.fail("these tests need a HIP device (they are selected with -m gpu)")
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=3, input_seq_length=ISL, scale=0.5)
    pos, pt = ds[0][0][None], ds[0][1][None]
    model = EGNN(64, 1, 0.01, ISL - 1, num_mp_steps=2)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :ISL], pt))
    eng = feats.engine
    th = model.train_handle(eng, params)
    view = th.model_handle()
    assert th.model_handle() is view and model.unroll_handle(eng, th, params) is view

    def both(handle=view):
        host = model.apply(model.unflatten(th.read("weights"), params), {}, (feats, pt))[0]["pos"]
        dev = model.apply_handle(handle, {}, (feats, pt))[0]["pos"]
        assert torch.isfinite(host).all() and np.array_equal(_np(host), _np(dev))
        return _np(host)

    first = both()
    target = {"pos": torch.as_tensor(first) + 1e-3, "vel": None, "acc": None}
    th.zero_grad()
    model.loss_grad(th, target, {"pos": 1.0, "vel": 0.0, "acc": 0.0})
    th.adamw_step(1e-3)
    assert not np.array_equal(both(), first)            # the view follows the optimiser
    view.close()                                        # lets go, frees nothing ...
    assert np.isfinite(th.read("weights")).all()
    again = th.model_handle()                           # ... the handle still has its view
    assert again is not view and view._h is None
    assert np.array_equal(_np(eng.egnn_forward(again)), both(again))
    th.close()
    assert again._h is None
    again.close()


# ------------------------------------------------------------------------------------------------ 6 - 8. Trainer
PUSHFORWARD = {"steps": [-1, -1, -1], "unrolls": [0, 1, 2], "probs": [1, 1, 1]}


def _lj_copy(tmp_path):
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    if not ds_dir.exists():
        shutil.copytree(LJ, ds_dir)
        md = json.load(open(ds_dir / "metadata.json"))
        md.setdefault("write_every", 1)
        json.dump(md, open(ds_dir / "metadata.json", "w"))
    return str(ds_dir)


def _trainer(ds_dir, kind, device_unroll, device_data=False):
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import EGNN, GNS, SEGNN
    from lagrangebench_amd.train import Trainer
    md = json.load(open(os.path.join(ds_dir, "metadata.json")))
    data_train = H5Dataset("train", ds_dir, name="lj3d", input_seq_length=ISL, extra_seq_length=3)
    data_valid = H5Dataset("valid", ds_dir, name="lj3d", input_seq_length=ISL, extra_seq_length=10)
    bounds = np.array(md["bounds"])
    cfg_model = {"magnitude_features": True} if kind == "segnn" else None
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, ISL, cfg_model=cfg_model, noise_std=3e-4)
    cfg_train = {"batch_size": 2, "noise_std": 3e-4, "device_unroll": device_unroll, "device_data": device_data,
                 "pushforward": PUSHFORWARD,
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    if kind == "egnn":
        model = EGNN(64, 1, md["dt"] * md["write_every"], ISL - 1, normalization_stats=case.normalization_stats, num_mp_steps=2)
        cfg_train["loss_weight"] = {"pos": 1.0, "vel": 0.0, "acc": 0.0}
    elif kind == "segnn":
        from lagrangebench_amd.models import node_irreps
        irr = node_irreps(md, ISL, False, True, True)
        model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=ISL - 1, homogeneous_particles=True)
    else:
        model = GNS(3, 32, 2, 2, 16)
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 1000}, input_seq_length=ISL, seed=0)
    return trainer, model


def _train8(tmp_path, monkeypatch, kind, device_unroll, device_data=False):
    """8 steps; -> (loss_log, flat weights, unroll counts drawn, read("weights") calls of the training handle)."""
    import lagrangebench_amd.train.trainer as T
    trainer, model = _trainer(_lj_copy(tmp_path), kind, device_unroll, device_data)
    drawn, reads = [], []
    from lagrangebench_amd.train.strats import push_forward_sample_steps as sample_steps

    def recording_sample_steps(key, step, pushforward):
        key, n = sample_steps(key, step, pushforward)
        drawn.append(n)
        return key, n

    monkeypatch.setattr(T, "push_forward_sample_steps", recording_sample_steps)
    train_handle = model.train_handle

    def counting_train_handle(engine, params):
        th = train_handle(engine, params)
        read = th.read
        th.read = lambda which="weights": (reads.append(which), read(which))[1]
        return th

    monkeypatch.setattr(model, "train_handle", counting_train_handle)
    params, _, opt = trainer.train(step_max=7)
    assert opt["count"] == 8 and len(trainer.loss_log) == 8, (opt["count"], trainer.loss_log)
    return trainer.loss_log, model.flatten(params), drawn, reads


@pytest.mark.parametrize("device_data", [False, True])
@pytest.mark.parametrize("kind", ["gns", "egnn"])
def test_trainer_is_bit_identical_with_the_key_on(tmp_path, monkeypatch, kind, device_data):
    off = _train8(tmp_path, monkeypatch, kind, False, device_data)
    on = _train8(tmp_path, monkeypatch, kind, True, device_data)
    print(f"[device unroll] {kind} device_data={device_data} unrolls {off[2]} losses {[l for _, l in off[0]]}")
    assert off[2] == on[2] and sum(n > 0 for n in off[2][:8]) >= 1      # the same draws, and at least one step unrolled
    assert np.isfinite([l for _, l in off[0]]).all() and off[0] == on[0], (off[0], on[0])
    assert np.array_equal(_bits(off[1]), _bits(on[1]))
    # 7. no host round trip: the weights are read back once per unrolled step with the key off - and, with it on, only for
    # the parameters the run returns
    unrolled = sum(n > 0 for n in off[2][:8])
    assert off[3].count("weights") == unrolled + 1, (off[3], off[2])
    assert on[3].count("weights") == 1 and on[3][0] == "weights", on[3]


def test_segnn_falls_back_to_the_host_route(tmp_path, monkeypatch, capsys):
    off = _train8(tmp_path, monkeypatch, "segnn", False)
    capsys.readouterr()
    on = _train8(tmp_path, monkeypatch, "segnn", True)
    assert capsys.readouterr().out.count("has no device route") == 1
    assert sum(n > 0 for n in off[2][:8]) >= 1 and off[0] == on[0] and np.array_equal(_bits(off[1]), _bits(on[1]))
    assert on[3].count("weights") == off[3].count("weights") > 1
