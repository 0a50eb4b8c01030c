"""EGNN on the device (csrc/lb_egnn.hip) against the torch restatement tests/_egnn_oracle.py: per-layer forward parity,
the run-time switches, the fused rollout (restatement, generic loop, determinism, kinematic particles), neighbor-list
overflow and the runner's inference route."""
import json
import os
import pickle
import shutil
from functools import partial

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._common import elementwise_stats, hip_case, oracle_case, rel_err  # noqa: E402
from tests._egnn_oracle import case_kwargs, egnn_forward, random_biases  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, b, box, periodic):
    """|a - b| with the minimum image on periodic boxes (a wrap across the box edge is not an error)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    if periodic:
        d = d - box * np.round(d / box)
    return np.abs(d)


def _pos_stats(a, b, box, periodic):
    """elementwise_stats on positions, the difference taken as the minimum image."""
    b = np.asarray(b, np.float64)
    return elementwise_stats(b + _dev(a, b, box, periodic), b)


def _case(name, B, scale=1.0, isl=6, free_space=False, extra=4):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=B, extra_seq_length=extra, input_seq_length=isl, scale=scale)
    if free_space:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos = np.stack([ds[i][0] for i in range(B)])
    pt = np.stack([ds[i][1] for i in range(B)])
    return ds, pos, pt


def _model(ds, H=128, L=5, isl=6, dt=0.01, **kw):
    """dt sets the initialiser scale of the (H, 1) outputs (UniformScaling(dt / L)).  The synthetic cases carry dt = 1:
    with that scale an untrained net moves particles by many spacings per layer and its latents grow without bound, so
    the tests use a dataset-like dt instead."""
    from lagrangebench_amd.models import EGNN
    return EGNN(H, 1, dt, isl - 1, num_mp_steps=L, **kw)


def _forward_parity(ds, pos, pt, model, params, flags):
    """Engine forward with taps vs the restatement in fp64 and fp32, trajectory by trajectory."""
    isl = ds.input_seq_length
    B, N, dim = pos.shape[0], pos.shape[1], len(ds.box)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    h = model.handle(feats.engine, params)
    tap_h, tap_x = h.set_tap(True)
    out = _np(model.apply(params, {}, (feats, pt))[0]["pos"])
    L = model._num_mp_steps
    assert out.dtype == np.float64 and out.shape == (B, N, dim)
    assert np.array_equal(out.reshape(B * N, dim), _np(tap_x[L]).astype(np.float64))
    kw = dict(case_kwargs(ds), num_mp_steps=L, n_vels=isl - 1, **flags)
    box, periodic = kw["box"], kw["periodic"]
    th, tx = _np(tap_h), _np(tap_x)
    for b in range(B):
        of, _ = ocase.allocate_eval((pos[b, :, :isl], pt[b]))
        h64, x64 = egnn_forward(params, of, pt[b], dtype=torch.float64, **kw)
        h32, x32 = egnn_forward(params, of, pt[b], dtype=torch.float32, **kw)
        sl = slice(b * N, (b + 1) * N)
        for layer in range(L + 1):
            e = rel_err(th[layer, sl], _np(h64[layer]))
            assert e <= 1e-5, (b, layer, e)
            _, m32, _ = _pos_stats(_np(x32[layer]), _np(x64[layer]), box, periodic)
            p99, mx, n = _pos_stats(tx[layer, sl], _np(x64[layer]), box, periodic)
            assert n > 0 and mx <= max(3 * m32, 2.0**-23), (b, layer, mx, m32)
    h.set_tap(False)
    return out


@pytest.mark.parametrize("name,B,scale,free,homog", [("rpf2d", 1, 1.0, False, True), ("rpf2d", 3, 1.0, False, True),
                                                     ("tgv3d", 1, 1.0, False, True), ("ldc3d", 1, 0.5, True, False)])
def test_forward_per_layer(name, B, scale, free, homog):
    _need_gpu()
    ds, pos, pt = _case(name, B, scale, free_space=free)
    model = _model(ds, homogeneous_particles=homog)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    _forward_parity(ds, pos, pt, model, params, dict(homogeneous=homog))


@pytest.mark.parametrize("sw", ["residual_off", "normalize", "tanh", "h64", "n_vels3"])
def test_forward_switches(sw):
    _need_gpu()
    isl = 4 if sw == "n_vels3" else 6
    ds, pos, pt = _case("rpf2d", 1, 0.5, isl=isl)
    kw = {"residual_off": dict(residual=False), "normalize": dict(normalize=True), "tanh": dict(tanh=True)}.get(sw, {})
    model = _model(ds, H=64 if sw == "h64" else 128, L=3, isl=isl, **kw)
    params = random_biases(model.init_params(9, True), 10)
    flags = dict(residual=kw.get("residual", True), normalize=kw.get("normalize", False), tanh=kw.get("tanh", False))
    _forward_parity(ds, pos, pt, model, params, flags)


def _rollouts(ds, pos, pt, model, params, n_steps):
    """(fused lb_egnn_rollout, generic Python loop driving EGNN.apply) through evaluate.rollout."""
    from lagrangebench_amd.evaluate.rollout import _eval_batched_rollout, _forward_eval
    hcase = hip_case(ds)
    isl = ds.input_seq_length
    out = []
    for fused in (True, False):
        apply = model.apply if fused else (lambda p, s, x: model.apply(p, s, x))
        fe = partial(_forward_eval, model_apply=apply, case_integrate=hcase.integrate)
        if fused:
            fe._lb_gns = model
        _, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
        preds, _, _ = _eval_batched_rollout(fe, hcase.preprocess_eval, hcase, params, {}, (pos, pt), nbrs,
                                            lambda a, b: {}, n_steps, isl)
        out.append(_np(preds))
    return out


def test_rollout_rpf2d():
    """20 fused steps on RPF2D x 2.  Each step is checked against the restatement run on the window the device had at
    that step (the device's own earlier predictions): two independent rollouts of an untrained net part ways as soon as
    one edge at the cutoff differs, which says nothing about the arithmetic of a step."""
    _need_gpu()
    n_steps, B = 20, 2
    ds, pos, pt = _case("rpf2d", B, extra=n_steps)
    model = _model(ds)
    params = random_biases(model.init_params(11, True), 12, scale=0.02)
    fused, generic = _rollouts(ds, pos, pt, model, params, n_steps)
    assert np.array_equal(fused, generic)
    fused2, _ = _rollouts(ds, pos, pt, model, params, n_steps)
    assert np.array_equal(fused, fused2)
    isl, dx = ds.input_seq_length, float(ds.metadata["dx"])
    ocase = oracle_case(ds)
    kw = dict(case_kwargs(ds), num_mp_steps=5, n_vels=isl - 1)
    box, periodic = kw["box"], kw["periodic"]
    for b in range(B):
        seq = np.concatenate([pos[b, :, :isl].astype(np.float64), np.transpose(fused[b], (1, 0, 2))], axis=1)
        for k in range(n_steps):
            of, _ = ocase.allocate_eval((seq[:, k:k + isl], pt[b]))
            x64 = _np(egnn_forward(params, of, pt[b], dtype=torch.float64, **kw)[1][-1])
            x32 = _np(egnn_forward(params, of, pt[b], dtype=torch.float32, **kw)[1][-1]).astype(np.float64)
            d32 = _dev(x32, x64, box, periodic).max()
            dg = _dev(fused[b, k], x64, box, periodic).max()
            assert dg <= max(3 * d32, 2.0**-23 * float(box.max())) and dg <= 1e-4 * dx, (b, k, dg, d32)


def test_rollout_kinematic_ldc3d():
    _need_gpu()
    n_steps = 5
    ds, pos, pt = _case("ldc3d", 1, 0.5, free_space=True, extra=n_steps)
    model = _model(ds, L=2, homogeneous_particles=False)
    params = random_biases(model.init_params(13, False), 14)
    fused, generic = _rollouts(ds, pos, pt, model, params, n_steps)
    assert np.array_equal(fused, generic)
    isl = ds.input_seq_length
    kin = (pt[0] == 1) | (pt[0] == 2)
    assert kin.any()
    for k in range(n_steps):
        assert np.array_equal(fused[0, k][kin], pos[0, kin, isl + k])
    assert not np.array_equal(fused[0, -1][~kin], pos[0, ~kin, isl + n_steps - 1])


def test_overflow_reallocation():
    _need_gpu()
    n_steps = 6
    ds, pos, pt = _case("rpf2d", 1, 0.5, extra=n_steps)
    model = _model(ds, L=2)
    params = random_biases(model.init_params(15, True), 16)
    hcase = hip_case(ds)
    traj = pos.astype(np.float64)
    eng = hcase.engine(1)
    eng.set_particle_type(pt)
    eng.load_window(traj, 0, 0)
    eng.nl_allocate()
    ref, n0 = eng.rollout(model.handle(eng, params), traj, n_steps)
    assert n0 == 0
    eng.load_window(traj, 0, 0)
    eng.nl_allocate()
    st = eng.stats()
    eng.nl_set_capacity(eng.cell_capacity, st["n_edges_total"] - 5)
    pred, n_realloc = eng.rollout(model.handle(eng, params), traj, n_steps)
    assert n_realloc >= 1
    assert np.array_equal(_np(pred), _np(ref))


def test_runner_infer_egnn_end_to_end(tmp_path):
    _need_gpu()
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.evaluate import infer
    from lagrangebench_amd.models import EGNN
    from lagrangebench_amd.runner import train_or_infer
    from lagrangebench_amd.utils import egnn_params_to_haiku, save_haiku
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "3D_LJ_3_1214every1")
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(root, ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    md.setdefault("write_every", 1)
    json.dump(md, open(ds_dir / "metadata.json", "w"))
    L, H, isl = 2, 32, 6
    model = EGNN(H, 1, md["dt"] * md["write_every"], isl - 1, num_mp_steps=L)
    params = random_biases(model.init_params(5, False), 6)
    ckp = str(tmp_path / "ckp")
    save_haiku(ckp, egnn_params_to_haiku(params, model), {}, None, {"step": 0, "loss": 1.0})
    cfg = {"mode": "infer", "load_ckp": ckp, "dataset": {"src": str(ds_dir), "name": "lj3d"},
           "model": {"name": "egnn", "num_mp_steps": L, "latent_dim": H, "input_seq_length": isl},
           "eval": {"n_rollout_steps": 10, "rollout_dir": str(tmp_path / "rollout"),
                    "infer": {"n_trajs": 1, "batch_size": 1, "metrics": ["mse"], "out_type": "pkl"}}}
    assert train_or_infer(cfg) == 0
    files = sorted(os.listdir(tmp_path / "rollout"))
    assert "rollout_0.pkl" in files and any(f.startswith("metrics") for f in files)
    r0 = pickle.load(open(tmp_path / "rollout" / "rollout_0.pkl", "rb"))
    assert r0["predicted_rollout"].shape == (16, 3, 3)
    # the same parameters through infer() directly
    from lagrangebench_amd.defaults import merge
    from lagrangebench_amd.runner import _RUN_DEFAULTS
    c = merge(_RUN_DEFAULTS, cfg)
    data = H5Dataset("test" if c.eval.test else "valid", dataset_path=str(ds_dir), name="lj3d", input_seq_length=isl,
                     extra_seq_length=10, nl_backend=c.neighbors.backend)
    bounds = np.array(md["bounds"])
    case = case_builder(box=bounds[:, 1] - bounds[:, 0], metadata=data.metadata, input_seq_length=isl,
                        cfg_neighbors=c.neighbors, cfg_model=c.model, noise_std=c.train.noise_std,
                        external_force_fn=data.external_force_fn, dtype=c.dtype)
    direct = str(tmp_path / "direct")
    infer(model, case, data, params=params, cfg_eval_infer={"n_trajs": 1, "batch_size": 1, "metrics": ["mse"],
                                                            "out_type": "pkl"}, rollout_dir=direct, n_rollout_steps=10)
    d0 = pickle.load(open(os.path.join(direct, "rollout_0.pkl"), "rb"))
    assert np.array_equal(r0["predicted_rollout"], d0["predicted_rollout"])
    assert not np.array_equal(r0["predicted_rollout"][isl:], r0["ground_truth_rollout"][isl:])
