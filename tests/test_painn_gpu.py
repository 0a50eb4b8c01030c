"""PaiNN on the device (csrc/lb_painn.hip) against the torch restatement tests/_painn_oracle.py: per-layer forward parity
at the runner's radius and at a radius where every edge is live, the constructor switches, determinism, the fused
rollout (generic loop, kinematic particles), neighbor-list overflow and inference from a Haiku checkpoint."""
import json
import os
import pickle
import shutil
from functools import partial

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._common import hip_case, oracle_case, rel_err  # noqa: E402
from tests._painn_oracle import painn_forward, random_biases  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


def _case(name, B, scale=1.0, isl=6, free_space=False, extra=4):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=B, extra_seq_length=extra, input_seq_length=isl, scale=scale)
    ds.magnitude_features = True  # PaiNN's scalars (the reference's runner asserts magnitude features)
    if free_space:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos = np.stack([ds[i][0] for i in range(B)])
    pt = np.stack([ds[i][1] for i in range(B)])
    return ds, pos, pt


def _model(ds, radius, H=128, L=5, isl=6, trainable=True, cutoff=True, **kw):
    """radius "runner": the runner's physical 1.5 * default_connectivity_radius; a number: that radius in the units of
    the network's norms (1.5: every edge of the list is live)."""
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    r = 1.5 * ds.metadata["default_connectivity_radius"] if radius == "runner" else float(radius)
    return PaiNN(H, 1, L, gaussian_rbf(20, r, trainable=trainable), cosine_cutoff(r) if cutoff else None, isl - 1,
                 **kw)


def _params(model, ds, seed, free_space=False):
    p, s = model.init_params(seed, ds.external_force_fn is not None, free_space)
    return random_biases(p, seed + 1), s


def _oracle_kw(model, params, state):
    return dict(num_mp_steps=model._num_mp_steps, n_vels=model._n_vels, rbf=model._rbf(params, state),
                cutoff=model.cutoff_fn.cutoff if model.cutoff_fn is not None else None,
                homogeneous=model._homogeneous_particles, shared_filters=model._shared_filters,
                shared_interactions=model._shared_interactions)


def _live_edges(of, cutoff):
    """(live, self, total) edges of the oracle's list at this cutoff (norm < cutoff).  A self-edge has norm sqrt(eps) =
    1e-4 and is live at any cutoff above that."""
    N = np.asarray(of["vel_hist"]).shape[0]
    snd, rcv = np.asarray(of["senders"]), np.asarray(of["receivers"])
    keep = (snd < N) & (rcv < N)
    rel = np.asarray(of["rel_disp"], np.float64)[keep]
    norm = np.sqrt(np.sum(rel ** 2, axis=1) + 1e-8)
    live = int(np.sum(norm < cutoff)) if cutoff is not None else int(keep.sum())
    return live, int(np.sum(snd[keep] == rcv[keep])), int(keep.sum())


def _forward_parity(ds, pos, pt, model, params, state):
    """Engine forward with taps vs the restatement in fp64 and fp32, trajectory by trajectory.  Returns the live-edge
    counts (live, total) of the first trajectory."""
    isl = ds.input_seq_length
    B, N, dim = pos.shape[0], pos.shape[1], len(ds.box)
    hcase, ocase = hip_case(ds), oracle_case(ds)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    h = model.handle(feats.engine, params, state)
    tap_s, tap_v = h.set_tap(True)
    out = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    L = model._num_mp_steps
    assert out.dtype == np.float32 and out.shape == (B, N, dim)
    kw = _oracle_kw(model, params, state)
    ts, tv = _np(tap_s), _np(tap_v)
    counts = None
    for b in range(B):
        of, _ = ocase.allocate_eval((pos[b, :, :isl], pt[b]))
        counts = counts or _live_edges(of, kw["cutoff"])
        s64, v64, a64 = painn_forward(params, of, pt[b], dtype=torch.float64, **kw)
        s32, v32, a32 = painn_forward(params, of, pt[b], dtype=torch.float32, **kw)
        sl = slice(b * N, (b + 1) * N)
        for layer in range(L + 1):
            # 1e-5 in the max norm, or 3x the fp32 restatement's own error where that is larger: latents near the +-100
            # clip of an untrained net with every edge live (ldc3d) and the readout, which ends in a small difference
            # of O(1) terms, put the fp32 restatement itself beyond 1e-5
            for dev, o64, o32 in ((ts[layer, sl], s64[layer], s32[layer]), (tv[layer, sl], v64[layer], v32[layer])):
                e32 = rel_err(_np(o32), _np(o64))
                e = rel_err(dev, _np(o64))
                assert e <= max(1e-5, 3 * e32), (b, layer, e, e32)
        e32 = rel_err(_np(a32), _np(a64))
        e = rel_err(out[b], _np(a64))
        assert e <= max(1e-5, 3 * e32), (b, e, e32)
        assert np.abs(out[b]).max() > 0
    h.set_tap(False)
    return out, counts


@pytest.mark.parametrize("radius", ["runner", 1.5])
@pytest.mark.parametrize("name,B,scale,free,homog", [("rpf2d", 1, 1.0, False, True), ("rpf2d", 3, 1.0, False, True),
                                                     ("tgv3d", 1, 1.0, False, True), ("ldc3d", 1, 0.5, True, False)])
def test_forward_per_layer(name, B, scale, free, homog, radius):
    _need_gpu()
    ds, pos, pt = _case(name, B, scale, free_space=free)
    # ldc3d: from layer 3 on, the untrained net's latents saturate the +-100 clips and the forward turns ill-conditioned
    # (the fp32 restatement itself is 4e-4 off fp64 at layer 3 and 12 % at layer 4): parity says nothing there
    model = _model(ds, radius, L=2 if name == "ldc3d" else 5, homogeneous_particles=homog)
    params, state = _params(model, ds, 7, free)
    _, (live, n_self, total) = _forward_parity(ds, pos, pt, model, params, state)
    assert total > 0 and n_self == pos.shape[1]  # the radius graph has every self-edge
    if radius == 1.5:
        assert live == total  # every message computed: the dead-edge skip never fires
    elif name in ("rpf2d", "ldc3d"):
        # the runner's physical radius (RPF2D 0.054, LDC3D 0.09) against norms in units of r_c: only the self-edges
        # are live
        assert live == n_self, (live, n_self, total)
    else:
        assert n_self < live < total, (live, n_self, total)


@pytest.mark.parametrize("sw", ["shared_filters", "shared_interactions", "rbf_state", "no_cutoff", "h64", "n_vels3"])
def test_forward_switches(sw):
    _need_gpu()
    isl = 4 if sw == "n_vels3" else 6
    ds, pos, pt = _case("rpf2d", 1, 0.5, isl=isl)
    kw = {"shared_filters": dict(shared_filters=True), "shared_interactions": dict(shared_interactions=True),
          "rbf_state": dict(trainable=False), "no_cutoff": dict(cutoff=False)}.get(sw, {})
    model = _model(ds, 1.5, H=64 if sw == "h64" else 128, L=3, isl=isl, **kw)
    params, state = _params(model, ds, 9)
    if sw == "rbf_state":
        assert "~" not in params and state["~"]["widths"].shape == (1, 20)
    _forward_parity(ds, pos, pt, model, params, state)


def test_forward_bit_identical():
    _need_gpu()
    ds, pos, pt = _case("tgv3d", 1)
    model = _model(ds, 1.5, L=3)
    params, state = _params(model, ds, 3)
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :ds.input_seq_length], pt))
    a = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    b = _np(model.apply(params, state, (feats, pt))[0]["acc"])
    assert np.array_equal(a, b)


def _rollouts(ds, pos, pt, model, params, state, n_steps):
    """(fused lb_painn_rollout, generic Python loop driving PaiNN.apply + case.integrate) through evaluate.rollout."""
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
        preds, _, _ = _eval_batched_rollout(fe, hcase.preprocess_eval, hcase, params, state, (pos, pt), nbrs,
                                            lambda a, b: {}, n_steps, isl)
        out.append(_np(preds))
    return out


def test_rollout_rpf2d():
    _need_gpu()
    n_steps, B = 20, 2
    ds, pos, pt = _case("rpf2d", B, extra=n_steps)
    model = _model(ds, 1.5)
    params, state = _params(model, ds, 11)
    fused, generic = _rollouts(ds, pos, pt, model, params, state, n_steps)
    assert np.array_equal(fused, generic)
    fused2, _ = _rollouts(ds, pos, pt, model, params, state, n_steps)
    assert np.array_equal(fused, fused2)
    isl = ds.input_seq_length
    assert not np.array_equal(fused[:, -1], np.transpose(pos, (0, 2, 1, 3))[:, isl + n_steps - 1])


def test_rollout_kinematic_ldc3d():
    _need_gpu()
    n_steps = 5
    ds, pos, pt = _case("ldc3d", 1, 0.5, free_space=True, extra=n_steps)
    # the runner's radius: with every edge live the untrained net's free-space positions overflow within two steps
    model = _model(ds, "runner", L=2, homogeneous_particles=False)
    params, state = _params(model, ds, 13, free_space=True)
    fused, generic = _rollouts(ds, pos, pt, model, params, state, n_steps)
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, generic)
    isl = ds.input_seq_length
    kin = (pt[0] == 1) | (pt[0] == 2)
    assert kin.any()
    for k in range(n_steps):
        assert np.array_equal(fused[0, k][kin], pos[0, kin, isl + k])
        assert np.array_equal(generic[0, k][kin], pos[0, kin, isl + k])
    assert not np.array_equal(fused[0, -1][~kin], pos[0, ~kin, isl + n_steps - 1])


def test_overflow_reallocation():
    _need_gpu()
    n_steps = 6
    ds, pos, pt = _case("rpf2d", 1, 0.5, extra=n_steps)
    model = _model(ds, 1.5, L=2)
    params, state = _params(model, ds, 15)
    hcase = hip_case(ds)
    traj = pos.astype(np.float64)
    eng = hcase.engine(1)
    eng.set_particle_type(pt)
    eng.load_window(traj, 0, 0)
    eng.nl_allocate()
    ref, n0 = eng.rollout(model.handle(eng, params, state), traj, n_steps)
    assert n0 == 0
    eng.load_window(traj, 0, 0)
    eng.nl_allocate()
    st = eng.stats()
    eng.nl_set_capacity(eng.cell_capacity, st["n_edges_total"] - 5)
    pred, n_realloc = eng.rollout(model.handle(eng, params, state), traj, n_steps)
    assert n_realloc >= 1
    assert np.array_equal(_np(pred), _np(ref))


def test_infer_from_haiku_checkpoint(tmp_path):
    _need_gpu()
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.defaults import merge
    from lagrangebench_amd.evaluate import infer
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    from lagrangebench_amd.runner import _RUN_DEFAULTS
    from lagrangebench_amd.utils import painn_params_to_haiku, save_haiku
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "3D_LJ_3_1214every1")
    ds_dir = tmp_path / "3D_LJ_3_1214every1"
    shutil.copytree(root, ds_dir)
    md = json.load(open(ds_dir / "metadata.json"))
    L, H, isl = 2, 32, 6
    model = PaiNN(H, 1, L, gaussian_rbf(20, 1.5, trainable=True), cosine_cutoff(1.5), isl - 1)
    params, state = model.init_params(5, False)
    params = random_biases(params, 6)
    ckp = str(tmp_path / "ckp")
    save_haiku(ckp, painn_params_to_haiku(params, model), state, None, {"step": 0, "loss": 1.0})
    c = merge(_RUN_DEFAULTS, {"model": {"input_seq_length": isl, "magnitude_features": True}})
    data = H5Dataset("test", dataset_path=str(ds_dir), name="lj3d", input_seq_length=isl, extra_seq_length=10,
                     nl_backend=c.neighbors.backend)
    bounds = np.array(md["bounds"])
    case = case_builder(box=bounds[:, 1] - bounds[:, 0], metadata=data.metadata, input_seq_length=isl,
                        cfg_neighbors=c.neighbors, cfg_model=c.model, noise_std=c.train.noise_std,
                        external_force_fn=data.external_force_fn, dtype=c.dtype)
    cfg_inf = {"n_trajs": 1, "batch_size": 1, "metrics": ["mse"], "out_type": "pkl"}
    from_ckp, direct = str(tmp_path / "from_ckp"), str(tmp_path / "direct")
    infer(model, case, data, load_ckp=ckp, cfg_eval_infer=cfg_inf, rollout_dir=from_ckp, n_rollout_steps=10)
    infer(model, case, data, params=params, state=state, cfg_eval_infer=cfg_inf, rollout_dir=direct, n_rollout_steps=10)
    r0 = pickle.load(open(os.path.join(from_ckp, "rollout_0.pkl"), "rb"))
    d0 = pickle.load(open(os.path.join(direct, "rollout_0.pkl"), "rb"))
    assert r0["predicted_rollout"].shape == (16, 3, 3)
    assert np.array_equal(r0["predicted_rollout"], d0["predicted_rollout"])
    assert not np.array_equal(r0["predicted_rollout"][isl:], r0["ground_truth_rollout"][isl:])
