"""Every device model on neighbor lists that hold edges in one direction only (tests/_asym.py).

A pair within one rounding of the cutoff can be an edge in one direction only (jax-md's periodic displacement is not
exactly antisymmetric); the reference sums such a list as it is.  Each test first proves its premise on the device: the
engine's list equals the oracle's bit for bit and holds the promised one-directional edges, after the allocation and
after an update to a later frame.  Then the model is held to the bars of its symmetric suite: GNS and SEGNN forward and
training (the training step's sender view falls back to the radix sort, and its first attempt must stay in bounds on a
fresh handle), EGNN forward, rollout and training, PaiNN forward and rollout, and bit-identical repeats of each."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lb_oracle as O  # noqa: E402
from tests._asym import asym_case, check_premise, one_directional_edges, oracle_edges  # noqa: E402
from tests._common import hip_case, oracle_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy()


def _premise(ds, pos, pt, pairs, dtype=np.float64):
    """The engine's list equals the oracle's bit for bit and holds the promised one-directional edges, after
    lb_nl_allocate on the window and after lb_nl_update to the window one frame later.  Returns the engine's case."""
    f32 = dtype == np.float32
    hcase = hip_case(ds, dtype="float32" if f32 else "float64")
    isl, B = ds.input_seq_length, pos.shape[0]
    _, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    for shift in (0, 1):
        if shift:
            _, nbrs = hcase.preprocess_eval((pos[:, :, shift:shift + isl], pt), nbrs)
            assert not bool(nbrs.did_buffer_overflow.any())
        idx, ne = _np(nbrs.idx), _np(nbrs.n_edges)
        for b in range(B):
            want = oracle_edges(ds, pos[b], pt[b], shift + isl, dtype=dtype)
            assert int(ne[b]) == want.shape[1] and np.array_equal(idx[b][:, :want.shape[1]], want), (b, shift)
            check_premise(want, pairs, b)
    return hcase


_PREMISE = [("tgv2d", 0.5, np.float64), ("tgv3d", 0.5, np.float64), ("tgv2d", 0.5, np.float32),
            ("tgv3d", 0.5, np.float32), ("rpf2d", 0.5, np.float64)]


@pytest.mark.parametrize("name,scale,dtype", _PREMISE, ids=[f"{n}-{np.dtype(d).name}" for n, _, d in _PREMISE])
def test_engine_list_holds_the_one_directional_edges(name, scale, dtype):
    ds, pos, pt, pairs = asym_case(name, scale=scale, dtype=dtype)
    _premise(ds, pos, pt, pairs, dtype)


# ------------------------------------------------------------------------------------------------ GNS
@pytest.mark.parametrize("fused", [True, False], ids=["fused_agg", "standalone_agg"])
@pytest.mark.parametrize("name", ["tgv2d", "tgv3d"])
def test_gns_forward(name, fused):
    from tests.test_gpu_parity import _gns_forward_check
    ds, pos, pt, pairs = asym_case(name)
    _premise(ds, pos, pt, pairs)
    a = _gns_forward_check(ds, pos, pt, 3, fused)
    b = _gns_forward_check(ds, pos, pt, 3, fused)
    assert np.array_equal(a, b)


def _gns_setup(name, dtype, L=2):
    from lagrangebench_amd.models import GNS
    from tests._common import make_params
    ds, pos, pt, pairs = asym_case(name, dtype=dtype)
    hcase = _premise(ds, pos, pt, pairs, dtype)
    isl, dim = ds.input_seq_length, len(ds.box)
    params = make_params(ds, num_mp_steps=L, decoder_scale=1.0)
    model = GNS(dim, 128, 2, L, 16)
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    target = torch.randn((pos.shape[0], pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    return ds, pos, pt, hcase, model, params, feats, nbrs, target


def _symmetric_window(ds, hcase, nbrs, pt, dtype):
    """The unmodified trajectories (no crafted pair), one frame on: the update path, a list with no one-directional edge."""
    B, isl = pt.shape[0], ds.input_seq_length
    pos = np.stack([ds[b][0] for b in range(B)]).astype(dtype).astype(np.float64)
    for b in range(B):
        assert not one_directional_edges(oracle_edges(ds, pos[b], pt[b], isl + 1, dtype=dtype)), b
    feats, nbrs = hcase.preprocess_eval((pos[:, :, 1:1 + isl], pt), nbrs)
    assert not bool(nbrs.did_buffer_overflow.any())
    return pos[:, :, 1:], feats


@pytest.mark.parametrize("name,dtype", [("tgv2d", np.float64), ("tgv3d", np.float32)], ids=["tgv2d-float64", "tgv3d-float32"])
def test_gns_training(name, dtype):
    """A fresh handle's first step on the asymmetric list (its sender view buffer has just been allocated: the attempt
    by transposition, which is thrown away, must stay in bounds), then a step on a symmetric frame with the same handle:
    loss and every gradient leaf against float64 autograd on the engine's own graph, the radix-sort fall-back counted."""
    from tests.test_train import _gns_grad_check
    L = 2
    ds, pos, pt, hcase, model, params, feats, nbrs, target = _gns_setup(name, dtype, L)
    th = model.train_handle(feats.engine, params)
    _gns_grad_check(model, th, feats, params, target, pt, L, 2, name + "-asym")
    n_sort = th.sort_fallbacks()
    assert n_sort >= 1
    _, feats2 = _symmetric_window(ds, hcase, nbrs, pt, dtype)
    _gns_grad_check(model, th, feats2, params, target, pt, L, 2, name + "-sym")
    assert th.sort_fallbacks() == n_sort   # back on the transposition path
    th.close()


_SORT_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, ".")
from tests.test_asym_lists_gpu import _gns_setup
ds, pos, pt, hcase, model, params, feats, nbrs, target = _gns_setup(sys.argv[2], np.float64)
th = model.train_handle(feats.engine, params)
th.zero_grad(); loss = th.loss_grad(target, 1.0)
np.save(sys.argv[1], th.read("grads")); print("LOSS", repr(loss), th.sort_fallbacks())
'''


def test_gns_training_transpose_fallback_equals_the_radix_sort(tmp_path):
    """The step that falls back from the transposition (one-directional edges) gives the gradients of a run that
    always sorts (LB_TRAIN_SORT=cub), bit for bit.  Subprocesses: the switch is read once per process."""
    outs = {}
    for mode in ("transpose", "cub"):
        env = dict(os.environ)
        env.pop("LB_TRAIN_SORT", None)
        if mode == "cub":
            env["LB_TRAIN_SORT"] = "cub"
        f = str(tmp_path / (mode + ".npy"))
        r = subprocess.run([sys.executable, "-c", _SORT_SCRIPT, f, "tgv3d"], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LOSS")][-1].split()
        outs[mode] = (np.load(f), line[1], int(line[2]))
    assert outs["transpose"][2] >= 1 and outs["cub"][2] == 0, (outs["transpose"][2], outs["cub"][2])
    assert outs["transpose"][1] == outs["cub"][1]
    assert np.abs(outs["cub"][0]).max() > 0 and np.array_equal(outs["transpose"][0], outs["cub"][0])


# ------------------------------------------------------------------------------------------------ SEGNN
def _segnn_model(ds, L, blocks=2):
    from lagrangebench_amd.models import SEGNN, node_irreps
    from oracle import segnn_oracle as S
    isl = ds.input_seq_length
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, True)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=True,
                  blocks_per_step=blocks)
    params = S.segnn_init(np.random.default_rng(11), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=L,
                          blocks_per_step=blocks, random_bias=True)
    return model, {k: v for k, v in params.items() if isinstance(v, dict)}


@pytest.mark.parametrize("name", ["tgv2d", "tgv3d"])
def test_segnn_forward_lmax1(name):
    from lagrangebench_amd.models import SEGNN, node_irreps
    from oracle import segnn_oracle as S
    from tests.test_segnn import _segnn_parity
    ds, pos, pt, pairs = asym_case(name)
    ds.magnitude_features = True
    _premise(ds, pos, pt, pairs)
    isl = ds.input_seq_length
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, True)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=isl - 1, homogeneous_particles=True)
    params = S.segnn_init(np.random.default_rng(7), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=2,
                          random_bias=True)
    a = _segnn_parity(ds, model, params, True, pos, pt, name + "-asym")
    assert np.array_equal(a, _segnn_parity(ds, model, params, True, pos, pt, name + "-asym"))


def test_segnn_forward_general_irreps():
    """hidden 20x0e+20x1o+20x2e, attributes up to 2e, on a 3D periodic batch of two."""
    from lagrangebench_amd.models import SEGNN, node_irreps
    from oracle import segnn_irreps_oracle as G
    from tests.test_segnn_irreps import _gen_parity
    ds, pos, pt, pairs = asym_case("tgv3d")
    ds.magnitude_features = True
    _premise(ds, pos, pt, pairs)
    isl, L = ds.input_seq_length, 2
    has_force = ds.external_force_fn is not None
    irr = node_irreps(ds.metadata, isl, has_force, True, True)
    model = SEGNN(irr, "1x1o+1x0e", 64, 2, 2, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=True,
                  norm=None, blocks_per_step=2)
    xn = G.node_chunks(isl - 1, False, has_force, True, True)
    params = G.segnn_init(np.random.default_rng(7), xn, num_mp_steps=L, scalar_units=64, lmax_hidden=2, lmax_attr=2,
                          blocks_per_step=2, norm=None, random_bias=True)
    _gen_parity(ds, model, params, True, pos, pt, None, "tgv3d-asym")


@pytest.mark.parametrize("name", ["tgv2d", "tgv3d"])
def test_segnn_training(name):
    from tests.test_segnn_train import _segnn_grad_check
    ds, pos, pt, pairs = asym_case(name)
    ds.magnitude_features = True
    hcase = _premise(ds, pos, pt, pairs)
    isl, dim, L = ds.input_seq_length, len(ds.box), 2
    model, params = _segnn_model(ds, L)
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    target = torch.randn((pos.shape[0], pos.shape[1], dim), generator=torch.Generator().manual_seed(5))
    th = model.train_handle(feats.engine, params)
    ocase = oracle_case(ds)
    _segnn_grad_check(model, th, params, ocase, pos, pt, target, L, 2, True, name + "-asym")
    n_sort = th.sort_fallbacks()
    assert n_sort >= 1
    pos2, _ = _symmetric_window(ds, hcase, nbrs, pt, np.float64)
    _segnn_grad_check(model, th, params, ocase, pos2, pt, target, L, 2, True, name + "-sym")
    assert th.sort_fallbacks() == n_sort
    th.close()


# ------------------------------------------------------------------------------------------------ EGNN
@pytest.mark.parametrize("name", ["rpf2d", "tgv3d"])
def test_egnn_forward_per_layer(name):
    from tests._egnn_oracle import random_biases
    from tests.test_egnn_gpu import _forward_parity, _model
    ds, pos, pt, pairs = asym_case(name)
    _premise(ds, pos, pt, pairs)
    model = _model(ds, L=3)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    a = _forward_parity(ds, pos, pt, model, params, dict(homogeneous=True))
    b = _forward_parity(ds, pos, pt, model, params, dict(homogeneous=True))
    assert np.array_equal(a, b)


def test_egnn_rollout():
    """Fused rollout = the generic loop, bit for bit, twice; every step against the restatement on the device's own
    window.  The pairs are kinematic, so every step's list holds the one-directional edges."""
    from tests._egnn_oracle import case_kwargs, egnn_forward, random_biases
    from tests.test_egnn_gpu import _dev, _model, _rollouts
    n_steps = 4
    ds, pos, pt, pairs = asym_case("rpf2d", extra=n_steps, kinematic=True)
    _premise(ds, pos, pt, pairs)
    model = _model(ds, L=3)
    params = random_biases(model.init_params(11, True), 12, scale=0.02)
    fused, generic = _rollouts(ds, pos, pt, model, params, n_steps)
    assert np.array_equal(fused, generic)
    fused2, _ = _rollouts(ds, pos, pt, model, params, n_steps)
    assert np.array_equal(fused, fused2)
    isl, dx = ds.input_seq_length, float(ds.metadata["dx"])
    ocase = oracle_case(ds)
    kw = dict(case_kwargs(ds), num_mp_steps=3, n_vels=isl - 1)
    box, periodic = kw["box"], kw["periodic"]
    for b in range(pos.shape[0]):
        free = ~O.get_kinematic_mask(pt[b])
        seq = np.concatenate([pos[b, :, :isl].astype(np.float64), np.transpose(fused[b], (1, 0, 2))], axis=1)
        for k in range(n_steps):
            of, nb = ocase.allocate_eval((seq[:, k:k + isl], pt[b]))
            check_premise(O.canonical_edges(nb.idx, pos.shape[1]), pairs, b)
            x64 = _np(egnn_forward(params, of, pt[b], dtype=torch.float64, **kw)[1][-1])
            x32 = _np(egnn_forward(params, of, pt[b], dtype=torch.float32, **kw)[1][-1]).astype(np.float64)
            d32 = _dev(x32, x64, box, periodic)[free].max()
            dg = _dev(fused[b, k], x64, box, periodic)[free].max()
            assert dg <= max(3 * d32, 2.0**-23 * float(box.max())) and dg <= 1e-4 * dx, (b, k, dg, d32)


def test_egnn_training():
    from lagrangebench_amd.models import EGNN
    from tests._egnn_oracle import case_kwargs, random_biases
    from tests.test_egnn_train import _egnn_grad_check
    isl, L = 6, 3
    ds, pos, pt, pairs = asym_case("rpf2d", isl=isl)
    hcase = _premise(ds, pos, pt, pairs)
    Bn, N, dim = pos.shape[0], pos.shape[1], len(ds.box)
    model = EGNN(128, 1, 0.01, isl - 1, num_mp_steps=L)
    params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    apply_pos = _np(model.apply(params, {}, (feats, pt))[0]["pos"])
    kw = dict(case_kwargs(ds), num_mp_steps=L, n_vels=isl - 1, homogeneous=True, residual=True, tanh=False)
    r_c = float(ds.metadata["default_connectivity_radius"])
    g = torch.Generator().manual_seed(3)
    tg = {"pos": torch.as_tensor(apply_pos) + 1e-2 * r_c * torch.randn((Bn, N, dim), generator=g, dtype=torch.float64),
          "vel": torch.randn((Bn, N, dim), generator=g, dtype=torch.float64),
          "acc": torch.randn((Bn, N, dim), generator=g, dtype=torch.float64)}
    lw = {"pos": 1.0, "vel": 0.5, "acc": 0.25}
    th = model.train_handle(feats.engine, params)
    _egnn_grad_check(th, model, params, oracle_case(ds), pos, pt, tg, lw, kw, apply_pos, "rpf2d-asym")
    th.close()


# ------------------------------------------------------------------------------------------------ PaiNN
def _painn_case(name, **kw):
    ds, pos, pt, pairs = asym_case(name, **kw)
    ds.magnitude_features = True
    _premise(ds, pos, pt, pairs)
    return ds, pos, pt


@pytest.mark.parametrize("radius", ["runner", 1.5])
@pytest.mark.parametrize("name", ["rpf2d", "tgv3d"])
def test_painn_forward_per_layer(name, radius):
    from tests.test_painn_gpu import _forward_parity, _model, _params
    ds, pos, pt = _painn_case(name)
    model = _model(ds, radius, L=3)
    params, state = _params(model, ds, 7)
    a, (live, n_self, total) = _forward_parity(ds, pos, pt, model, params, state)
    if radius == 1.5:
        assert live == total
    b, _ = _forward_parity(ds, pos, pt, model, params, state)
    assert np.array_equal(a, b)


def test_painn_rollout():
    from tests.test_painn_gpu import _model, _params, _rollouts
    n_steps = 4
    ds, pos, pt = _painn_case("rpf2d", extra=n_steps, kinematic=True)
    model = _model(ds, 1.5, L=3)
    params, state = _params(model, ds, 11)
    fused, generic = _rollouts(ds, pos, pt, model, params, state, n_steps)
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, generic)
    fused2, _ = _rollouts(ds, pos, pt, model, params, state, n_steps)
    assert np.array_equal(fused, fused2)
