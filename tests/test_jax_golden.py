"""Consumers of the JAX-reference fixtures written by tests/golden/make_jax_golden.py.

The fixtures (`tests/golden/jax_gns_{2d,3d}.npz`, `jax_segnn_*.npz`) hold inputs, Haiku weights and
outputs of the REAL reference (lagrangebench on JAX).  They cannot be produced in the build
container (JAX is not installable offline), so until somebody runs the generator on a JAX machine
and commits the files these tests skip with that reason - and the network layer of the oracle
stays "parity unpinned".  With the files present:
  * CPU (`-m "not gpu"`): oracle/lb_oracle.py vs the reference - neighbor list, features, GNS
    accelerations (1e-5 rel), integrator, 5-step rollout.
  * GPU (`-m gpu`): the HIP engine vs the reference on the same inputs.
Without the files the GPU consumers still run, on a fixture in the generator's format whose expected values come from
the CPU oracle (see "No JAX fixture committed" below): reader, engine and assertions are the same, the pin to JAX is not.
"""
import glob
import json
import os

import numpy as np
import pytest

from oracle import lb_oracle as O
from tests._common import rel_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GNS_FILES = sorted(glob.glob(os.path.join(GOLD, "jax_gns_*.npz")))
SEGNN_FILES = sorted(glob.glob(os.path.join(GOLD, "jax_segnn_*.npz")))
NO_FIXTURE = ("no JAX-reference fixture committed: run tests/golden/make_jax_golden.py where "
              "lagrangebench imports (parity of the network layer is unpinned until then)")


def _load(path):
    return _unpack(np.load(path, allow_pickle=False))


def _unpack(z):
    md = json.loads(str(z["metadata_json"]))
    hk = {}
    for k in z.files:
        if k.startswith("param//"):
            parts = k.split("//")[1:]
            hk.setdefault("/".join(parts[:-1]), {})[parts[-1]] = z[k]
    return z, md, hk


def _gns_params(hk, L):
    from lagrangebench_amd.utils import gns_params_from_haiku
    return gns_params_from_haiku(hk, L, 2)


def test_generator_exists_and_is_skipped_cleanly_without_jax():
    """The generator must be runnable as a plain script and must not write anything when the
    reference does not import (exit code 2)."""
    import subprocess
    import sys
    gen = os.path.join(GOLD, "make_jax_golden.py")
    assert os.path.exists(gen)
    try:
        import jax  # noqa: F401
        pytest.skip("JAX is importable here: run the generator for real instead")
    except ImportError:
        pass
    before = set(os.listdir(GOLD))
    r = subprocess.run([sys.executable, gen, "--ref", "/nonexistent"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "nothing written" in r.stdout
    assert set(os.listdir(GOLD)) == before


@pytest.mark.parametrize("path", GNS_FILES or [None])
def test_oracle_matches_jax_reference_gns(path):
    if path is None:
        pytest.skip(NO_FIXTURE)
    z, md, hk = _load(path)
    L = int(z["num_mp_steps"])
    pos, pt = z["position"], z["particle_type"]
    isl = 6
    box = np.array([b[1] - b[0] for b in md["bounds"]])
    case = O.case_builder(box, md, isl, cfg_neighbors={"multiplier": 1.25},
                          cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)
    feats, nbrs = case.allocate_eval((pos[:, :isl].astype(np.float64), pt))
    n = len(pt)
    assert nbrs.idx.shape == z["idx"].shape
    assert (nbrs.idx == z["idx"]).all(), "edge ORDER differs from jax-md's"
    for k in ("vel_hist", "rel_disp", "rel_dist"):
        assert np.allclose(feats[k], z[f"feat//{k}"], rtol=0, atol=1e-12), k
    params = _gns_params(hk, L)
    acc = O.gns_apply(params, feats, pt, num_mp_steps=L)["acc"]
    assert rel_err(acc, z["acc"]) < 1e-5
    nxt = case.integrate({"acc": z["acc"]}, pos[:, :isl].astype(np.float64))
    assert np.allclose(nxt, z["next_position"], rtol=0, atol=1e-12)

    def apply(p, state, sample):
        f, ptype = sample
        return O.gns_apply(p, f, ptype, num_mp_steps=L, skip_padding=True), state
    T = z["rollout"].shape[0]
    pred, _, _ = O.eval_batched_rollout(apply, case, params, {}, (pos[None].astype(np.float64), pt[None]), nbrs,
                                        n_rollout_steps=T, t_window=isl)
    assert np.abs(pred[0] - z["rollout"]).max() < 1e-6 * md["dx"]
    assert n == z["acc"].shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("path", GNS_FILES or [None])
def test_engine_matches_jax_reference_gns(path):
    """path None: no JAX fixture committed - the oracle-made fixture of the generator's 3D GNS case instead."""
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.models import GNS
    z, md, hk = _load(path) if path is not None else _unpack(_oracle_gns_fixture())
    L = int(z["num_mp_steps"])
    pos, pt = z["position"], z["particle_type"]
    isl, dim, n = 6, md["dim"], len(pt)
    box = np.array([b[1] - b[0] for b in md["bounds"]])
    case = case_builder(box, md, isl, cfg_neighbors={"multiplier": 1.25},
                        cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)
    feats, nbrs = case.allocate_eval((pos[:, :isl], pt))
    assert (O.canonical_edges(nbrs.idx.cpu().numpy(), n) == O.canonical_edges(z["idx"], n)).all()
    params = _gns_params(hk, L)
    model = GNS(dim, 128, 2, L, 16)
    acc = model.apply(params, {}, (feats, pt))[0]["acc"].cpu().numpy()
    assert rel_err(acc, z["acc"]) < 1e-5
    eng = case.engine(1)
    eng.set_particle_type(pt[None])
    T = z["rollout"].shape[0]
    pred, _ = eng.rollout(model.handle(eng, params), pos[None].astype(np.float64), T)
    assert np.abs(pred.cpu().numpy()[0] - z["rollout"]).max() < 1e-6 * md["dx"]
    assert torch.isfinite(pred).all()


def _segnn_from_fixture(z, md, hk, isl=6):
    """The fixture's SEGNN as this package's model + parameters, and the oracle evaluation of its forward pass: the lmax-1
    oracle for the shipped switches, the general-irreps oracle (A7 - A10) for lmax 2 / norm (fixtures *_l22_*, *_bn_*, ..)."""
    from lagrangebench_amd.models import SEGNN, node_irreps
    from lagrangebench_amd.utils import segnn_params_from_haiku
    L = int(z["num_mp_steps"])
    lh = int(z["lmax_hidden"]) if "lmax_hidden" in z else 1
    la = int(z["lmax_attributes"]) if "lmax_attributes" in z else 1
    norm = str(z["norm"]) if "norm" in z else "none"
    irr = node_irreps(md, isl, False, False, False)
    model = SEGNN(irr, "1x1o+1x0e", 64, lh, la, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=False,
                  norm=norm, blocks_per_step=2)
    return model, segnn_params_from_haiku(hk, model)


def _segnn_oracle_acc(model, params, feats, pt, isl=6):
    if not model.generic:
        from oracle import segnn_oracle as S
        return S.segnn_apply(params, feats, pt, isl - 1, False)["acc"]
    from oracle import segnn_irreps_oracle as G
    p = dict(params)
    p.update({"hidden": model.hidden_chunks(), "blocks": model._blocks_per_step, "layers": model._num_mp_steps,
              "lmax_attr": model._lmax_attributes, "norm": {0: None, 1: "instance", 2: "batch"}[model._norm],
              "x_node": model._node_chunks})
    return G.segnn_apply(p, feats, pt, isl - 1, False, norm_eps=model.norm_eps)["acc"]


@pytest.mark.parametrize("path", SEGNN_FILES or [None])
def test_oracle_matches_jax_reference_segnn(path):
    if path is None:
        pytest.skip(NO_FIXTURE)
    z, md, hk = _load(path)
    pos, pt = z["position"], z["particle_type"]
    isl = 6
    box = np.array([b[1] - b[0] for b in md["bounds"]])
    case = O.case_builder(box, md, isl, cfg_neighbors={"multiplier": 1.25},
                          cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)
    feats, _ = case.allocate_eval((pos[:, :isl].astype(np.float64), pt))
    model, params = _segnn_from_fixture(z, md, hk, isl)
    acc = _segnn_oracle_acc(model, params, feats, pt, isl)
    # (norm fixtures: the float32 evaluation itself is only ~1e-4-reproducible, tests/test_segnn_irreps.py)
    assert rel_err(acc[:, :md["dim"]], z["acc"]) < (1e-5 if model._norm == 0 else 3e-4)


def test_segnn_fixture_reader_on_a_synthetic_fixture():
    """No JAX here, so the SEGNN consumer above has never seen a fixture: build one in the generator's format from this
    package's own model (Haiku leaf names through segnn_params_to_haiku, the generator's "param//<module>//<leaf>" keys,
    lmax / norm scalars) and check that the reader reconstructs model and parameters - for the shipped switches and for a
    general one."""
    from lagrangebench_amd.models import SEGNN, node_irreps
    from lagrangebench_amd.utils import segnn_params_to_haiku
    md = {"periodic_boundary_conditions": [True, True, True], "dim": 3}
    irr = node_irreps(md, 6, False, False, False)
    for lh, la, norm in ((1, 1, "none"), (2, 2, "batch")):
        src = SEGNN(irr, "1x1o+1x0e", 64, lh, la, "1x1o", num_mp_steps=2, n_vels=5, homogeneous_particles=False, norm=norm)
        params = src.init_params(1)
        z = {"num_mp_steps": np.array(2), "lmax_hidden": np.array(lh), "lmax_attributes": np.array(la), "norm": np.array(norm)}
        hk = segnn_params_to_haiku(params, src)
        model, back = _segnn_from_fixture(z, md, hk)
        assert model.generic == src.generic
        assert np.array_equal(model.flatten(back), src.flatten(params))


# ---------------------------------------------------------------------------------------------------- jax_extras.npz
EXTRAS = os.path.join(GOLD, "jax_extras.npz")
NO_EXTRAS = ("no jax_extras.npz committed: run tests/golden/make_jax_golden.py where lagrangebench imports (Sinkhorn, "
             "dense-cell neighbor order, save_haiku file layout and get_dataset_stats are pinned by it)")


def _extras():
    if not os.path.exists(EXTRAS):
        pytest.skip(NO_EXTRAS)
    return np.load(EXTRAS, allow_pickle=False)


def _dense_case(z, builder):
    md = json.loads(str(z["dense//metadata_json"]))
    box = np.array([b[1] - b[0] for b in md["bounds"]])
    case = builder(box, md, 6, cfg_neighbors={"multiplier": 1.25},
                   cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)
    return md, case


def test_oracle_matches_jax_reference_extras(tmp_path):
    """CPU side of jax_extras.npz: jax-md's RAW slot order with several particles per cell (allocate and update path),
    Sinkhorn through both OT backends, get_dataset_stats, and a checkpoint written by the reference's save_haiku read
    back by this package's load_haiku and evaluated by the oracle."""
    z = _extras()
    pos = z["dense//position"]
    pt = np.zeros(len(pos), np.int32)
    md, case = _dense_case(z, O.case_builder)
    feats, nbrs = case.allocate_eval((pos[:, :6].astype(np.float64), pt))
    assert int(z["dense//cell_capacity"]) == 0 or int(z["dense//cell_capacity"]) >= 3
    assert nbrs.idx.shape == z["dense//idx"].shape and (nbrs.idx == z["dense//idx"]).all(), "raw slot order (allocate)"
    assert np.allclose(feats["rel_disp"], z["dense//rel_disp"], rtol=0, atol=1e-12)
    _, n2 = case.preprocess_eval((pos[:, 3:9].astype(np.float64), pt), nbrs)
    assert (n2.idx == z["dense//idx_update"]).all(), "raw slot order (update)"
    # Sinkhorn (evaluate/metrics.py:127-213), frames 0, 10, 20
    from oracle import sinkhorn_oracle as SK
    from oracle import sinkhorn_pot_oracle as SP
    pred, targ = z["sinkhorn//pred"], z["sinkhorn//target"]
    if "sinkhorn//ott" in z.files:
        got = SK.sinkhorn_rollout(case.displacement, pred, targ, 10)
        assert np.allclose(got, z["sinkhorn//ott"], rtol=1e-4, atol=1e-9 * float(np.abs(z["sinkhorn//ott"]).max() + 1e-30))
    if "sinkhorn//pot" in z.files:
        got = np.array([SP.sinkhorn_divergence_pot(case.displacement, p, t) for p, t in zip(pred[::10], targ[::10])])
        assert np.allclose(got, z["sinkhorn//pot"], rtol=2e-5, atol=1e-7)
    # get_dataset_stats (data/utils.py:9-45)
    from lagrangebench_amd.data.utils import get_dataset_stats
    mds = json.loads(str(z["stats//metadata_json"]))
    for iso in (0, 1):
        st = get_dataset_stats(mds, bool(iso), 3e-4)
        for q in ("acceleration", "velocity"):
            for m in ("mean", "std"):
                assert np.allclose(st[q][m], z[f"stats//iso{iso}//{q}//{m}"], rtol=1e-6, atol=0), (iso, q, m)
    # the reference's checkpoint files -> load_haiku -> oracle forward
    from lagrangebench_amd.utils import gns_params_from_haiku, load_haiku
    ck = tmp_path / "ckp"
    ck.mkdir()
    for k in z.files:
        if k.startswith("ckpt//") and k.count("//") == 1 and k.split("//")[1] not in ("acc", "num_mp_steps"):
            (ck / k.split("//")[1]).write_bytes(z[k].tobytes())
    params_hk, _, _, step = load_haiku(str(ck))
    assert step == 7
    L = int(z["ckpt//num_mp_steps"])
    params = gns_params_from_haiku(params_hk, L, 2)
    f = {k.split("//")[2]: z[k] for k in z.files if k.startswith("ckpt//feat//")}
    acc = O.gns_apply(params, f, pt, num_mp_steps=L)["acc"]
    assert rel_err(acc, z["ckpt//acc"]) < 1e-5


@pytest.mark.gpu
def test_engine_matches_jax_reference_extras(tmp_path):
    """GPU side of jax_extras.npz: the engine's edge list (canonical order) and Sinkhorn kernels against the reference,
    and the reference's checkpoint evaluated by the HIP engine.  Without jax_extras.npz: the oracle-made fixture."""
    import torch
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.evaluate.metrics import MetricsComputer
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.utils import gns_params_from_haiku, load_haiku
    z = np.load(EXTRAS, allow_pickle=False) if os.path.exists(EXTRAS) else _oracle_extras_fixture()
    pos = z["dense//position"]
    n = len(pos)
    pt = np.zeros(n, np.int32)
    md, case = _dense_case(z, case_builder)
    feats, nbrs = case.allocate_eval((pos[:, :6], pt))
    assert (O.canonical_edges(nbrs.idx.cpu().numpy(), n) == O.canonical_edges(z["dense//idx"], n)).all()
    pred = torch.as_tensor(z["sinkhorn//pred"], device="cuda")
    targ = torch.as_tensor(z["sinkhorn//target"], device="cuda")
    for backend, tol in (("ott", 1e-4), ("pot", 2e-5)):
        if f"sinkhorn//{backend}" not in z.files:
            continue
        mc = MetricsComputer(["sinkhorn"], case.displacement, md, 6, stride=10, ot_backend=backend, case=case)
        got = mc(pred, targ)["sinkhorn"].cpu().numpy()
        assert np.allclose(got, z[f"sinkhorn//{backend}"], rtol=tol, atol=1e-7), backend
    ck = tmp_path / "ckp"
    ck.mkdir()
    for k in z.files:
        if k.startswith("ckpt//") and k.count("//") == 1 and k.split("//")[1] not in ("acc", "num_mp_steps"):
            (ck / k.split("//")[1]).write_bytes(z[k].tobytes())
    params_hk, _, _, _ = load_haiku(str(ck))
    L = int(z["ckpt//num_mp_steps"])
    params = gns_params_from_haiku(params_hk, L, 2)
    acc = GNS(md["dim"], 128, 2, L, 16).apply(params, {}, (feats, pt))[0]["acc"].cpu().numpy()
    assert rel_err(acc, z["ckpt//acc"]) < 1e-5


# ------------------------------------------------------------------------------------------ No JAX fixture committed
# The GPU consumers above read the real reference's outputs, which only make_jax_golden.py on a machine with JAX can
# write.  Until those files are committed they read fixtures built here in the generator's format: the generator's own
# inputs (_cloud / _metadata, same cases and seeds), weights under Haiku module names (gns_params_to_haiku, and the files
# of this package's save_haiku for the checkpoint), expected values from the CPU oracle.  The CPU consumers keep skipping:
# the oracle against itself would check nothing.
class _Fixture(dict):
    """dict with the .files of an NpzFile."""
    @property
    def files(self):
        return list(self)


def _golden_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_jax_golden", os.path.join(GOLD, "make_jax_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _oracle_params(box, md, isl, L, decoder_scale):
    from types import SimpleNamespace
    from tests._common import make_params
    ds = SimpleNamespace(box=box, metadata=md, input_seq_length=isl, external_force_fn=None)
    return make_params(ds, num_mp_steps=L, decoder_scale=decoder_scale)


def _oracle_case(box, md, isl):
    return O.case_builder(box, md, isl, cfg_neighbors={"multiplier": 1.25},
                          cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)


def _oracle_gns_fixture():
    """jax_gns_3d.npz's case (make_jax_golden.py main: dim 3, 8^3 particles, every 8th a wall, 2 MP steps, 5-step
    rollout) with the oracle's neighbor list, accelerations and rollout."""
    from lagrangebench_amd.utils import gns_params_to_haiku
    G = _golden_generator()
    dim, n_side, L, isl, n_extra, dx = 3, 8, 2, 6, 5, 0.05
    pos, box = G._cloud(n_side, dim, dx, isl, n_extra, seed=dim)
    n = len(pos)
    pt = np.zeros(n, np.int32)
    pt[: n // 8] = 1
    md = G._metadata(dim, n, box, dx, 1.45 * dx, isl + n_extra)
    case = _oracle_case(box, md, isl)
    p64 = pos.astype(np.float64)
    feats, nbrs = case.allocate_eval((p64[:, :isl], pt))
    params = _oracle_params(box, md, isl, L, decoder_scale=0.01)

    def apply(p, state, sample):
        return O.gns_apply(p, sample[0], sample[1], num_mp_steps=L, skip_padding=True), state
    roll, _, _ = O.eval_batched_rollout(apply, case, params, {}, (p64[None], pt[None]), nbrs, n_rollout_steps=n_extra,
                                        t_window=isl)
    z = _Fixture(position=pos, particle_type=pt, metadata_json=np.array(json.dumps(md)), idx=np.asarray(nbrs.idx),
                 acc=O.gns_apply(params, feats, pt, num_mp_steps=L)["acc"], rollout=np.asarray(roll)[0],
                 num_mp_steps=np.array(L))
    for module, leaves in gns_params_to_haiku(params, L, 2).items():
        for leaf, v in leaves.items():
            z[f"param//{module}//{leaf}"] = np.asarray(v)
    return z


def _oracle_extras_fixture():
    """jax_extras.npz's dense-cell case, Sinkhorn pair and checkpoint (make_jax_golden.py extras) with the oracle's
    neighbor list, Sinkhorn divergences (OTT and POT formulations) and accelerations; the checkpoint files are written by
    this package's save_haiku."""
    import tempfile
    from lagrangebench_amd.utils import gns_params_to_haiku, save_haiku
    from oracle import sinkhorn_oracle as SK
    from oracle import sinkhorn_pot_oracle as SP
    G = _golden_generator()
    dim, n_side, isl, n_extra, dx, L = 2, 18, 6, 21, 0.02, 2
    pos, box = G._cloud(n_side, dim, dx, isl, n_extra, seed=11)
    n = len(pos)
    pt = np.zeros(n, np.int32)
    md = G._metadata(dim, n, box, dx, 3.0 * dx, isl + n_extra)
    case = _oracle_case(box, md, isl)
    feats, nbrs = case.allocate_eval((pos[:, :isl].astype(np.float64), pt))
    z = _Fixture()
    z["dense//position"] = pos
    z["dense//metadata_json"] = np.array(json.dumps(md))
    z["dense//idx"] = np.asarray(nbrs.idx)
    pred = np.transpose(pos[:, isl:], (1, 0, 2)).astype(np.float64)
    targ = np.mod(pred + np.random.default_rng(5).normal(0, 0.4 * dx, pred.shape), box)
    z["sinkhorn//pred"], z["sinkhorn//target"] = pred, targ
    z["sinkhorn//ott"] = SK.sinkhorn_rollout(case.displacement, pred, targ, 10)
    z["sinkhorn//pot"] = np.array([SP.sinkhorn_divergence_pot(case.displacement, p, t) for p, t in zip(pred[::10], targ[::10])])
    params = _oracle_params(box, md, isl, L, decoder_scale=1.0)
    with tempfile.TemporaryDirectory() as d:
        save_haiku(d, gns_params_to_haiku(params, L, 2), {}, None, {"step": 7, "loss": 0.5})
        for fn in sorted(os.listdir(d)):
            fp = os.path.join(d, fn)
            if os.path.isfile(fp):
                with open(fp, "rb") as f:
                    z[f"ckpt//{fn}"] = np.frombuffer(f.read(), dtype=np.uint8)
    z["ckpt//acc"] = O.gns_apply(params, feats, pt, num_mp_steps=L)["acc"]
    z["ckpt//num_mp_steps"] = np.array(L)
    return z


def test_oracle_fixtures_have_the_generators_layout():
    """The oracle-made fixtures the GPU consumers fall back to carry every key the generator writes that those consumers
    read, with the generator's shapes, and their weights / checkpoint read back through this package's readers."""
    import tempfile
    from lagrangebench_amd.utils import gns_params_from_haiku, load_haiku
    z = _oracle_gns_fixture()
    _, md, hk = _unpack(z)
    n, L = len(z["particle_type"]), int(z["num_mp_steps"])
    assert z["position"].shape == (n, 11, 3) and z["position"].dtype == np.float32 and md["dim"] == 3
    assert z["acc"].shape == (n, 3) and z["rollout"].shape == (5, n, 3) and z["idx"].shape[0] == 2
    assert np.isfinite(z["rollout"]).all() and np.abs(z["acc"]).max() > 0
    back = gns_params_from_haiku(hk, L, 2)
    ref = _oracle_params(np.array([b[1] - b[0] for b in md["bounds"]]), md, 6, L, 0.01)
    assert sorted(back) == sorted(ref) and all(np.array_equal(back[k][q], ref[k][q]) for k in ref for q in ref[k])
    x = _oracle_extras_fixture()
    assert {"dense//position", "dense//metadata_json", "dense//idx", "sinkhorn//pred", "sinkhorn//target", "sinkhorn//ott",
            "sinkhorn//pot", "ckpt//acc", "ckpt//num_mp_steps"} <= set(x.files)
    assert x["sinkhorn//ott"].shape == x["sinkhorn//pot"].shape == (3,) and (x["sinkhorn//ott"] > 0).all()
    with tempfile.TemporaryDirectory() as d:
        for k in x.files:
            if k.startswith("ckpt//") and k.count("//") == 1 and k.split("//")[1] not in ("acc", "num_mp_steps"):
                with open(os.path.join(d, k.split("//")[1]), "wb") as f:
                    f.write(x[k].tobytes())
        params_hk, _, _, step = load_haiku(d)
    assert step == 7 and len(gns_params_from_haiku(params_hk, int(x["ckpt//num_mp_steps"]), 2)) > 0
