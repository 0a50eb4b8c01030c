"""SEGNN (lmax 1): the oracle's O(3)-equivariance (the reference's own SEGNN test,
tests/models_test.py:70-87) on CPU; HIP forward / rollout against the oracle on the GPU.

Parity with e3nn-jax itself is unpinned (oracle/segnn_oracle.py header): tolerance 1e-5 relative
to the largest output, HIP fp32 MFMA vs NumPy fp32."""
import numpy as np
import pytest
import torch

from oracle import lb_oracle as O
from oracle import segnn_oracle as S
from tests._common import elementwise_stats, hip_case, oracle_case, rel_err


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ------------------------------------------------------------------------------- CPU
def _random_graph_features(R, n=40, K=5, E=200):
    r = np.random.default_rng(1)
    vh = r.standard_normal((n, K, 3))
    force = r.standard_normal((n, 3))
    bound = r.standard_normal((n, 2, 3))
    s = np.concatenate([r.integers(0, n, E), np.arange(n)])
    rc = np.concatenate([r.integers(0, n, E), np.arange(n)])
    rd = r.standard_normal((E + n, 3))
    rd[E:] = 0  # self edges
    vh, force, bound, rd = vh @ R.T, force @ R.T, bound @ R.T, rd @ R.T
    return {"vel_hist": vh.reshape(n, -1), "vel_mag": np.linalg.norm(vh, axis=-1), "force": force,
            "bound": np.concatenate([bound[:, 0], bound[:, 1]], -1), "rel_disp": rd,
            "rel_dist": np.linalg.norm(rd, axis=-1, keepdims=True), "senders": s, "receivers": rc}


def test_oracle_is_o3_equivariant():
    from scipy.stats import ortho_group
    n, K = 40, 5
    pt = np.random.default_rng(2).integers(0, 3, n)
    p = S.segnn_init(np.random.default_rng(0), node_ns=K + 9, node_nv=K + 3, num_mp_steps=3, random_bias=True)
    out0 = S.segnn_apply(p, _random_graph_features(np.eye(3)), pt, K, False)["acc"]
    assert np.abs(out0).max() > 1e-3
    dets = []
    for seed in range(4):
        R = ortho_group.rvs(3, random_state=seed)
        dets.append(np.sign(np.linalg.det(R)))
        out1 = S.segnn_apply(p, _random_graph_features(R), pt, K, False)["acc"]
        assert np.abs(out1 - out0 @ R.T).max() < 2e-6 * max(1.0, np.abs(out0).max())
    assert -1 in dets and 1 in dets  # reflections and rotations both covered


def test_gate_normalisation_constants():
    from scipy.integrate import quad
    g = lambda z: np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    m_silu = quad(lambda z: (z / (1 + np.exp(-z))) ** 2 * g(z), -12, 12)[0]
    m_sig = quad(lambda z: (1 / (1 + np.exp(-z))) ** 2 * g(z), -12, 12)[0]
    # the oracle follows e3nn's 1e6-point quantile grid, which clips the tails: ~2e-5 off the integral
    assert abs(S.C_SILU - m_silu ** -0.5) < 1e-4
    assert abs(S.C_SIGMOID - m_sig ** -0.5) < 1e-4


def test_spherical_harmonics_l1():
    v = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0]])
    y = S.spherical_harmonics(v)
    assert np.allclose(y[0], [0.5 / np.sqrt(np.pi), 0, 0, 0])
    assert np.allclose(y[1, 1:], np.sqrt(3 / (4 * np.pi)) * np.array([0.6, 0.0, 0.8]), atol=1e-7)
    # "integral" normalisation: sum_m Y_1m^2 = 3 / (4 pi)
    assert np.isclose((y[1, 1:] ** 2).sum(), 3 / (4 * np.pi), atol=1e-7)


def test_tensor_product_component_normalisation():
    """e3nn's irrep_normalization="component" (A3) is DEFINED by: unit-variance inputs give
    unit-variance output components on every path.  Checks the 1/sqrt(3) of 1o x 1o -> 0e and the
    unit factors of the other three paths; then the "element" Linear (A4) keeps that variance for
    U(-1,1)*sqrt(3) (unit-variance) weights."""
    rng = np.random.default_rng(0)
    R, C = 20000, 8
    x = S.SV(rng.standard_normal((R, C)), rng.standard_normal((R, C, 3)))
    attr = rng.standard_normal((R, 4)).astype(np.float32)
    xs, xv = S.tp_inputs([x], attr)
    var_s = xs.var(axis=0)          # [s*a0 (C) | (v.a)/sqrt3 (C)]
    var_v = xv.var(axis=(0, 2))     # [s*a_c (C) | v_c*a0 (C)]
    assert np.allclose(var_s, 1.0, atol=0.08) and np.allclose(var_v, 1.0, atol=0.08)
    p = {"ws": (rng.uniform(-1, 1, (2 * C, 64)) * np.sqrt(3)).astype(np.float32),
         "wv": (rng.uniform(-1, 1, (2 * C, 64)) * np.sqrt(3)).astype(np.float32), "b": np.zeros(64, np.float32)}
    out = S.o3_tensor_product(p, [x], attr)
    assert abs(out.s.var() - 1.0) < 0.15 and abs(out.v.var() - 1.0) < 0.15


def test_model_shapes_match_oracle():
    from lagrangebench_amd.models import SEGNN, node_irreps
    from lagrangebench_amd.models.segnn import parse_irreps
    md = {"periodic_boundary_conditions": [False, False]}
    irr = node_irreps(md, 6, True, True, False)
    assert irr == "5x1o+2x1o+1x1o+5x0e+9x0e"
    assert parse_irreps(irr) == (14, 8)
    m = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=3, n_vels=5, homogeneous_particles=False)
    p = S.segnn_init(np.random.default_rng(0), node_ns=14, node_nv=8, num_mp_steps=3)
    for name, K, ms, mv in m.block_shapes():
        assert p[name]["ws"].shape == (K, ms) and p[name]["wv"].shape == (K, mv), name
    assert m.flatten(p).size == sum(v["ws"].size + v["wv"].size + v["b"].size
                                    for v in p.values() if isinstance(v, dict))
    # (round 5: lmax 2 and the norm switches are built - tests/test_segnn_irreps.py; they take the general-irreps kernels)
    assert SEGNN(irr, "1x1o+1x0e", 64, 2, 1, "1x1o", 3, 5).generic
    assert SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", 3, 5, norm="instance").generic
    assert not m.generic
    with pytest.raises(NotImplementedError):
        SEGNN(irr, "1x1o+1x0e", 64, 3, 1, "1x1o", 3, 5)


# ------------------------------------------------------------------------------- GPU
def _setup(name, scale, L, magnitudes=True, seed=7, out_scale=1.0):
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps
    ds = make_case(name, n_trajs=2, extra_seq_length=6, scale=scale)
    ds.magnitude_features = magnitudes
    isl = ds.input_seq_length
    homog = bool(np.all(ds[0][1] == 0))
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, magnitudes, homog)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=L, n_vels=isl - 1,
                  homogeneous_particles=homog)
    params = S.segnn_init(np.random.default_rng(seed), node_ns=model._node_ns, node_nv=model._node_nv,
                          num_mp_steps=L, random_bias=True)
    params["output"]["wv"] = (params["output"]["wv"] * out_scale).astype(np.float32)
    return ds, model, params, homog


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale,L,mag", [("small2d", 1.0, 2, True), ("small3d", 1.0, 3, True),
                                              ("dam2d", 0.3, 3, True), ("rpf2d", 0.5, 10, False),
                                              ("ldc3d", 0.5, 2, True)])
def test_segnn_forward_parity(name, scale, L, mag):
    _need_gpu()
    ds, model, params, homog = _setup(name, scale, L, mag)
    pos = np.stack([ds[0][0], ds[1][0]])
    pt = np.stack([ds[0][1], ds[1][1]])
    _segnn_parity(ds, model, params, homog, pos, pt, name)


def _segnn_parity(ds, model, params, homog, pos, pt, name):
    """lmax-1 SEGNN forward of a batch of two on the engine (hidden-state taps, acceleration) against the float32 oracle
    and element-wise against its float64 evaluation.  Returns the accelerations."""
    ocase, hcase = oracle_case(ds), hip_case(ds)
    isl = ds.input_seq_length
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    handle = model.handle(eng, params)
    tap = handle.set_tap(True)
    pred, _ = model.apply(params, {}, (feats, pt))
    acc, tap = _np(pred["acc"]), _np(tap)
    N = pos.shape[1]
    for b in range(2):
        of, _ = ocase.allocate_eval((pos[b][:, :isl].astype(np.float64), pt[b]))
        ref, lat = S.segnn_apply(params, of, pt[b], isl - 1, homog, return_latents=True)
        for k, f in enumerate(lat):
            got = tap[k][b * N:(b + 1) * N]
            want = np.concatenate([f.s, f.v[:, :, 0], f.v[:, :, 1], f.v[:, :, 2]], axis=1)
            assert rel_err(got, want) < 1e-5, f"hidden state {k}"
        assert rel_err(acc[b], ref["acc"]) < 1e-5
        # element-wise (the max-norm lets an entry 100x below the largest be 1e-3 off).  Yardstick =
        # the same restatement in float64; bar = 4x what the float32 restatement itself achieves against it (f16x2 products
        # carry 2^-22, fp32 products 2^-24; entries below 1e-3 of the largest are differences of O(1) terms: no float32
        # evaluation keeps 1e-5 relative there).
        with S.precision(np.float64):
            truth = S.segnn_apply(params, of, pt[b], isl - 1, homog)["acc"]
        assert truth.dtype == np.float64
        p999_h, max_h, n_h = elementwise_stats(acc[b], truth)
        p999_o, max_o, _ = elementwise_stats(ref["acc"], truth)
        print(f"[elementwise segnn {name} b={b}] engine vs f64: p99.9 {p999_h:.2e} max {max_h:.2e} | f32 oracle vs f64: "
              f"p99.9 {p999_o:.2e} max {max_o:.2e} ({n_h} entries)")
        # measured (round 4): engine p99.9 8e-6 .. 1.2e-4, float32 restatement 5e-6 .. 7e-5 on the same entries: 1 - 2x on
        # four cases, 4.4x on small2d (the gates run on v_exp_f32 / v_rcp_f32, ~1 ulp each, the restatement on libm).  The
        # absolute floors are for that case; all of it is 1e-7 of the largest acceleration in absolute terms.
        assert p999_h <= max(4.0 * p999_o, 2e-4), (p999_h, p999_o)
        assert max_h <= max(4.0 * max_o, 5e-4), (max_h, max_o)
    handle.set_tap(False)
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale,L", [("dam2d", 0.3, 3), ("small3d", 1.0, 2)])
def test_segnn_forward_parity_float32_geometry(name, scale, L):
    """dtype=float32 (case.py:169; VERDICT r03 missing item 3: float32 geometry for SEGNN, incl. DAM2D's external force):
    the engine's float32 geometry feeds the SEGNN transform and network; against the oracle run in float32."""
    _need_gpu()
    ds, model, params, homog = _setup(name, scale, L, True)
    ocase, hcase = oracle_case(ds, dtype=np.float32), hip_case(ds, dtype="float32")
    isl = ds.input_seq_length
    pos, pt = ds[0]
    feats, nbrs = hcase.allocate_eval((pos[None, :, :isl], pt[None]))
    pred, _ = model.apply(params, {}, (feats, pt[None]))
    acc = _np(pred["acc"])[0]
    of, _ = ocase.allocate_eval((pos[:, :isl].astype(np.float32), pt))
    if ds.external_force_fn is not None:
        assert np.array_equal(_np(feats["force"])[0].astype(np.float32), np.asarray(of["force"], np.float32))
    ref = S.segnn_apply(params, of, pt, isl - 1, homog)
    assert rel_err(acc, ref["acc"]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3])
def test_segnn_other_block_depths(blocks):
    """blocks_per_step != 2 (configs use 2) runs through the per-block kernel instead of the fused
    message / update kernels."""
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps
    ds = make_case("small3d", n_trajs=1, extra_seq_length=2)
    ds.magnitude_features = True
    isl = ds.input_seq_length
    irr = node_irreps(ds.metadata, isl, False, True, True)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=isl - 1, blocks_per_step=blocks)
    params = S.segnn_init(np.random.default_rng(3), node_ns=model._node_ns, node_nv=model._node_nv,
                          num_mp_steps=2, blocks_per_step=blocks, random_bias=True)
    ocase, hcase = oracle_case(ds), hip_case(ds)
    pos, pt = ds[0]
    feats, _ = hcase.allocate_eval((pos[:, :isl], pt))
    acc = _np(model.apply(params, {}, (feats, pt))[0]["acc"])
    of, _ = ocase.allocate_eval((pos[:, :isl].astype(np.float64), pt))
    ref = S.segnn_apply(params, of, pt, isl - 1, True)["acc"]
    assert rel_err(acc, ref) < 1e-5


@pytest.mark.gpu
def test_segnn_forward_is_bitwise_deterministic():
    """No atomics, fixed summation order: repeated forwards must agree bit for bit.  (Also the
    regression test for the MFMA accumulate-chain spacing issue described in DESIGN.md: it showed up
    as rare, run-to-run varying 1e-3 errors in single 16-edge tiles.)"""
    _need_gpu()
    ds, model, params, homog = _setup("small2d", 1.0, 3, True)
    hcase = hip_case(ds)
    isl = ds.input_seq_length
    pos = np.stack([ds[0][0], ds[1][0]])
    pt = np.stack([ds[0][1], ds[1][1]])
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    handle = model.handle(feats.engine, params)
    tap = handle.set_tap(True)
    ref = None
    for _ in range(12):
        model.apply(params, {}, (feats, pt))
        cur = _np(tap).copy()
        if ref is None:
            ref = cur
        assert np.array_equal(cur, ref)
    handle.set_tap(False)


@pytest.mark.gpu
def test_segnn_full_size_dam2d_properties():
    """BASELINE.json configs[4] at full size (DamBreak2D, SEGNN-10-64, free surface): the oracle is
    too slow here, so size-independent properties are checked on a 20-step device rollout:
    bitwise determinism, batch consistency, kinematic particles follow the ground truth, finite."""
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps
    n_steps = 20
    ds = make_case("dam2d", n_trajs=2, extra_seq_length=n_steps)
    ds.magnitude_features = True
    isl = ds.input_seq_length
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, False)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=10, n_vels=isl - 1, homogeneous_particles=False)
    params = model.init_params(5)
    params["output"]["wv"] = (params["output"]["wv"] * 0.01).astype(np.float32)
    hcase = hip_case(ds)
    pos = np.stack([ds[0][0], ds[1][0]])
    pt = np.stack([ds[0][1], ds[1][1]])
    dx = 1.0 / 80

    def run(p, t):
        eng = hcase.engine(p.shape[0])
        eng.set_particle_type(t)
        traj = eng.prepare_traj(p)
        return _np(eng.rollout(model.handle(eng, params), traj, n_steps)[0])

    a = run(pos, pt)
    b = run(pos, pt)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)                                   # deterministic, bit for bit
    solo = run(pos[:1], pt[:1])
    assert np.array_equal(solo[0], a[0])                          # slot 0: same tiles, same bits
    solo1 = run(pos[1:], pt[1:])
    assert np.abs(solo1[0] - a[1]).max() < 1e-6 * dx              # slot 1: other tile boundaries
    kin = (pt[0] == 1) | (pt[0] == 2)
    assert kin.any()
    truth = np.transpose(pos[0][:, isl:isl + n_steps], (1, 0, 2))  # (T, N, dim)
    assert np.array_equal(a[0][:, kin], truth[:, kin])            # walls take the target positions
    assert np.abs(a[0][:, ~kin] - truth[:, ~kin]).max() < 0.5     # fluid stays in the box scale


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale", [("small2d", 1.0), ("dam2d", 0.3)])
def test_segnn_rollout_parity(name, scale):
    """lb_segnn_rollout (device step loop) against the oracle's eval loop, 5 steps."""
    _need_gpu()
    from lagrangebench_amd.evaluate.rollout import _eval_batched_rollout, _forward_eval
    from functools import partial
    ds, model, params, homog = _setup(name, scale, 2, True, out_scale=0.02)
    ocase, hcase = oracle_case(ds), hip_case(ds)
    isl = ds.input_seq_length
    n_steps = 5
    pos = np.stack([ds[0][0], ds[1][0]])
    pt = np.stack([ds[0][1], ds[1][1]])
    feats, nbrs = hcase.allocate_eval((pos[:, :, :isl], pt))
    fwd = partial(_forward_eval, model_apply=model.apply, case_integrate=hcase.integrate)
    fwd._lb_gns = model
    metrics = lambda pred, target: {}
    pred, _, _ = _eval_batched_rollout(fwd, hcase.preprocess_eval, hcase, params, {}, (pos, pt), nbrs,
                                       metrics, n_steps, isl)
    pred = _np(pred)

    def oracle_apply(p, state, sample):
        f, ptype = sample
        return S.segnn_apply(p, f, ptype, isl - 1, homog), state

    for b in range(2):
        _, onbrs = ocase.allocate_eval((pos[b][:, :isl].astype(np.float64), pt[b]))
        ref, _, _ = O.eval_batched_rollout(oracle_apply, ocase, params, {}, (pos[b:b + 1], pt[b:b + 1]), onbrs,
                                           n_steps, isl)
        dx = float(ds.metadata["dx"]) if "dx" in ds.metadata else 1.0 / 16
        assert np.abs(pred[b] - np.asarray(ref)[0]).max() < 1e-6 * dx


@pytest.mark.gpu
@pytest.mark.parametrize("sym", ["cycle_xyz", "reflect_x", "swap_xy_reflect_z"])
def test_segnn_engine_is_equivariant_under_box_symmetries(sym):
    """The reference pins its equivariant models through an equivariance property (tests/models_test.py:70-87:
    rotate the inputs, the outputs rotate with them).  Here on the whole ENGINE path - neighbor search, features,
    SEGNN on the HIP kernels - with the symmetries a cubic periodic box admits (axis permutations, reflections):
    transforming the position window must transform the predicted accelerations, up to fp32 re-association of
    the sums (the cell hashing, hence the edge order inside the tiles, changes with the transform)."""
    _need_gpu()
    ds, model, params, homog = _setup("small3d", 1.0, 3, True)
    assert ds.external_force_fn is None and bool(np.all(np.asarray(ds.metadata["periodic_boundary_conditions"])))
    box = np.asarray(ds.box, np.float64)
    assert np.allclose(box, box[0])          # cubic: the transforms below map the box onto itself
    isl = ds.input_seq_length
    pos, pt = ds[0][0].astype(np.float64), ds[0][1]
    perm, sign = {"cycle_xyz": ([1, 2, 0], [1, 1, 1]), "reflect_x": ([0, 1, 2], [-1, 1, 1]),
                  "swap_xy_reflect_z": ([1, 0, 2], [1, 1, -1])}[sym]
    sign = np.asarray(sign, np.float64)

    def transform_pos(p):       # p (N, T, 3) -> R p  (reflections about the box centre, positions stay in [0, L))
        q = p[..., perm]
        return np.where(sign < 0, np.mod(box[0] - q, box[0]), q)

    def acc_of(p):
        feats, _ = hip_case(ds).allocate_eval((p[None, :, :isl], pt[None]))
        pred, _ = model.apply(params, {}, (feats, pt[None]))
        return _np(pred["acc"])[0].astype(np.float64)
    a0 = acc_of(pos)
    a1 = acc_of(transform_pos(pos))
    want = a0[:, perm] * sign
    assert rel_err(a1, want) < 2e-5, (sym, rel_err(a1, want))
    assert rel_err(a1, a0) > 1e-2           # the transform is not a no-op for this model / input
