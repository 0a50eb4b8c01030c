"""PaiNN on the host: parameter tree, layouts, checkpoint mapping, the refusals, and the torch restatement's own
properties (O(3) equivariance, precision, the direction of the sender sum)."""
import numpy as np
import pytest
import torch

from tests._painn_oracle import painn_forward, random_biases


def _painn(H=128, L=5, n_vels=5, radius=0.054, **kw):
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    trainable = kw.pop("trainable", True)
    return PaiNN(H, 1, L, gaussian_rbf(20, radius, trainable=trainable), cosine_cutoff(radius), n_vels, **kw)


def test_param_tree_rpf2d_painn_5_128():
    """runner.py:270-284 on RPF2D (n_vels 5, external force, periodic: no boundary features)."""
    m = _painn()
    p, state = m.init_params(3, has_force=True)
    assert sum(v.size for leaves in p.values() for v in leaves.values()) == 1010218
    assert m.flatten(p, state).size == 1010218
    H = 128
    assert p["scalar_embedding"]["w"].shape == (5, H) and p["vector_embedding"]["w"].shape == (6, H)
    assert set(p["vector_embedding"]) == {"w"}
    assert p["filter_net"]["w"].shape == (20, 5 * 3 * H)
    assert p["readout_0/gate_0"]["w"].shape == (H + H // 2, H)
    assert p["readout_out/gate_0"]["w"].shape == (H // 2 + 1, H // 2)
    assert p["readout_out/gate_1"]["w"].shape == (H // 2, 2)
    np.testing.assert_array_equal(p["~"]["offset"], np.linspace(0, 0.054, 20, dtype=np.float32))
    np.testing.assert_allclose(p["~"]["widths"], 0.054 / 20, rtol=1e-6)
    assert state["~"]["cutoff"] == np.float32(0.054)
    for mod, leaves in p.items():
        if mod == "~":
            continue
        if "b" in leaves:
            assert not leaves["b"].any(), mod
        w = leaves["w"]
        lim = np.sqrt(6.0 / (w.shape[0] + w.shape[1]))
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.5 * lim, mod


@pytest.mark.parametrize("kw", [{}, {"shared_filters": True}, {"shared_interactions": True},
                                {"trainable": False, "homogeneous_particles": False}])
def test_flatten_and_haiku_round_trip(tmp_path, kw):
    from lagrangebench_amd.utils import load_haiku, painn_params_from_haiku, painn_params_to_haiku, save_haiku
    m = _painn(H=32, L=3, n_vels=3, **dict(kw))
    has_force, has_bound = not kw, bool(kw)
    p, state = m.init_params(1, has_force, has_bound)
    p = random_biases(p, 2)
    blob = m.flatten(p, state)
    back, st2 = m.unflatten(blob, has_force, has_bound)
    assert np.array_equal(m.flatten(back, st2), blob)
    n_sets = 1 if kw.get("shared_interactions") else 3
    assert sum(k.startswith("layer_") and k.endswith("/mixing_0") for k in p) == n_sets
    assert p["filter_net"]["w"].shape[1] == (1 if kw.get("shared_filters") else 3) * 3 * 32
    assert ("~" in p) == kw.get("trainable", True)
    hk = painn_params_to_haiku(p, m)
    assert "painn/~/scalar_embedding" in hk and "painn/~/filter_net" in hk
    assert set(hk["painn/~/layer_0/~/vector_mixing_block"]) == {"w"}
    assert "painn/~/layer_0/~/linear_xav_3" in hk and "painn/readout_block_out/~/vector_mix_net" in hk
    assert "painn/readout_block_0/~/linear_xav_1" in hk
    assert (f"painn/~/layer_{n_sets}/~/linear_xav" not in hk) and f"painn/~/layer_{n_sets - 1}/~/linear_xav" in hk
    if "~" in p:
        assert set(hk["~"]) == {"widths", "offset"}
    save_haiku(str(tmp_path / "ckp"), hk, state, None, {"step": 0})
    hk2, st3, _, _ = load_haiku(str(tmp_path / "ckp"))
    p2 = painn_params_from_haiku(hk2, m)
    assert np.array_equal(m.flatten(p2, st3), blob)


def test_refusals():
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    rbf, cut = gaussian_rbf(20, 1.0, trainable=True), cosine_cutoff(1.0)
    with pytest.raises(NotImplementedError, match="activation"):
        PaiNN(64, 1, 2, rbf, cut, 5, activation=torch.nn.functional.relu)
    with pytest.raises(NotImplementedError, match="output_size"):
        PaiNN(64, 3, 2, rbf, cut, 5)
    with pytest.raises(NotImplementedError, match="centered"):
        gaussian_rbf(20, 1.0, centered=True)
    for H in (24, 144):
        with pytest.raises(NotImplementedError, match="hidden_size"):
            PaiNN(H, 1, 2, rbf, cut, 5)
    PaiNN(64, 1, 2, rbf, None, 5, activation="silu")  # cutoff_fn None is built


def test_trainer_refuses_painn():
    from lagrangebench_amd.train.trainer import Trainer
    with pytest.raises(NotImplementedError, match="no device training step"):
        Trainer(_painn(H=32, L=2), None, None, None)


def test_runner_painn_still_refused():
    from lagrangebench_amd.runner import setup_model
    with pytest.raises(NotImplementedError, match="painn/linear are not built"):
        setup_model({"model": {"name": "painn"}}, metadata={"dim": 2})


def _random_graph(N, dim, n_vels, seed, with_bound=True):
    r = np.random.default_rng(seed)
    vel = r.standard_normal((N, n_vels, dim))
    s, q = np.nonzero(~np.eye(N, dtype=bool))
    pos = r.uniform(0, 1, (N, dim))
    f = {"vel_hist": vel.reshape(N, -1), "vel_mag": np.linalg.norm(vel, axis=-1),
         "force": r.standard_normal((N, dim)), "senders": s, "receivers": q, "rel_disp": pos[s] - pos[q]}
    if with_bound:
        f["bound"] = r.uniform(-1, 1, (N, 2 * dim))
    return f


def _rotate(f, R):
    g = dict(f)
    N, dim = f["vel_hist"].shape[0], R.shape[0]
    g["vel_hist"] = (f["vel_hist"].reshape(N, -1, dim) @ R.T).reshape(N, -1)
    g["force"] = f["force"] @ R.T
    g["rel_disp"] = f["rel_disp"] @ R.T
    return g


def test_restatement_equivariance_and_precision():
    """Rotations and reflections of the vector inputs rotate the acceleration (no boundary features: they are
    axis-aligned and not equivariant); fp32 agrees with fp64."""
    m = _painn(H=32, L=3, n_vels=3, radius=1.5)
    p, state = m.init_params(4, True, False)
    p = random_biases(p, 5)
    kw = dict(num_mp_steps=3, n_vels=3, rbf=m._rbf(p, state), cutoff=1.5)
    f = _random_graph(12, 3, 3, 6, with_bound=False)
    _, _, a = painn_forward(p, f, np.zeros(12, int), dtype=torch.float64, **kw)
    q, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((3, 3)))
    for R in (q, -q):
        _, _, ar = painn_forward(p, _rotate(f, R), np.zeros(12, int), dtype=torch.float64, **kw)
        np.testing.assert_allclose(ar.numpy(), a.numpy() @ R.T, atol=1e-12 * max(1.0, float(a.abs().max())))
    _, _, a32 = painn_forward(p, f, np.zeros(12, int), dtype=torch.float32, **kw)
    assert float((a32.double() - a).abs().max() / a.abs().max()) < 1e-4
    assert float(a.abs().max()) > 0


def test_restatement_sender_sum_direction():
    """One directed edge (sender 0, receiver 1): the message is built from the RECEIVER's x and v and lands on the
    SENDER (painn.py:297-303)."""
    m = _painn(H=16, L=1, n_vels=2, radius=1.5)
    p, state = m.init_params(8, True, False)
    p = random_biases(p, 9)
    kw = dict(num_mp_steps=1, n_vels=2, rbf=m._rbf(p, state), cutoff=1.5)
    f = _random_graph(2, 2, 2, 10, with_bound=False)
    f["senders"], f["receivers"] = np.array([0]), np.array([1])
    f["rel_disp"] = np.array([[0.3, -0.4]])
    s0, v0, _ = painn_forward(p, {**f, "senders": np.array([], int), "receivers": np.array([], int),
                                  "rel_disp": np.zeros((0, 2))}, np.zeros(2, int), dtype=torch.float64, **kw)
    s1, v1, _ = painn_forward(p, f, np.zeros(2, int), dtype=torch.float64, **kw)
    assert not torch.equal(s1[1][0], s0[1][0]) and not torch.equal(v1[1][0], v0[1][0])  # the sender moved
    assert torch.equal(s1[1][1], s0[1][1]) and torch.equal(v1[1][1], v0[1][1])          # the receiver did not
    # node 0's message uses node 1's features: changing node 0's own inputs only changes it through its own update
    g = dict(f)
    g["vel_hist"] = f["vel_hist"].copy()
    g["vel_hist"][1] *= 2.0
    g["vel_mag"] = f["vel_mag"].copy()
    g["vel_mag"][1] *= 2.0
    s2, _, _ = painn_forward(p, g, np.zeros(2, int), dtype=torch.float64, **kw)
    h0, _, _ = painn_forward(p, {**g, "senders": np.array([], int), "receivers": np.array([], int),
                                 "rel_disp": np.zeros((0, 2))}, np.zeros(2, int), dtype=torch.float64, **kw)
    assert torch.equal(h0[1][0], s0[1][0]) and not torch.equal(s2[1][0], s1[1][0])
