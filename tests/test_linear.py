"""models.Linear off the device: parameter tree, blob, checkpoint names, the runner's construction, and the closed-form
gradient of the restatement (tests/_linear_oracle.py) that the device gradients are held to."""
import numpy as np
import pytest
import torch

from tests import _linear_oracle as LO


def _features(rng, N, dim, K, mag, bound, force):
    f = {"vel_hist": rng.standard_normal((N, K * dim))}
    if mag:
        f["vel_mag"] = np.abs(rng.standard_normal((N, K)))
    if bound:
        f["bound"] = rng.uniform(-1, 1, (N, 2 * dim))
    if force:
        f["force"] = rng.standard_normal((N, dim))
    return f


@pytest.mark.parametrize("dim,K,mag,bound,force,n_in", [
    (2, 5, True, False, True, 18),    # RPF2D with magnitudes: 10 + 5 + 2 + type
    (3, 5, True, True, False, 27),    # LDC3D in free space with magnitudes: 15 + 5 + 6 + type
    (3, 5, False, True, False, 22),
    (3, 2, False, False, False, 7),   # the LJ set, input_seq_length 3
    (3, 9, True, True, True, 46),     # the widest published case
])
def test_parameter_tree_and_blob(dim, K, mag, bound, force, n_in):
    from lagrangebench_amd.models import Linear
    rng = np.random.default_rng(0)
    f = _features(rng, 12, dim, K, mag, bound, force)
    model = Linear(dim)
    params, state = model.init(np.array([3]), (f, np.zeros(12, np.int64)))
    assert state == {} and set(params) == {"linear"} and set(params["linear"]) == {"w", "b"}
    w, b = params["linear"]["w"], params["linear"]["b"]
    assert w.shape == (n_in, dim) and w.dtype == np.float32 and b.shape == (dim,) and not b.any()
    assert np.abs(w).max() <= 2.0 / np.sqrt(n_in) and w.std() > 0   # truncated normal, std 1 / sqrt(fan_in), cut at 2 std
    params["linear"]["b"] = rng.standard_normal(dim).astype(np.float32)
    blob = model.flatten(params)
    assert blob.dtype == np.float32 and blob.shape == ((n_in + 1) * dim,)
    assert np.array_equal(blob[:n_in * dim].reshape(n_in, dim), w) and np.array_equal(blob[n_in * dim:], params["linear"]["b"])
    back = model.unflatten(blob, params)
    assert np.array_equal(back["linear"]["w"], w) and np.array_equal(back["linear"]["b"], params["linear"]["b"])
    assert np.array_equal(model.flatten(back), blob)
    p2, _ = model.init(np.array([3]), (f, np.zeros(12, np.int64)))
    assert np.array_equal(p2["linear"]["w"], w)   # the key decides


def test_haiku_round_trip(tmp_path):
    from lagrangebench_amd.models import Linear
    from lagrangebench_amd.utils import load_haiku, save_haiku
    model = Linear(3)
    params = model.init_params(5, 7)
    params["linear"]["b"] = np.arange(3, dtype=np.float32)
    hk = model.params_to_haiku(params)
    assert set(hk) == {"linear/~/linear"} and set(hk["linear/~/linear"]) == {"w", "b"}
    assert model.params_to_haiku(hk) is hk and model.params_from_haiku(params) is params
    save_haiku(str(tmp_path / "ckp"), hk, {}, None, {"step": 3, "loss": 1.0})
    loaded, state, _, step = load_haiku(str(tmp_path / "ckp"))
    assert step == 3 and set(loaded) == {"linear/~/linear"}
    back = model.params_from_haiku(loaded)
    assert np.array_equal(back["linear"]["w"], params["linear"]["w"]) and np.array_equal(back["linear"]["b"], params["linear"]["b"])
    with pytest.raises(ValueError, match="linear/~/linear"):
        model.params_from_haiku({"gns/~/x": {}})


def test_setup_model_builds_linear_and_still_refuses_painn():
    from lagrangebench_amd import models
    from lagrangebench_amd.runner import setup_model
    model, cls = setup_model({"model": {"name": "linear"}}, metadata={"dim": 3})
    assert cls is models.Linear and isinstance(model, models.Linear) and model._dim_out == 3
    model.check_trainable()
    assert model._PADDED_OK is False and model._FORWARD == "linear_forward" and model._OUTPUT == "acc"
    with pytest.raises(NotImplementedError) as e:
        setup_model({"model": {"name": "painn"}}, metadata={"dim": 3})
    assert str(e.value) == "model 'painn': 'gns', 'segnn' and 'egnn' are built (painn/linear are not built)"
    with pytest.raises(NotImplementedError, match="painn/linear are not built"):
        setup_model({"model": {"name": "mlp"}}, metadata={"dim": 3})


def test_wider_than_one_node_row_is_refused():
    from lagrangebench_amd.models import Linear
    model = Linear(3)
    f = {"vel_hist": np.zeros((4, 63))}
    assert model.init(None, (f, np.zeros(4, np.int64)))[0]["linear"]["w"].shape == (64, 3)
    f = {"vel_hist": np.zeros((4, 64))}
    with pytest.raises(NotImplementedError, match="65 inputs"):
        model.init(None, (f, np.zeros(4, np.int64)))
    with pytest.raises(NotImplementedError):
        model.flatten({"linear": {"w": np.zeros((65, 3), np.float32), "b": np.zeros(3, np.float32)}})


@pytest.mark.parametrize("dim,K,mag,bound,force", [(2, 5, True, False, True), (3, 5, True, True, False), (3, 2, False, False, False)])
def test_closed_form_gradient_equals_autograd(dim, K, mag, bound, force):
    """2 / n_nk X^T (M * (X W + b - T)) against float64 autograd of the restatement, kinematic particles included: 1e-12
    relative (both are float64 sums of the same terms in different orders)."""
    rng = np.random.default_rng(2)
    N = 57
    f = _features(rng, N, dim, K, mag, bound, force)
    pt = rng.choice([0, 1, 2, 5, -1], size=N)
    n_in = LO.concat(f, pt).shape[1]
    w = torch.tensor(rng.standard_normal((n_in, dim)), requires_grad=True)
    b = torch.tensor(rng.standard_normal(dim), requires_grad=True)
    tgt = rng.standard_normal((N, dim))
    loss = LO.mse(LO.linear_forward(w, b, f, pt), tgt, pt)
    loss.backward()
    l_cf, dw, db = LO.closed_form(w.detach().numpy(), b.detach().numpy(), f, pt, tgt)
    assert abs(l_cf.item() - loss.item()) <= 1e-12 * abs(loss.item())
    assert (dw - w.grad).abs().max() <= 1e-12 * w.grad.abs().max()
    assert (db - b.grad).abs().max() <= 1e-12 * b.grad.abs().max()
    kin = ~LO.non_kinematic(pt).numpy()
    assert kin.any() and not kin.all()
    # the type column enters as a value: its row of dW is the type-weighted residual sum
    assert dw[-1].abs().max() > 0
