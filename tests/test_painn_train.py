"""PaiNN training without a device (csrc/lb_train_painn.h's yardstick and the Python binding).

The float64 torch restatement of the reference (tests/_painn_oracle.py) under the masked _mse (train/trainer.py:35-60) is
differentiated by autograd and checked against central finite differences: the gradients the device step is then held to
(tests/test_painn_train_gpu.py).  Then the refusals, the symbol the training handle is created through, and the
unflatten(blob, like) form the Trainer and DeviceModule use."""
import numpy as np
import pytest
import torch

from tests._painn_oracle import random_biases
from tests._painn_train import oracle_kw, painn_loss, tparams
from tests.test_painn import _random_graph


def _painn(H=16, L=2, n_vels=3, radius=1.5, trainable=True, **kw):
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    return PaiNN(H, 1, L, gaussian_rbf(20, radius, trainable=trainable), cosine_cutoff(radius), n_vels, **kw)


def test_restatement_loss_gradients_match_finite_differences():
    N, dim, n_vels, L = 10, 3, 3, 2
    m = _painn(16, L, n_vels)
    params, state = m.init_params(4, True, True)
    params = random_biases(params, 5)
    f = _random_graph(N, dim, n_vels, 6)
    pt = np.zeros(N, np.int64)
    pt[3] = 1   # one kinematic particle: masked out of the loss
    rng = np.random.default_rng(7)
    tg = rng.standard_normal((N, dim))
    tp = tparams(params)
    loss, _ = painn_loss(tp, f, pt, tg, **oracle_kw(m, tp, state))
    loss.backward()
    checked = 0
    leaves = [("scalar_embedding", "w"), ("scalar_embedding", "b"), ("vector_embedding", "w"), ("filter_net", "w"),
              ("filter_net", "b"), ("layer_0/interaction_0", "w"), ("layer_1/interaction_1", "w"),
              ("layer_0/interaction_1", "b"), ("layer_0/mixing_0", "w"), ("layer_1/mixing_1", "w"), ("layer_1/mixing_0", "b"),
              ("layer_0/vector_mixing", "w"), ("layer_1/vector_mixing", "w"), ("readout_0/vector_mix", "w"),
              ("readout_0/gate_0", "w"), ("readout_0/gate_1", "w"), ("readout_0/gate_1", "b"), ("readout_out/vector_mix", "w"),
              ("readout_out/gate_0", "w"), ("readout_out/gate_0", "b"), ("readout_out/gate_1", "w"), ("~", "widths"),
              ("~", "offset")]
    for mod, leaf in leaves:
        g = tp[mod][leaf].grad.numpy().ravel()
        v = tp[mod][leaf].detach().numpy().ravel()
        assert np.abs(g).max() > 0, (mod, leaf)
        for j in rng.choice(v.size, size=min(2, v.size), replace=False):
            vals = []
            for sgn in (1, -1):
                p2 = {a: {b: x.detach().clone() for b, x in lv.items()} for a, lv in tp.items()}
                p2[mod][leaf].view(-1)[j] += sgn * 1e-6
                vals.append(float(painn_loss(p2, f, pt, tg, **oracle_kw(m, p2, state))[0]))
            fd = (vals[0] - vals[1]) / 2e-6
            assert abs(fd - g[j]) <= 1e-5 * max(1.0, abs(g).max()), (mod, leaf, j, fd, g[j])
            checked += 1
    assert checked >= 30


def test_check_trainable_by_hidden_size():
    from lagrangebench_amd.train import Trainer
    for H in (64, 128):
        _painn(H).check_trainable()
    small = _painn(32)
    with pytest.raises(NotImplementedError, match="no device training step"):
        small.check_trainable()
    with pytest.raises(NotImplementedError, match="no device training step"):
        small.train_handle(None, None)
    with pytest.raises(NotImplementedError, match="no device training step"):
        Trainer(small, None, None, None)


class _StubEngine:
    has_pads = False

    def __init__(self):
        self.created = []

    def _new_handle(self, cls, symbol, desc, blob, *extra):
        self.created.append((cls, symbol, desc, np.array(blob), extra))
        return self.created[-1]


@pytest.mark.parametrize("trainable", [True, False])
def test_train_handle_is_created_through_lb_painn_train_create(trainable):
    from lagrangebench_amd import _lib
    from lagrangebench_amd.engine import GnsTrainHandle
    m = _painn(64, 2, trainable=trainable)
    params, state = m.init_params(1, True, False)
    if not trainable:
        state["~"]["widths"] = state["~"]["widths"] * 1.5   # the frozen basis the handle must carry
    eng = _StubEngine()
    m.train_handle(eng, params, state)
    (cls, symbol, desc, blob, extra), = eng.created
    assert symbol == "lb_painn_train_create" and issubclass(cls, GnsTrainHandle)
    assert extra == (int(trainable),) and desc.hidden == 64
    assert np.array_equal(blob, m.flatten(params, state))
    # the table entry the call goes through: (engine, desc, weights, n_floats, rbf_trainable, &handle)
    assert len(_lib._SIGS["lb_painn_train_create"][1]) == 6 and len(_lib._SIGS["lb_painn_train_model"][1]) == 2


@pytest.mark.parametrize("trainable", [True, False])
def test_unflatten_like_round_trip(trainable):
    m = _painn(64, 3, trainable=trainable, shared_filters=True)
    params, state = m.init_params(2, True, True)
    params = random_biases(params, 3)
    assert ("~" in params) == trainable
    blob = m.flatten(params, state)
    for tree in (m.unflatten(blob, params), m.unflatten(blob, like=params)):
        assert set(tree) == set(params)
        for mod, lv in params.items():
            for leaf, v in lv.items():
                assert np.array_equal(tree[mod][leaf], v), (mod, leaf)
        assert np.array_equal(m.flatten(tree, state), blob)
    p2, s2 = m.unflatten(blob, True, True)   # the earlier form stays
    assert np.array_equal(m.flatten(p2, s2), blob) and ("widths" in s2.get("~", {})) == (not trainable)
    with pytest.raises(TypeError):
        m.unflatten(blob)
