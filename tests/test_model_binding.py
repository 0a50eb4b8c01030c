"""The binding of GNS, SEGNN, EGNN and PaiNN to their device handles (models/base.py), driven against a stub engine with
no device: the handle cache and its content stamp, apply's refusals, the checkpoint routing and the training refusal."""
import numpy as np
import pytest
import torch


class _StubHandle:
    def __init__(self, engine, symbol, blob):
        self.engine, self.symbol, self.blob = engine, symbol, blob


class _StubEngine:
    """Records every create call; the forwards return zeros of the engine's shape."""
    node_in, dim, B, N, version = 30, 2, 1, 4, 0

    def __init__(self):
        self.created = []

    def _new_handle(self, cls, symbol, desc, blob):
        h = _StubHandle(self, symbol, np.array(blob))
        self.created.append(h)
        return h

    def _out(self, h):
        assert h.engine is self
        return torch.zeros((self.B, self.N, self.dim))

    gns_forward = segnn_forward = egnn_forward = painn_forward = _out


class _Features:
    def __init__(self, engine, batched=False):
        self.engine, self.version, self.batched = engine, engine.version, batched


def _gns():
    from lagrangebench_amd.models import GNS
    m = GNS(2, 16, 2, 2, 16)
    return m, m.init_params(0, _StubEngine.node_in, 3), {}


def _segnn():
    from lagrangebench_amd.models import SEGNN, node_irreps
    irr = node_irreps({"periodic_boundary_conditions": [True, True]}, 6, True, False, True)
    m = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=5)
    return m, m.init_params(0), {}


def _egnn():
    from lagrangebench_amd.models import EGNN
    m = EGNN(32, 1, 0.1, 5, num_mp_steps=2)
    return m, m.init_params(0, has_force=True), {}


def _painn():
    from lagrangebench_amd.models import PaiNN
    from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
    m = PaiNN(32, 1, 2, gaussian_rbf(8, 0.05, trainable=False), cosine_cutoff(0.05), 5)
    p, state = m.init_params(0, has_force=True)
    return m, p, state


MODELS = {"gns": _gns, "segnn": _segnn, "egnn": _egnn, "painn": _painn}


def _first_leaf(tree):
    mod = sorted(k for k in tree if k != "~")[0]
    return tree[mod][sorted(tree[mod])[0]]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_handle_cache(name):
    model, params, state = MODELS[name]()
    eng = _StubEngine()
    h = model.handle(eng, params, state)
    assert model.handle(eng, params, state) is h and len(eng.created) == 1
    _first_leaf(params).reshape(-1)[0] += 1.0     # an in-place edit of one leaf
    h2 = model.handle(eng, params, state)
    assert h2 is not h and len(eng.created) == 2
    assert not np.array_equal(h2.blob, h.blob)
    assert model.handle(eng, params, state) is h2
    other = _StubEngine()                           # the same tree on another engine
    assert model.handle(other, params, state).engine is other


def test_tree_with_bare_values():
    """The oracle's SEGNN trees carry their configuration beside the modules ({"hidden": 32, "norm": None, ...})."""
    model, params, state = _segnn()
    params.update(hidden=32, blocks=2, layers=2, norm=None, x_node=[(5, 1), (1, 1)])
    eng = _StubEngine()
    h = model.handle(eng, params, state)
    assert model.handle(eng, params, state) is h
    params["output"]["wv"][0, 0] += 1.0
    assert model.handle(eng, params, state) is not h


def test_painn_state_edit_gives_a_new_handle():
    model, params, state = _painn()
    eng = _StubEngine()
    h = model.handle(eng, params, state)
    state["~"]["widths"][0, 0] *= 2.0
    h2 = model.handle(eng, params, state)
    assert h2 is not h and not np.array_equal(h2.blob, h.blob)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_cache_keeps_at_most_four_handles(name):
    model, params, state = MODELS[name]()
    eng = _StubEngine()
    trees = [{k: dict(v) for k, v in params.items()} for _ in range(6)]
    for t in trees:
        model.handle(eng, t, state)
    assert len(eng.created) == 6 and len(model._handles) == 4
    # the least recently used went first: the last four are still cached
    for t in trees[2:]:
        model.handle(eng, t, state)
    assert len(eng.created) == 6


@pytest.mark.parametrize("name", sorted(MODELS))
def test_apply(name):
    model, params, state = MODELS[name]()
    eng = _StubEngine()
    with pytest.raises(TypeError, match=f"{type(model).__name__}.apply needs the FeatureDict"):
        model.apply(params, state, ({"vel_hist": None}, None))
    feats = _Features(eng)
    eng.version += 1
    with pytest.raises(RuntimeError, match="stale"):
        model.apply(params, state, (feats, None))
    out, st = model.apply(params, state, (_Features(eng), None))
    key = "pos" if name == "egnn" else "acc"
    assert set(out) == {key} and out[key].shape == (eng.N, eng.dim) and st is state
    out, _ = model(params, state, (_Features(eng, batched=True), None))
    assert out[key].shape == (eng.B, eng.N, eng.dim)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_checkpoint_routing(name):
    model, params, _ = MODELS[name]()
    assert model.params_from_haiku(params) is params
    hk = model.params_to_haiku(params)
    assert set(hk).isdisjoint(params)
    assert model.params_to_haiku(hk) is hk
    back = model.params_from_haiku(hk)
    assert set(back) == set(params)
    for mod in params:
        for leaf in params[mod]:
            np.testing.assert_array_equal(np.asarray(back[mod][leaf]), np.asarray(params[mod][leaf]), err_msg=mod)


def test_trainer_refuses_painn():
    from lagrangebench_amd.train import Trainer
    with pytest.raises(NotImplementedError, match="no device training step"):
        Trainer(_painn()[0], None, None, None)
    with pytest.raises(NotImplementedError, match="no device training step"):
        _painn()[0].train_handle(_StubEngine(), _painn()[1])


def test_training_refusals_come_from_the_model():
    from lagrangebench_amd.models import EGNN, GNS
    from lagrangebench_amd.train import Trainer
    with pytest.raises(NotImplementedError, match="latent_size <= 128"):
        Trainer(GNS(2, 256, 2, 2, 16), None, None, None)
    with pytest.raises(NotImplementedError, match="latent_size <= 128"):
        GNS(2, 16, 9, 2, 16).train_handle(_StubEngine(), {})
    with pytest.raises(NotImplementedError, match="normalize"):
        EGNN(32, 1, 0.1, 5, normalize=True).train_handle(_StubEngine(), {})
    for make in (_gns, _segnn, _egnn):
        model, params, _ = make()
        model.check_trainable()
        assert model.train_handle(_StubEngine(), params).symbol.endswith("_train_create")
