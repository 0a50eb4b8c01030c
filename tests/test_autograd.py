"""Differentiable model step (lagrangebench_amd/autograd.py, lb_train_forward / lb_train_backward): CPU side.

The two exports exist and refuse null handles; the float64 torch restatement of the feature builder
(tests/_features_torch.py) equals oracle.lb_oracle's feature_transform and its autograd gradient agrees with central
finite differences - it is the yardstick the device's position gradient is held to in tests/test_autograd_gpu.py; the
bookkeeping of DeviceModule (tickets, recomputation, gradient blob) on a stub handle with CPU tensors.
"""
import numpy as np
import pytest
import torch

from oracle import lb_oracle as O
from tests._common import oracle_case
from tests._features_torch import case_constants, features_torch


def test_abi_has_the_two_exports_and_they_refuse_null_handles():
    from lagrangebench_amd import _lib
    lib = _lib.load()
    assert lib.lb_train_forward(None, None) == -1
    assert lib.lb_train_backward(None, None, None) == -1


# ------------------------------------------------------------------------------------------------ the restatement
def _case(name, scale, free):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=1, extra_seq_length=3, scale=scale)
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos, pt = ds[0]
    isl = ds.input_seq_length
    window = pos[:, :isl].astype(np.float64)
    feats, _ = oracle_case(ds).allocate_eval((window, pt))
    n = window.shape[0]
    rcv, snd = np.asarray(feats["receivers"]), np.asarray(feats["senders"])
    real = rcv < n
    return ds, window, pt, feats, rcv, snd, real


_CASES = {}


def _cached(name, scale, free):
    key = (name, scale, free)
    if key not in _CASES:
        _CASES[key] = _case(name, scale, free)
    return _CASES[key]


@pytest.mark.parametrize("name,scale,free,n", [("rpf2d", 0.25, False, 200), ("ldc3d", 0.5, True, 1020)])
def test_restatement_equals_the_oracle_feature_transform(name, scale, free, n):
    ds, window, pt, feats, rcv, snd, real = _cached(name, scale, free)
    assert window.shape[0] == n
    kw = case_constants(ds)
    force = torch.as_tensor(np.asarray(feats["force"])) if "force" in feats else None
    got = features_torch(torch.as_tensor(window), torch.as_tensor(rcv[real]).long(), torch.as_tensor(snd[real]).long(),
                         force=force, **kw)
    for k in ("vel_hist", "bound", "force"):
        assert (k in got) == (k in feats), k
        if k in feats:
            assert np.abs(got[k].numpy() - np.asarray(feats[k])).max() <= 1e-12, k
    assert np.abs(got["rel_disp"].numpy() - np.asarray(feats["rel_disp"])[real]).max() <= 1e-12
    assert np.abs(got["rel_dist"].numpy() - np.asarray(feats["rel_dist"])[real]).max() <= 1e-12
    # magnitude features: the oracle's feature_transform with the switch on
    ds.magnitude_features = True
    try:
        fm, _ = oracle_case(ds).allocate_eval((window, pt))
        gm = features_torch(torch.as_tensor(window), torch.as_tensor(rcv[real]).long(), torch.as_tensor(snd[real]).long(),
                            force=force, **case_constants(ds))
    finally:
        ds.magnitude_features = False
    assert np.abs(gm["vel_mag"].numpy() - np.asarray(fm["vel_mag"])).max() <= 1e-12
    assert gm["node"].shape[1] == got["node"].shape[1] + window.shape[1] - 1


def _scalar_of_features(f, wn, we):
    """A fixed smooth function of every feature column: random projections through tanh, so each column carries its own
    weight and the non-linearity mixes them."""
    return torch.tanh(f["node"] @ wn).sum() + torch.tanh(f["edge"] @ we).sum()


def _fd_check(ds, window, rcv, snd, force, coords, magnitude):
    kw = case_constants(ds)
    kw["magnitude"] = magnitude
    r, s = torch.as_tensor(rcv).long(), torch.as_tensor(snd).long()
    w = torch.tensor(window, requires_grad=True)
    f = features_torch(w, r, s, force=force, **kw)
    g = torch.Generator().manual_seed(3)
    wn = torch.randn((f["node"].shape[1], 4), generator=g, dtype=torch.float64)
    we = torch.randn((f["edge"].shape[1], 4), generator=g, dtype=torch.float64)
    _scalar_of_features(f, wn, we).backward()
    grad = w.grad.numpy()
    gmax = np.abs(grad).max()
    h = 1e-6
    for (i, fr, d) in coords:
        vals = []
        for sgn in (1.0, -1.0):
            wp = window.copy()
            wp[i, fr, d] += sgn * h
            with torch.no_grad():
                vals.append(float(_scalar_of_features(features_torch(torch.as_tensor(wp), r, s, force=force, **kw), wn, we)))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - grad[i, fr, d]) <= 1e-5 * max(1.0, gmax), ((i, fr, d), fd, grad[i, fr, d])


@pytest.mark.parametrize("magnitude", [False, True])
def test_restatement_gradient_matches_finite_differences_periodic(magnitude):
    """rpf2d 0.25: the sample holds a particle whose velocity wraps and both endpoints of an edge that wraps."""
    ds, window, pt, feats, rcv, snd, real = _cached("rpf2d", 0.25, False)
    rcv, snd = rcv[real], snd[real]
    box = np.asarray(ds.box)
    raw_v = window[:, 1:] - window[:, :-1]
    vel_wraps = np.argwhere(np.abs(raw_v) > 0.5 * box)          # (particle, k, d)
    assert len(vel_wraps) > 0
    newest = window[:, -1]
    raw_e = newest[rcv] - newest[snd]
    edge_wraps = np.argwhere(np.abs(raw_e) > 0.5 * box)         # (edge, d)
    assert len(edge_wraps) > 0
    assert (rcv == snd).sum() == window.shape[0]                 # the radius graph holds every self-edge
    i, k, d = vel_wraps[0]
    e, de = edge_wraps[0]
    coords = [(int(i), int(k), int(d)), (int(i), int(k) + 1, int(d)),
              (int(rcv[e]), window.shape[1] - 1, int(de)), (int(snd[e]), window.shape[1] - 1, int(de))]
    rng = np.random.default_rng(0)
    while len(coords) < 32:
        coords.append((int(rng.integers(window.shape[0])), int(rng.integers(window.shape[1])), int(rng.integers(2))))
    force = torch.as_tensor(np.asarray(feats["force"]))
    _fd_check(ds, window, rcv, snd, force, coords, magnitude)


def test_restatement_gradient_matches_finite_differences_walls():
    """ldc3d in free space, 0.5: clipped and unclipped wall features, three particle types."""
    ds, window, pt, feats, rcv, snd, real = _cached("ldc3d", 0.5, True)
    rcv, snd = rcv[real], snd[real]
    assert set(np.unique(pt)) >= {0, 1, 2}
    bound = np.asarray(feats["bound"])
    dim = window.shape[2]
    clipped = np.argwhere(np.abs(bound) == 1.0)
    inside = np.argwhere(np.abs(bound) < 1.0)
    assert len(clipped) > 0 and len(inside) > 0
    # an unclipped feature stays unclipped under the +-1e-6 probe
    far = inside[np.abs(np.abs(bound[inside[:, 0], inside[:, 1]]) - 1.0) > 1e-4]
    last = window.shape[1] - 1
    coords = [(int(clipped[0][0]), last, int(clipped[0][1] % dim)), (int(far[0][0]), last, int(far[0][1] % dim)),
              (int(far[-1][0]), last, int(far[-1][1] % dim))]
    rng = np.random.default_rng(1)
    while len(coords) < 32:
        coords.append((int(rng.integers(window.shape[0])), int(rng.integers(window.shape[1])), int(rng.integers(dim))))
    _fd_check(ds, window, rcv, snd, None, coords, False)


# ------------------------------------------------------------------------------------------------ DeviceModule plumbing
class _StubEngine:
    B, N, isl, dim, e_cap = 1, 3, 2, 2, 8

    def __init__(self, log):
        self.log, self.version = log, 0

    def set_particle_type(self, pt):
        self.log.append("ptype")

    def load_window(self, w, t0=0, step=0):
        self.log.append("load")
        self.window = w.clone()

    def nl_update(self):
        self.log.append("update")

    def nl_flags(self):
        return torch.zeros(1, dtype=torch.int32)


class _StubHandle:
    """pred = weights[0] * newest frame; d weights[0] = sum(dpred * newest), accumulated like the device blob."""

    def __init__(self, engine, log):
        self.engine, self.log = engine, log
        self.w = torch.tensor([2.0, 0.0], dtype=torch.float32)
        self.g = torch.full((2,), 7.0)   # stale gradients: the module must zero them before the backward
        self.live = False

    def device_blob(self, which):
        return {"weights": self.w, "grads": self.g}[which]

    def forward(self):
        self.log.append("forward")
        self.live = True
        self.x = self.engine.window[:, :, -1].float()
        return self.w[0].detach() * self.x

    def exact_math(self, on):
        self.exact_log = getattr(self, "exact_log", []) + [bool(on)]

    def zero_grad(self):
        self.log.append("zero")
        self.g.zero_()

    def backward(self, dpred, want_dpos=False):
        assert self.live, "backward without a live forward"
        self.log.append("backward" + ("+dpos" if want_dpos else ""))
        self.live = False
        self.g[0] += (dpred * self.x).sum()
        if not want_dpos:
            return None
        dpos = torch.zeros_like(self.engine.window)
        dpos[:, :, -1] = (self.w[0].detach() * dpred).double()
        return dpos

    def read(self, which):
        return self.w.numpy().copy()


class _StubCase:
    def __init__(self, engine):
        self._e = engine

    def engine(self, batch):
        return self._e


class _StubModel:
    _OUTPUT = "acc"

    def __init__(self, log, window_grad):
        self.log, self._WINDOW_GRAD = log, window_grad

    def train_handle(self, engine, params):
        return _StubHandle(engine, self.log)

    def unflatten(self, blob, like):
        return {"w": blob}


def _stub_module(window_grad=True):
    from lagrangebench_amd.autograd import DeviceModule
    log = []
    eng = _StubEngine(log)
    return DeviceModule(_StubModel(log, window_grad), _StubCase(eng), {}, 1), log


def test_device_module_aliases_weights_and_returns_a_clone_of_the_zeroed_gradient_blob():
    mod, log = _stub_module()
    assert mod.weights.data_ptr() == mod.handle.w.data_ptr()
    w = torch.arange(12, dtype=torch.float64).reshape(1, 3, 2, 2)
    out = mod(w)["acc"]
    assert out.dtype == torch.float32 and out.grad_fn is not None
    out.sum().backward()
    assert log == ["load", "update", "forward", "zero", "backward"]
    expect = float(w[:, :, -1].sum())
    assert float(mod.weights.grad[0]) == expect            # not 7 + ...: the blob was zeroed first
    assert mod.weights.grad.data_ptr() != mod.handle.g.data_ptr()
    mod.handle.g.fill_(-1.0)
    assert float(mod.weights.grad[0]) == expect            # a clone
    assert mod.recomputed == 0
    assert mod.params()["w"][0] == 2.0


def test_device_module_recomputes_a_superseded_forward_in_order():
    mod, log = _stub_module()
    w1 = torch.arange(12, dtype=torch.float64).reshape(1, 3, 2, 2).requires_grad_(True)
    w2 = (torch.arange(12, dtype=torch.float64).reshape(1, 3, 2, 2) * 0.5).requires_grad_(True)
    o1 = mod(w1)["acc"]
    o2 = mod(w2)["acc"]
    del log[:]
    (o1.sum() + 3.0 * o2.sum()).backward()
    # the second forward is the live one: its backward runs as is; the first reloads, updates, forwards again
    assert log.count("load") == 1 and log.count("forward") == 1 and log.count("backward+dpos") == 2
    j = log.index("load")
    assert log[j:j + 5] == ["load", "update", "forward", "zero", "backward+dpos"]
    assert mod.recomputed == 1
    assert torch.equal(w1.grad[:, :, -1], torch.full((1, 3, 2), 2.0, dtype=torch.float64))
    assert torch.equal(w2.grad[:, :, -1], torch.full((1, 3, 2), 6.0, dtype=torch.float64))
    assert float(mod.weights.grad[0]) == float((w1[:, :, -1].sum() + 3.0 * w2[:, :, -1].sum()).detach())


def test_device_module_refuses_window_gradients_for_other_models_and_stale_weights():
    mod, _ = _stub_module(window_grad=False)
    w = torch.zeros((1, 3, 2, 2), dtype=torch.float64)
    mod(w)                                                   # fine without a gradient
    with pytest.raises(NotImplementedError, match="GNS only"):
        mod(w.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="float64"):
        mod(w.float())
    mod2, _ = _stub_module()
    out = mod2(w)["acc"]
    with torch.no_grad():
        mod2.weights.add_(1.0)                               # an optimiser step between forward and backward
    with pytest.raises(RuntimeError, match="modified in place"):
        out.sum().backward()


def test_device_module_arithmetic_rule_exact_forward_for_relu_models():
    """A model with ReLU kinks (_EXACT_FORWARD) gets an exact forward; the backward is exact only where the window's
    gradient is asked for.  Other models keep the default unless the window needs a gradient."""
    w = torch.zeros((1, 3, 2, 2), dtype=torch.float64)
    for relu, want, expect in [(True, False, [True, False]), (True, True, [True, True]), (False, False, [False, False]),
                               (False, True, [True, True])]:
        mod, _ = _stub_module()
        mod._exact_forward = relu
        mod(w.clone().requires_grad_(want))["acc"].sum().backward()
        assert mod.handle.exact_log == expect, (relu, want, mod.handle.exact_log)


def test_non_kinematic_mask_follows_the_loss_weight_rule():
    from lagrangebench_amd.autograd import non_kinematic_mask
    pt = np.array([0, 1, 2, 3, -1, 5])
    assert np.array_equal(non_kinematic_mask(torch.as_tensor(pt)).numpy(), ~O.get_kinematic_mask(pt))
