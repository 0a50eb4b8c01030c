"""models.TorchModel and graph.Graph without a device: the parameter and state trees, flatten / unflatten, init, the ABI
entries, the dtype check of the graph ops, and the CPU restatement of the graph ops the GPU tests compare with."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._torch_models import CpuGraph, TinyMP  # noqa: E402


def _model(node_in=7, dim=2, hidden=8):
    from lagrangebench_amd.models import TorchModel
    torch.manual_seed(3)
    return TorchModel(TinyMP(node_in, dim, hidden)), TinyMP(node_in, dim, hidden)


def test_tree_follows_named_parameters_and_round_trips():
    model, mod = _model()
    params, state = model.init(np.array([5]), None)
    names = [n for n, _ in mod.named_parameters()]
    assert names[0] == "gain"   # a parameter of the module itself: named_parameters() lists it first
    assert set(params) == {"enc", "edge.0", "edge.2", "node.0", "node.2", "dec", "~"}
    assert set(params["edge.0"]) == {"weight", "bias"} and set(params["~"]) == {"gain"}
    for n, p in mod.named_parameters():
        m, _, leaf = n.rpartition(".")
        a = params[m or "~"][leaf]
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == tuple(p.shape)
    blob = model.flatten(params)
    assert blob.dtype == np.float32 and blob.size == sum(p.numel() for p in mod.parameters())
    # named_parameters() order: the blob is the leaves one after the other in that order
    off = 0
    for n, p in mod.named_parameters():
        m, _, leaf = n.rpartition(".")
        assert np.array_equal(blob[off:off + p.numel()], params[m or "~"][leaf].ravel()), n
        off += p.numel()
    back = model.unflatten(np.arange(blob.size, dtype=np.float32))
    assert np.array_equal(model.flatten(back), np.arange(blob.size, dtype=np.float32))
    assert np.array_equal(model.flatten(model.unflatten(blob, params)), blob)
    with pytest.raises(ValueError, match="floats"):
        model.unflatten(blob[:-1])
    bad = {k: dict(v) for k, v in params.items()}
    bad["dec"]["bias"] = np.zeros(5, np.float32)
    with pytest.raises(ValueError, match="shape"):
        model.flatten(bad)
    del bad["~"]
    with pytest.raises(ValueError, match="missing"):
        model.flatten(bad)
    # checkpoints keep the tree as it is
    assert model.params_to_haiku(params) is params and model.params_from_haiku(params) is params


def test_checkpoint_round_trip(tmp_path):
    from lagrangebench_amd.utils import load_haiku, save_haiku
    model, _ = _model()
    params, state = model.init(np.array([11]), None)
    save_haiku(str(tmp_path / "ckp"), model.params_to_haiku(params), state, None, {"step": 3, "loss": 1.0})
    loaded, lstate, _, step = load_haiku(str(tmp_path / "ckp"))
    assert step == 3
    assert np.array_equal(model.flatten(model.params_from_haiku(loaded)).view(np.uint32), model.flatten(params).view(np.uint32))
    assert np.array_equal(lstate["~"]["in_scale"], state["~"]["in_scale"])


def test_init_is_deterministic_and_leaves_the_global_rng_alone():
    model, _ = _model()
    torch.manual_seed(1234)
    before = torch.random.get_rng_state().clone()
    a, _ = model.init(np.array([0, 42]), None)
    assert torch.equal(torch.random.get_rng_state(), before)
    expect = torch.rand(3)
    b, _ = model.init(np.array([0, 42]), None)
    c, _ = model.init(np.array([0, 43]), None)
    torch.manual_seed(1234)
    assert torch.equal(torch.rand(3), expect)   # the draw after init is the draw without it
    fa, fb, fc = model.flatten(a), model.flatten(b), model.flatten(c)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and not np.array_equal(fa, fc)
    assert np.all(a["~"]["gain"] == 1.0)   # the module's own reset_parameters ran
    # a and b are copies: editing one leaves the other alone
    a["dec"]["bias"][:] = 7.0
    assert not np.array_equal(a["dec"]["bias"], b["dec"]["bias"])


def test_persistent_buffers_are_the_state_tree():
    from lagrangebench_amd.models import TorchModel

    class WithBuffers(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2)
            self.register_buffer("scale", torch.tensor([1.0, 2.0, 3.0]))
            self.register_buffer("scratch", torch.zeros(4), persistent=False)
            self.lin.register_buffer("shift", torch.tensor([0.5, -0.5]))

        def forward(self, features, particle_type, graph):
            return self.lin(features["x"] * self.scale) + self.lin.shift

    model = TorchModel(WithBuffers(), output="vel")
    params, state = model.init(None, None)
    assert set(params) == {"lin"} and set(state) == {"~", "lin"}
    assert set(state["~"]) == {"scale"} and set(state["lin"]) == {"shift"}   # the non-persistent buffer is not state
    assert np.array_equal(state["~"]["scale"], [1.0, 2.0, 3.0]) and model._OUTPUT == "vel"
    # apply's module is built from (params, state): a changed state reaches the copy, not the wrapped module
    state2 = {"~": {"scale": np.array([2.0, 2.0, 2.0], np.float32)}, "lin": {"shift": state["lin"]["shift"]}}

    class Eng:
        device = torch.device("cpu")
    mod = model._device_module(Eng(), params, state2)
    assert torch.equal(mod.scale, torch.tensor([2.0, 2.0, 2.0])) and torch.equal(mod.lin.shift, torch.tensor([0.5, -0.5]))
    assert np.array_equal(model.state_of()["~"]["scale"], [1.0, 2.0, 3.0])
    model.set_state(state2)
    assert np.array_equal(model.state_of()["~"]["scale"], [2.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="acc"):
        TorchModel(WithBuffers(), output="force")
    with pytest.raises(TypeError, match="float32"):
        TorchModel(WithBuffers().double())


def test_trainable_and_routed_to_the_generic_rollout():
    from functools import partial
    from lagrangebench_amd.evaluate.rollout import _gns_of
    from lagrangebench_amd.models import GNS, BaseModel, Linear
    model, _ = _model()
    model.check_trainable()   # does not raise
    assert model._PADDED_OK is False
    assert _gns_of(model.apply) is None and _gns_of(partial(model.apply)) is None
    lin = Linear(2)
    assert BaseModel._FUSED_ROLLOUT is True and _gns_of(lin.apply) is lin and _gns_of(GNS(2, 32, 2, 1, 16).apply) is not None


def test_abi_lists_the_new_symbols():
    import ctypes as C
    from lagrangebench_amd import _lib
    P = C.c_void_p
    assert _lib._SIGS["lb_graph_gather"] == (C.c_int, [P, C.c_int32, P, P, C.c_int32])
    assert _lib._SIGS["lb_graph_segment_sum"] == (C.c_int, [P, C.c_int32, P, P, C.c_int32])
    assert _lib._SIGS["lb_blob_train_create"] == (C.c_int, [P, C.POINTER(C.c_float), C.c_int64, C.POINTER(P)])
    import os
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "lbhip.h")).read()
    for sym in ("lb_graph_gather", "lb_graph_segment_sum", "lb_blob_train_create"):
        assert f"int {sym}(" in hdr, sym


class _StubEngine:
    version, B, N, e_cap, device = 4, 1, 3, 5, torch.device("cpu")


class _StubFeatures:
    engine, version, batched = _StubEngine(), 4, True


def test_graph_refuses_other_dtypes_before_touching_the_engine():
    from lagrangebench_amd.graph import Graph
    g = Graph(_StubFeatures())
    for op, shape in ((g.gather, (1, 3, 2)), (g.segment_sum, (1, 5, 2))):
        for dt in (torch.float64, torch.float16, torch.int32):
            with pytest.raises(TypeError, match="float32"):
                op(torch.zeros(shape, dtype=dt), "senders")
    with pytest.raises(ValueError, match="role"):
        g.gather(torch.zeros((1, 3, 2)), "neighbours")
    with pytest.raises(TypeError, match="FeatureDict"):
        Graph({"vel_hist": torch.zeros(3)})
    stale = _StubFeatures()
    stale.version = 3
    with pytest.raises(RuntimeError, match="stale"):
        Graph(stale).gather(torch.zeros((1, 3, 2)), "senders")


def test_cpu_graph_is_the_adjoint_pair():
    """Not a test of the feature: a sanity check of the test helper CpuGraph, the restatement tests/test_torch_model_gpu.py
    holds the device to - gather and segment_sum on a small padded list against a loop, and <gather(x), m> = <x,
    segment_sum(m)> in float64."""
    N, E = 4, 7
    recv = np.array([[0, 0, 1, 2, 2, 4, 4], [1, 3, 3, 3, 4, 4, 4]])
    send = np.array([[1, 2, 0, 2, 3, 4, 4], [0, 0, 1, 2, 4, 4, 4]])
    ne = np.array([5, 4])
    g = CpuGraph(send, recv, ne, N)
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((2, N, 3)))
    m = torch.tensor(rng.standard_normal((2, E, 3)))
    m_nan = m.clone()
    for b in range(2):
        m_nan[b, ne[b]:] = float("nan")
    for role, idx in (("senders", send), ("receivers", recv)):
        xs, agg = g.gather(x, role), g.segment_sum(m_nan, role)
        want_agg = torch.zeros((2, N, 3), dtype=torch.float64)
        for b in range(2):
            for j in range(E):
                if j < ne[b]:
                    assert torch.equal(xs[b, j], x[b, idx[b, j]])
                    want_agg[b, idx[b, j]] += m[b, j]
                else:
                    assert torch.equal(xs[b, j], torch.zeros(3, dtype=torch.float64))
        assert torch.allclose(agg, want_agg, rtol=0, atol=1e-15) and torch.isfinite(agg).all()
        m_real = torch.where(g.real[..., None], m, torch.zeros((), dtype=torch.float64))
        assert abs(float((xs * m_real).sum() - (x * agg).sum())) < 1e-12
