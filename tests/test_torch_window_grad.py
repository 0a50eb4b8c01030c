"""The window gradient of a TorchModel, the parts that need no device: the new export's declaration against the ctypes table,
``autograd.advance_window`` against a float64 closed form written here and against ``torch.autograd.gradcheck``, and the
refusals of ``TorchModule``, ``advance_window`` and ``graph.differentiable_features`` that are raised before an engine is used.
"""
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._common import hip_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lb_graph_features_backward"


# ------------------------------------------------------------------------------------------------ the export
def test_header_and_ctypes_table_declare_the_export_alike():
    import ctypes as C
    from lagrangebench_amd import _lib
    src = open(os.path.join(ROOT, "include", "lbhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{SYMBOL} is not declared in include/lbhip.h"
    args = [" ".join(a.split()) for a in m.group(2).split(",")]
    assert m.group(1) == "int"
    assert [re.sub(r"\s*\w+$", "", a) for a in args] == ["lb_engine*"] + ["const float*"] * 6 + ["double*"]
    res, table = _lib._SIGS[SYMBOL]
    assert res is C.c_int
    assert list(table) == [C.c_void_p] * len(args)      # every argument of the declaration is a pointer
    from lagrangebench_amd import build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    lib = _lib.load()
    assert lib.lb_graph_features_backward(None, None, None, None, None, None, None, None) == -1   # LB_ERR_ARG: no engine


# ------------------------------------------------------------------------------------------------ advance_window
def _case(name, free):
    from lagrangebench_amd.data import make_case
    ds = make_case(name, n_trajs=2, extra_seq_length=3, scale=0.25)
    if free:
        ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
    pos = np.stack([ds[b][0] for b in range(2)]).astype(np.float64)
    pt = np.stack([ds[b][1] for b in range(2)])
    return ds, hip_case(ds), pos, pt


def _closed_form(case, w, pred, output):
    """integrate_fn (case.py:230-259) and the shift of the window, float64 numpy."""
    L = np.asarray(case.box, np.float64)
    s = case.normalization_stats
    newest, previous = w[..., -1, :], w[..., -2, :]
    if output == "pos":
        new = pred
    else:
        if output == "vel":
            vel = np.asarray(s["velocity"]["mean"], np.float64) + pred * np.asarray(s["velocity"]["std"], np.float64)
        else:
            d = newest - previous
            if case.periodic:
                d = np.mod(d + 0.5 * L, L) - 0.5 * L
            vel = d + np.asarray(s["acceleration"]["mean"], np.float64) + pred * np.asarray(s["acceleration"]["std"], np.float64)
        new = newest + vel
        if case.periodic:
            new = np.mod(new, L)
    return np.concatenate([w[..., 1:, :], new[..., None, :]], axis=-2)


@pytest.mark.parametrize("output", ["acc", "vel", "pos"])
@pytest.mark.parametrize("box", ["periodic", "free"])
def test_advance_window_equals_the_closed_form(box, output):
    from lagrangebench_amd.autograd import advance_window
    ds, case, pos, pt = _case("rpf2d" if box == "periodic" else "ldc3d", box == "free")
    assert case.periodic == (box == "periodic")
    isl = ds.input_seq_length
    w = pos[:, :, :isl]
    rng = np.random.default_rng(3)
    if output == "pos":
        pred = rng.random(w[:, :, 0].shape) * np.asarray(case.box)
    else:
        pred = rng.standard_normal(w[:, :, 0].shape)
    got = advance_window(case, torch.as_tensor(w), torch.as_tensor(pred), output).numpy()
    ref = _closed_form(case, w, pred, output)
    assert got.shape == w.shape and got.dtype == np.float64
    err = np.abs(got - ref)
    print(f"[advance_window {box} {output}] largest deviation / box side {float((err / np.asarray(case.box)).max()):.2e}")
    assert float((err / np.asarray(case.box)).max()) <= 1e-12
    if case.periodic and output != "pos":
        assert (got[:, :, -1] >= 0).all() and (got[:, :, -1] < np.asarray(case.box)).all()
    # batched and un-batched agree
    one = advance_window(case, torch.as_tensor(w[0]), torch.as_tensor(pred[0]), output).numpy()
    assert np.array_equal(one, got[0])
    # kinematic and pad particles take their targets
    pt2 = pt.copy()
    pt2[:, :3] = (1, 2, -1)
    tgt = rng.random(pred.shape)
    fixed = advance_window(case, torch.as_tensor(w), torch.as_tensor(pred), output, particle_type=pt2,
                           target_pos=torch.as_tensor(tgt).requires_grad_(True))
    kin = (pt2 == 1) | (pt2 == 2) | (pt2 == -1)
    assert not fixed.requires_grad                                   # the targets are detached
    assert np.array_equal(fixed.numpy()[:, :, -1][kin], tgt[kin])
    assert np.array_equal(fixed.numpy()[:, :, -1][~kin], got[:, :, -1][~kin])


@pytest.mark.parametrize("output", ["acc", "vel", "pos"])
@pytest.mark.parametrize("box", ["periodic", "free"])
def test_advance_window_gradcheck(box, output):
    from lagrangebench_amd.autograd import advance_window
    ds, case, pos, pt = _case("rpf2d" if box == "periodic" else "ldc3d", box == "free")
    isl = ds.input_seq_length
    w = torch.as_tensor(pos[0, :6, :isl]).clone().requires_grad_(True)      # six particles: a small Jacobian
    g = torch.Generator().manual_seed(5)
    pred = torch.randn((6, w.shape[-1]), generator=g, dtype=torch.float64).requires_grad_(True)
    pt6 = np.array([0, 0, 1, 0, 2, 0])
    tgt = torch.rand((6, w.shape[-1]), generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda a, b: advance_window(case, a, b, output), (w, pred))
    assert torch.autograd.gradcheck(lambda a, b: advance_window(case, a, b, output, particle_type=pt6, target_pos=tgt), (w, pred))
    out = advance_window(case, w, pred, output, particle_type=pt6, target_pos=tgt)
    (dw, dp) = torch.autograd.grad(out[:, -1].sum(), (w, pred), allow_unused=True)
    assert float(dp[[2, 4]].abs().max()) == 0.0 and float(dp[[0, 1, 3, 5]].abs().min()) > 0   # no gradient through a target


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_that_need_no_engine():
    from lagrangebench_amd.autograd import TorchModule, advance_window
    from lagrangebench_amd.graph import differentiable_features
    from lagrangebench_amd.models import GNS
    ds, case, pos, pt = _case("rpf2d", False)
    isl = ds.input_seq_length
    with pytest.raises(TypeError, match="DeviceModule"):
        TorchModule(GNS(2, 128, 2, 2, 16), case, {}, 1)
    with pytest.raises(TypeError, match="DeviceModule"):
        TorchModule(torch.nn.Linear(2, 2), case, {}, 1)
    w = torch.as_tensor(pos[:, :, :isl])
    pred = torch.zeros(w[:, :, 0].shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="'acc', 'vel' or 'pos'"):
        advance_window(case, w, pred, "force")
    with pytest.raises(ValueError, match="float64"):
        advance_window(case, w.float(), pred)
    with pytest.raises(ValueError, match="pred must be"):
        advance_window(case, w, pred[:, :-1])
    with pytest.raises(ValueError, match="particle_type"):
        advance_window(case, w, pred, target_pos=pred)
    # differentiable_features: a plain dict, float32 geometry, a window of another shape or dtype
    with pytest.raises(TypeError, match="FeatureDict"):
        differentiable_features({"vel_hist": torch.zeros(3)}, w)
    eng = types.SimpleNamespace(B=2, N=w.shape[1], isl=isl, dim=2, geometry_f32=True, device=torch.device("cpu"), version=0)
    feats = types.SimpleNamespace(engine=eng, version=0, batched=True)
    with pytest.raises(NotImplementedError, match="float64 geometry"):
        differentiable_features(feats, w)
    eng.geometry_f32 = False
    with pytest.raises(ValueError, match="float64"):
        differentiable_features(feats, w.float())
    with pytest.raises(ValueError, match="window must be"):
        differentiable_features(feats, w[:, :, 1:])
    eng.version = 1
    with pytest.raises(RuntimeError, match="stale"):
        differentiable_features(feats, w)
