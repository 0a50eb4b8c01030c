"""What GNS weight loading (csrc/lb_gns_weights.hip) decides on its own, at the fused depth (two Linears per MLP) and on
the one-Linear-per-launch path (three): a uniformly small weight matrix switches the engine to exact fp32, and a blob of
the wrong length is refused without harming the engine."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests._common import hip_case, make_params  # noqa: E402


def _engine(ds):
    if not torch.cuda.is_available():
        pytest.fail("these tests need a HIP device (they are selected with -m gpu)")
    pos = ds[0][0][None, :, :ds.input_seq_length]
    pt = ds[0][1][None]
    feats, _ = hip_case(ds).allocate_eval((pos, pt))
    return feats, pt


@pytest.mark.parametrize("nl", [2, 3])
def test_small_weight_matrix_switches_engine_to_fp32(nl):
    """The f16x2 split carries a weight as fp16 hi + lo with an absolute floor of 2^-25: a matrix with rms < 2^-7 would
    miss the 1e-5 class, so creating the handle on a guarded engine (mode 1) leaves it in exact fp32 (mode 0)."""
    if "LB_MATH" in os.environ:
        pytest.skip("LB_MATH fixes the arithmetic mode")
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    ds = make_case("small2d", n_trajs=1, extra_seq_length=2)
    model = GNS(2, 128, nl, 1, 16)
    params = make_params(ds, num_mp_steps=1, decoder_scale=1.0, blocks_per_step=nl)

    feats, _ = _engine(ds)
    assert feats.engine.math_mode()[0] == 1
    model.handle(feats.engine, params)
    assert feats.engine.math_mode()[0] == 1
    assert "f16x2" in feats.engine.kernel_names()["edge"] and "f16x2" in feats.engine.kernel_names()["node"]

    small = {k: dict(v) for k, v in params.items()}
    small["proc0_node/linear_0"]["w"] = params["proc0_node/linear_0"]["w"] * np.float32(2.0 ** -10)
    feats, pt = _engine(ds)
    assert feats.engine.math_mode()[0] == 1
    model.handle(feats.engine, small)
    assert feats.engine.math_mode()[0] == 0
    names = feats.engine.kernel_names()
    assert "f32" in names["edge"] and "f32" in names["node"] and "f16x2" not in names["edge"] + names["node"]
    assert torch.isfinite(model.apply(small, {}, (feats, pt))[0]["acc"]).all()


@pytest.mark.parametrize("latent", [128, 64])
@pytest.mark.parametrize("nl", [2, 3])
def test_wrong_blob_length_is_refused_and_engine_stays_usable(nl, latent):
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.engine import GnsHandle
    from lagrangebench_amd.models import GNS
    ds = make_case("small2d", n_trajs=1, extra_seq_length=2)
    model = GNS(2, latent, nl, 1, 16)
    params = make_params(ds, num_mp_steps=1, latent_size=latent, blocks_per_step=nl)
    feats, pt = _engine(ds)
    blob = model.flatten(params)
    for bad in (blob[:-1], np.append(blob, np.float32(0))):
        with pytest.raises(LbHipError, match=r"\(-1: bad argument\): weight blob has %d floats" % bad.size):
            feats.engine._new_handle(GnsHandle, "lb_gns_create", model._desc(feats.engine), bad)
    acc = model.apply(params, {}, (feats, pt))[0]["acc"]
    assert torch.isfinite(acc).all() and float(acc.abs().max()) > 0
