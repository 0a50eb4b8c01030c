"""The frame the device training steps share (csrc/lb_train.hip: train_handle_init, train_step_begin / _end, train_ensure,
train_loss_grad_guarded, the lb_train_model record of each model), on each model's smallest training case with a latent /
hidden size below 128, so the caller's blob reaches the padded device layout through the handle's index map (Linear has no
padding)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

KINDS = ["gns", "segnn", "egnn", "linear", "painn"]


def _setup(kind):
    """-> (make, engine, blob, step): make() = a new training handle of the case's parameters, step(th) = one loss +
    gradient pass on the engine's window, returns the loss."""
    from lagrangebench_amd.data import make_case
    from tests._common import hip_case, make_params
    g = torch.Generator().manual_seed(5)
    extra = ()
    if kind == "linear":   # tests/test_linear_gpu.py: rpf2d_b1
        from lagrangebench_amd.models import Linear
        isl, B = 6, 1
        ds = make_case("rpf2d", n_trajs=B, extra_seq_length=6, input_seq_length=isl, scale=0.25)
        ds.magnitude_features = True
        model = Linear(len(ds.box))
        params = model.init_params(7, 18)
        params["linear"]["b"] = (0.1 * np.random.default_rng(8).standard_normal(len(ds.box))).astype(np.float32)
        blob = model.flatten(params)
    elif kind == "painn":   # tests/test_painn_train_gpu.py: h64_nocut
        from lagrangebench_amd.models import PaiNN
        from lagrangebench_amd.models.painn import gaussian_rbf
        from tests._painn_oracle import random_biases
        isl, B = 6, 1
        ds = make_case("rpf2d", n_trajs=B, extra_seq_length=3, input_seq_length=isl, scale=0.25)
        ds.magnitude_features = True
        model = PaiNN(64, 1, 3, gaussian_rbf(20, 1.5, trainable=True), None, isl - 1)
        params, state = model.init_params(7, ds.external_force_fn is not None, False)
        params = random_biases(params, 8)
        extra = (state,)
        blob = model.flatten(params, state)
    elif kind == "egnn":   # tests/test_egnn_train.py: rpf2d_b1 at the width of h64
        from lagrangebench_amd.models import EGNN
        from tests._egnn_oracle import random_biases
        isl, B = 6, 1
        ds = make_case("rpf2d", n_trajs=B, extra_seq_length=3, input_seq_length=isl, scale=0.5)
        model = EGNN(64, 1, 0.01, isl - 1, num_mp_steps=3)
        params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
        blob = model.flatten(params)
    elif kind == "segnn":   # tests/test_segnn_train.py: small2d, L = 2, B = 2, two blocks
        from lagrangebench_amd.models import SEGNN, node_irreps
        from oracle import segnn_oracle as S
        B = 2
        ds = make_case("small2d", n_trajs=B, extra_seq_length=3)
        ds.magnitude_features = True
        isl = ds.input_seq_length
        homog = bool(np.all(ds[0][1] == 0))
        irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog)
        model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=isl - 1, homogeneous_particles=homog,
                      blocks_per_step=2)
        params = S.segnn_init(np.random.default_rng(11), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=2,
                              blocks_per_step=2, random_bias=True)
        params = {k: v for k, v in params.items() if isinstance(v, dict)}
        blob = model.flatten(params)
    else:   # tests/test_train.py: small3d, L = 2, B = 1, at latent 64
        from lagrangebench_amd.models import GNS
        B = 1
        ds = make_case("small3d", n_trajs=B, extra_seq_length=3)
        isl = ds.input_seq_length
        params = make_params(ds, num_mp_steps=2, decoder_scale=1.0, latent_size=64)
        model = GNS(len(ds.box), 64, 2, 2, 16)
        blob = model.flatten(params)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    feats, _ = hip_case(ds).allocate_eval((pos[:, :, :isl], pt))
    shape = (B, pos.shape[1], len(ds.box))
    if kind == "egnn":
        tg = {"pos": torch.as_tensor(pos[:, :, isl - 1], dtype=torch.float64) + 1e-3 * torch.randn(shape, generator=g, dtype=torch.float64)}
        step = lambda th: th.loss_grad(tg, {"pos": 1.0, "vel": 0.0, "acc": 0.0})   # noqa: E731
    else:
        target = torch.randn(shape, generator=g)
        step = lambda th: th.loss_grad(target, 1.0)   # noqa: E731
    eng = feats.engine
    return (lambda: model.train_handle(eng, params, *extra)), eng, np.asarray(blob, np.float32), step


def _once(h, step):
    h.zero_grad()
    loss = step(h)
    return loss, h.read("grads").tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_training_frame_is_reproducible_across_calls_writes_and_handles(kind):
    """On one handle: (a) two zero_grad + loss_grad passes give the same loss and the same gradient bytes; (b) so does a pass
    after write("weights", read("weights")) - the initialiser and write scatter through the same map, and the packed operands
    follow a weight change; (c) no step was repeated by the guard; (d) a second handle made from the same parameters gives
    the bytes of the first; (e) the GNS entry still refuses an EGNN handle."""
    make, eng, blob, step = _setup(kind)
    th = make()
    if kind == "linear":
        assert th.n_floats == th.device_floats()   # (w, b) as they are: no padding
    else:
        assert th.n_floats < th.device_floats()   # padded device layout: the index map is in use

    def once(h):
        return _once(h, step)

    loss_a, g_a = once(th)
    assert np.isfinite(loss_a) and np.abs(np.frombuffer(g_a, np.float32)).max() > 0
    assert once(th) == (loss_a, g_a)                                   # (a)
    w = th.read("weights")
    assert np.array_equal(w, blob)
    th.write("weights", w)
    assert th.read("weights").tobytes() == w.tobytes()
    assert once(th) == (loss_a, g_a)                                   # (b)
    assert th.math_fallbacks() == 0 and th.sort_fallbacks() == 0       # (c)
    th2 = make()
    assert once(th2) == (loss_a, g_a)                                  # (d)
    assert th2.math_fallbacks() == 0 and th2.sort_fallbacks() == 0
    th2.close()
    if kind == "egnn":                                                 # (e)
        from lagrangebench_amd._lib import LbHipError
        from lagrangebench_amd.engine import GnsTrainHandle
        with pytest.raises(LbHipError, match="an EGNN training handle: its loss needs the pos / vel / acc targets"):
            GnsTrainHandle.loss_grad(th, torch.zeros((eng.B, eng.N, eng.dim)))
    th.close()


_NAME = {"gns": "GNS", "segnn": "SEGNN", "egnn": "EGNN", "linear": "Linear", "painn": "PaiNN"}
_BLOB = "a blob training handle (lb_blob_train_create) holds optimiser state only"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS + ["blob"])
def test_shared_entries_dispatch_on_the_model_of_the_handle(kind):
    """What the shared entries decide by the model a handle holds, with the library's texts: the window gradient is refused
    for every model but GNS, by name, and leaves the forward live; lb_gns_train_sync_model, the three lb_*_train_model
    accessors and the SEGNN / EGNN loss entries refuse a handle of another kind; exact_math(False) gives the f16x2 products
    back to no model that was created without them (same gradient bytes, no repeated step); a blob handle is refused by
    every entry that runs a model."""
    from lagrangebench_amd._lib import LbHipError, check, ptr
    make, eng, blob, step = _setup("linear" if kind == "blob" else kind)
    lib = eng.lib
    th = eng.blob_train_handle(blob) if kind == "blob" else make()
    d = 1e-3 * torch.randn((eng.B, eng.N, eng.dim), generator=torch.Generator().manual_seed(9))

    def refused(text, call, *args):
        with pytest.raises(LbHipError, match=re.escape(text)):
            check(call(th._h, *args), call.__name__)

    if kind == "blob":
        with pytest.raises(LbHipError, match=re.escape("lb_train_forward: " + _BLOB)):
            th.forward()
        with pytest.raises(LbHipError, match=re.escape("lb_train_backward: " + _BLOB)):
            th.backward(d)
        with pytest.raises(LbHipError, match=re.escape("lb_gns_train_loss_grad: " + _BLOB)):
            th.loss_grad(d)
    else:
        loss_a, g_a = _once(th, step)
        th.zero_grad()
        th.forward()
        if kind == "gns":
            dpos = th.backward(d, want_dpos=True)
            assert tuple(dpos.shape) == (eng.B, eng.N, eng.isl, eng.dim) and bool(torch.isfinite(dpos).all())
        else:
            with pytest.raises(LbHipError, match=re.escape("the gradient with respect to the window is built for GNS only, "
                                                           f"not for {_NAME[kind]} handles")):
                th.backward(d, want_dpos=True)
            th.backward(d)   # the refusal left the forward live
        assert np.abs(th.read("grads")).max() > 0
        with pytest.raises(LbHipError, match="needs a live forward"):
            th.backward(d)
        th.exact_math(False)
        assert _once(th, step) == (loss_a, g_a)
        assert th.math_fallbacks() == 0
    # the typed entries on a handle of another kind (the handle's own pointer stands in for the inference model: a refusal
    # reads nothing behind it)
    if kind != "gns":
        refused("lb_gns_train_sync_model: " + _BLOB if kind == "blob" else "not a GNS training handle",
                lib.lb_gns_train_sync_model, th._h)
    out = C.c_void_p()
    for name, text in (("egnn", "not an EGNN training handle"), ("linear", "not a Linear training handle"),
                       ("painn", "not a PaiNN training handle")):
        if kind != name:
            refused(text, getattr(lib, f"lb_{name}_train_model"), C.byref(out))
    tgt, loss = d.to(eng.device).reshape(-1, eng.dim).contiguous(), C.c_double()
    if kind != "segnn":
        refused("lb_segnn_train_loss_grad: " + _BLOB if kind == "blob" else "null argument / not a SEGNN training handle",
                lib.lb_segnn_train_loss_grad, ptr(tgt), C.c_float(1.0), C.byref(loss), None)
    if kind != "egnn":
        refused("lb_egnn_train_loss_grad: " + _BLOB if kind == "blob" else "null argument / not an EGNN training handle",
                lib.lb_egnn_train_loss_grad, None, None, None, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), C.byref(loss), None)
    th.close()
