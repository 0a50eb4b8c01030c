"""The frame the three device training steps share (csrc/lb_train.hip: train_handle_init, train_step_begin / _end,
train_ensure, train_loss_grad_guarded), on each model's smallest training case with a latent / hidden size below 128, so the
caller's blob reaches the padded device layout through the handle's index map."""
import numpy as np
import pytest
import torch


def _setup(kind):
    """-> (model, engine, params, blob, step): step(th) = one loss + gradient pass on the engine's window, returns the loss."""
    from lagrangebench_amd.data import make_case
    from tests._common import hip_case, make_params
    g = torch.Generator().manual_seed(5)
    if kind == "egnn":   # tests/test_egnn_train.py: rpf2d_b1 at the width of h64
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
    return model, feats.engine, params, np.asarray(blob, np.float32), step


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gns", "segnn", "egnn"])
def test_training_frame_is_reproducible_across_calls_writes_and_handles(kind):
    """On one handle: (a) two zero_grad + loss_grad passes give the same loss and the same gradient bytes; (b) so does a pass
    after write("weights", read("weights")) - the initialiser and write scatter through the same map, and the packed operands
    follow a weight change; (c) no step was repeated by the guard; (d) a second handle made from the same parameters gives
    the bytes of the first; (e) the GNS entry still refuses an EGNN handle."""
    model, eng, params, blob, step = _setup(kind)
    th = model.train_handle(eng, params)
    assert th.n_floats < th.device_floats()   # padded device layout: the index map is in use

    def once(h):
        h.zero_grad()
        loss = step(h)
        return loss, h.read("grads").tobytes()

    loss_a, g_a = once(th)
    assert np.isfinite(loss_a) and np.abs(np.frombuffer(g_a, np.float32)).max() > 0
    assert once(th) == (loss_a, g_a)                                   # (a)
    w = th.read("weights")
    assert np.array_equal(w, blob)
    th.write("weights", w)
    assert th.read("weights").tobytes() == w.tobytes()
    assert once(th) == (loss_a, g_a)                                   # (b)
    assert th.math_fallbacks() == 0 and th.sort_fallbacks() == 0       # (c)
    th2 = model.train_handle(eng, params)
    assert once(th2) == (loss_a, g_a)                                  # (d)
    assert th2.math_fallbacks() == 0 and th2.sort_fallbacks() == 0
    th2.close()
    if kind == "egnn":                                                 # (e)
        from lagrangebench_amd._lib import LbHipError
        from lagrangebench_amd.engine import GnsTrainHandle
        with pytest.raises(LbHipError, match="an EGNN training handle: its loss needs the pos / vel / acc targets"):
            GnsTrainHandle.loss_grad(th, torch.zeros((eng.B, eng.N, eng.dim)))
    th.close()
