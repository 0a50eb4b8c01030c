"""Device memory of the engine-side objects (csrc/lb_arena.h): closing an object gives back what it took, and a training
handle whose buffers were regrown computes what a fresh handle computes.  Smallest cases of the suite: small3d / small2d
with two message-passing steps, rpf2d at scale 0.5 for EGNN."""
import functools
import gc

import numpy as np
import pytest
import torch

from tests._common import hip_case, make_params

pytestmark = pytest.mark.gpu

FORWARD = ["gns", "gns_mlp3", "segnn", "segnn_gen_norm", "egnn", "painn"]
TRAIN = ["gns_train", "segnn_train", "egnn_train"]


@functools.lru_cache(maxsize=None)
def _static(kind):
    """What a cycle does not have to make again: dataset, model, parameters, positions (B, N, T, dim), particle types."""
    from lagrangebench_amd.data import make_case
    state, isl = {}, None
    if kind in ("gns", "gns_mlp3", "gns_train"):   # tests/test_train_frame_gpu.py: small3d, L = 2, B = 1, latent 64
        from lagrangebench_amd.models import GNS
        B, depth = 1, 3 if kind == "gns_mlp3" else 2
        ds = make_case("small3d", n_trajs=B, extra_seq_length=3)
        params = make_params(ds, num_mp_steps=2, decoder_scale=1.0, latent_size=64, blocks_per_step=depth)
        model = GNS(len(ds.box), 64, depth, 2, 16)
    elif kind in ("segnn", "segnn_train"):   # tests/test_segnn.py, tests/test_segnn_train.py: small2d, L = 2, B = 2
        from lagrangebench_amd.models import SEGNN, node_irreps
        from oracle import segnn_oracle as S
        B = 2
        ds = make_case("small2d", n_trajs=B, extra_seq_length=3)
        ds.magnitude_features = True
        homog = bool(np.all(ds[0][1] == 0))
        irr = node_irreps(ds.metadata, ds.input_seq_length, ds.external_force_fn is not None, True, homog)
        model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=2, n_vels=ds.input_seq_length - 1,
                      homogeneous_particles=homog, blocks_per_step=2)
        params = S.segnn_init(np.random.default_rng(11), node_ns=model._node_ns, node_nv=model._node_nv, num_mp_steps=2,
                              blocks_per_step=2, random_bias=True)
        if kind == "segnn_train":
            params = {k: v for k, v in params.items() if isinstance(v, dict)}
    elif kind == "segnn_gen_norm":   # tests/test_segnn_irreps.py: small2d, attributes up to l = 2, BatchNorm
        from lagrangebench_amd.models import SEGNN, node_irreps
        from oracle import segnn_irreps_oracle as G
        B = 2
        ds = make_case("small2d", n_trajs=B, extra_seq_length=3)
        ds.magnitude_features = True
        homog = bool(np.all(ds[0][1] == 0))
        has_force = ds.external_force_fn is not None
        irr = node_irreps(ds.metadata, ds.input_seq_length, has_force, True, homog)
        model = SEGNN(irr, "1x1o+1x0e", 64, 1, 2, "1x1o", num_mp_steps=2, n_vels=ds.input_seq_length - 1,
                      homogeneous_particles=homog, norm="batch", blocks_per_step=2)
        assert model.generic
        params = G.segnn_init(np.random.default_rng(7), model._node_chunks, num_mp_steps=2, scalar_units=64, lmax_hidden=1,
                              lmax_attr=2, blocks_per_step=2, norm="batch", random_bias=True)
    elif kind in ("egnn", "egnn_train"):   # tests/test_egnn_train.py: rpf2d at scale 0.5, B = 1, hidden 64
        from lagrangebench_amd.models import EGNN
        from tests._egnn_oracle import random_biases
        B, isl = 1, 6
        ds = make_case("rpf2d", n_trajs=B, extra_seq_length=3, input_seq_length=isl, scale=0.5)
        model = EGNN(64, 1, 0.01, isl - 1, num_mp_steps=3)
        params = random_biases(model.init_params(7, ds.external_force_fn is not None), 8)
    else:   # tests/test_painn_gpu.py at hidden 32, L = 2
        from lagrangebench_amd.models import PaiNN
        from lagrangebench_amd.models.painn import cosine_cutoff, gaussian_rbf
        from tests._painn_oracle import random_biases
        assert kind == "painn"
        B, isl = 1, 6
        ds = make_case("small3d", n_trajs=B, extra_seq_length=3, input_seq_length=isl)
        ds.magnitude_features = True
        r = 1.5 * ds.metadata["default_connectivity_radius"]
        model = PaiNN(32, 1, 2, gaussian_rbf(20, r, trainable=True), cosine_cutoff(r), isl - 1)
        params, state = model.init_params(3, ds.external_force_fn is not None, False)
        params = random_biases(params, 4)
    pos = np.stack([ds[b][0] for b in range(B)])
    pt = np.stack([ds[b][1] for b in range(B)])
    return dict(kind=kind, ds=ds, model=model, params=params, state=state, pos=pos, pt=pt, isl=isl or ds.input_seq_length)


def _load(st, case, pos):
    """Window `pos[:, :, :isl]` and a freshly allocated neighbor list on `case`'s engine (made at the first call)."""
    feats, _ = case.allocate_eval((pos[:, :, :st["isl"]], st["pt"]))
    return feats


def _step(st, th, pos):
    """One loss + gradient pass of training handle `th` on the engine's window (`pos`: what was loaded)."""
    g = torch.Generator().manual_seed(5)
    shape = (pos.shape[0], pos.shape[1], pos.shape[3])
    if st["kind"] == "egnn_train":
        tg = {"pos": torch.as_tensor(pos[:, :, st["isl"] - 1], dtype=torch.float64) + 1e-3 * torch.randn(shape, generator=g, dtype=torch.float64)}
        return th.loss_grad(tg, {"pos": 1.0, "vel": 0.0, "acc": 0.0})
    return th.loss_grad(torch.randn(shape, generator=g), 1.0)


def _free_bytes():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def _cycle(st, measure=False):
    """engine -> model or training handle -> one forward / loss_grad -> close everything.  measure: the free device memory
    while everything is still open."""
    model, case = st["model"], hip_case(st["ds"])
    feats = _load(st, case, st["pos"])
    eng = feats.engine
    if st["kind"] in TRAIN:
        h = model.train_handle(eng, st["params"])
        h.zero_grad()
        assert np.isfinite(_step(st, h, st["pos"]))
    else:
        h = model.handle(eng, st["params"], st["state"])
        out = model.apply(st["params"], st["state"], (feats, st["pt"]))[0]
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        del out
        model._handles.clear()
    torch.cuda.synchronize()
    used = torch.cuda.mem_get_info()[0] if measure else None
    h.close()
    eng.close()
    case._engines.clear()
    del h, eng, feats, case
    return used


@pytest.mark.parametrize("kind", FORWARD + TRAIN)
def test_create_destroy_cycles_give_the_memory_back(kind):
    """Ten cycles; free device memory after the tenth is not below that after the second by more than one object's
    footprint, measured as the drop across the first create-and-use.  Catches a destroy that frees nothing or a regrow set
    that is never released (one small leaked buffer is tests/test_device_memory.py's business)."""
    st = _static(kind)
    free0 = _free_bytes()
    footprint = free0 - _cycle(st, measure=True)
    free = [_free_bytes()]
    for _ in range(9):
        _cycle(st)
        free.append(_free_bytes())
    print(f"{kind}: footprint {footprint} B, free after cycles 1, 2, 10: {free[0]}, {free[1]}, {free[9]}")
    assert free[1] - free[9] <= footprint


@pytest.mark.parametrize("kind", TRAIN)
def test_regrown_training_handle_equals_a_fresh_one(kind):
    """A handle stepped on window A, then on window B = A contracted by 0.6 about the box centre (a clump with more edges than
    the growth rule E + E / 8 + 1024 left room for, so the engine's edge buffers and the handle's scratch are regrown),
    gives on B the loss and gradient bytes of a fresh handle that only ever saw B."""
    st = _static(kind)
    model, pos_a = st["model"], st["pos"]
    c = 0.5 * np.asarray(st["ds"].box, np.float64)
    pos_b = c + 0.6 * (pos_a - c)

    def once(h, pos):
        h.zero_grad()
        loss = _step(st, h, pos)
        return loss, h.read("grads").tobytes()

    case = hip_case(st["ds"])
    eng = _load(st, case, pos_a).engine
    th = model.train_handle(eng, st["params"])
    once(th, pos_a)
    e_a = eng.stats()["n_edges_total"]
    assert _load(st, case, pos_b).engine is eng
    e_b = eng.stats()["n_edges_total"]
    print(f"{kind}: E_A = {e_a}, E_B = {e_b}, bound {e_a + e_a // 8 + 1024}")
    assert e_b > e_a + e_a // 8 + 1024
    regrown = once(th, pos_b)

    case2 = hip_case(st["ds"])
    eng2 = _load(st, case2, pos_b).engine
    assert eng2 is not eng and eng2.stats()["n_edges_total"] == e_b
    th2 = model.train_handle(eng2, st["params"])
    fresh = once(th2, pos_b)
    assert np.isfinite(fresh[0]) and np.abs(np.frombuffer(fresh[1], np.float32)).max() > 0
    assert regrown[0] == fresh[0]
    assert regrown[1] == fresh[1]
    assert th.math_fallbacks() == th2.math_fallbacks()
    for h in (th, th2):
        h.close()
    for e in (eng, eng2):
        e.close()
