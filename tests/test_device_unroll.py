"""Push-forward from device weights (train.device_unroll), the parts that need no device.

lb_gns_pack_selftest stages the GNS inference images twice on the host - with the packers lb_gns_create uses, and by
replaying the job table that lb_gns_train_sync_model replays on the device, through the element function the device kernel
is compiled from and from the training handle's 128-padded weight layout - and counts the differing bytes: 0, for every
packing kind, depth, latent width and source assembly.  Then the C ABI, the default and the model contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from lagrangebench_amd import build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    from lagrangebench_amd import _lib
    return _lib.load()


def _model_and_blob(latent, depth, L, types, node_in, dim=2, seed=3, weight_scale=1.0, head_scale=1.0):
    """A GNS with random weights, biases and LayerNorm parameters (nothing 0 or 1 that a misplaced vector could hide behind)."""
    from lagrangebench_amd.models import GNS
    model = GNS(dim, latent, depth, L, 16, num_particle_types=types)
    params = model.init_params(seed, node_in, dim + 1)
    rng = np.random.default_rng(seed + 1)
    for name, leaves in params.items():
        for leaf, v in leaves.items():
            if leaf in ("b", "offset"):
                leaves[leaf] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
            elif leaf == "scale":
                leaves[leaf] = (1.0 + 0.2 * rng.standard_normal(v.shape)).astype(np.float32)
            elif leaf == "w":
                leaves[leaf] = (v * np.float32(weight_scale)).astype(np.float32)
    head = params[f"decoder/linear_{depth - 1}"]
    head["w"] = (head["w"] * np.float32(head_scale)).astype(np.float32)
    return model, params


def _desc(model, node_in, dim):
    from lagrangebench_amd._lib import GnsDesc
    d = GnsDesc()
    d.latent_size, d.blocks_per_step, d.num_mp_steps = model._latent_size, model._blocks_per_step, model._mp_steps
    d.embedding_size, d.num_particle_types = model._embedding_size, model._num_particle_types
    d.node_in, d.edge_in, d.out_dim = node_in, dim + 1, dim
    return d


def _selftest(lib, model, params, node_in, dim, kq=0):
    blob = np.ascontiguousarray(model.flatten(params), np.float32)
    n_bytes = C.c_int64(0)
    d = _desc(model, node_in, dim)
    diff = lib.lb_gns_pack_selftest(C.byref(d), kq, blob.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(blob.size),
                                    C.byref(n_bytes))
    assert diff >= 0, lib.lb_last_error()
    return int(diff), int(n_bytes.value)


# latent, depth (num_mlp_layers), message-passing steps, particle types (1: no embedding), node input columns, dim
MODELS = [
    (128, 2, 2, 1, 14, 2),     # the published shape; node input of one 32-column class (kq_node 4)
    (112, 2, 1, 9, 14, 2),     # a latent that is no power of two, with the embedding (14 + 16 = 30 columns: still kq_node 4)
    (64, 2, 3, 9, 30, 3),      # cmap path, three layers, 30 + 16 = 46 columns: the next kq_node class (8)
    (32, 2, 0, 1, 14, 2),      # no message passing: the encoder's launch has no projection piece, the decoder no M-split copy
    (128, 3, 1, 9, 14, 2),     # dense images
    (32, 3, 3, 1, 40, 3),      # dense, narrow, node input of the second class without the embedding
    (64, 4, 1, 1, 14, 2),      # dense, two middle Linears
    (128, 2, 1, 9, 14, 3),     # three output columns
]


@pytest.mark.parametrize("latent,depth,L,types,node_in,dim", MODELS)
def test_recorded_table_reproduces_the_host_packers(lib, latent, depth, L, types, node_in, dim):
    model, params = _model_and_blob(latent, depth, L, types, node_in, dim)
    diff, n_bytes = _selftest(lib, model, params, node_in, dim)
    assert n_bytes > 100_000 and diff == 0, (diff, n_bytes)


@pytest.mark.parametrize("head_scale", [2.0 ** -20, 2.0 ** 9])
@pytest.mark.parametrize("latent", [128, 64])
def test_scaled_decoder_head(lib, latent, head_scale):
    """The f16x2 copy of the head is packed times 2^sh, sh from max |w|: far below and far above fp16's comfortable range."""
    model, params = _model_and_blob(latent, 2, 1, 1, 14, head_scale=head_scale)
    assert _selftest(lib, model, params, 14, 2)[0] == 0


@pytest.mark.parametrize("depth", [2, 3])
def test_weights_whose_lo_halves_are_fp16_subnormals(lib, depth):
    """Weights around 2^-6: hi is a normal fp16, lo = fp16(w - hi) lies below 2^-14 - the conversion must round subnormals
    to nearest even exactly as the host packers do."""
    model, params = _model_and_blob(128, depth, 1, 1, 14, weight_scale=2.0 ** -6 * np.sqrt(128))
    w = params["proc0_edge/linear_1"]["w"]
    hi = w.astype(np.float16).astype(np.float32)
    lo = np.abs(w - hi)
    assert ((lo > 0) & (lo < 2.0 ** -14)).mean() > 0.5   # most lo halves are subnormal
    assert _selftest(lib, model, params, 14, 2)[0] == 0


def test_wider_node_rows_and_argument_checks(lib):
    model, params = _model_and_blob(32, 2, 1, 1, 14)
    assert _selftest(lib, model, params, 14, 2, kq=8)[0] == 0          # rows padded to 64 columns instead of 32
    blob = np.ascontiguousarray(model.flatten(params), np.float32)
    d = _desc(model, 14, 2)
    ptr = blob.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.lb_gns_pack_selftest(C.byref(d), 0, ptr, C.c_int64(blob.size - 1), None) < 0
    assert b"floats" in lib.lb_last_error()
    assert lib.lb_gns_pack_selftest(C.byref(d), 3, ptr, C.c_int64(blob.size), None) < 0
    assert lib.lb_gns_pack_selftest(None, 0, ptr, C.c_int64(blob.size), None) < 0
    assert lib.lb_gns_train_sync_model(None, None) == -1 and lib.lb_egnn_train_model(None, None) == -1
    assert lib.lb_gns_image_bytes(None) == -1


def test_header_and_ctypes_table_agree_on_the_new_entries(lib):
    from lagrangebench_amd import _lib
    src = open(os.path.join(ROOT, "include", "lbhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    new = ["lb_gns_train_sync_model", "lb_gns_image_bytes", "lb_gns_image_read", "lb_gns_pack_selftest", "lb_egnn_train_model"]
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib._SIGS and hasattr(lib, name), name
    assert _lib._SIGS["lb_gns_pack_selftest"][0] is C.c_int64 and _lib._SIGS["lb_gns_image_bytes"][0] is C.c_int64


def test_default_is_off_and_independent_of_device_data():
    from lagrangebench_amd.defaults import defaults
    assert defaults.train.device_unroll is False and defaults.train.device_data is False


def test_base_model_has_no_device_route():
    from lagrangebench_amd.models import SEGNN
    from lagrangebench_amd.models.base import BaseModel

    class StubEngine:
        has_pads = False

    class Stub(BaseModel):
        def init(self, key, sample):
            return {}, {}

    assert Stub().unroll_handle(StubEngine(), object(), {}) is None
    assert SEGNN.unroll_handle is BaseModel.unroll_handle       # SEGNN: the Trainer falls back to the host route
