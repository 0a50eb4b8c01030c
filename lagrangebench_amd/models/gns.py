"""GNS behind the reference's model API - lagrangebench/models/gns.py:18-171.

Construction arguments are the reference's (gns.py:36-44).  ``init`` draws haiku-default
initial parameters; ``apply`` runs the HIP forward pass on the engine
state the ``features`` came from (encoder -> num_mp_steps x [edge MLP, segment_sum, node MLP]
-> decoder, lagrangebench_amd/csrc/lb_gns.hip).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .._lib import GnsDesc
from ..engine import GnsHandle, GnsTrainHandle
from ..utils import NodeType, gns_params_from_haiku, gns_params_to_haiku
from .base import BaseModel


def layer_names(num_mp_steps: int) -> List[str]:
    """MLP blocks in module-creation order (gns.py:65-133)."""
    names = ["enc_node", "enc_edge"]
    for k in range(num_mp_steps):
        names += [f"proc{k}_edge", f"proc{k}_node"]
    return names + ["decoder"]


def _trunc_normal(rng, shape, stddev):
    out = rng.standard_normal(size=shape)
    bad = np.abs(out) > 2.0
    while bad.any():
        out[bad] = rng.standard_normal(size=int(bad.sum()))
        bad = np.abs(out) > 2.0
    return (out * stddev).astype(np.float32)


class GNS(BaseModel):
    _PADDED_OK = True  # pads are in no edge and outside the loss (csrc/lb_neighbor.hip, csrc/lb_train.hip)
    def __init__(self, particle_dimension: int, latent_size: int, blocks_per_step: int,
                 num_mp_steps: int, particle_type_embedding_size: int,
                 num_particle_types: int = NodeType.SIZE):
        self._output_size = particle_dimension
        self._latent_size = latent_size
        self._blocks_per_step = blocks_per_step
        self._mp_steps = num_mp_steps
        self._num_particle_types = num_particle_types
        self._embedding_size = particle_type_embedding_size
        self._handles: Dict[Tuple[int, int], tuple] = {}

    # ------------------------------------------------------------------ parameters
    def _widths(self, features) -> Tuple[int, int]:
        node_in = sum(int(np.prod(features[k].shape[-1:])) for k in ["vel_hist", "vel_mag", "bound", "force"]
                      if k in features)
        edge_in = int(features["rel_disp"].shape[-1]) + 1
        return node_in, edge_in

    def init_params(self, seed, node_in: int, edge_in: int, decoder_scale: float = 1.0) -> Dict:
        """Haiku defaults: Linear w ~ TruncatedNormal(1/sqrt(fan_in)), b = 0; LayerNorm scale 1,
        offset 0; Embed ~ TruncatedNormal(1).  Keys: "embed", "<block>/linear_{0,1}",
        "<block>/layer_norm" (see layer_names)."""
        rng = np.random.default_rng(seed)
        p: Dict[str, Dict[str, np.ndarray]] = {}
        L, D = self._mp_steps, self._latent_size
        if self._num_particle_types > 1:
            p["embed"] = {"embeddings": _trunc_normal(rng, (self._num_particle_types, self._embedding_size), 1.0)}
            node_in = node_in + self._embedding_size

        def mlp(name, fan_in, out, ln=True, scale=1.0):
            sizes = [D] * (self._blocks_per_step - 1) + [out]
            d = fan_in
            for li, s in enumerate(sizes):
                w = _trunc_normal(rng, (d, s), 1.0 / np.sqrt(d))
                if li == len(sizes) - 1 and scale != 1.0:
                    w = (w * scale).astype(np.float32)
                p[f"{name}/linear_{li}"] = {"w": w, "b": np.zeros((s,), np.float32)}
                d = s
            if ln:
                p[f"{name}/layer_norm"] = {"scale": np.ones((out,), np.float32),
                                           "offset": np.zeros((out,), np.float32)}

        mlp("enc_node", node_in, D)
        mlp("enc_edge", edge_in, D)
        for k in range(L):
            mlp(f"proc{k}_edge", 3 * D, D)
            mlp(f"proc{k}_node", 2 * D, D)
        mlp("decoder", D, self._output_size, ln=False, scale=decoder_scale)
        return p

    def init(self, key, sample):
        features, _ = sample
        node_in, edge_in = self._widths(features)
        seed = int(np.asarray(key).ravel()[-1]) if key is not None else 0
        return self.init_params(seed, node_in, edge_in), {}

    def flatten(self, params) -> np.ndarray:
        """Weights in the order lb_gns_create expects (include/lbhip.h)."""
        out = []
        if self._num_particle_types > 1:
            out.append(np.asarray(params["embed"]["embeddings"], np.float32).ravel())
        for name in layer_names(self._mp_steps):
            for li in range(self._blocks_per_step):
                lin = params[f"{name}/linear_{li}"]
                out += [np.asarray(lin["w"], np.float32).ravel(), np.asarray(lin["b"], np.float32).ravel()]
            ln = params.get(f"{name}/layer_norm")
            if ln is not None:
                out += [np.asarray(ln["scale"], np.float32).ravel(), np.asarray(ln["offset"], np.float32).ravel()]
        return np.concatenate(out)

    def unflatten(self, blob, like) -> Dict:
        """Inverse of flatten: the flat blob (weights, gradients or optimiser moments of the training handle) back
        into a parameter tree shaped like `like`."""
        blob = np.asarray(blob, np.float32)
        out, o = {}, 0

        def take(mod, leaf):
            nonlocal o
            shape = np.asarray(like[mod][leaf]).shape
            n = int(np.prod(shape))
            out.setdefault(mod, {})[leaf] = blob[o:o + n].reshape(shape).copy()
            o += n
        if self._num_particle_types > 1:
            take("embed", "embeddings")
        for name in layer_names(self._mp_steps):
            for li in range(self._blocks_per_step):
                take(f"{name}/linear_{li}", "w")
                take(f"{name}/linear_{li}", "b")
            if f"{name}/layer_norm" in like:
                take(f"{name}/layer_norm", "scale")
                take(f"{name}/layer_norm", "offset")
        assert o == blob.size, (o, blob.size)
        return out

    # ------------------------------------------------------------------ engine binding (models/base.py)
    _FORWARD, _OUTPUT, _HAIKU_KEY = "gns_forward", "acc", "enc_node/linear_0"
    _WINDOW_GRAD = True
    _EXACT_FORWARD = True

    def _desc(self, engine) -> GnsDesc:
        d = GnsDesc()
        d.latent_size, d.blocks_per_step, d.num_mp_steps = self._latent_size, self._blocks_per_step, self._mp_steps
        d.embedding_size, d.num_particle_types = self._embedding_size, self._num_particle_types
        d.node_in, d.edge_in, d.out_dim = engine.node_in, engine.dim + 1, self._output_size
        return d

    def _create(self, engine, params, state):
        return engine._new_handle(GnsHandle, "lb_gns_create", self._desc(engine), self.flatten(params))

    def _from_haiku(self, hk_params):
        return gns_params_from_haiku(hk_params, self._mp_steps, self._blocks_per_step)

    def _to_haiku(self, params):
        return gns_params_to_haiku(params, self._mp_steps, self._blocks_per_step)

    # ------------------------------------------------------------------ training
    def check_trainable(self) -> None:
        if not 4 <= self._latent_size <= 128 or not 2 <= self._blocks_per_step <= 8:
            # csrc/lb_train.hip: the training step runs on 128-wide rows (narrower latents are zero-padded) with two to
            # eight Linears per MLP
            raise NotImplementedError(
                f"training is built for GNS with latent_size <= 128 and 2 <= num_mlp_layers <= 8 (got latent_size "
                f"{self._latent_size}, num_mlp_layers {self._blocks_per_step}); inference runs every size")

    def _train_create(self, engine, params):
        """csrc/lb_train.hip."""
        return engine._new_handle(GnsTrainHandle, "lb_gns_train_create", self._desc(engine), self.flatten(params))

    def unroll_handle(self, engine, th, params_like):
        """csrc/lb_gns_repack.hip: one inference handle per training handle, made by the host route (``_create`` from
        `params_like`) the first time and kept for the life of `th`; at EVERY use its packed images are re-made on the device
        from th's current weights (``th.sync_model``), so what it computes never depends on `params_like`'s values."""
        self._check_padded(engine)
        h = getattr(th, "_unroll_model", None)
        if h is None or not h._h or h.engine is not engine:
            h = th._unroll_model = self._create(engine, params_like, None)
        th.sync_model(h)
        return h
