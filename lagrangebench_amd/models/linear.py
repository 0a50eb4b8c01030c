"""The Linear baseline behind the reference's model API - lagrangebench/models/linear.py.

``Linear(dim_out)`` as in the reference (linear.py:21-28).  ``apply`` runs the HIP forward pass (csrc/lb_linear.hip) on the
engine state the ``features`` came from and returns ``{"acc": (B, N, dim)}``, the normalised acceleration in fp32 (the
reference runs every model under an fp32 policy, runner.py:71-72); the rollout integrates it with the case's integrator,
as it does GNS's.

``acc_i = x_i W + b`` with ``x_i = [vel_hist | vel_mag | bound | force | float(particle_type_i)]``, each block present only
if the case has it (linear.py:35-41): the engine's node features in the engine's own column order, then the raw type id as
a value (no one-hot).  ``W`` is ``(F + 1, dim_out)`` with ``F = engine.node_in``; ``F + 1 > 64`` (one node row of the
engine) is not built (``NotImplementedError``).

Parameters: ``{"linear": {"w": (F + 1, dim_out), "b": (dim_out,)}}``; the Haiku tree names the same two leaves
``linear/~/linear`` (``hk.Linear`` made in ``Linear.__init__``).  The blob of ``flatten`` is ``w`` row-major, then ``b``
(include/lbhip.h: lb_linear_create).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .._lib import LinearDesc
from ..engine import LinearHandle, LinearTrainHandle
from .base import BaseModel

MAX_IN = 64  # one node row of the engine (csrc/lb_linear.hip: LN_KPAD)
_HAIKU_MODULE = "linear/~/linear"


class Linear(BaseModel):
    def __init__(self, dim_out: int):
        if not 1 <= int(dim_out) <= 3:
            raise ValueError(f"Linear: dim_out {dim_out} must be the particle dimension (1 .. 3)")
        self._dim_out = int(dim_out)
        self._handles: Dict[Tuple[int, int], tuple] = {}

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def n_in(features) -> int:
        """Width of [vel_hist | vel_mag | bound | force | particle_type] for the blocks `features` holds (linear.py:35-39)."""
        engine = getattr(features, "engine", None)
        if engine is not None:   # a FeatureDict: the engine knows its row without fetching a block
            return engine.node_in + 1
        return sum(int(features[k].shape[-1]) for k in ("vel_hist", "vel_mag", "bound", "force") if k in features) + 1

    def _check_width(self, n_in: int) -> None:
        if n_in > MAX_IN:
            raise NotImplementedError(f"Linear: {n_in} inputs are not built (up to {MAX_IN}: one {MAX_IN}-float node row)")

    def init_params(self, seed, n_in: int) -> Dict:
        """hk.Linear's initialisers: w ~ TruncatedNormal(stddev = 1 / sqrt(fan_in)) (a standard normal cut at +-2, times
        stddev), b = 0."""
        self._check_width(n_in)
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((n_in, self._dim_out))
        bad = np.abs(z) > 2.0
        while bad.any():   # resample the tails: the truncated normal on [-2, 2]
            z[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(z) > 2.0
        w = (z / np.sqrt(n_in)).astype(np.float32)
        return {"linear": {"w": w, "b": np.zeros((self._dim_out,), np.float32)}}

    def init(self, key, sample):
        features, _ = sample
        seed = int(np.asarray(key).ravel()[-1]) if key is not None else 0
        return self.init_params(seed, self.n_in(features)), {}

    def flatten(self, params, state=None) -> np.ndarray:
        """Weights in the order lb_linear_create expects (include/lbhip.h): w row-major, then b."""
        w = np.asarray(params["linear"]["w"], np.float32)
        b = np.asarray(params["linear"]["b"], np.float32)
        if w.ndim != 2 or w.shape[1] != self._dim_out or b.shape != (self._dim_out,):
            raise ValueError(f"Linear params: expected w (F + 1, {self._dim_out}) and b ({self._dim_out},), got {w.shape}, {b.shape}")
        self._check_width(w.shape[0])
        return np.concatenate([w.ravel(), b])

    def unflatten(self, blob, like=None) -> Dict:
        """Inverse of flatten (the input width follows from the blob's length)."""
        blob = np.asarray(blob, np.float32)
        d = self._dim_out
        if blob.ndim != 1 or blob.size % d or blob.size < 2 * d:
            raise ValueError(f"Linear.unflatten: a blob of {blob.size} floats is no (F + 1, {d}) matrix and ({d},) bias")
        n_in = blob.size // d - 1
        return {"linear": {"w": blob[:n_in * d].reshape(n_in, d).copy(), "b": blob[n_in * d:].copy()}}

    def _desc(self, params) -> LinearDesc:
        d = LinearDesc()
        d.n_in, d.out_dim = int(np.asarray(params["linear"]["w"]).shape[0]), self._dim_out
        return d

    # ------------------------------------------------------------------ engine binding (models/base.py)
    _FORWARD, _OUTPUT, _HAIKU_KEY = "linear_forward", "acc", "linear"
    _PADDED_OK = False   # padded input stays GNS only

    def _create(self, engine, params, state):
        return engine._new_handle(LinearHandle, "lb_linear_create", self._desc(params), self.flatten(params))

    def _from_haiku(self, hk_params):
        if _HAIKU_MODULE not in hk_params:
            raise ValueError(f"Linear checkpoint: module {_HAIKU_MODULE!r} missing (found {sorted(hk_params)})")
        m = hk_params[_HAIKU_MODULE]
        return {"linear": {"w": np.asarray(m["w"], np.float32), "b": np.asarray(m["b"], np.float32)}}

    def _to_haiku(self, params):
        m = params["linear"]
        return {_HAIKU_MODULE: {"w": np.asarray(m["w"], np.float32), "b": np.asarray(m["b"], np.float32)}}

    # ------------------------------------------------------------------ training
    def check_trainable(self) -> None:
        pass

    def _train_create(self, engine, params):
        """csrc/lb_train_linear.h: GnsTrainHandle's calls (one "acc" target), and ``model_handle()``."""
        return engine._new_handle(LinearTrainHandle, "lb_linear_train_create", self._desc(params), self.flatten(params))

    def unroll_handle(self, engine, th, params_like):
        """The training handle's own inference view (csrc/lb_train_linear.h): it reads th's weight blob, nothing to refresh."""
        self._check_padded(engine)
        return th.model_handle()
