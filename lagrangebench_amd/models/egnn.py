"""EGNN behind the reference's model API - lagrangebench/models/egnn.py:209-400.

Construction arguments are the reference's (egnn.py:250-266).  ``apply`` runs the HIP forward pass
(csrc/lb_egnn.hip) on the engine state the ``features`` came from and returns ``{"pos": (B, N, dim)}``
fp64 tensors that hold the network's fp32 positions (the reference runs EGNN under an fp32 policy,
runner.py:71-72, and ``jnp.concatenate`` promotes the prediction back into the fp64 window).

* ``displacement_fn`` / ``shift_fn`` are taken for signature parity only: the device code applies the
  case's own space (periodic minimum image / ``mod`` on periodic boxes, plain differences and sums in free
  space), which is what the runner passes (runner.py:247-254).
* ``normalization_stats`` likewise: the velocity is un-normalised with the case's statistics, the ones the
  runner passes (runner.py:264).
* Not built (``NotImplementedError``): ``attention=True`` (no config uses it), an activation other than
  SiLU, and a hidden size that is not a multiple of 16 or exceeds 128; training (``train_handle``,
  csrc/lb_train_egnn.h) with ``normalize=True``.

Parameters: ``{"scalar_emb": {"w", "b"}, "layer_{n}/edge_{0,1}", "layer_{n}/node_{0,1}", "layer_{n}/pos_0",
"layer_{n}/vel_0": {"w", "b"}, "layer_{n}/pos_1", "layer_{n}/vel_1": {"w"}}`` with ``w`` of shape
(fan_in, fan_out); ``utils.egnn_params_to_haiku`` / ``egnn_params_from_haiku`` map them onto the Haiku
module names (include/lbhip.h: lb_egnn_create lists both).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from .._lib import EgnnDesc
from ..engine import EgnnHandle, EgnnTrainHandle
from ..utils import NodeType, egnn_params_from_haiku, egnn_params_to_haiku
from .base import BaseModel


def _is_silu(fn) -> bool:
    if fn is None or (isinstance(fn, str) and fn.lower() == "silu"):
        return True
    try:
        import torch
        if fn is torch.nn.functional.silu or fn is torch.nn.SiLU or isinstance(fn, torch.nn.SiLU):
            return True
    except ImportError:  # pragma: no cover
        pass
    return getattr(fn, "__name__", "") == "silu"


class EGNN(BaseModel):
    def __init__(self, hidden_size: int, output_size: int, dt: float, n_vels: int, displacement_fn=None,
                 shift_fn=None, normalization_stats: Optional[Dict] = None, act_fn=None, num_mp_steps: int = 4,
                 homogeneous_particles: bool = True, residual: bool = True, attention: bool = False,
                 normalize: bool = False, tanh: bool = False):
        if attention:
            raise NotImplementedError("EGNN: attention=True is not built (no published config uses it)")
        if not _is_silu(act_fn):
            raise NotImplementedError(f"EGNN: act_fn {act_fn!r} is not built (SiLU only)")
        if hidden_size % 16 or not 16 <= hidden_size <= 128:
            raise NotImplementedError(f"EGNN: hidden_size {hidden_size} is not built (a multiple of 16 up to 128)")
        if num_mp_steps < 1:
            raise ValueError("EGNN: num_mp_steps must be >= 1")
        if not 1 <= n_vels <= 9:
            raise NotImplementedError(f"EGNN: n_vels {n_vels} is not built (1 .. 9)")
        self._hidden_size = hidden_size
        self._output_size = output_size
        self._num_mp_steps = num_mp_steps
        self._residual = residual
        self._attention = attention
        self._normalize = normalize
        self._tanh = tanh
        self._dt = dt / num_mp_steps  # egnn.py:301: the layers' UniformScaling(dt) initialiser scale
        self._displacement_fn = displacement_fn
        self._shift_fn = shift_fn
        self._normalization_stats = normalization_stats
        self._n_vels = n_vels
        self._homogeneous_particles = homogeneous_particles
        self._handles: Dict[Tuple[int, int], tuple] = {}

    # ------------------------------------------------------------------ parameters
    def node_in(self) -> int:
        return self._n_vels + (0 if self._homogeneous_particles else NodeType.SIZE)

    def leaves(self, has_force: bool) -> List[Tuple[str, str, Tuple[int, ...]]]:
        """(module, leaf, shape) in lb_egnn_create's blob order."""
        H, A = self._hidden_size, 1 if has_force else 0
        out = [("scalar_emb", "w", (self.node_in(), H)), ("scalar_emb", "b", (H,))]
        for n in range(self._num_mp_steps):
            p = f"layer_{n}/"
            out += [(p + "edge_0", "w", (2 * H + 2, H)), (p + "edge_0", "b", (H,)),
                    (p + "edge_1", "w", (H, H)), (p + "edge_1", "b", (H,)),
                    (p + "node_0", "w", (2 * H + A, H)), (p + "node_0", "b", (H,)),
                    (p + "node_1", "w", (H, H)), (p + "node_1", "b", (H,)),
                    (p + "pos_0", "w", (H, H)), (p + "pos_0", "b", (H,)), (p + "pos_1", "w", (H, 1)),
                    (p + "vel_0", "w", (H, H)), (p + "vel_0", "b", (H,)), (p + "vel_1", "w", (H, 1))]
        return out

    def init_params(self, seed, has_force: bool) -> Dict:
        """The reference's initialisers (models/utils.py:12-53, egnn.py:95-112): every weight Xavier-uniform
        (VarianceScaling(1, fan_avg, uniform): U(+-sqrt(6 / (fan_in + fan_out)))), biases 0; the two (H, 1)
        outputs UniformScaling(dt / num_mp_steps): U(+-(dt / L) sqrt(3 / H))."""
        rng = np.random.default_rng(seed)
        p: Dict[str, Dict[str, np.ndarray]] = {}
        for mod, leaf, shape in self.leaves(has_force):
            if leaf == "b":
                v = np.zeros(shape)
            elif mod.endswith("pos_1") or mod.endswith("vel_1"):
                lim = self._dt * np.sqrt(3.0 / shape[0])
                v = rng.uniform(-lim, lim, size=shape)
            else:
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                v = rng.uniform(-lim, lim, size=shape)
            p.setdefault(mod, {})[leaf] = v.astype(np.float32)
        return p

    def init(self, key, sample):
        features, _ = sample
        seed = int(np.asarray(key).ravel()[-1]) if key is not None else 0
        return self.init_params(seed, "force" in features), {}

    @staticmethod
    def _has_force(params) -> bool:
        first = next(k for k in params if k.endswith("node_0"))
        H = np.asarray(params[first]["w"]).shape[1]
        return np.asarray(params[first]["w"]).shape[0] == 2 * H + 1

    def flatten(self, params) -> np.ndarray:
        """Weights in the order lb_egnn_create expects (include/lbhip.h)."""
        out = []
        for mod, leaf, shape in self.leaves(self._has_force(params)):
            v = np.asarray(params[mod][leaf], np.float32)
            if v.shape != shape:
                raise ValueError(f"EGNN params[{mod!r}][{leaf!r}]: expected {shape}, got {v.shape}")
            out.append(v.ravel())
        return np.concatenate(out)

    def unflatten(self, blob, like=None, has_force: Optional[bool] = None) -> Dict:
        """Inverse of flatten (`like` or `has_force` tells whether the node MLP has the |force| row)."""
        blob = np.asarray(blob, np.float32)
        if has_force is None:
            has_force = self._has_force(like) if like is not None else \
                blob.size == sum(int(np.prod(s)) for _, _, s in self.leaves(True))
        out, o = {}, 0
        for mod, leaf, shape in self.leaves(has_force):
            n = int(np.prod(shape))
            out.setdefault(mod, {})[leaf] = blob[o:o + n].reshape(shape).copy()
            o += n
        if o != blob.size:
            raise ValueError(f"EGNN.unflatten: blob has {blob.size} floats, the model {o}")
        return out

    def _desc(self) -> EgnnDesc:
        d = EgnnDesc()
        d.hidden, d.num_mp_steps, d.n_vels = self._hidden_size, self._num_mp_steps, self._n_vels
        d.homogeneous = int(bool(self._homogeneous_particles))
        d.residual, d.normalize, d.tanh_pos = int(bool(self._residual)), int(bool(self._normalize)), int(bool(self._tanh))
        return d

    # ------------------------------------------------------------------ engine binding (models/base.py)
    _FORWARD, _OUTPUT, _HAIKU_KEY = "egnn_forward", "pos", "scalar_emb"

    def _create(self, engine, params, state):
        return engine._new_handle(EgnnHandle, "lb_egnn_create", self._desc(), self.flatten(params))

    def _from_haiku(self, hk_params):
        return egnn_params_from_haiku(hk_params, self)

    def _to_haiku(self, params):
        return egnn_params_to_haiku(params, self)

    # ------------------------------------------------------------------ training
    NORMALIZE_REFUSAL = ("EGNN training with normalize=True is not built: every radius graph holds self-edges, and the "
                         "derivative of coord_diff / (sqrt(radial) + 1e-8) at radial = 0 is 0 * inf - the reference's own "
                         "gradient is NaN for num_mp_steps >= 2 (inference runs it)")

    def check_trainable(self) -> None:
        if self._normalize:
            raise NotImplementedError(self.NORMALIZE_REFUSAL)

    def _train_create(self, engine, params):
        """csrc/lb_train_egnn.h: ``loss_grad(targets, loss_weight, want_pred=False)`` takes the case's {"pos", "vel",
        "acc"} targets and the loss weights."""
        return engine._new_handle(EgnnTrainHandle, "lb_egnn_train_create", self._desc(), self.flatten(params))

    def unroll_handle(self, engine, th, params_like):
        """The training handle's own inference view (csrc/lb_train_egnn.h): it reads th's weight blob, nothing to refresh."""
        self._check_padded(engine)
        return th.model_handle()

    def loss_grad(self, th, target, loss_weight) -> float:
        """_mse over every output the model predicts (pos, vel, acc)."""
        self._check_padded(th.engine)
        return th.loss_grad(target, loss_weight)
