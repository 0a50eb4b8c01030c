"""PaiNN behind the reference's model API - lagrangebench/models/painn.py.

Construction arguments are the reference's (painn.py:372-386).  ``apply`` runs the HIP forward pass
(csrc/lb_painn.hip) on the engine state the ``features`` came from and returns ``{"acc": (B, N, dim)}``, the
normalised acceleration in fp32 (the reference runs every model under an fp32 policy, runner.py:71-72); the
rollout integrates it with the case's integrator, as it does GNS's.

* ``radial_basis_fn`` is a ``gaussian_rbf`` and ``cutoff_fn`` a ``cosine_cutoff`` (or None): small descriptor
  objects standing for the reference's closures, since there is no ``hk.transform`` here.  As in the reference,
  their radius is taken as given - the runner passes the physical ``1.5 * default_connectivity_radius`` while the
  network's norms are in units of that radius.
* The case must carry the velocity magnitudes (``magnitude_features``): they are the model's scalar inputs
  (the reference's runner asserts it).
* Not built (``NotImplementedError``): an activation other than SiLU, ``output_size != 1``,
  ``gaussian_rbf(centered=True)`` (broken in the reference: it reads an undefined ``width``) and a hidden size
  that is not a multiple of 16 or exceeds 128; training (``train_handle``, csrc/lb_train_painn.h) with a hidden
  size below 64.

Parameters: ``{"scalar_embedding": {"w", "b"}, "vector_embedding": {"w"}, "filter_net": {"w", "b"},
"layer_{p}/interaction_{0,1}", "layer_{p}/mixing_{0,1}": {"w", "b"}, "layer_{p}/vector_mixing": {"w"},
"readout_{0,out}/vector_mix": {"w"}, "readout_{0,out}/gate_{0,1}": {"w", "b"}, "~": {"widths", "offset"}}`` with
``w`` of shape (fan_in, fan_out).  With ``gaussian_rbf(trainable=False)`` the radial basis lives in the state
instead: ``{"~": {"widths": (1, R), "offsets": (1, R)}}`` as the reference's ``hk.set_state``.
``utils.painn_params_to_haiku`` / ``painn_params_from_haiku`` map the parameters onto Haiku module names
(include/lbhip.h: lb_painn_create lists both).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from .._lib import PainnDesc
from ..engine import PainnHandle, PainnTrainHandle
from ..utils import NodeType, painn_params_from_haiku, painn_params_to_haiku
from .base import BaseModel
from .egnn import _is_silu


class gaussian_rbf:  # noqa: N801 - the reference's function name
    """gaussian_rbf(n_rbf, cutoff, start, centered, trainable) of painn.py:108-143: offsets linspace(start, cutoff,
    n_rbf), widths |cutoff - start| / n_rbf; phi_k(x) = exp(-0.5 / width_k^2 (x - offset_k)^2)."""

    def __init__(self, n_rbf: int, cutoff: float, start: float = 0.0, centered: bool = False,
                 trainable: bool = False):
        if centered:
            raise NotImplementedError("gaussian_rbf(centered=True) is not built: the reference's branch reads an "
                                      "undefined `width` and cannot run")
        if not 1 <= n_rbf <= 64:
            raise NotImplementedError(f"gaussian_rbf: n_rbf {n_rbf} is not built (1 .. 64)")
        self.n_rbf, self.cutoff, self.start = int(n_rbf), float(cutoff), float(start)
        self.centered, self.trainable = centered, trainable

    def initial(self) -> Tuple[np.ndarray, np.ndarray]:
        """(widths, offsets) as the reference computes them in fp32."""
        offset = np.linspace(self.start, self.cutoff, self.n_rbf, dtype=np.float32)
        width = (np.float32(abs(self.cutoff - self.start)) / np.float32(self.n_rbf)
                 * np.ones_like(offset)).astype(np.float32)
        return width, offset


class cosine_cutoff:  # noqa: N801
    """cosine_cutoff(cutoff) of painn.py:146-170: 0.5 (cos(pi x / cutoff) + 1) for x < cutoff, else 0."""

    def __init__(self, cutoff: float):
        self.cutoff = float(cutoff)


class PaiNN(BaseModel):
    def __init__(self, hidden_size: int, output_size: int, num_mp_steps: int, radial_basis_fn, cutoff_fn,
                 n_vels: int, homogeneous_particles: bool = True, activation=None, shared_interactions: bool = False,
                 shared_filters: bool = False, eps: float = 1e-8):
        if radial_basis_fn is None:
            raise ValueError("PaiNN: a radial_basis_fn must be provided")
        if not isinstance(radial_basis_fn, gaussian_rbf):
            raise NotImplementedError("PaiNN: radial_basis_fn must be models.painn.gaussian_rbf")
        if cutoff_fn is not None and not isinstance(cutoff_fn, cosine_cutoff):
            raise NotImplementedError("PaiNN: cutoff_fn must be models.painn.cosine_cutoff or None")
        if not _is_silu(activation):
            raise NotImplementedError(f"PaiNN: activation {activation!r} is not built (SiLU only)")
        if output_size != 1:
            raise NotImplementedError(f"PaiNN: output_size {output_size} is not built (1: the acceleration)")
        if hidden_size % 16 or not 16 <= hidden_size <= 128:
            raise NotImplementedError(f"PaiNN: hidden_size {hidden_size} is not built (a multiple of 16 up to 128)")
        if eps != 1e-8:
            raise NotImplementedError("PaiNN: eps other than 1e-8 is not built")
        if num_mp_steps < 1:
            raise ValueError("PaiNN: num_mp_steps must be >= 1")
        if not 1 <= n_vels <= 9:
            raise NotImplementedError(f"PaiNN: n_vels {n_vels} is not built (1 .. 9)")
        self._hidden_size = hidden_size
        self._output_size = output_size
        self._num_mp_steps = num_mp_steps
        self.radial_basis_fn = radial_basis_fn
        self.cutoff_fn = cutoff_fn
        self._n_vels = n_vels
        self._homogeneous_particles = homogeneous_particles
        self._shared_interactions = shared_interactions
        self._shared_filters = shared_filters
        self._eps = eps
        self._handles: Dict[Tuple[int, int], tuple] = {}

    # ------------------------------------------------------------------ parameters
    def n_scalars(self) -> int:
        return self._n_vels + (0 if self._homogeneous_particles else NodeType.SIZE)

    def n_vectors(self, has_force: bool, has_bound: bool) -> int:
        return self._n_vels + (1 if has_force else 0) + (2 if has_bound else 0)

    def leaves(self, has_force: bool, has_bound: bool) -> List[Tuple[str, str, Tuple[int, ...]]]:
        """(module, leaf, shape) in lb_painn_create's blob order, the radial basis last."""
        H, Hh, R = self._hidden_size, self._hidden_size // 2, self.radial_basis_fn.n_rbf
        F = 1 if self._shared_filters else self._num_mp_steps
        P = 1 if self._shared_interactions else self._num_mp_steps
        out = [("scalar_embedding", "w", (self.n_scalars(), H)), ("scalar_embedding", "b", (H,)),
               ("vector_embedding", "w", (self.n_vectors(has_force, has_bound), H)),
               ("filter_net", "w", (R, F * 3 * H)), ("filter_net", "b", (F * 3 * H,))]
        for p in range(P):
            q = f"layer_{p}/"
            out += [(q + "interaction_0", "w", (H, H)), (q + "interaction_0", "b", (H,)),
                    (q + "interaction_1", "w", (H, 3 * H)), (q + "interaction_1", "b", (3 * H,)),
                    (q + "mixing_0", "w", (2 * H, H)), (q + "mixing_0", "b", (H,)),
                    (q + "mixing_1", "w", (H, 3 * H)), (q + "mixing_1", "b", (3 * H,)),
                    (q + "vector_mixing", "w", (H, 2 * H))]
        out += [("readout_0/vector_mix", "w", (H, H)),
                ("readout_0/gate_0", "w", (H + Hh, H)), ("readout_0/gate_0", "b", (H,)),
                ("readout_0/gate_1", "w", (H, H)), ("readout_0/gate_1", "b", (H,)),
                ("readout_out/vector_mix", "w", (Hh, 2)),
                ("readout_out/gate_0", "w", (Hh + 1, Hh)), ("readout_out/gate_0", "b", (Hh,)),
                ("readout_out/gate_1", "w", (Hh, 2)), ("readout_out/gate_1", "b", (2,))]
        return out

    def init_params(self, seed, has_force: bool, has_bound: bool = False) -> Tuple[Dict, Dict]:
        """The reference's initialisers (models/utils.py LinearXav): every weight Xavier-uniform (VarianceScaling(1,
        fan_avg, uniform): U(+-sqrt(6 / (fan_in + fan_out)))), biases 0; the radial basis from its linspace, in the
        parameters (trainable) or in the state.  Returns (params, state)."""
        rng = np.random.default_rng(seed)
        p: Dict[str, Dict[str, np.ndarray]] = {}
        for mod, leaf, shape in self.leaves(has_force, has_bound):
            if leaf == "b":
                v = np.zeros(shape)
            else:
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                v = rng.uniform(-lim, lim, size=shape)
            p.setdefault(mod, {})[leaf] = v.astype(np.float32)
        width, offset = self.radial_basis_fn.initial()
        state: Dict[str, Dict[str, np.ndarray]] = {}
        if self.radial_basis_fn.trainable:
            p["~"] = {"widths": width, "offset": offset}
        else:
            state["~"] = {"widths": width[None], "offsets": offset[None]}
        if self.cutoff_fn is not None:
            state.setdefault("~", {})["cutoff"] = np.float32(self.cutoff_fn.cutoff)
        return p, state

    def init(self, key, sample):
        features, _ = sample
        seed = int(np.asarray(key).ravel()[-1]) if key is not None else 0
        return self.init_params(seed, "force" in features, "bound" in features)

    def _io(self, params) -> Tuple[bool, bool]:
        """(has_force, has_bound) from the vector embedding's fan-in."""
        c = np.asarray(params["vector_embedding"]["w"]).shape[0] - self._n_vels
        if c not in (0, 1, 2, 3):
            raise ValueError(f"PaiNN: vector_embedding has {c + self._n_vels} inputs for n_vels {self._n_vels}")
        return bool(c & 1), bool(c & 2)

    def _rbf(self, params, state) -> Tuple[np.ndarray, np.ndarray]:
        if self.radial_basis_fn.trainable:
            r = params["~"]
            return np.asarray(r["widths"], np.float32).ravel(), np.asarray(r["offset"], np.float32).ravel()
        r = (state or {}).get("~", {})
        if "widths" in r:
            return np.asarray(r["widths"], np.float32).ravel(), np.asarray(r["offsets"], np.float32).ravel()
        return self.radial_basis_fn.initial()

    def flatten(self, params, state=None) -> np.ndarray:
        """Weights in the order lb_painn_create expects (include/lbhip.h)."""
        out = []
        for mod, leaf, shape in self.leaves(*self._io(params)):
            v = np.asarray(params[mod][leaf], np.float32)
            if v.shape != shape:
                raise ValueError(f"PaiNN params[{mod!r}][{leaf!r}]: expected {shape}, got {v.shape}")
            out.append(v.ravel())
        w, o = self._rbf(params, state)
        R = self.radial_basis_fn.n_rbf
        if w.size != R or o.size != R:
            raise ValueError(f"PaiNN radial basis: expected {R} widths and offsets, got {w.size}, {o.size}")
        return np.concatenate(out + [w, o])

    def unflatten(self, blob, has_force=None, has_bound: bool = False, like=None):
        """Inverse of flatten.  ``unflatten(blob, has_force, has_bound)`` -> (params, state).  With a parameter tree of
        the model's shapes as the second argument (or ``like=``), as the Trainer and DeviceModule call every model:
        -> the parameter tree alone (a frozen radial basis, which flatten takes from the state, is not part of it)."""
        blob = np.asarray(blob, np.float32)
        if isinstance(has_force, dict):
            has_force, like = None, has_force
        if like is not None:
            return self.unflatten(blob, *self._io(like))[0]
        if has_force is None:
            raise TypeError("PaiNN.unflatten: give has_force (and has_bound), or a parameter tree to take them from")
        out, o = {}, 0
        for mod, leaf, shape in self.leaves(has_force, has_bound):
            n = int(np.prod(shape))
            out.setdefault(mod, {})[leaf] = blob[o:o + n].reshape(shape).copy()
            o += n
        R = self.radial_basis_fn.n_rbf
        if o + 2 * R != blob.size:
            raise ValueError(f"PaiNN.unflatten: blob has {blob.size} floats, the model {o + 2 * R}")
        w, off = blob[o:o + R].copy(), blob[o + R:o + 2 * R].copy()
        state: Dict[str, Dict[str, np.ndarray]] = {}
        if self.radial_basis_fn.trainable:
            out["~"] = {"widths": w, "offset": off}
        else:
            state["~"] = {"widths": w[None], "offsets": off[None]}
        if self.cutoff_fn is not None:
            state.setdefault("~", {})["cutoff"] = np.float32(self.cutoff_fn.cutoff)
        return out, state

    def _desc(self) -> PainnDesc:
        d = PainnDesc()
        d.hidden, d.num_mp_steps, d.n_vels = self._hidden_size, self._num_mp_steps, self._n_vels
        d.homogeneous = int(bool(self._homogeneous_particles))
        d.shared_filters, d.shared_interactions = int(bool(self._shared_filters)), int(bool(self._shared_interactions))
        d.n_rbf = self.radial_basis_fn.n_rbf
        d.has_cutoff = int(self.cutoff_fn is not None)
        d.cutoff = self.cutoff_fn.cutoff if self.cutoff_fn is not None else 0.0
        return d

    # ------------------------------------------------------------------ engine binding (models/base.py)
    _FORWARD, _OUTPUT, _HAIKU_KEY = "painn_forward", "acc", "scalar_embedding"

    def _create(self, engine, params, state):
        return engine._new_handle(PainnHandle, "lb_painn_create", self._desc(), self.flatten(params, state))

    def _from_haiku(self, hk_params):
        return painn_params_from_haiku(hk_params, self)

    def _to_haiku(self, params):
        return painn_params_to_haiku(params, self)

    # ------------------------------------------------------------------ training
    MIN_TRAIN_HIDDEN = 64

    def check_trainable(self) -> None:
        if self._hidden_size < self.MIN_TRAIN_HIDDEN:
            raise NotImplementedError(f"PaiNN with hidden_size {self._hidden_size}: the model has no device training step "
                                      f"(csrc/lb_train_painn.h is built for {self.MIN_TRAIN_HIDDEN} <= hidden_size <= 128)")

    def train_handle(self, engine, params, state=None):
        """Device-resident training state for `params`; `state` carries a frozen radial basis (gaussian_rbf(trainable=
        False)), else the basis' initial values are taken."""
        self.check_trainable()
        self._check_padded(engine)
        return self._train_create(engine, params, state)

    def _train_create(self, engine, params, state=None):
        """csrc/lb_train_painn.h: a GnsTrainHandle (one "acc" target).  The radial basis is the blob's tail: parameters
        with gaussian_rbf(trainable=True), otherwise frozen - zero gradient, untouched by AdamW."""
        return engine._new_handle(PainnTrainHandle, "lb_painn_train_create", self._desc(), self.flatten(params, state),
                                  int(bool(self.radial_basis_fn.trainable)))

    def unroll_handle(self, engine, th, params_like):
        """The training handle's own inference view (csrc/lb_train_painn.h): it reads th's weight blob, nothing to refresh."""
        self._check_padded(engine)
        return th.model_handle()
