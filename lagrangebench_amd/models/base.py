"""BaseModel contract - lagrangebench/models/base.py:11-41, and the binding of a model object to its device handle."""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Dict, Tuple

import numpy as np


class BaseModel(ABC):
    """``model.init(key, sample) -> (params, state)`` and
    ``model.apply(params, state, sample) -> (pred_dict, state)`` are what the reference gets from
    ``hk.without_apply_rng(hk.transform_with_state(model))`` (runner.py:67); models here expose
    them directly.  ``sample = (features, particle_type)``; the prediction dict has one of the
    keys "acc" / "vel" / "pos" with a (N, dim) (or (B, N, dim)) array.

    A device model names, on its class, the engine forward it runs (``_FORWARD``) and the key of its prediction
    (``_OUTPUT``), and supplies ``_create(engine, params, state)`` (a new engine handle), ``_HAIKU_KEY`` (a module
    name only the engine layout of its parameter tree has) and ``_from_haiku`` / ``_to_haiku``.  Everything that
    turns a parameter tree into a device handle and runs it lives here."""

    _FORWARD = ""
    _OUTPUT = "acc"
    _HAIKU_KEY = ""
    _PADDED_OK = False  # runs on padded trajectories (particles of type NodeType.PAD_VALUE): GNS only
    _EXACT_FORWARD = False  # autograd.DeviceModule runs the forward in exact-fp32 products: networks with ReLU kinks (GNS)
    _FUSED_ROLLOUT = True  # evaluate.rollout runs the model's handle through the device loop (engine.rollout); False: the
    #                        generic Python loop drives apply + case.integrate step by step (models.TorchModel)
    _WINDOW_GRAD = False  # the training handle's backward also gives d loss / d window (autograd.DeviceModule): GNS only
    _MAX_HANDLES = 4  # device copies kept per model object (LRU): a training loop that hands over a fresh
    #                   parameter tree every step must not accumulate one packed weight blob per step

    @abstractmethod
    def init(self, key, sample) -> Tuple[Dict, Dict]:
        raise NotImplementedError

    # ------------------------------------------------------------------ engine binding
    def _create(self, engine, params, state):
        raise NotImplementedError

    @staticmethod
    def _fingerprint(tree) -> tuple:
        """Cheap content stamp of a parameter (or state) tree, None and {} included: a few strided samples + the sum
        of every leaf.  An in-place update of the weights (an optimiser step, a test editing one bias) must not reuse
        the device copy made for the old values.  Only the modules (dicts of arrays) are stamped: a bare value beside
        them (the sizes some trees carry) never enters a weight blob."""
        out = []
        for mod in sorted(tree or {}):
            if not isinstance(tree[mod], dict):
                continue
            for leaf in sorted(tree[mod]):
                a = np.asarray(tree[mod][leaf])
                flat = a.reshape(-1)
                out.append((mod, leaf, a.shape, float(flat.sum(dtype=np.float64)),
                            float(flat[:: max(1, flat.size // 7)].astype(np.float64).sum())))
        return tuple(out)

    def _check_padded(self, engine) -> None:
        if getattr(engine, "has_pads", False) and not self._PADDED_OK:
            raise NotImplementedError(f"{type(self).__name__}: padded trajectories (particles of type NodeType.PAD_VALUE, "
                                      "the matscipy backend's variable particle counts) run with GNS only")

    def handle(self, engine, params, state=None):
        """The engine handle of (params, state): reused while `params` is the same object with the same content on the
        same engine, else created anew."""
        self._check_padded(engine)
        handles = self._handles  # {(id(engine), id(params)): (handle, params, stamp)}, set by the model's __init__
        key = (id(engine), id(params))
        hit = handles.get(key)
        stamp = (self._fingerprint(params), self._fingerprint(state))
        if hit is not None and hit[1] is params and hit[2] == stamp and hit[0].engine is engine:
            handles[key] = handles.pop(key)  # most recently used last
            return hit[0]
        handles.pop(key, None)
        while len(handles) >= self._MAX_HANDLES:
            # drop OUR reference to the least recently used handle: its __del__ frees the device blob once no caller
            # holds it any more
            handles.pop(next(iter(handles)))
        h = self._create(engine, params, state)
        handles[key] = (h, params, stamp)
        return h

    def _engine_of(self, sample):
        """The engine whose state `sample`'s features describe; refuses features the engine has moved on from."""
        features, particle_type = sample
        engine = getattr(features, "engine", None)
        if engine is None:
            raise TypeError(f"{type(self).__name__}.apply needs the FeatureDict returned by case.preprocess_eval/"
                            "allocate_eval (it names the engine state to run on)")
        if features.version != engine.version:
            raise RuntimeError("features are stale: the engine state changed since they were produced")
        return engine

    def apply(self, params, state, sample):
        engine = self._engine_of(sample)
        return self.apply_handle(self.handle(engine, params, state), state, sample)

    def apply_handle(self, handle, state, sample):
        """``apply`` on a device handle the caller holds (``unroll_handle``) instead of a parameter tree."""
        engine = self._engine_of(sample)
        if handle.engine is not engine:
            raise ValueError(f"{type(self).__name__}.apply_handle: the handle belongs to another engine than the features")
        self._check_padded(engine)
        out = getattr(engine, self._FORWARD)(handle)
        return {self._OUTPUT: out if sample[0].batched else out[0]}, state

    def __call__(self, params, state, sample):
        return self.apply(params, state, sample)

    # ------------------------------------------------------------------ checkpoints
    def params_from_haiku(self, hk_params) -> Dict:
        """A checkpoint's parameter tree in this model's engine layout (unchanged when it already is)."""
        return hk_params if self._HAIKU_KEY in hk_params else self._from_haiku(hk_params)

    def params_to_haiku(self, params) -> Dict:
        """The engine-layout tree under the reference's Haiku module names (unchanged when it already has them)."""
        return self._to_haiku(params) if self._HAIKU_KEY in params else params

    def _from_haiku(self, hk_params) -> Dict:
        raise NotImplementedError

    def _to_haiku(self, params) -> Dict:
        raise NotImplementedError

    # ------------------------------------------------------------------ training
    def check_trainable(self) -> None:
        """Raise NotImplementedError unless the device training step is built for this configuration."""
        raise NotImplementedError("Trainer: the model has no device training step (GNS: csrc/lb_train.hip, SEGNN: "
                                  "csrc/lb_train_segnn.h, EGNN: csrc/lb_train_egnn.h, PaiNN: csrc/lb_train_painn.h)")

    def train_handle(self, engine, params):
        """Device-resident training state (weights, gradients, AdamW moments) for `params` on `engine`."""
        self.check_trainable()
        self._check_padded(engine)
        return self._train_create(engine, params)

    def _train_create(self, engine, params):
        raise NotImplementedError

    def loss_grad(self, th, target, loss_weight) -> float:
        """One loss + gradient accumulation of the training handle `th` against the case's targets (trainer.py:35-89):
        _mse of the normalised acceleration."""
        self._check_padded(th.engine)
        return th.loss_grad(target["acc"], loss_weight.get("acc", 1.0))

    def unroll_handle(self, engine, th, params_like):
        """An inference handle on `engine` that runs on the CURRENT weights of training handle `th` without copying them
        to the host (``train.device_unroll``), or None: the model has no such route and the
        push-forward unroll goes through ``th.read("weights")`` and ``apply``.  `params_like`: a parameter tree of the
        model's shapes (the one `th` was created from)."""
        return None
