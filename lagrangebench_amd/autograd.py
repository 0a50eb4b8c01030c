"""torch autograd over the device training step: any torch loss, optimiser or scheduler on the hand-written HIP backward.

The reference user wraps ``jax.grad`` around ``model.apply`` and ``case.integrate`` (trainer.py:63-89 does so for ``_mse``
only).  Here ``DeviceModule`` is the ``torch.nn.Module`` with that role: its forward is the training handle's forward with
saved activations (``lb_train_forward``), its backward the handle's backward from the ``d loss / d pred`` autograd hands
over (``lb_train_backward``).  Gradients flow to ``weights`` (GNS, SEGNN, EGNN, PaiNN) and to the input window (GNS), so losses
other than the MSE, gradients with respect to positions and unrolls with gradients through time are a few lines of torch.
``Trainer`` keeps its fused ``_mse`` step; this is a second road beside it.

    mod = DeviceModule(model, case, params, batch=2)          # after case.allocate(...) sized the neighbor list
    opt = torch.optim.AdamW([mod.weights], lr=1e-4)
    pred = mod(window, particle_type)["acc"]
    torch.nn.functional.huber_loss(pred[mask], target[mask]).backward()
    opt.step()

``TorchModule`` plays the same role for a user's own network behind ``models.TorchModel``: torch holds the network and its
autograd, the graph ops are HIP (``graph.Graph``), and the window's gradient comes from ``graph.differentiable_features``
(``lb_graph_features_backward``).  ``advance_window`` is ``case.integrate`` plus the window shift in differentiable torch, so
an unroll through time is

    mod = TorchModule(model, case, params, batch=1)
    p1 = mod(w1, particle_type)["acc"]
    p2 = mod(advance_window(case, w1, p1, "acc"))["acc"]
    (loss(p1, t1) + loss(p2, t2)).backward()                  # gradients to mod.parameters() and to w1

Arithmetic: the forward of a GNS runs in exact-fp32 products (its backward's ReLU masks are the forward's signs, and the
default f16x2 forward leaves ten times as many units on the wrong side of a kink), the backward in the handle's default
ones - unless the window's gradient is asked for, which is per particle and runs exact throughout.

What is differentiated: the network, and for the window the feature builder (velocity history and magnitudes, wall
distances, relative displacements and distances of the edges).  The neighbor list is held fixed, and the external force
is a constant of the positions: exact for ``ForceSpec.piecewise`` / ``constant`` almost everywhere (what JAX gives too); for
a ``ForceSpec.callable`` this DIFFERS from ``jax.grad``, which would differentiate the callable.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

__all__ = ["DeviceModule", "TorchModule", "advance_window", "non_kinematic_mask"]


def non_kinematic_mask(particle_type: torch.Tensor) -> torch.Tensor:
    """True for the particles the reference's loss counts (utils.py:28-35): not a wall (1), not a moving wall (2), not a
    pad (-1) - the rule of the device step's per-node loss weight."""
    pt = torch.as_tensor(particle_type)
    return ~((pt == 1) | (pt == 2) | (pt == -1))


class _Step(torch.autograd.Function):
    """One model step as an autograd node over (weights, window)."""

    @staticmethod
    def forward(ctx, weights, window, mod, ticket):
        ctx.mod, ctx.ticket, ctx.want_dpos = mod, ticket, bool(window.requires_grad)
        ctx.version = mod.weights._version
        ctx.set_materialize_grads(False)
        return mod._run_forward(ctx.want_dpos)

    @staticmethod
    def backward(ctx, dpred):
        mod = ctx.mod
        if dpred is None:
            return None, None, None, None
        th = mod.handle
        if mod.weights._version != ctx.version:
            raise RuntimeError("DeviceModule: the weights were modified in place (an optimiser step?) between this graph's "
                               "forward and its backward; run the forward again")
        if mod._live != ctx.ticket:
            # another forward (or a backward) has used the handle since: bring this node's state back - same positions,
            # frozen capacities and a deterministic search give the same list - and run its forward again
            mod.recomputed += 1
            saved = mod._saved.get(ctx.ticket)
            if saved is not None:
                saved = saved[:2]
            if saved is None:
                raise RuntimeError("DeviceModule: this graph's window is gone (its backward already ran without "
                                   "retain_graph, or the module was reset)")
            mod._load(*saved)
            mod._run_forward(ctx.want_dpos)
        th.zero_grad()
        dpos = th.backward(dpred, want_dpos=ctx.want_dpos)
        mod._live = None   # the backward consumed the forward's scratch
        grad = mod._grads.clone()
        return grad, dpos, None, None


class DeviceModule(torch.nn.Module):
    """``model`` (GNS, SEGNN, EGNN or PaiNN) on the device as a differentiable torch module.

    ``weights``: an ``nn.Parameter`` that ALIASES the training handle's device weight blob (device layout: latents padded to
    128, the padding zero): an optimiser that steps it in place trains the handle.  ``params()`` reads the current
    weights back as the model's parameter tree (checkpoints, ``model.apply``); ``handle`` is the training handle.

    ``mod(window, particle_type=None, features=None) -> {"acc" | "pos": (B, N, dim) float32 with a grad_fn}``.  `window`:
    (B, N, isl, dim) float64 on the device.  Without `features` the module loads the window into the engine and updates
    the neighbor list (sized before by ``case.allocate*``); with the ``FeatureDict`` that ``case.preprocess*`` just made
    for this window it skips that.  ``window.requires_grad`` gives ``d loss / d window`` (GNS only).

    Several graphs may be alive at once (an unroll through time, two backward calls): each forward saves its window and
    particle types, and a backward whose forward is no longer the handle's live one reloads them and runs the forward
    again - one recomputed forward per such step (``recomputed`` counts them).
    """

    def __init__(self, model, case, params, batch: int):
        super().__init__()
        self.model, self.case, self.batch = model, case, int(batch)
        self.engine = case.engine(self.batch)
        self.handle = model.train_handle(self.engine, params)   # check_trainable and the padded-input check apply
        self._like = params
        self._window_grad = bool(getattr(model, "_WINDOW_GRAD", False))
        self._exact_forward = bool(getattr(model, "_EXACT_FORWARD", False))
        self.weights = torch.nn.Parameter(self.handle.device_blob("weights"), requires_grad=True)
        self._grads = self.handle.device_blob("grads")
        self._ticket = 0
        self._live: Optional[int] = None
        self._saved: Dict[int, tuple] = {}
        self.recomputed = 0   # backward calls that had to reload their window and run the forward again

    # ------------------------------------------------------------------ engine state
    def _load(self, window: torch.Tensor, particle_type: Optional[torch.Tensor]) -> None:
        eng = self.engine
        if eng.e_cap <= 0:
            raise RuntimeError("DeviceModule: the engine has no neighbor list yet - size it through the case first "
                               "(case.allocate / allocate_eval on a sample of this batch size)")
        if particle_type is not None:
            eng.set_particle_type(particle_type)
        eng.load_window(window, t0=0, step=0)
        eng.nl_update()
        if bool(eng.nl_flags().any()):
            raise RuntimeError("DeviceModule: the neighbor list overflowed its capacity for this window - re-allocate "
                               "through the case (case.allocate / allocate_eval) and call the module again")

    def _run_forward(self, want_dpos: bool) -> torch.Tensor:
        """The handle's forward, then the arithmetic of the backward that may follow.  A ReLU network (GNS) runs its forward
        in exact-fp32 products: the backward's masks are the forward's signs, and a unit within rounding of zero that lands
        on the other side of its kink than an exact evaluation moves its particle's gradient by per cent - the f16x2
        forward has about ten times as many such units.  The backward keeps the default arithmetic unless the window's
        gradient, a per-particle quantity, is asked for (include/lbhip.h: lb_train_exact_math)."""
        th = self.handle
        th.exact_math(self._exact_forward or want_dpos)
        pred = th.forward()
        th.exact_math(want_dpos)
        return pred

    def forward(self, window: torch.Tensor, particle_type=None, features=None):
        eng = self.engine
        if window.requires_grad and not self._window_grad:
            raise NotImplementedError(f"DeviceModule: the gradient with respect to the window is built for GNS only, not "
                                      f"for {type(self.model).__name__} (detach the window)")
        if tuple(window.shape) != (eng.B, eng.N, eng.isl, eng.dim) or window.dtype != torch.float64:
            raise ValueError(f"DeviceModule: window must be ({eng.B}, {eng.N}, {eng.isl}, {eng.dim}) float64, got "
                             f"{tuple(window.shape)} {window.dtype}")
        w = window.detach()
        pt = None if particle_type is None else torch.as_tensor(particle_type).detach().clone()
        if features is None:
            self._load(w, pt)
        else:
            if self.model._engine_of((features, particle_type)) is not eng:
                raise ValueError("DeviceModule: the features belong to another engine than the module's")
        self._ticket += 1
        ticket = self._ticket
        if torch.is_grad_enabled():
            self._saved[ticket] = (w.clone(), pt)
            while len(self._saved) > 64:   # graphs that never ran a backward must not pile up windows
                self._saved.pop(next(iter(self._saved)))
        out = _Step.apply(self.weights, window, self, ticket)
        self._live = ticket
        return {self.model._OUTPUT: out}

    # ------------------------------------------------------------------ weights
    def params(self) -> Dict:
        """The current weights as the model's parameter tree (a host copy)."""
        return self.model.unflatten(self.handle.read("weights"), self._like)

    def reset(self) -> None:
        """Forget every saved window (graphs that will not be differentiated any more)."""
        self._saved.clear()
        self._live = None


class _Restore(torch.autograd.Function):
    """Identity on one step's output.  Every op of the step lies upstream of it, so its backward runs first for that step:
    the place to bring the engine back to the step's window and list."""

    @staticmethod
    def forward(ctx, out, mod, ticket):
        ctx.mod, ctx.ticket = mod, ticket
        return out.view_as(out)

    @staticmethod
    def backward(ctx, d):
        ctx.mod._restore(ctx.ticket)
        return d, None, None


class TorchModule(torch.nn.Module):
    """``model`` (a ``models.TorchModel``) on the device as a differentiable torch module: the role ``DeviceModule`` plays
    for the device models.

    The network is a device copy of the wrapped module holding `params` (and `state`, default: the wrapped module's
    buffers), registered as ``self.module``: ``parameters()``, any torch optimiser and ``state_dict()`` work.  With
    ``handle=`` (from ``model.train_handle``) it runs on ``handle.module`` instead: gradients accumulate in the handle's
    gradient blob and ``handle.adamw_step`` trains it.

    ``mod(window, particle_type=None, features=None) -> {"acc" | "vel" | "pos": (B, N, dim) float32 with a grad_fn}``.
    `window`: (B, N, isl, dim) float64 on the device.  Without `features` the module loads the window into the engine and
    updates the neighbor list (sized before by ``case.allocate*``); with the ``FeatureDict`` that ``case.preprocess*`` just
    made for this window it skips that.  Gradients flow to the parameters and, when ``window.requires_grad``, to the window
    (``graph.differentiable_features``: the neighbor list is held fixed, the external force is a constant).  A model made
    with ``autocast=torch.bfloat16`` runs its module under that autocast context here too; the output is float32 either way.

    Several graphs may be alive at once (an unroll through time, two backward calls).  Each forward saves its window and
    particle types (64 at most).  A backward whose step is no longer the engine's live one reloads them and rebuilds the list -
    the same positions under frozen capacities and a deterministic search give the same list; a different edge count raises -
    and makes the step's ``FeatureDict`` and ``Graph`` fresh again (``restored`` counts these).  Nothing of the network is
    recomputed: torch holds the activations.
    """

    def __init__(self, model, case, params, batch: int, state=None, handle=None):
        super().__init__()
        from .models.torch_model import TorchModel
        if not isinstance(model, TorchModel):
            raise TypeError(f"TorchModule wraps a models.TorchModel, not {type(model).__name__}; the device models (GNS, SEGNN, "
                            "EGNN, PaiNN) go through DeviceModule")
        self.model, self.case, self.batch = model, case, int(batch)
        self.engine = case.engine(self.batch)
        model._check_padded(self.engine)
        self.handle = handle
        if handle is not None:
            if handle.engine is not self.engine or getattr(handle, "module", None) is None:
                raise ValueError("TorchModule: `handle` must be an open handle of model.train_handle on the case's engine of "
                                 "this batch size")
            self.module = handle.module
        else:
            model._check_state(state)
            self.module = model._device_module(self.engine, params, model.state_of() if state is None else state)
        self._ticket = 0
        self._live: Optional[int] = None
        self._saved: Dict[int, tuple] = {}
        self.restored = 0   # backward calls that had to reload their window and rebuild the list

    # ------------------------------------------------------------------ engine state
    def _load(self, window: torch.Tensor, particle_type: Optional[torch.Tensor]) -> None:
        eng = self.engine
        if eng.e_cap <= 0:
            raise RuntimeError("TorchModule: the engine has no neighbor list yet - size it through the case first "
                               "(case.allocate / allocate_eval on a sample of this batch size)")
        if particle_type is not None:
            eng.set_particle_type(particle_type)
        eng.load_window(window, t0=0, step=0)
        eng.nl_update()
        if bool(eng.nl_flags().any()):
            raise RuntimeError("TorchModule: the neighbor list overflowed its capacity for this window - re-allocate "
                               "through the case (case.allocate / allocate_eval) and call the module again")

    def _restore(self, ticket: int) -> None:
        eng = self.engine
        saved = self._saved.get(ticket)
        if saved is None:
            raise RuntimeError("TorchModule: this graph's window is gone (more than 64 forwards since, or the module was reset)")
        window, pt, features, graph, n_edges = saved
        if self._live == ticket and features.version == eng.version:
            return
        self._load(window, pt)
        if not torch.equal(eng.nl_idx()[1], n_edges):
            raise RuntimeError("TorchModule: the neighbor list rebuilt for this graph's backward has another edge count than "
                               "its forward's (were the capacities changed in between?)")
        features.version = graph.version = eng.version
        self._live = ticket
        self.restored += 1

    def forward(self, window: torch.Tensor, particle_type=None, features=None):
        from .case_setup.features import FeatureDict
        from .graph import Graph, _plain, differentiable_features
        eng = self.engine
        if tuple(window.shape) != (eng.B, eng.N, eng.isl, eng.dim) or window.dtype != torch.float64:
            raise ValueError(f"TorchModule: window must be ({eng.B}, {eng.N}, {eng.isl}, {eng.dim}) float64, got "
                             f"{tuple(window.shape)} {window.dtype}")
        w = window.detach()
        pt = None if particle_type is None else torch.as_tensor(particle_type).detach().clone()
        if features is None:
            self._load(w, pt)
            features = FeatureDict(eng, w, True)
        elif self.model._engine_of((features, particle_type)) is not eng:
            raise ValueError("TorchModule: the features belong to another engine than the module's")
        self.model._check_padded(eng)
        types = pt if pt is not None else eng.particle_type
        if types is None:
            raise RuntimeError("TorchModule: the engine has no particle types yet - pass particle_type")
        types = types.to(device=eng.device, dtype=torch.int64).reshape(eng.B, eng.N)
        if window.requires_grad:
            fd = differentiable_features(features, window)
        else:
            fd = {k: _plain(features, k) for k in features.keys()}
        graph = Graph(features, batched=True)
        out = self.model._call_module(self.module, eng, "TorchModule", fd, types, graph)   # (the model's autocast setting)
        self._ticket += 1
        ticket = self._ticket
        if torch.is_grad_enabled():
            self._saved[ticket] = (w.clone(), pt, features, graph, graph.n_edges.clone())
            while len(self._saved) > 64:   # graphs that never ran a backward must not pile up windows
                self._saved.pop(next(iter(self._saved)))
            out = _Restore.apply(out, self, ticket)
        self._live = ticket
        return {self.model._OUTPUT: out}

    # ------------------------------------------------------------------ weights
    def params(self) -> Dict:
        """The current parameters as the model's parameter tree (a host copy)."""
        return self.model.params_of(self.module)

    def reset(self) -> None:
        """Forget every saved window (graphs that will not be differentiated any more)."""
        self._saved.clear()
        self._live = None


def advance_window(case, window: torch.Tensor, pred: torch.Tensor, output: str = "acc", particle_type=None,
                   target_pos=None) -> torch.Tensor:
    """``case.integrate`` (case.py:230-259) plus the window shift, in differentiable float64 torch: the window of the next step.

    `window` (..., N, isl, dim) float64, `pred` (..., N, dim) the model's output under key `output`: "acc" (normalised
    acceleration: new = shift(newest, displacement(newest, previous) + mean + pred std)), "vel" (normalised velocity) or "pos"
    (the position itself), with the case's normalisation statistics; displacement and shift are the case's, periodic with
    derivative 1.  With `target_pos` (..., N, dim), kinematic and pad particles (`particle_type` 1, 2, -1) take their targets,
    detached.  Gradients flow to `window` and `pred`."""
    if output not in ("acc", "vel", "pos"):
        raise ValueError(f"advance_window: output {output!r} must be 'acc', 'vel' or 'pos'")
    if not isinstance(window, torch.Tensor) or window.dtype != torch.float64 or window.dim() < 3 or window.shape[-2] < 2:
        raise ValueError(f"advance_window: window must be (..., N, isl >= 2, dim) float64, got "
                         f"{tuple(getattr(window, 'shape', ()))} {getattr(window, 'dtype', type(window))}")
    if tuple(pred.shape) != tuple(window.shape[:-2]) + (window.shape[-1],):
        raise ValueError(f"advance_window: pred must be {tuple(window.shape[:-2]) + (window.shape[-1],)}, got {tuple(pred.shape)}")
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=torch.float64, device=window.device)
    p = pred.to(torch.float64)
    newest = window[..., -1, :]
    if output == "pos":
        new = p
    else:
        if output == "vel":
            s = case.normalization_stats["velocity"]
            vel = t(s["mean"]) + p * t(s["std"])
        else:
            s = case.normalization_stats["acceleration"]
            vel = case.displacement(newest, window[..., -2, :]) + (t(s["mean"]) + p * t(s["std"]))
        new = case.shift(newest, vel)
    if target_pos is not None:
        if particle_type is None:
            raise ValueError("advance_window: target_pos needs particle_type (which particles are kinematic)")
        fixed = ~non_kinematic_mask(torch.as_tensor(particle_type)).to(window.device)
        tgt = torch.as_tensor(target_pos).detach().to(device=window.device, dtype=torch.float64)
        new = torch.where(fixed[..., None], tgt, new)
    return torch.cat([window[..., 1:, :], new[..., None, :]], dim=-2)
