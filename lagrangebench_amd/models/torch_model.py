"""A user's own ``torch.nn.Module`` behind the reference's model API: the tutorial's "subclass BaseModel and train your
network" path (lagrangebench/models/base.py, notebooks/tutorial.ipynb).

``TorchModel(module, output="acc")`` is a first-class model: ``init / apply``, ``Trainer`` (``train.device_data``,
push-forward with and without ``train.device_unroll``; data parallel goes through the same gathered AdamW step and has
not been run with more than one process), checkpoints, ``eval_rollout`` and ``infer``.  The
neighbor list, features, noise, integrator, AdamW and checkpoints are the engine's; the dense layers and their autograd are
torch's; gather and segment sum on the graph are the HIP ops of ``lagrangebench_amd.graph``.

The module:  ``forward(features, particle_type, graph) -> (B, N, dim)`` float32, always batched.
  features       a plain dict with the FeatureDict's keys: abs_pos (B, N, isl, dim), vel_hist, [vel_mag], [bound], [force],
                 rel_disp (B, E_cap, dim), rel_dist (B, E_cap, 1) as float32; senders / receivers (B, E_cap) as int64
  particle_type  (B, N) int64
  graph          ``graph.Graph`` on the engine's current list: ``gather(x, role)``, ``segment_sum(msg, role)``

Parameter tree: from ``named_parameters()`` - ``"a.b.weight"`` is ``params["a.b"]["weight"]``, a top-level parameter goes under
module ``"~"``; leaves are numpy float32; ``flatten`` / ``unflatten`` run in ``named_parameters()`` order.  Persistent buffers
travel the same way as the ``state`` tree: ``apply`` loads them, training never changes them.  The training copy takes the
buffers the wrapped module holds (``set_state`` puts a loaded state there); while a training handle is open, ``apply`` refuses
a state that differs from them (``RuntimeError``), so the loss step and the rollouts cannot silently use different buffers.
Checkpoints keep the tree as it is (``_to_haiku`` / ``_from_haiku`` are the identity).

Training: ``_train_create`` makes an ``engine.BlobTrainHandle`` (optimiser state only) and re-points every parameter of a
device copy of the module at its slice of the handle's weight blob and every ``.grad`` at its slice of the gradient blob,
without a copy.  ``loss_grad`` is the reference's ``_mse`` in torch; its ``backward()`` accumulates straight into the gradient
blob, and the library's AdamW kernels (``lb_adamw_step``, ``lb_adamw_step_gathered``) update the weights in place.  There is
no fused rollout: ``evaluate.rollout`` drives ``apply`` step by step through its generic loop.

Mixed precision: ``TorchModel(module, autocast=torch.bfloat16)`` runs the module under
``torch.autocast(device, dtype=torch.bfloat16)`` wherever the model runs it - ``apply``, ``loss_grad``, the push-forward
unroll, ``eval_rollout``, ``infer``, ``autograd.TorchModule``.  The parameters, the training handle's blob, AdamW and the
checkpoints stay float32, as autocast expects; ``Linear`` and the like then return bfloat16, the graph ops take and return
bfloat16 (``graph.py`` states their contract), and the module's (B, N, dim) output may be bfloat16: it is widened to float32
before the loss and the integrator.  The features the module receives stay float32 - ``torch.cat([h, features["rel_disp"]],
-1)`` with a bfloat16 ``h`` promotes to float32 unless the module casts the features.  A module written for float32 runs
unchanged.  float16 is not offered (it would need loss scaling).

Losses and training schemes of the user's own - gradients with respect to the input window, unrolls through time - go through
``autograd.TorchModule``, which runs the same module as a differentiable torch module on the engine.
"""
from __future__ import annotations

import copy
import weakref
from typing import Dict, List, Tuple

import numpy as np
import torch

from ..autograd import non_kinematic_mask
from ..case_setup.features import FeatureDict
from ..graph import Graph
from .base import BaseModel

_TOP = "~"   # module name of a parameter (or buffer) that belongs to the wrapped module itself


def _split(name: str) -> Tuple[str, str]:
    mod, _, leaf = name.rpartition(".")
    return (mod or _TOP), leaf


class _TorchHandle:
    """The device copy of the module on one engine (what ``BaseModel.handle`` caches); nothing to destroy."""

    def __init__(self, engine, module: torch.nn.Module):
        self.engine, self.module = engine, module

    def close(self):
        pass


class TorchModel(BaseModel):
    _FUSED_ROLLOUT = False   # no device rollout: evaluate.rollout's generic loop
    _PADDED_OK = False

    def __init__(self, module: torch.nn.Module, output: str = "acc", autocast=None):
        if not isinstance(module, torch.nn.Module):
            raise TypeError(f"TorchModel wraps a torch.nn.Module, got {type(module).__name__}")
        if output not in ("acc", "vel", "pos"):
            raise ValueError(f"TorchModel: output {output!r} must be 'acc', 'vel' or 'pos'")
        if autocast is not None and autocast is not torch.bfloat16:
            raise ValueError(f"TorchModel: autocast {autocast!r} must be None or torch.bfloat16")
        self._OUTPUT = output
        self.autocast = autocast
        self._module = copy.deepcopy(module).to("cpu")   # the template: shapes, names, buffers; init() resets it
        self._names: List[str] = [n for n, _ in self._module.named_parameters()]
        bad = [n for n, p in self._module.named_parameters() if p.dtype != torch.float32]
        if bad:
            raise TypeError(f"TorchModel: parameters must be float32 (not {bad})")
        if not self._names:
            raise ValueError("TorchModel: the module has no parameters")
        self._buffers: List[str] = [k for k in self._module.state_dict() if k not in set(self._names)]
        self._handles: Dict[Tuple[int, int], tuple] = {}
        self._training = None   # weak reference to the last training handle made (_check_state)

    # ------------------------------------------------------------------ parameter and state trees
    def _tree(self, names, tensors) -> Dict:
        out: Dict = {}
        for n in names:
            mod, leaf = _split(n)
            out.setdefault(mod, {})[leaf] = tensors[n].detach().cpu().numpy().copy()
        return out

    def params_of(self, module: torch.nn.Module = None) -> Dict:
        """The parameter tree of `module` (default: the wrapped module as it stands)."""
        return self._tree(self._names, dict((module or self._module).named_parameters()))

    def state_of(self, module: torch.nn.Module = None) -> Dict:
        """The persistent buffers of `module` as the state tree."""
        return self._tree(self._buffers, (module or self._module).state_dict())

    def init(self, key, sample=None):
        """Every submodule's ``reset_parameters()`` under a forked RNG seeded from `key`: equal keys give equal bits and the
        global generators are left as they were."""
        seed = int(np.asarray(key).ravel()[-1]) if key is not None else 0
        with torch.random.fork_rng(devices=[]):
            torch.default_generator.manual_seed(seed)   # (the CPU generator only: the template lives on the CPU)
            for m in self._module.modules():
                if callable(getattr(m, "reset_parameters", None)):
                    m.reset_parameters()
        return self.params_of(), self.state_of()

    def flatten(self, params, state=None) -> np.ndarray:
        """The weight blob: every parameter in ``named_parameters()`` order, row-major."""
        shapes = dict((n, tuple(p.shape)) for n, p in self._module.named_parameters())
        parts = []
        for n in self._names:
            mod, leaf = _split(n)
            try:
                a = np.asarray(params[mod][leaf], np.float32)
            except KeyError:
                raise ValueError(f"TorchModel params: leaf {mod!r}/{leaf!r} is missing") from None
            if tuple(a.shape) != shapes[n]:
                raise ValueError(f"TorchModel params: {mod!r}/{leaf!r} has shape {tuple(a.shape)}, the module's is {shapes[n]}")
            parts.append(a.ravel())
        return np.concatenate(parts)

    def unflatten(self, blob, like=None) -> Dict:
        blob = np.asarray(blob, np.float32).reshape(-1)
        sizes = [(n, tuple(p.shape), p.numel()) for n, p in self._module.named_parameters()]
        if blob.size != sum(s[2] for s in sizes):
            raise ValueError(f"TorchModel.unflatten: a blob of {blob.size} floats, the module has {sum(s[2] for s in sizes)}")
        out: Dict = {}
        off = 0
        for n, shape, size in sizes:
            mod, leaf = _split(n)
            out.setdefault(mod, {})[leaf] = blob[off:off + size].reshape(shape).copy()
            off += size
        return out

    def set_state(self, state) -> None:
        """Load a state tree (persistent buffers) into the wrapped module: what the next training copy starts from."""
        self._load_buffers(self._module, state)

    def _load_buffers(self, module, state) -> None:
        if not state:
            return
        target = module.state_dict()   # (references to the buffers themselves)
        with torch.no_grad():
            for n in self._buffers:
                mod, leaf = _split(n)
                if mod in state and leaf in state[mod]:
                    target[n].copy_(torch.as_tensor(np.asarray(state[mod][leaf])).to(target[n].dtype))

    def _device_module(self, engine, params, state) -> torch.nn.Module:
        mod = copy.deepcopy(self._module).to(engine.device)
        blob = torch.from_numpy(self.flatten(params)).to(engine.device)
        off = 0
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(blob[off:off + p.numel()].view(p.shape))
                off += p.numel()
        self._load_buffers(mod, state)
        return mod

    # ------------------------------------------------------------------ engine binding (models/base.py)
    def _create(self, engine, params, state):
        return _TorchHandle(engine, self._device_module(engine, params, state))

    def _from_haiku(self, hk_params):
        return hk_params

    def _to_haiku(self, params):
        return params

    def _forward(self, module, engine, features, particle_type) -> torch.Tensor:
        """module(features as a plain batched float32 dict, particle types (B, N) int64, Graph) -> (B, N, dim) float32."""
        batched = bool(features.batched)
        fd = {}
        for k in features.keys():
            v = features[k]
            v = v if batched else v[None]
            fd[k] = v.to(torch.int64) if k in ("senders", "receivers") else v.to(torch.float32)
        pt = torch.as_tensor(np.asarray(particle_type) if not isinstance(particle_type, torch.Tensor) else particle_type)
        pt = pt.to(device=engine.device, dtype=torch.int64).reshape(engine.B, engine.N)
        return self._call_module(module, engine, "TorchModel", fd, pt, Graph(features, batched=True))

    def _call_module(self, module, engine, who: str, fd, pt, graph) -> torch.Tensor:
        """module(fd, pt, graph) under the model's autocast setting -> its (B, N, dim) output as float32 (a bfloat16 output is
        accepted under autocast only)."""
        if self.autocast is None:
            out = module(fd, pt, graph)
        else:
            with torch.autocast(engine.device.type, dtype=self.autocast):
                out = module(fd, pt, graph)
        dtypes = (torch.float32,) if self.autocast is None else (torch.float32, self.autocast)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (engine.B, engine.N, engine.dim) or out.dtype not in dtypes:
            raise ValueError(f"{who}: the module must return a ({engine.B}, {engine.N}, {engine.dim}) float32 tensor"
                             f"{'' if self.autocast is None else ' (or bfloat16 under autocast)'}, got "
                             f"{tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__} "
                             f"{getattr(out, 'dtype', '')}")
        return out.float()

    def apply_handle(self, handle, state, sample):
        engine = self._engine_of(sample)
        if handle.engine is not engine:
            raise ValueError("TorchModel.apply_handle: the handle belongs to another engine than the features")
        self._check_padded(engine)
        self._check_state(state)
        with torch.no_grad():
            out = self._forward(handle.module, engine, sample[0], sample[1])
        return {self._OUTPUT: out if sample[0].batched else out[0]}, state

    # ------------------------------------------------------------------ training
    def check_trainable(self) -> None:
        pass

    def _train_create(self, engine, params):
        """An engine.BlobTrainHandle whose weight and gradient blobs ARE the parameters and gradients of a device copy of the
        module (no copy: slices of ``device_blob``): torch autograd accumulates into the blob, the library's AdamW steps it."""
        th = engine.blob_train_handle(self.flatten(params))
        mod = self._device_module(engine, params, self.state_of())
        # (views that do not reference th: th keeps the module, the module must not keep th - engine.BlobTrainHandle)
        w, g = th.device_blob("weights", keep_alive=False), th.device_blob("grads", keep_alive=False)
        off = 0
        for p in mod.parameters():
            n = p.numel()
            p.data = w[off:off + n].view(p.shape)
            p.grad = g[off:off + n].view(p.shape)
            p.requires_grad_(True)
            off += n
        th.module, th.view = mod, _TorchHandle(engine, mod)
        self._training = weakref.ref(th)
        return th

    def _check_state(self, state) -> None:
        """While a training handle of this model is open, `state` must be the buffers its module holds.  The Trainer hands
        `state` to apply only (push-forward on the host route, eval_rollout, checkpoints); loss_grad and the device unroll
        run on the training copy, made from the wrapped module's buffers.  A state that differs - a checkpoint's, after
        ``train(load_ckp=...)`` - would make the two sides compute with different buffers without a word: refuse it and name
        ``set_state``.  Leaves the state does not hold count as the wrapped module's."""
        th = self._training() if self._training is not None else None
        if th is None or th.module is None or not self._buffers or not state:
            return
        held = th.module.state_dict()
        for n in self._buffers:
            mod, leaf = _split(n)
            if mod in state and leaf in state[mod]:
                a = np.asarray(state[mod][leaf])
                b = held[n].detach().cpu().numpy()
                if a.shape != b.shape or not np.array_equal(a.astype(b.dtype), b):
                    raise RuntimeError(f"TorchModel: the state handed to apply differs from the buffers of the open training "
                                       f"handle's module (buffer {n!r}); call model.set_state(state) before Trainer.train / "
                                       "train_handle so that the training copy is made from it")

    def loss_grad(self, th, target, loss_weight) -> float:
        """The reference's _mse (trainer.py:35-60) on the engine's current window and list: squared error summed over dim,
        averaged over the non-kinematic particles of each trajectory, weighted by loss_weight[output]; the gradients of
        the batch are summed (into th's gradient blob), the return value is the mean of the per-trajectory losses."""
        engine = th.engine
        self._check_padded(engine)
        if engine.particle_type is None:
            raise RuntimeError("TorchModel.loss_grad: the engine has no particle types yet (case.preprocess sets them)")
        features = FeatureDict(engine, engine.read_window(), True)
        pt = engine.particle_type
        pred = self._forward(th.module, engine, features, pt)
        tgt = torch.as_tensor(target[self._OUTPUT]).to(device=engine.device, dtype=torch.float32).reshape(pred.shape)
        mask = non_kinematic_mask(pt)
        per_particle = torch.where(mask, ((pred - tgt) ** 2).sum(-1), torch.zeros((), device=engine.device))
        per_traj = float(loss_weight.get(self._OUTPUT, 1.0)) * per_particle.sum(1) / mask.sum(1)
        per_traj.sum().backward()
        return float(per_traj.detach().mean())

    def unroll_handle(self, engine, th, params_like):
        """The handle on the training handle's live module: its weights already are the device weights."""
        self._check_padded(engine)
        return th.view
