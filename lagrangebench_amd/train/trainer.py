"""Trainer - mirror of lagrangebench/train/trainer.py.

Same loop as the reference (trainer.py:209-421): shuffled windows of the training split -> push-forward
unroll length (strats.py:86-109) -> ``case.preprocess`` (random-walk noise, neighbor list, features,
normalised acceleration target) -> optional no-grad unroll steps -> MSE over the non-kinematic particles
(:35-60) -> gradients summed over the batch, loss averaged (:63-89) -> AdamW(weight_decay 1e-8) on an
exponentially decaying learning rate (:183-193) -> every ``eval_steps``: validation rollouts through
``eval_rollout`` (the fused HIP loop) + checkpoint in the reference's on-disk format (:385-407).

What runs where: neighbor list, feature assembly, integrator, every evaluation rollout AND the loss step are the
HIP engine: ``lb_gns_train_loss_grad`` (csrc/lb_train.hip: forward with saved activations, masked MSE, hand-written
backward kernels, MFMA products of our own for the dense contractions) accumulates the gradients of the whole batch,
``lb_adamw_step`` applies optax.adamw on the device; weights, gradients and both moments stay in HBM as fp32.
Arithmetic of the products (include/lbhip.h, ``lb_gns_train_math_fallbacks``): by default three fp16 MFMA passes over hi / lo
splits of the fp32 operands under exact power-of-two scaling, fp32 accumulate (error per term <= 2^-22 of the operand
block's scale; gradients within 1e-4 per leaf of float64 autograd), with a range guard on the weight-gradient kernel's
activation operand: a step that trips it is repeated with the site's X scale re-centred, or scaled per chunk, in f16x2;
``LB_TRAIN_MATH=f32`` in the environment when the handle is created selects the exact-fp32 MFMA kernels throughout (1.7x
slower).
torch is used for the noise / sampling random streams and as the tensor container only.  Trainable: GNS (latent <= 128,
two to eight Linears per MLP), since round 5 SEGNN (lmax 1, hidden <= 32x0e+32x1o: ``lb_segnn_train_loss_grad``,
csrc/lb_train_segnn.h) and EGNN (``lb_egnn_train_loss_grad``, csrc/lb_train_egnn.h: the inference forward, a hand-written
backward on the exact-fp32 MFMA products; the loss covers every output the model predicts - pos, vel, acc - weighted by
``loss_weight`` against the case's targets, as _mse does; ``normalize=True`` is refused), PaiNN of hidden size 64 to 128
(csrc/lb_train_painn.h: the inference forward, a hand-written backward on the same exact-fp32 products, the radial basis
trained or frozen as ``gaussian_rbf(trainable=...)`` says) and the Linear baseline
(csrc/lb_train_linear.h, exact fp32) - the loop below is the
reference's model-agnostic one; wandb logging is not wired (stdout).

Data parallel (one process per GPU under torchrun, lagrangebench_amd/dist.py): ``train.batch_size``
stays the GLOBAL batch.  Every rank draws the same permutation and the same push-forward unroll count from the common random
stream and trains on its ``shard_batch`` slice of each batch (noise: a stream of its own); the gradient blobs are all-gathered
and ONE HIP kernel sums them in rank order and applies AdamW (``lb_adamw_step_gathered``), so every rank holds the same weight
bits after every step - checked at each evaluation.  The semantics are the single-process ones: gradients summed over the
global batch, loss averaged, learning rate as configured.  One rank runs the code below exactly as before.

``train.device_data`` (default off): the train split is uploaded once (data.DeviceDataset) and the
sample of a step - window, random-walk noise, shift, targets - is made by one HIP launch (``case.preprocess_device``) instead
of on the host.  Permutation and unroll count still come from the common stream; the noise is keyed by (seed, step, global
slot), so a rank's shard gets the single-process noise of its slots.  With the key off nothing below changes.

``train.device_unroll`` (default off): the push-forward unroll of GNS, EGNN and PaiNN runs on an
inference handle fed from the training handle's device weights (``model.unroll_handle``: ``lb_gns_train_sync_model`` re-packs
the GNS images in HIP, EGNN and PaiNN lend their views) instead of ``th.read("weights")`` + a host repack; same bits, every rank does the same.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import dist as lbdist
from ..defaults import defaults, merge
from ..evaluate import MetricsComputer, averaged_metrics, eval_rollout
from ..evaluate.rollout import _Loader
from ..models.base import BaseModel
from ..utils import broadcast_from_batch, get_kinematic_mask, load_haiku, save_haiku
from .strats import push_forward_build, push_forward_sample_steps


def exponential_decay(step: int, init_value: float, transition_steps: float, decay_rate: float,
                      end_value: float) -> float:
    """optax.exponential_decay(init, transition_steps, decay_rate, end_value) as used at trainer.py:183-188:
    init * rate ** (step / transition_steps), clipped at end_value."""
    v = init_value * decay_rate ** (step / transition_steps)
    return max(v, end_value) if decay_rate < 1 else min(v, end_value)


class _ShuffledLoader:
    """DataLoader(dataset, batch_size, shuffle=True, drop_last=True, collate_fn=numpy_collate), in process.  `shard`: the
    slice of every batch that is read and yielded (data parallel: the permutation is the common one, a rank reads its part).
    `indices_only` (train.device_data): nothing is read; a batch is (the shard's window numbers, their slot numbers in the
    global batch) - the same permutation, drawn the same way."""

    def __init__(self, dataset, batch_size: int, generator: torch.Generator, shard: slice = slice(None),
                 indices_only: bool = False):
        self.dataset, self.batch_size, self.generator, self.shard = dataset, batch_size, generator, shard
        self.indices_only = indices_only

    def __iter__(self):
        n = len(self.dataset)
        perm = torch.randperm(n, generator=self.generator).tolist()
        for s in range(0, n - self.batch_size + 1, self.batch_size):
            if self.indices_only:
                yield perm[s:s + self.batch_size][self.shard], list(range(self.batch_size))[self.shard]
                continue
            items = [self.dataset[k] for k in perm[s:s + self.batch_size][self.shard]]
            yield (np.stack([it[0] for it in items]), np.stack([it[1] for it in items]))


class Trainer:
    def __init__(self, model: BaseModel, case, data_train, data_valid, cfg_train=None, cfg_eval=None, cfg_logging=None,
                 input_seq_length: int = defaults.model.input_seq_length, seed: int = defaults.seed):
        model.check_trainable()   # fail HERE, before datasets and neighbor lists are set up
        self.model, self.case, self.input_seq_length = model, case, input_seq_length
        self.cfg_train = merge(defaults.train, cfg_train)
        # data parallel: this rank's slice of every (global) batch; an indivisible batch_size fails HERE as well
        self.rank, self.local_rank, self.world = lbdist.env_world()
        self.shard = lbdist.shard_batch(self.cfg_train.batch_size, self.rank, self.world)
        self.seed = int(seed)
        self.device_data = bool(self.cfg_train.get("device_data", False))
        self.device_unroll = bool(self.cfg_train.get("device_unroll", False))
        self._dd = None
        if self.device_data:
            from ..data.device import trajectory_source
            trajectory_source(data_train)   # TypeError HERE for a dataset that does not expose its trajectories
        self.cfg_eval = merge(defaults.eval, cfg_eval)
        self.cfg_logging = merge(defaults.logging, cfg_logging)
        available = data_valid.subseq_length - input_seq_length
        assert self.cfg_eval.n_rollout_steps <= available, (
            "The loss cannot be evaluated on longer than a ground truth trajectory "
            f"({self.cfg_eval.n_rollout_steps} > {available})")
        assert self.cfg_eval.train.n_trajs <= data_valid.num_samples, (
            f"Number of requested validation trajectories exceeds the available ones "
            f"({self.cfg_eval.train.n_trajs} > {data_valid.num_samples})")
        if self.cfg_eval.train.n_trajs == -1:
            self.cfg_eval.train.n_trajs = data_valid.num_samples
        self.loss_weight = dict(self.cfg_train.loss_weight)
        self.base_key = torch.Generator()
        self.base_key.manual_seed(int(seed))
        self.loader_train = _ShuffledLoader(data_train, self.cfg_train.batch_size, self.base_key, self.shard,
                                            indices_only=self.device_data)
        self.loader_valid = _Loader(data_valid, self.cfg_eval.infer.batch_size)
        self.loader_valid.dataset = data_valid
        self.metrics_computer = MetricsComputer(self.cfg_eval.train.metrics, dist_fn=case.displacement,
                                                metadata=data_train.metadata, input_seq_length=input_seq_length,
                                                stride=self.cfg_eval.train.metrics_stride, case=case)

    def _lr(self, step: int) -> float:
        o = self.cfg_train.optimizer
        return exponential_decay(step, o.lr_start, o.lr_decay_steps, o.lr_decay_rate, o.lr_final)

    def _check_drift(self, th, device) -> None:
        """Every rank must hold the same weight bits (the rank-ordered sum guarantees it from equal starts): compare an
        fp64 sum and strided samples of the device weights across the ranks; raises on EVERY rank on a mismatch."""
        w = th.device_blob("weights").cpu().numpy()
        sig = np.concatenate([[w.sum(dtype=np.float64)], w[::max(1, w.size // 61)].astype(np.float64)])
        rows = lbdist.all_gather_rows(torch.from_numpy(sig).to(device)).cpu().numpy()
        bad = [r for r in range(rows.shape[0]) if not np.array_equal(rows[r].view(np.uint64), rows[0].view(np.uint64))]
        if bad:
            raise RuntimeError(f"data-parallel training: the weights of rank(s) {bad} differ from rank 0's (fp64 sums "
                               f"{[float(rows[r, 0]) for r in bad]} vs {float(rows[0, 0])}): the ranks no longer train "
                               "the same model")

    def train(self, step_max: int = defaults.train.step_max, params=None, state=None, opt_state=None,
              store_ckp: Optional[str] = None, load_ckp: Optional[str] = None, wandb_config=None
              ) -> Tuple[Dict, Dict, Dict]:
        """trainer.py:209-421.  Returns (params as numpy, state, opt_state = {"m", "v", "step"} flat AdamW moments)."""
        model, case, cfg_train, cfg_eval, cfg_logging = self.model, self.case, self.cfg_train, self.cfg_eval, self.cfg_logging
        noise_std, pushforward = cfg_train.noise_std, cfg_train.pushforward
        isl = self.input_seq_length
        rank, world = self.rank, self.world
        ddp = world > 1
        if ddp:
            # the process group: RCCL with one GPU per rank; LB_DIST_BACKEND=gloo when ranks share a device
            lbdist.init()
            if case.device is None:
                torch.cuda.set_device(lbdist.local_device(self.local_rank))
            # the common stream (base_key: permutations, unroll counts, the initial weights) steers control flow and is
            # identical on all ranks; the noise of a rank's shard comes from a stream of its own
            noise_key = torch.Generator()
            noise_key.manual_seed((self.seed * 1000003 + rank + 1) % (2**63 - 1))
        say = print if rank == 0 else (lambda *a, **k: None)
        key = self.base_key
        raw_batch = next(iter(self.loader_train))
        dd = None
        if self.device_data:
            # the train split goes to the device once; a sample is then (window number, global slot) and its noise is keyed
            # by (seed, step, slot) - on every rank the single-process noise of that slot (noise_key is not used)
            from ..data.device import DeviceDataset
            if self._dd is None:
                self._dd = DeviceDataset(self.loader_train.dataset, device=case.device)
            dd = self._dd
            raw_sample = tuple(self.loader_train.dataset[raw_batch[0][0]])   # the one host read: sizes lists and weights
        else:
            raw_sample = (raw_batch[0][0], raw_batch[1][0])
        key, features, _, neighbors = case.allocate(key, raw_sample)
        device = case.engine(1).device

        step = 0
        if params is not None:
            state = {} if state is None else state
        elif load_ckp:
            params, state, opt_state, step = load_haiku(load_ckp)
            params = model.params_from_haiku(params)
        else:
            params, state = model.init(torch.randint(0, 2**31 - 1, (1,), generator=key).numpy(), (features, raw_sample[1]))
        B = self.shard.stop - self.shard.start   # the local batch (= train.batch_size on one rank)
        th = model.train_handle(case.engine(B), params)   # weights, gradients, AdamW moments: device resident
        if isinstance(opt_state, dict) and "m" in opt_state and "v" in opt_state:
            th.write("m", np.asarray(opt_state["m"], np.float32))
            # `count` = AdamW steps taken (optax's count); checkpoints of round 3 only carried the loop index `step`
            th.write("v", np.asarray(opt_state["v"], np.float32), step=int(opt_state.get("count", opt_state.get("step", step))))
        o = cfg_train.optimizer

        def current_params():
            return model.unflatten(th.read("weights"), params)

        def opt_state_dict():
            # count: the device's AdamW step counter - NOT the loop index (it is step + 1 after an update, and differs
            # again after neighbor-list overflow `continue`s); a resumed run restores it, as optax does from opt_state
            return {"kind": "lagrangebench_amd adamw (flat blobs in the model's flatten order)", "m": th.read("m"),
                    "v": th.read("v"), "step": int(step), "count": th.step_count()}
        if store_ckp is not None and rank == 0:
            os.makedirs(os.path.join(store_ckp, "best"), exist_ok=True)

        push_forward = push_forward_build(model.apply, case)
        # train.device_unroll: the unroll's model is a device handle on th's weights.  Asked for HERE, while `params` are
        # the weights th holds, so that a model that makes its handle by the host route does not read them back for it.
        push_forward_dev = None
        if self.device_unroll:
            if model.unroll_handle(case.engine(B), th, params) is None:
                say(f"train.device_unroll: {type(model).__name__} has no device route; the unroll copies the weights to the host")
            else:
                push_forward_dev = push_forward_build(model.apply_handle, case)   # (its "params" are the handle)
        log = []
        while step < step_max + 1:
            for raw_batch in self.loader_train:
                key, unroll_steps = push_forward_sample_steps(key, step, pushforward)
                sample = (raw_batch[0], raw_batch[1])   # (this rank's shard of the batch)
                if dd is not None:
                    idx, slots = raw_batch
                    sample = (None, dd.particle_types(idx))
                    features_batch, target_batch, neighbors = case.preprocess_device(dd, idx, slots, self.seed, step, noise_std,
                                                                                     neighbors, unroll_steps)
                elif ddp:
                    _, features_batch, target_batch, neighbors = case.preprocess(noise_key, sample, noise_std, neighbors,
                                                                                 unroll_steps)
                else:
                    key, features_batch, target_batch, neighbors = case.preprocess(key, sample, noise_std, neighbors,
                                                                                   unroll_steps)
                if unroll_steps > 0 and not bool(neighbors.did_buffer_overflow.sum() > 0):
                    if push_forward_dev is not None:
                        # (GNS: its images re-made from the weights of the last AdamW step; no host copy of them)
                        pf, params_np = push_forward_dev, model.unroll_handle(case.engine(B), th, params)
                    else:
                        pf, params_np = push_forward, current_params()
                    # the noisy positions the features were computed from ARE the engine's window
                    cur = case.engine(B).read_window()
                    tshift = unroll_steps
                    for _ in range(unroll_steps):
                        if neighbors.did_buffer_overflow.sum() > 0:
                            break
                        cur, neighbors, features_batch = pf(features_batch, cur, torch.as_tensor(sample[1]), neighbors,
                                                            params_np, state)
                    del tshift
                overflow = bool(neighbors.did_buffer_overflow.sum() > 0)
                # a step is skipped by ALL ranks or by none (no rank may reach a collective that another one skips); only
                # the ranks whose list overflowed re-allocate
                skip = lbdist.max_over_ranks(float(overflow), device) > 0 if ddp else overflow
                if overflow:
                    say(f"Reallocate neighbors list at step {step}")
                    ind = int(torch.argmax(neighbors.did_buffer_overflow.int()))
                    old = neighbors.max_occupancy
                    akey = noise_key if ddp else key
                    if dd is not None:
                        sel = slice(None) if case.engine(B).has_pads else ind   # the same two branches, on the device
                        _, _, neighbors = case.allocate_device(dd, idx[sel], slots[sel], self.seed, step, noise_std)
                    elif case.engine(B).has_pads:
                        # padded trajectories: a list sized on ONE sample cannot serve a batch that mixes particle counts
                        # (the next, larger trajectory overflows it again, and so on): size it on the whole batch
                        _, _, _, neighbors = case.allocate(akey, sample, noise_std)
                    else:
                        _, _, _, neighbors = case.allocate(akey, (sample[0][ind], sample[1][ind]), noise_std)
                    say(f"From (2, {old}) to (2, {neighbors.max_occupancy})")
                if skip:
                    continue
                # value_and_grad of _mse vmapped over the batch, gradients summed, loss averaged (trainer.py:63-89) +
                # optax.adamw(lr(step), weight_decay 1e-8): on the engine's current window / neighbor list
                th.zero_grad()
                loss = model.loss_grad(th, target_batch, self.loss_weight)
                if ddp:
                    # every rank's gradient blob -> every rank; summed in rank order and applied in one launch
                    th.adamw_step_gathered(lbdist.all_gather_rows(th.device_blob("grads")), self._lr(step), 0.9, 0.999, 1e-8,
                                           float(getattr(o, "weight_decay", 1e-8)))
                else:
                    th.adamw_step(self._lr(step), 0.9, 0.999, 1e-8, float(getattr(o, "weight_decay", 1e-8)))

                if step % cfg_logging.log_steps == 0:
                    if ddp:
                        # mean over the (equal) shards of the local means = the mean over the global batch; fp64, rank order
                        loss = sum(lbdist.gather_scalars(float(loss), device)) / world
                    step_str = str(step).zfill(len(str(int(step_max))))
                    say(f"{step_str}, train/loss: {float(loss):.5f}.")
                    log.append((step, float(loss)))
                if step % cfg_logging.eval_steps == 0 and step > 0:
                    params_np = current_params()
                    if ddp:
                        self._check_drift(th, device)
                    eval_metrics = eval_rollout(model_apply=model.apply, case=case, params=params_np, state=state,
                                                loader_eval=self.loader_valid, neighbors=broadcast_from_batch(neighbors, 0),
                                                metrics_computer=self.metrics_computer,
                                                n_rollout_steps=cfg_eval.n_rollout_steps, n_trajs=cfg_eval.train.n_trajs,
                                                rollout_dir=cfg_eval.rollout_dir, out_type=cfg_eval.train.out_type)
                    metrics = averaged_metrics(eval_metrics)
                    if store_ckp is not None and rank == 0:
                        save_haiku(store_ckp, model.params_to_haiku(params_np), state, opt_state_dict(), {"step": step, "loss": metrics.get("val/loss", None)})
                    say(metrics)
                    # the validation rollouts re-sized / re-used the engine: the training list is rebuilt
                    key, _, _, neighbors = case.allocate(key, raw_sample)
                step += 1
                if step == step_max + 1:
                    break
        self.loss_log = log
        out = (current_params(), state, opt_state_dict())
        th.close()
        if ddp:
            lbdist.barrier(device)   # rank 0's last checkpoint is on disk before any rank goes on to load it
        return out
