"""Shared pieces of the PaiNN training tests: the masked _mse (train/trainer.py:35-60) over tests/_painn_oracle's
restatement with the autograd graph kept, and the device-gradient check of csrc/lb_train_painn.h against it."""
import numpy as np
import torch

import tests._painn_oracle as PO


class _NpPass:
    """numpy whose asarray / ravel pass torch tensors through (the restatement then keeps the autograd graph)."""

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def asarray(a, *args, **kw):
        return a if isinstance(a, torch.Tensor) else np.asarray(a, *args, **kw)

    @staticmethod
    def ravel(a):
        return a.reshape(-1) if isinstance(a, torch.Tensor) else np.ravel(a)


class _TorchPass:
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def as_tensor(a, dtype=None, device=None):
        return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=dtype, device=device)


def kinematic(pt):
    pt = np.asarray(pt)
    return (pt == 1) | (pt == 2) | (pt == -1)   # utils.py:28-35


def tparams(params):
    """float64 torch leaves of a parameter tree, "~" (a trainable radial basis) included."""
    return {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in lv.items()}
            for m, lv in params.items()}


def oracle_kw(model, tp, state):
    """painn_forward's keywords for `model`; the radial basis as torch leaves when it is trainable."""
    if model.radial_basis_fn.trainable:
        rbf = (tp["~"]["widths"], tp["~"]["offset"])
    else:
        rbf = model._rbf(None, state)
    return dict(num_mp_steps=model._num_mp_steps, n_vels=model._n_vels, rbf=rbf,
                cutoff=model.cutoff_fn.cutoff if model.cutoff_fn is not None else None,
                homogeneous=model._homogeneous_particles, shared_filters=model._shared_filters,
                shared_interactions=model._shared_interactions)


def painn_forward_graph(tp, features, particle_type, dtype=torch.float64, **kw):
    """tests/_painn_oracle.painn_forward with the autograd graph kept -> (ss, vs, acc)."""
    old_np, old_torch = PO.np, PO.torch
    PO.np, PO.torch = _NpPass(), _TorchPass()
    try:
        return PO.painn_forward(tp, features, particle_type, dtype=dtype, **kw)
    finally:
        PO.np, PO.torch = old_np, old_torch


def painn_loss(tp, features, particle_type, target, *, dtype=torch.float64, loss_weight=1.0, **kw):
    """_mse of one trajectory: sum over dim of (acc - target)^2, masked to the non-kinematic particles, / their number."""
    _, _, acc = painn_forward_graph(tp, features, particle_type, dtype=dtype, **kw)
    tot = loss_weight * ((acc.double() - torch.as_tensor(np.asarray(target), dtype=torch.float64)) ** 2).sum(-1)
    nk = torch.as_tensor(~kinematic(particle_type))
    return torch.where(nk, tot, torch.zeros_like(tot)).sum() / nk.sum(), acc


def batch_autograd(model, params, state, ocase, pos, pt, target, dtype, loss_fn=None):
    """Leaves with .grad = the gradient of the batch's summed per-trajectory losses, and the mean loss, on the oracle's
    graphs.  loss_fn(acc (N, dim), b) -> scalar replaces the masked _mse."""
    isl = model._n_vels + 1
    tp = tparams(params)
    losses = []
    for b in range(pos.shape[0]):
        of, _ = ocase.allocate_eval((pos[b, :, :isl].astype(np.float64), pt[b]))
        kw = oracle_kw(model, tp, state)
        if loss_fn is None:
            lb, _ = painn_loss(tp, of, pt[b], np.asarray(target[b]), dtype=dtype, **kw)
        else:
            lb = loss_fn(painn_forward_graph(tp, of, pt[b], dtype=dtype, **kw)[2], b)
        lb.backward()
        losses.append(float(lb.detach()))
    return tp, float(np.mean(losses))


def compare_leaves(g_h, tp64, tp32, tag):
    """Every leaf within 1e-4 of its largest entry against float64 autograd, else within 3x the float32 restatement's own
    deviation (printed)."""
    worst, loose, bad = 0.0, [], []
    for mod, lv in tp64.items():
        for leaf, v in lv.items():
            ref = v.grad.numpy().reshape(-1)
            dev = np.abs(np.asarray(g_h[mod][leaf], np.float64).reshape(-1) - ref).max()
            err = dev / max(np.abs(ref).max(), 1e-30)
            if err >= 1e-4:
                dev32 = np.abs(tp32[mod][leaf].grad.numpy().reshape(-1) - ref).max()
                if dev <= 3 * dev32:
                    loose.append(f"{mod}/{leaf}")
                else:
                    bad.append((mod, leaf, float(err), float(dev), float(dev32)))
                    print(f"[painn grad {tag}] {mod}/{leaf}: relative error {err:.3e} (fp32 restatement {dev32:.3e} absolute)")
            else:
                worst = max(worst, err)
    assert not bad, (tag, bad)
    print(f"[painn grad {tag}] worst relative gradient error {worst:.2e}; leaves held to the fp32 restatement: "
          f"{loose or 'none'}")
    return worst


def painn_grad_check(th, model, params, state, ocase, pos, pt, target, apply_acc, tag):
    """One lb_gns_train_loss_grad on the engine's current window / list: prediction = PaiNN.apply's bits, loss within 1e-5
    of the oracle's, every leaf by compare_leaves, two further calls the same bits, read("weights") = flatten.
    Returns (loss, gradient tree, flat gradients, float64 leaves)."""
    th.zero_grad()
    loss_h, pred_h = th.loss_grad(target, 1.0, want_pred=True)
    assert np.array_equal(pred_h.cpu().numpy(), apply_acc)
    g_flat = th.read("grads")
    for _ in range(2):
        th.zero_grad()
        assert th.loss_grad(target, 1.0) == loss_h and np.array_equal(th.read("grads"), g_flat)
    assert np.array_equal(th.read("weights"), model.flatten(params, state))
    assert np.isfinite(g_flat).all() and np.abs(g_flat).max() > 0
    g_h = model.unflatten(g_flat, like=params)
    tp64, loss64 = batch_autograd(model, params, state, ocase, pos, pt, target, torch.float64)
    tp32, _ = batch_autograd(model, params, state, ocase, pos, pt, target, torch.float32)
    print(f"[painn grad {tag}] loss {loss_h:.9e} oracle {loss64:.9e}")
    assert abs(loss_h - loss64) <= 1e-5 * abs(loss64), (loss_h, loss64)
    compare_leaves(g_h, tp64, tp32, tag)
    return loss_h, g_h, g_flat, tp64
