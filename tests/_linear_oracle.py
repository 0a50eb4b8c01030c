"""Torch restatement of the reference's Linear baseline (lagrangebench/models/linear.py:30-42) and of the loss it is trained
with (train/trainer.py:35-60), written from the reference.

    x_i   = [vel_hist | vel_mag | bound | force | float(particle_type_i)]     (each block only if the case has it)
    acc_i = x_i W + b
    loss  = sum over the non-kinematic particles of |acc_i - target_i|^2 / their number

The loss is quadratic in (W, b), so its gradient has the closed form
    dW = 2 / n_nk X^T (M * (X W + b - T)),  db = 2 / n_nk sum_i (M * (X W + b - T))_i
with M the 0 / 1 mask of the non-kinematic rows."""
from __future__ import annotations

import numpy as np
import torch

ORDER = ("vel_hist", "vel_mag", "bound", "force")   # linear.py:35-38


def concat(features, particle_type, dtype=torch.float64) -> torch.Tensor:
    """The model's input rows (N, F + 1) from an oracle-case feature dict."""
    x = [torch.as_tensor(np.asarray(features[k]), dtype=dtype) for k in ORDER if k in features]
    x.append(torch.as_tensor(np.asarray(particle_type), dtype=dtype)[:, None])
    return torch.cat(x, dim=-1)


def linear_forward(w, b, features, particle_type, dtype=torch.float64) -> torch.Tensor:
    """acc (N, dim) in `dtype`; w (F + 1, dim) and b (dim,) are arrays or tensors (tensors keep their autograd graph)."""
    x = concat(features, particle_type, dtype)
    w = w.to(dtype) if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w), dtype=dtype)
    b = b.to(dtype) if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b), dtype=dtype)
    return x @ w + b


def non_kinematic(particle_type) -> torch.Tensor:
    pt = torch.as_tensor(np.asarray(particle_type))
    return ~((pt == 1) | (pt == 2) | (pt == -1))   # utils.py:28-35


def mse(pred: torch.Tensor, target, particle_type) -> torch.Tensor:
    """_mse with the kinematic mask, residuals in float64."""
    t = torch.as_tensor(np.asarray(target), dtype=torch.float64)
    nk = non_kinematic(particle_type)
    per = ((pred.double() - t) ** 2).sum(-1)
    return torch.where(nk, per, torch.zeros_like(per)).sum() / nk.sum()


def closed_form(w, b, features, particle_type, target):
    """(loss, dW, db) in float64 from the closed form above."""
    x = concat(features, particle_type, torch.float64)
    w = torch.as_tensor(np.asarray(w), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64)
    t = torch.as_tensor(np.asarray(target), dtype=torch.float64)
    m = non_kinematic(particle_type).double()[:, None]
    n = m.sum()
    r = m * (x @ w + b - t)
    return (r ** 2).sum() / n, 2.0 / n * (x.T @ r), 2.0 / n * r.sum(0)
