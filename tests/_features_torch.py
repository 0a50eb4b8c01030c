"""Differentiable torch restatement of the reference feature builder (case_setup/features.py:47-126), float64.

Written from the reference, not from the device kernels: TEST INFRASTRUCTURE for the position gradient of the device step
(csrc/lb_train.hip: k_feat_bwd).  The edge index is an INPUT (the neighbor search is not differentiated) and the external
force is a constant array, as in the device step.

  velocity_sequence = displacement(pos[:, 1:], pos[:, :-1])              features.py:58-66
  vel_hist = (velocity_sequence - mean) / std, flattened; vel_mag = |.|   features.py:68-78
  bound = clip([pos - lo, hi - pos] / r_c, -1, 1) when no axis is periodic features.py:80-101
  force                                                                   features.py:103-107
  rel_disp = displacement(pos[recv], pos[send]) / r_c, rel_dist = |rel_disp| (space.distance: safe sqrt)   features.py:109-124
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch


def case_constants(ds) -> Dict:
    """What feature_transform closes over, for a synthetic dataset, as the oracle case computes it."""
    from oracle import lb_oracle as O
    stats = O.get_dataset_stats(ds.metadata, ds.isotropic_norm, ds.noise_std)
    pbc = list(ds.metadata["periodic_boundary_conditions"])
    return dict(box=np.asarray(ds.box, np.float64), periodic=bool(np.any(pbc)), has_bound=not any(pbc),
                bounds=np.asarray(ds.metadata["bounds"], np.float64), rc=float(ds.metadata["default_connectivity_radius"]),
                vel_mean=np.asarray(stats["velocity"]["mean"], np.float64),
                vel_std=np.asarray(stats["velocity"]["std"], np.float64),
                acc_mean=np.asarray(stats["acceleration"]["mean"], np.float64),
                acc_std=np.asarray(stats["acceleration"]["std"], np.float64),
                magnitude=bool(getattr(ds, "magnitude_features", False)))


def displacement_torch(a: torch.Tensor, b: torch.Tensor, box, periodic: bool) -> torch.Tensor:
    """jax_md.space.periodic / free: mod(a - b + L / 2, L) - L / 2 (jnp.mod: sign of the divisor), or a - b."""
    d = a - b
    if not periodic:
        return d
    side = torch.as_tensor(np.asarray(box, np.float64), dtype=d.dtype, device=d.device)
    return torch.remainder(d + 0.5 * side, side) - 0.5 * side


def _safe_norm(x: torch.Tensor) -> torch.Tensor:
    """space.distance: sqrt of the squared norm with value and gradient 0 at 0 (jax-md's safe_mask)."""
    s = (x * x).sum(-1)
    ok = s > 0
    return torch.where(ok, torch.sqrt(torch.where(ok, s, torch.ones_like(s))), torch.zeros_like(s))


def features_torch(window: torch.Tensor, receivers: torch.Tensor, senders: torch.Tensor, *, box, periodic: bool,
                   has_bound: bool, bounds, rc: float, vel_mean, vel_std, magnitude: bool = False,
                   force: Optional[torch.Tensor] = None, **_unused) -> Dict[str, torch.Tensor]:
    """window (N, isl, dim) float64, receivers / senders (E,) int64 of the REAL edges -> the feature dict of
    feature_transform plus "node" (N, F) in the column order of GNS._transform (gns.py:135-157: vel_hist, vel_mag, bound,
    force) and "edge" (E, dim + 1) = [rel_disp | rel_dist]."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=window.dtype, device=window.device)
    N = window.shape[0]
    newest = window[:, -1]
    vel = displacement_torch(window[:, 1:], window[:, :-1], box, periodic)
    nvel = (vel - t(vel_mean)) / t(vel_std)
    out = {"vel_hist": nvel.reshape(N, -1)}
    if magnitude:
        out["vel_mag"] = _safe_norm(nvel)
    if has_bound:
        b = t(bounds)
        d2b = torch.cat([newest - b[:, 0][None], b[:, 1][None] - newest], dim=1)
        out["bound"] = torch.clamp(d2b / rc, -1.0, 1.0)
    if force is not None:
        out["force"] = force.to(window.dtype).detach()
    rel = displacement_torch(newest[receivers], newest[senders], box, periodic) / rc
    out["rel_disp"] = rel
    out["rel_dist"] = _safe_norm(rel)[:, None]
    out["node"] = torch.cat([out[k] for k in ("vel_hist", "vel_mag", "bound", "force") if k in out], dim=-1)
    out["edge"] = torch.cat([out["rel_disp"], out["rel_dist"]], dim=-1)
    return out
