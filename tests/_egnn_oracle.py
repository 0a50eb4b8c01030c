"""Torch restatement of the reference EGNN (lagrangebench/models/egnn.py) in any dtype.

Written from the reference, not from csrc/lb_egnn.hip:
  _transform       egnn.py:318-359   node input |v_k| (+ one-hot of 9 types), edge_attr = rel_dist,
                                     node_attr = |force|, pos = abs_pos[:, -1]
  __call__         egnn.py:372-400   h0 = scalar_emb(x); vel = vel_hist[:, -1] * std + mean; num_mp_steps layers
  _coord2radial    egnn.py:166-173   coord_diff = displacement(x[senders], x[receivers]); radial = |.|^2;
                                     normalize: coord_diff / (sqrt(radial) + 1e-8)
  _message         egnn.py:128-145   silu(silu([h_s, h_r, radial, edge_attr] W0 + b0) W1 + b1)  (MLPXav, activate_final)
  GraphNetwork     jraph             agg = segment_sum(messages, receivers)
  _update          egnn.py:147-164   h' = h + (silu([h, agg, node_attr] Wn0 + bn0) Wn1 + bn1)   (residual)
  _pos_update      egnn.py:119-126   x <- shift(x, segment_sum(coord_diff * phi(m), SENDERS))
                   egnn.py:95-104    phi = silu(m Wx0 + bx0) wx1 [tanh]
  velocity         egnn.py:106-112,203-204   x <- shift(x, psi(h') * vel), psi = silu(h' Wv0 + bv0) wv1

Features and the edge list come from oracle.lb_oracle's case (its feature transform); padded edges (index N) are
dropped, as segment_sum with num_segments = N drops them in the reference.  Returns the per-layer h and x.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

NODE_TYPE_SIZE = 9


def _silu(x):
    return x * torch.sigmoid(x)


def space(box, periodic: bool, dtype):
    """jax_md.space.periodic / free (oracle/lb_oracle.py: space_periodic) in torch."""
    if not periodic:
        return (lambda a, b: a - b), (lambda r, dr: r + dr)
    side = torch.as_tensor(np.asarray(box, np.float64), dtype=dtype)

    def mod(x):
        return torch.remainder(x, side)  # sign of the divisor, as jnp.mod

    return (lambda a, b: mod(a - b + 0.5 * side) - 0.5 * side), (lambda r, dr: mod(r + dr))


def egnn_forward(params: Dict, features: Dict, particle_type, *, box, periodic: bool, vel_mean, vel_std,
                 num_mp_steps: int, n_vels: int, homogeneous: bool = True, residual: bool = True,
                 normalize: bool = False, tanh: bool = False, dtype=torch.float64
                 ) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """One trajectory.  params: models.EGNN layout.  Returns ([h_0 .. h_L], [x_0 .. x_L])."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    P = {m: {k: t(v) for k, v in leaves.items()} for m, leaves in params.items()}
    disp, shift = space(box, periodic, dtype)
    abs_pos = t(features["abs_pos"])
    N = abs_pos.shape[0]
    vel_hist = t(features["vel_hist"]).reshape(N, n_vels, -1)
    pos = abs_pos[:, -1]
    edge_attr = t(features["rel_dist"]).reshape(-1, 1)
    node_attr = None
    if "force" in features:
        node_attr = torch.sqrt(torch.sum(t(features["force"]) ** 2, dim=-1, keepdim=True))
    x_in = torch.cat([torch.sqrt(torch.sum(vel_hist[:, i, :] ** 2, dim=-1, keepdim=True)) for i in range(n_vels)], -1)
    if not homogeneous:
        pt = torch.as_tensor(np.asarray(particle_type), dtype=torch.int64)
        oh = torch.zeros((N, NODE_TYPE_SIZE), dtype=dtype)
        ok = (pt >= 0) & (pt < NODE_TYPE_SIZE)
        oh[torch.arange(N)[ok], pt[ok]] = 1
        x_in = torch.cat([x_in, oh], -1)
    senders = torch.as_tensor(np.asarray(features["senders"]), dtype=torch.int64)
    receivers = torch.as_tensor(np.asarray(features["receivers"]), dtype=torch.int64)
    keep = (senders < N) & (receivers < N)
    senders, receivers, edge_attr = senders[keep], receivers[keep], edge_attr[keep]

    lin = lambda m, x: x @ P[m]["w"] + P[m]["b"] if "b" in P[m] else x @ P[m]["w"]
    h = lin("scalar_emb", x_in)
    vel = vel_hist[:, -1] * t(vel_std) + t(vel_mean)
    x = pos.clone()
    hs, xs = [h], [x]
    for n in range(num_mp_steps):
        p = f"layer_{n}/"
        coord_diff = disp(x[senders], x[receivers])
        radial = torch.sum(coord_diff ** 2, dim=1, keepdim=True)
        if normalize:
            coord_diff = coord_diff / (torch.sqrt(radial) + 1e-8)
        msg = torch.cat([h[senders], h[receivers], radial, edge_attr], -1)
        msg = _silu(lin(p + "edge_1", _silu(lin(p + "edge_0", msg))))
        agg = torch.zeros((N, msg.shape[1]), dtype=dtype).index_add_(0, receivers, msg)
        u = torch.cat([h, agg] + ([node_attr] if node_attr is not None else []), -1)
        u = lin(p + "node_1", _silu(lin(p + "node_0", u)))
        h = h + u if residual else u
        phi = lin(p + "pos_1", _silu(lin(p + "pos_0", msg)))
        if tanh:
            phi = torch.tanh(phi)
        trans = torch.zeros((N, x.shape[1]), dtype=dtype).index_add_(0, senders, coord_diff * phi)
        x = shift(x, trans)
        psi = lin(p + "vel_1", _silu(lin(p + "vel_0", h)))
        x = shift(x, psi * vel)
        hs.append(h)
        xs.append(x)
    return hs, xs


def case_kwargs(ds, ocase=None) -> Dict:
    """box / periodic / velocity statistics of a synthetic dataset, as the oracle case computes them."""
    from oracle import lb_oracle as O
    stats = O.get_dataset_stats(ds.metadata, ds.isotropic_norm, ds.noise_std)
    return dict(box=np.asarray(ds.box, np.float64), periodic=bool(np.any(ds.metadata["periodic_boundary_conditions"])),
                vel_mean=np.asarray(stats["velocity"]["mean"], np.float64),
                vel_std=np.asarray(stats["velocity"]["std"], np.float64))


def random_biases(params: Dict, seed: int, scale: float = 0.1) -> Dict:
    """Copy of `params` with random non-zero biases (the initialiser's zeros would leave them untested)."""
    r = np.random.default_rng(seed)
    out = {m: {k: np.array(v, copy=True) for k, v in leaves.items()} for m, leaves in params.items()}
    for m, leaves in out.items():
        if "b" in leaves:
            leaves["b"] = (scale * r.standard_normal(leaves["b"].shape)).astype(np.float32)
    return out
