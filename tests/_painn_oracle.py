"""Torch restatement of the reference PaiNN (lagrangebench/models/painn.py) in any dtype.

Written from the reference, not from csrc/lb_painn.hip:
  _transform        scalars vel_mag (+ one-hot of 9 types); vectors (N, dim, C) = [vel_hist (N, K, dim)^T | force[..., None]
                    | bound (N, 2, dim)^T]; edges rel_disp
  __call__          norm = sqrt(|rel_disp|^2 + eps); dir = rel_disp / (norm + eps)
  _get_filters      W = filter_net(rbf(norm)) * (cutoff(norm) or norm), split per layer (or shared)
  gaussian_rbf      exp(-0.5 / widths^2 (norm - offset)^2)
  cosine_cutoff     0.5 (cos(norm pi / rc) + 1) (norm < rc)
  _embed            s = scalar_embedding(scalars), v = vector_embedding(vectors) (no bias)
  _message          x = Linear(3H)(silu(Linear(H)(s))); ds, dv1, dv2 = split(W x[receivers]);
                    dv = dv1 dir + dv2 v[receivers]; segment_sum at SENDERS; s += clip(ds), v += clip(dv)
  _update           v_l, v_r = split(vector_mixing_block(v)); |v_r| = sqrt(sum_dim v_r^2 + eps);
                    ds, dv, dsv = split(mixing_block([s, |v_r|])); s += clip(ds + dsv sum_dim v_r v_l); v += clip(v_l dv)
  PaiNNReadout      GatedEquivariantBlock(H, H/2, H/2) then (H/2, 1, 1); acc = squeeze(v)

Features and the edge list come from oracle.lb_oracle's case; padded edges (index N) are dropped, as segment_sum with
num_segments = N drops them in the reference.  Returns the per-layer s (N, H), v (N, dim, H) and the acc (N, dim).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

NODE_TYPE_SIZE = 9
EPS = 1e-8


def _silu(x):
    return x * torch.sigmoid(x)


def painn_forward(params: Dict, features: Dict, particle_type, *, num_mp_steps: int, n_vels: int, rbf: Tuple,
                  cutoff: Optional[float], homogeneous: bool = True, shared_filters: bool = False,
                  shared_interactions: bool = False, dtype=torch.float64
                  ) -> Tuple[List[torch.Tensor], List[torch.Tensor], torch.Tensor]:
    """One trajectory.  params: models.PaiNN layout; rbf = (widths, offsets); cutoff None = no cutoff_fn."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    P = {m: {k: t(v) for k, v in leaves.items()} for m, leaves in params.items() if m != "~"}
    lin = lambda m, x: x @ P[m]["w"] + P[m]["b"] if "b" in P[m] else x @ P[m]["w"]

    vel_hist = t(features["vel_hist"])
    N = vel_hist.shape[0]
    vecs = [vel_hist.reshape(N, n_vels, -1).transpose(1, 2)]
    if "force" in features:
        vecs.append(t(features["force"])[..., None])
    if "bound" in features:
        vecs.append(t(features["bound"]).reshape(N, 2, -1).transpose(1, 2))
    vectors = torch.cat(vecs, -1)                                   # (N, dim, C)
    scalars = t(features["vel_mag"])
    if not homogeneous:
        pt = torch.as_tensor(np.asarray(particle_type), dtype=torch.int64)
        oh = torch.zeros((N, NODE_TYPE_SIZE), dtype=dtype)
        ok = (pt >= 0) & (pt < NODE_TYPE_SIZE)
        oh[torch.arange(N)[ok], pt[ok]] = 1
        scalars = torch.cat([scalars, oh], -1)

    senders = torch.as_tensor(np.asarray(features["senders"]), dtype=torch.int64)
    receivers = torch.as_tensor(np.asarray(features["receivers"]), dtype=torch.int64)
    rel = t(features["rel_disp"])
    keep = (senders < N) & (receivers < N)
    senders, receivers, rel = senders[keep], receivers[keep], rel[keep]

    norm = torch.sqrt(torch.sum(rel ** 2, dim=1, keepdim=True) + EPS)   # (E, 1)
    direction = rel / (norm + EPS)
    widths, offsets = t(np.ravel(rbf[0])), t(np.ravel(rbf[1]))
    phi = torch.exp((-0.5 / widths ** 2) * (norm - offsets) ** 2)     # (E, R)
    if cutoff is not None:
        scale = 0.5 * (torch.cos(norm * math.pi / cutoff) + 1.0) * (norm < cutoff).to(dtype)
    else:
        scale = norm
    filters = lin("filter_net", phi) * scale
    H = P["scalar_embedding"]["w"].shape[1]
    fl = [filters] * num_mp_steps if shared_filters else list(torch.split(filters, 3 * H, dim=-1))

    s = lin("scalar_embedding", scalars)                            # (N, H)
    v = vectors @ P["vector_embedding"]["w"]                        # (N, dim, H)
    ss, vs = [s], [v]
    for n in range(num_mp_steps):
        q = "layer_0/" if shared_interactions else f"layer_{n}/"
        x = lin(q + "interaction_1", _silu(lin(q + "interaction_0", s)))
        w = fl[n] * x[receivers]
        ds, dv1, dv2 = torch.split(w, H, dim=-1)
        dv = dv1[:, None, :] * direction[:, :, None] + dv2[:, None, :] * v[receivers]
        ds = torch.zeros_like(s).index_add_(0, senders, ds)
        dv = torch.zeros_like(v).index_add_(0, senders, dv)
        s = s + torch.clamp(ds, -100.0, 100.0)
        v = v + torch.clamp(dv, -100.0, 100.0)
        vm = v @ P[q + "vector_mixing"]["w"]
        v_l, v_r = vm[..., :H], vm[..., H:]
        v_norm = torch.sqrt(torch.sum(v_r ** 2, dim=1) + EPS)      # (N, H)
        m = lin(q + "mixing_1", _silu(lin(q + "mixing_0", torch.cat([s, v_norm], -1))))
        ds, dvm, dsv = torch.split(m, H, dim=-1)
        s = s + torch.clamp(ds + dsv * torch.sum(v_r * v_l, dim=1), -100.0, 100.0)
        v = v + torch.clamp(v_l * dvm[:, None, :], -100.0, 100.0)
        ss.append(s)
        vs.append(v)

    def gated(prefix, s, v, n_out):
        vm = v @ P[prefix + "vector_mix"]["w"]
        v_l, v_r = vm[..., :n_out], vm[..., n_out:]
        g = torch.cat([s, torch.sqrt(torch.sum(v_r ** 2, dim=1) + EPS)], -1)
        y = lin(prefix + "gate_1", _silu(lin(prefix + "gate_0", g)))
        return y[:, :n_out], v_l * y[:, n_out:][:, None, :]

    s1, v1 = gated("readout_0/", s, v, H // 2)
    _, v2 = gated("readout_out/", s1, v1, 1)
    return ss, vs, v2[..., 0]


def rbf_of(model, params, state) -> Tuple[np.ndarray, np.ndarray]:
    """(widths, offsets) the model runs with."""
    return model._rbf(params, state)


def random_biases(params: Dict, seed: int, scale: float = 0.1) -> Dict:
    """Copy of `params` with random non-zero biases (the initialiser's zeros would leave them untested)."""
    r = np.random.default_rng(seed)
    out = {m: {k: np.array(v, copy=True) for k, v in leaves.items()} for m, leaves in params.items()}
    for m, leaves in out.items():
        if "b" in leaves:
            leaves["b"] = (scale * r.standard_normal(leaves["b"].shape)).astype(np.float32)
    return out
