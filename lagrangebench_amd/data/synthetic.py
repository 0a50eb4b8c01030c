"""Seeded synthetic stand-ins for the LagrangeBench datasets (there is no network: the Zenodo
files can not be fetched).  Geometry, particle counts, connectivity radii and feature layout
follow the real cases (reference data_gen/lagrangebench_data/*.sh,
notebooks/datasets.ipynb), so neighbor counts, node/edge feature widths and capacities are
representative; the dynamics are an analytic advection field, not SPH.

Every case returns an in-memory dataset object shaped like the reference's ``H5Dataset`` in
eval mode (data/data.py:33-269): ``ds[i] -> (pos (N,T,dim) float32, particle_type (N,) int32)``,
``ds.metadata`` (the keys case_builder / MetricsComputer read), ``ds.input_seq_length``,
``ds.num_samples`` and ``ds.force`` (a ForceSpec or None, standing in for ``force.py``).
"""
from __future__ import annotations

import math
import copy
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


class SyntheticDataset:
    def __init__(self, name, metadata, input_seq_length, extra_seq_length, n_trajs, make_traj,
                 force=None, force_numpy=None, multiplier=1.25, noise_std=3e-4, isotropic_norm=False):
        self.name = name
        self.metadata = metadata
        self.input_seq_length = input_seq_length
        self.extra_seq_length = extra_seq_length
        self.subseq_length = input_seq_length + extra_seq_length
        self.num_samples = n_trajs
        self._make = make_traj
        self.force = force                  # engine-side ForceSpec parameters (dict) or None
        self.external_force_fn = force_numpy  # numpy callable pos(n,dim)->(n,dim) (oracle side)
        self.multiplier = multiplier        # configs/*/base.yaml neighbors.multiplier
        self.noise_std = noise_std          # configs/*/gns.yaml train.noise_std
        self.isotropic_norm = isotropic_norm
        self._cache: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx: int):
        if idx < 0 or idx >= self.num_samples:
            raise IndexError(idx)
        if idx not in self._cache:
            self._cache[idx] = self._make(idx)
        return self._cache[idx]

    @property
    def box(self) -> np.ndarray:
        b = np.array(self.metadata["bounds"], dtype=np.float64)
        return b[:, 1] - b[:, 0]


def _meta(dim, n, box, pbc, rc, dx, vel_std, acc_std, T, name):
    return {
        "case": name, "solver": "synthetic", "dim": dim, "dx": dx, "dt": 1.0, "write_every": 1,
        "num_particles_max": int(n), "periodic_boundary_conditions": [bool(p) for p in pbc],
        "bounds": [[0.0, float(b)] for b in box], "default_connectivity_radius": float(rc),
        "vel_mean": [0.0] * dim, "vel_std": [float(vel_std)] * dim,
        "acc_mean": [0.0] * dim, "acc_std": [float(acc_std)] * dim,
        "sequence_length_test": int(T), "num_trajs_test": 1,
    }


def _lattice(counts, dx, origin=None):
    axes = [(np.arange(c) + 0.5) * dx for c in counts]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(counts))
    if origin is not None:
        g = g + np.asarray(origin)
    return g


def _advect(pos0, ptype, T, box, pbc, field, step_scale, rng, moving_vel=None, jitter=0.0):
    """x_{t+1} = wrap(x_t + step_scale * field(x_t) + jitter-noise); walls follow moving_vel."""
    N, dim = pos0.shape
    out = np.empty((N, T, dim), dtype=np.float64)
    x = pos0.copy()
    fluid = ptype == 0
    for t in range(T):
        out[:, t] = x
        dxv = step_scale * field(x)
        if jitter > 0:
            dxv = dxv + rng.normal(0.0, jitter, size=x.shape)
        dxv[~fluid] = 0.0
        if moving_vel is not None:
            dxv[ptype == 2] = moving_vel
        x = x + dxv
        if any(pbc):
            x = np.mod(x, box)
    return out.astype(np.float32)


def _tgv2d_field(L):
    k = 2 * math.pi / L
    return lambda x: np.stack([np.sin(k * x[:, 0]) * np.cos(k * x[:, 1]),
                               -np.cos(k * x[:, 0]) * np.sin(k * x[:, 1])], axis=-1)


def _tgv3d_field():
    return lambda x: np.stack([np.sin(x[:, 0]) * np.cos(x[:, 1]) * np.cos(x[:, 2]),
                               -np.cos(x[:, 0]) * np.sin(x[:, 1]) * np.cos(x[:, 2]),
                               np.zeros(len(x))], axis=-1)


def make_case(name: str, n_trajs: int = 1, extra_seq_length: int = 20, input_seq_length: int = 6,
              scale: float = 1.0, vel_amp: float = 1.0) -> SyntheticDataset:
    """name in {tgv2d, rpf2d, tgv3d, ldc3d, dam2d, small2d, small3d}.  ``scale`` multiplies the
    lattice counts per side (tests use small2d / small3d or scale < 1).  ``vel_amp`` multiplies the per-frame
    displacement of the analytic advection (and its jitter): a rollout with UNTRAINED weights is ballistic
    (x' = x + (x - x_prev) + ~0), so at the datasets' velocity scale (vel_amp 1) a 20-step rollout compresses the lattice
    and the neighbour count drifts (TGV3D: 13.6 -> 18.5 -> 17 per particle); ``vel_amp`` ~ 0.03 keeps the particles
    within half a spacing of their lattice sites over 40 steps, i.e. the neighbour count at the datasets' own value
    (13.1 per particle for TGV3D) - bench.py's `stationary` line."""
    name = name.lower()
    isl = input_seq_length
    T = isl + extra_seq_length

    def counts(c):
        return [max(4, int(round(v * scale))) for v in c]

    if name in ("tgv2d", "small2d"):
        c = counts([50, 50]) if name == "tgv2d" else [16, 16]
        dx = 1.0 / c[0]
        box = np.array([c[0] * dx, c[1] * dx])
        rc = 1.45 * dx  # 0.029 at dx = 0.02
        vel_std, acc_std = 0.318 * dx, 0.0438 * dx
        md = _meta(2, c[0] * c[1], box, [True, True], rc, dx, vel_std, acc_std, T, name)
        field = _tgv2d_field(box[0])

        def make(i):
            rng = np.random.default_rng(i)
            p0 = np.mod(_lattice(c, dx) + rng.normal(0, 0.1 * dx, size=(c[0] * c[1], 2)), box)
            pt = np.zeros(len(p0), np.int32)
            return _advect(p0, pt, T, box, [True] * 2, field, 1.4 * vel_std * vel_amp, rng, jitter=0.01 * dx * vel_amp), pt

        return SyntheticDataset(name, md, isl, extra_seq_length, n_trajs, make)

    if name == "rpf2d":
        c = counts([40, 80])
        dx = 1.0 / c[0]
        box = np.array([c[0] * dx, c[1] * dx])
        rc = 1.44 * dx  # 0.036 at dx = 0.025
        vel_std, acc_std = 0.3 * dx, 0.04 * dx
        md = _meta(2, c[0] * c[1], box, [True, True], rc, dx, vel_std, acc_std, T, name)
        half = box[1] / 2
        fmag = 1.0
        field = lambda x: np.stack([np.where(x[:, 1] > half, -1.0, 1.0) * np.sin(math.pi * (x[:, 1] % half) / half),
                                    np.zeros(len(x))], axis=-1)
        force = dict(kind="piecewise", axis=1, split=float(half), f_lo=[fmag, 0.0], f_hi=[-fmag, 0.0])
        fnp = lambda r: np.where(r[..., 1:2] > half, -1.0, 1.0) * np.array([fmag, 0.0])

        def make(i):
            rng = np.random.default_rng(i)
            p0 = np.mod(_lattice(c, dx) + rng.normal(0, 0.1 * dx, size=(c[0] * c[1], 2)), box)
            pt = np.zeros(len(p0), np.int32)
            return _advect(p0, pt, T, box, [True] * 2, field, 1.4 * vel_std * vel_amp, rng, jitter=0.01 * dx * vel_amp), pt

        return SyntheticDataset(name, md, isl, extra_seq_length, n_trajs, make, force=force, force_numpy=fnp)

    if name in ("tgv3d", "small3d"):
        c = counts([20, 20, 20]) if name == "tgv3d" else [8, 8, 8]
        L = 2 * math.pi
        dx = L / c[0]
        box = np.array([L, L, L])
        rc = 0.46 * (dx / 0.314159265)  # 0.46 at dx = 2*pi/20
        vel_std, acc_std = 0.3 * dx, 0.04 * dx
        n = c[0] * c[1] * c[2]
        md = _meta(3, n, box, [True] * 3, rc, dx, vel_std, acc_std, T, name)
        field = _tgv3d_field()

        def make(i):
            rng = np.random.default_rng(i)
            p0 = np.mod(_lattice(c, dx) + rng.normal(0, 0.1 * dx, size=(n, 3)), box)
            pt = np.zeros(n, np.int32)
            return _advect(p0, pt, T, box, [True] * 3, field, 1.4 * vel_std * vel_amp, rng, jitter=0.01 * dx * vel_amp), pt

        return SyntheticDataset(name, md, isl, extra_seq_length, n_trajs, make)

    if name == "ldc3d":
        # lid-driven cavity: fluid block 32x18x12 inside a one-particle wall shell in x,y; z periodic;
        # the top (y-max) wall row is the MOVING lid (type 2), the rest SOLID_WALL (type 1).  34 x 20 x 12 = 8160
        # particles: the dataset's count (3D_LDC_8160_10kevery100, notebooks/datasets.ipynb cell 5).
        c = counts([34, 20, 12])
        dx = 1.0 / 24.0 / max(scale, 1e-9) if scale != 1.0 else 1.0 / 24.0
        box = np.array([c[0] * dx, c[1] * dx, c[2] * dx])
        rc = 1.44 * dx  # 0.06 at dx = 1/24
        vel_std, acc_std = 0.3 * dx, 0.04 * dx
        lat = _lattice(c, dx)
        ij = np.stack(np.meshgrid(*[np.arange(v) for v in c], indexing="ij"), axis=-1).reshape(-1, 3)
        wall = (ij[:, 0] == 0) | (ij[:, 0] == c[0] - 1) | (ij[:, 1] == 0) | (ij[:, 1] == c[1] - 1)
        lid = ij[:, 1] == c[1] - 1
        ptype0 = np.where(lid, 2, np.where(wall, 1, 0)).astype(np.int32)
        n = len(lat)
        md = _meta(3, n, box, [True] * 3, rc, dx, vel_std, acc_std, T, name)
        cx, cy = box[0] / 2, box[1] / 2
        field = lambda x: np.stack([(x[:, 1] - cy) / cy, -(x[:, 0] - cx) / cx, np.zeros(len(x))], axis=-1) * \
            (np.sin(math.pi * x[:, 0] / box[0]) * np.sin(math.pi * x[:, 1] / box[1]))[:, None]

        def make(i):
            rng = np.random.default_rng(i)
            p0 = lat.copy()
            fl = ptype0 == 0
            p0[fl] += rng.normal(0, 0.08 * dx, size=(int(fl.sum()), 3))
            p0 = np.mod(p0, box)
            return _advect(p0, ptype0, T, box, [True] * 3, field, 1.2 * vel_std * vel_amp, rng,
                           moving_vel=np.array([0.09 * dx / (1.0 / 24.0), 0.0, 0.0]), jitter=0.01 * dx * vel_amp), ptype0.copy()

        return SyntheticDataset(name, md, isl, extra_seq_length, n_trajs, make, multiplier=2.0)

    if name == "dam2d":
        # dam break: fluid column 100x50 in the lower-left corner of a [5.486, 2.12] tank with a
        # wall frame; free surface => strongly non-uniform cell occupancy; gravity force feature.
        dx = 0.02 / max(scale, 1e-9) if scale != 1.0 else 0.02
        fl_c = counts([100, 50])
        box = np.array([5.486, 2.12]) * (dx / 0.02)
        rc = 1.45 * dx
        vel_std, acc_std = 0.3 * dx, 0.04 * dx
        nwx, nwy = int(box[0] / dx) - 1, int(box[1] / dx) - 1
        fluid = _lattice(fl_c, dx, origin=[2 * dx, 2 * dx])
        bottom = _lattice([nwx, 1], dx, origin=[0.5 * dx, 0.5 * dx])
        left = _lattice([1, nwy - 1], dx, origin=[0.5 * dx, 1.5 * dx])
        right = _lattice([1, nwy - 1], dx, origin=[(nwx - 0.5) * dx, 1.5 * dx])
        walls = np.concatenate([bottom, left, right])
        if scale == 1.0 and len(fluid) + len(walls) < 5740:
            # the dataset has 5740 particles (2D_DAM_5740_20kevery100: three wall layers); a second floor row below the
            # first brings the synthetic case to the same count
            extra = 5740 - len(fluid) - len(walls)
            walls = np.concatenate([walls, _lattice([extra, 1], dx, origin=[0.5 * dx, -0.5 * dx])])
        lat = np.concatenate([fluid, walls])
        ptype0 = np.concatenate([np.zeros(len(fluid), np.int32), np.ones(len(walls), np.int32)])
        n = len(lat)
        md = _meta(2, n, box, [True, True], rc, dx, vel_std, acc_std, T, name)
        g = 1.0
        field = lambda x: np.stack([np.ones(len(x)) * (x[:, 1] / (fl_c[1] * dx)), -0.15 * np.ones(len(x))], axis=-1)
        force = dict(kind="piecewise", axis=0, split=0.0, f_lo=[0.0, -g], f_hi=[0.0, -g])
        fnp = lambda r: np.zeros_like(r) + np.array([0.0, -g])

        def make(i):
            rng = np.random.default_rng(i)
            p0 = lat.copy()
            fl = ptype0 == 0
            p0[fl] += rng.normal(0, 0.08 * dx, size=(int(fl.sum()), 2))
            p0[fl, 1] = np.maximum(p0[fl, 1], 1.6 * dx)
            p0 = np.mod(p0, box)
            tr = _advect(p0, ptype0, T, box, [True, True], field, 1.0 * vel_std * vel_amp, rng, jitter=0.01 * dx * vel_amp)
            # keep the fluid above the floor (no real pressure solve here)
            tr[fl, :, 1] = np.maximum(tr[fl, :, 1], np.float32(1.3 * dx))
            return tr, ptype0.copy()

        return SyntheticDataset(name, md, isl, extra_seq_length, n_trajs, make, force=force, force_numpy=fnp,
                                multiplier=2.0, noise_std=1e-3, isotropic_norm=True)

    raise ValueError(f"unknown synthetic case {name!r}")


# ------------------------------------------------------------------------------------ padded trajectories
PAD_VALUE = -1  # utils.NodeType.PAD_VALUE


def _pad(pos: np.ndarray, pt: np.ndarray, n_max: int) -> Tuple[np.ndarray, np.ndarray]:
    """H5Dataset._matscipy_pad: trailing rows, position 0, particle type PAD_VALUE."""
    k = n_max - pos.shape[0]
    return (np.pad(pos, ((0, k), (0, 0), (0, 0)), mode="constant", constant_values=0.0),
            np.pad(pt, (0, k), mode="constant", constant_values=PAD_VALUE).astype(np.int32))


def make_padded_case(name: str, n_particles: Sequence[int], n_max: Optional[int] = None, extra_seq_length: int = 20,
                     input_seq_length: int = 6, scale: float = 1.0, vel_amp: float = 1.0) -> SyntheticDataset:
    """A dataset whose trajectory i has ``n_particles[i]`` real particles, every sample already padded to ``n_max``
    (default: the largest count) the way the reference pads variable-N data for its `matscipy` backend: trailing rows at
    position 0 with particle type -1; ``metadata["num_particles_max"] == n_max``.  ``ds.n_real[i]`` is the real count.

    ``name == "waterdrop2d"``: shaped like the GNS WaterDrop data - 2D, no periodic axis, bounds [0.1, 0.9]^2 (so the
    boundary-distance features are on), no wall particles; a block of fluid falling under gravity.  Any ``make_case``
    name (tgv2d, small2d, small3d, tgv3d, ...; ``scale`` / ``vel_amp`` as there): trajectory i is ``n_particles[i]``
    randomly chosen particles (seeded, index order kept) of that case's trajectory i."""
    name = name.lower()
    counts = [int(n) for n in n_particles]
    n_max = max(counts) if n_max is None else int(n_max)
    assert counts and min(counts) > 0 and n_max >= max(counts)
    isl = input_seq_length
    T = isl + extra_seq_length
    if name == "waterdrop2d":
        dx = 0.008
        lo, hi = 0.1, 0.9
        rc = 1.45 * dx
        vel_std, acc_std = 0.3 * dx, 0.04 * dx
        md = _meta(2, n_max, [hi - lo, hi - lo], [False, False], rc, dx, vel_std, acc_std, T, name)
        md["bounds"] = [[lo, hi], [lo, hi]]

        def make(i):
            rng = np.random.default_rng(1000 + i)
            n = counts[i]
            w = max(2, int(math.ceil(math.sqrt(2.0 * n))))          # a block about twice as wide as high
            lat = _lattice([w, (n + w - 1) // w], dx)[:n]
            org = np.array([lo + 0.1 + 0.25 * rng.random() * (hi - lo - 0.2 - w * dx), 0.45 + 0.1 * rng.random()])
            p0 = lat + org + rng.normal(0, 0.08 * dx, size=(n, 2))
            v0 = vel_amp * vel_std * np.array([0.8, 0.0]) + rng.normal(0, 0.05 * vel_std * vel_amp, size=(n, 2))
            g = vel_amp * np.array([0.0, -0.5 * acc_std])
            t = np.arange(T, dtype=np.float64)[None, :, None]
            tr = p0[:, None, :] + v0[:, None, :] * t + 0.5 * g * t * t
            tr = np.clip(tr, lo + 0.5 * dx, hi - 0.5 * dx).astype(np.float32)
            return _pad(tr, np.zeros(n, np.int32), n_max)

        # multiplier 2: a cell of this lattice holds 1 to 4 particles, and int(3 * 1.25) = 3 slots sized on one sample would
        # not hold another sample's fourth
        ds = SyntheticDataset(name, md, isl, extra_seq_length, len(counts), make, multiplier=2.0)
    else:
        base = make_case(name, n_trajs=len(counts), extra_seq_length=extra_seq_length, input_seq_length=isl, scale=scale,
                         vel_amp=vel_amp)
        n0 = int(base.metadata["num_particles_max"])
        assert max(counts) <= n0, f"{name} (scale {scale}) has {n0} particles"
        md = copy.deepcopy(base.metadata)
        md["num_particles_max"] = n_max

        def make(i):
            pos, pt = base[i]
            keep = np.sort(np.random.default_rng(2000 + i).choice(n0, counts[i], replace=False))
            return _pad(pos[keep], pt[keep], n_max)

        ds = SyntheticDataset(name, md, isl, extra_seq_length, len(counts), make, force=base.force,
                              force_numpy=base.external_force_fn, multiplier=base.multiplier, noise_std=base.noise_std,
                              isotropic_norm=base.isotropic_norm)
    ds.n_real = counts
    return ds


def write_padded_h5(ds: SyntheticDataset, path: str, splits: Sequence[str] = ("train", "valid", "test")) -> str:
    """Write a (padded) synthetic dataset as a LagrangeBench dataset directory: ``{split}.h5`` with one group per
    trajectory (``position`` (T, n_i, dim) float32, ``particle_type`` (n_i,) int32 - the pads are stripped, so the shapes
    differ from group to group, as in the variable-N data the reference reads with ``nl_backend="matscipy"``) and
    ``metadata.json``.  Every split holds the same trajectories."""
    from . import h5
    os.makedirs(path, exist_ok=True)
    groups = {}
    for i in range(len(ds)):
        pos, pt = ds[i]
        real = pt != PAD_VALUE
        groups[f"{i:05d}"] = {"position": np.ascontiguousarray(pos[real].transpose(1, 0, 2), dtype=np.float32),
                              "particle_type": np.ascontiguousarray(pt[real], dtype=np.int32)}
    for split in splits:
        h5.write_file(os.path.join(path, split + ".h5"), groups)
    md = copy.deepcopy(ds.metadata)
    T = ds.input_seq_length + ds.extra_seq_length
    md.update({"sequence_length_train": T, "num_trajs_train": len(ds), "sequence_length_test": T, "num_trajs_test": len(ds)})
    with open(os.path.join(path, "metadata.json"), "w") as f:
        json.dump(md, f, indent=1)
    return path
