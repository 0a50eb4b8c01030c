"""Shared by tests/test_metrics.py (CPU) and tests/test_metrics_gpu.py (device): the inputs of the rollout-metric tests off
the 64-multiple, their oracle results (computed once, never modified), the checks both sides are held to, and NumPy twins of
the device tiling of k_metrics / k_ekin (lb_state.hip) and lb_sinkhorn / lb_sinkhorn_pot (lb_sinkhorn.hip).

The twins restate HOW the kernels walk their data, which the oracles do not: SK_QB = 4 outputs per wave with the clamp
q = min(q0 + k, nq - 1) and the guarded store, sources swept 64 lanes at a time with an online (max, sum) pair per lane, the
xor-merge tree of lb_lse_merge over lanes that may never have seen a source (m = -inf, s = 0), and the 256-thread strided sum
with its LDS tree.  A twin takes ``mut``: one of MUTATIONS, a subtly wrong variant of that walk.  The CPU test shows that every
mutation misses a check on at least one case of the grid - the evidence that the grid would see the same slip in the kernel.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import lb_oracle as O
from oracle import sinkhorn_oracle as SK
from oracle import sinkhorn_pot_oracle as PK

# particle counts: 3 < SK_QB (clamp, three idle-lane merges per output); 5: a second wave with one live output; 61 / 67: just
# under / over one 64-lane sweep and nq % 16 != 0; 190: np % 64 == 62, nq % 4 == 2; 257: four full sweeps plus one source, a
# second strided pass of one element in k_sk_scalar / k_pot_ctrl, N * dim = 514 / 771 in k_metrics
NS = (3, 5, 61, 67, 190, 257)
GEOMS = {"free2d": (np.array([0.8, 0.8]), False),        # the free-space branch of lb_disp1
         "per3d": (np.array([1.0, 1.0, 1.0]), True),
         "per2d_1x2": (np.array([1.0, 2.0]), True)}     # unequal sides: a swapped box[d] shows
DT, WRITE_EVERY, DX = 0.002, 5, 0.05                     # dt * write_every = 0.01, not 1
MUTATIONS = ("drop_tail_sources", "drop_tail_outputs", "idle_lane_zero", "box0_every_axis", "skip_wrap", "pred_T_frames")


def metadata(N, box, periodic):
    dim = len(box)
    return {"case": "metrics", "solver": "synthetic", "dim": dim, "dx": DX, "dt": DT, "write_every": WRITE_EVERY,
            "num_particles_max": int(N), "periodic_boundary_conditions": [bool(periodic)] * dim,
            "bounds": [[0.0, float(b)] for b in box], "default_connectivity_radius": 0.1,
            "vel_mean": [0.0] * dim, "vel_std": [0.01] * dim, "acc_mean": [0.0] * dim, "acc_std": [0.001] * dim,
            "sequence_length_test": 30, "num_trajs_test": 1}


def hip_case_of(md):
    from lagrangebench_amd.case_setup import case_builder
    b = np.asarray(md["bounds"], np.float64)
    return case_builder(b[:, 1] - b[:, 0], md, 6, cfg_neighbors={"multiplier": 1.25},
                        cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4,
                        external_force_fn=None, dtype="float64")


def displacement(box, periodic):
    return O.space_periodic(np.asarray(box, np.float64))[0] if periodic else O.space_free()[0]


def rollouts(N, geom, B, pred_T, target_T=None, sigma=0.02, seed=None):
    """(pred (B, pred_T, N, dim), target (B, target_T, N, dim)), frame pair after frame pair from one generator: target uniform in
    the box, pred = target + sigma * standard_normal (sigma a number or per axis), wrapped when periodic.  The first pair is the
    pair the iteration counts of the issue were probed on (default_rng(N + dim))."""
    box, periodic = GEOMS[geom]
    dim = len(box)
    target_T = pred_T if target_T is None else target_T
    rng = np.random.default_rng(N + dim if seed is None else seed)
    T = max(pred_T, target_T)
    pred, target = np.empty((B, T, N, dim)), np.empty((B, T, N, dim))
    for b in range(B):
        for t in range(T):
            target[b, t] = rng.random((N, dim)) * box
            p = target[b, t] + sigma * rng.standard_normal((N, dim))
            pred[b, t] = np.mod(p, box) if periodic else p
    return np.ascontiguousarray(pred[:, :pred_T]), np.ascontiguousarray(target[:, :target_T])


# ---------------------------------------------------------------------------------------------------- the cases
GRID = [f"{g}-{N}" for g in GEOMS for N in NS]
# mse / mae: the grid at B = 3, the wrap case (displacements of 0.3 box) and LDC3D at scale 0.5 read as free space (N = 1020:
# twelve strided passes); every case with pred_T = 9, target_T = 12, n_steps = 7
METRIC_CASES = GRID + ["per2d_1x2-67-wrap", "per3d-190-wrap", "ldc3d-1020"]
PRED_T, TARGET_T, N_STEPS = 9, 12, 7
EKIN_T, EKIN_STRIDES = 24, (1, 3, 10)
# sinkhorn: the grid at B = 2, T = 3, stride 2 (two frames a trajectory, four problems) and a free-space cloud with one stray
# target particle: its column of the xy cost is ~1200 eps from every source, so exp(m - 0) underflows where an idle lane
# counts as (0, 0) - the one input on which that slip is not absorbed by lb_lse_merge's rescaling
SK_CASES = GRID + ["free2d-61-stray"]
SK_B, SK_T, SK_STRIDE = 2, 3, 2
PADDED = ("waterdrop2d", (190, 61), 257)


def _parse(cid):
    g, n = cid.split("-")[:2]
    return g, int(n)


@functools.lru_cache(maxsize=None)
def metric_case(cid):
    """-> dict(md, box, periodic, pred, target) for mse / mae (B = 3)."""
    if cid == "ldc3d-1020":
        from lagrangebench_amd.data import make_case
        ds = make_case("ldc3d", n_trajs=3, extra_seq_length=TARGET_T, scale=0.5)
        md = dict(ds.metadata)
        md["periodic_boundary_conditions"] = [False] * 3
        md["dt"], md["write_every"] = DT, WRITE_EVERY
        assert md["num_particles_max"] == 1020
        isl = ds.input_seq_length
        target = np.stack([np.transpose(ds[b][0][:, isl:], (1, 0, 2)) for b in range(3)]).astype(np.float64)
        pred = target[:, :PRED_T] + 0.02 * float(md["dx"]) * np.random.default_rng(1020).standard_normal(target[:, :PRED_T].shape)
        return dict(md=md, box=ds.box, periodic=False, pred=np.ascontiguousarray(pred), target=target)
    g, N = _parse(cid)
    box, periodic = GEOMS[g]
    pred, target = rollouts(N, g, 3, PRED_T, TARGET_T, sigma=0.3 * box if cid.endswith("wrap") else 0.02)
    return dict(md=metadata(N, box, periodic), box=box, periodic=periodic, pred=pred, target=target)


@functools.lru_cache(maxsize=None)
def ekin_case(cid):
    """-> dict(md, box, periodic, roll (3, 24, N, dim)): a random walk with steps of 0.15 box an axis - a good part of the frame
    to frame displacements exceeds half the shorter side, so the wrap and the side it uses decide the value."""
    g, N = _parse(cid)
    box, periodic = GEOMS[g]
    rng = np.random.default_rng(1000 + N + len(box))
    x = rng.random((3, 1, N, len(box))) * box
    roll = x + np.cumsum(0.15 * box * rng.standard_normal((3, EKIN_T, N, len(box))), axis=1)
    return dict(md=metadata(N, box, periodic), box=box, periodic=periodic, roll=np.mod(roll, box) if periodic else roll)


@functools.lru_cache(maxsize=None)
def sk_case(cid):
    """-> dict(md, box, periodic, pred, target (2, 3, N, dim)) for both Sinkhorn backends."""
    g, N = _parse(cid)
    box, periodic = GEOMS[g]
    pred, target = rollouts(N, g, SK_B, SK_T)
    if cid.endswith("stray"):
        target[:, :, 0] += 40.0 * box
    return dict(md=metadata(N, box, periodic), box=box, periodic=periodic, pred=pred, target=target)


@functools.lru_cache(maxsize=None)
def padded_case():
    """waterdrop2d, 190 and 61 real particles padded to 257 (pads at position 0 in both clouds), B = 2: pred / target
    (2, 4, 257, 2) and the dataset."""
    from lagrangebench_amd.data import make_padded_case
    name, counts, n_max = PADDED
    ds = make_padded_case(name, counts, n_max=n_max, extra_seq_length=4)
    isl = ds.input_seq_length
    target = np.stack([np.transpose(ds[b][0][:, isl:], (1, 0, 2)) for b in range(2)]).astype(np.float64)
    pred = target + 0.1 * float(ds.metadata["dx"]) * np.random.default_rng(257).standard_normal(target.shape)
    for b, n in enumerate(counts):
        pred[b, :, n:] = 0.0
        assert not target[b, :, n:].any()
    md = dict(ds.metadata)
    md["dt"], md["write_every"] = DT, WRITE_EVERY
    return dict(ds=ds, md=md, box=ds.box, periodic=False, pred=pred, target=target)


def sk_frames(c):
    """The (b, k, pred frame, target frame) problems of a Sinkhorn case, in the order of the output slots."""
    T = min(c["pred"].shape[1], c["target"].shape[1], SK_T)
    return [(b, k, c["pred"][b, t], c["target"][b, t]) for b in range(c["pred"].shape[0])
            for k, t in enumerate(range(0, T, SK_STRIDE))]


def _case_of(cid):
    return padded_case() if cid == "padded" else sk_case(cid)


@functools.lru_cache(maxsize=None)
def sk_oracle(cid):
    """[(divergence, info)] per problem of the case (info["traces"]: the error at every check)."""
    c = _case_of(cid)
    disp = displacement(c["box"], c["periodic"])
    return [SK.sinkhorn_divergence(disp, x, y, return_info=True) for _, _, x, y in sk_frames(c)]


@functools.lru_cache(maxsize=None)
def pot_oracle(cid):
    c = _case_of(cid)
    disp = displacement(c["box"], c["periodic"])
    return [PK.sinkhorn_divergence_pot(disp, x, y, return_info=True) for _, _, x, y in sk_frames(c)]


def mse_mae_oracle(c, n_steps=None):
    """per trajectory: {"mse": (B, n_steps), "mae": (B, n_steps)}"""
    n = min(c["pred"].shape[1], c["target"].shape[1]) if n_steps is None else n_steps
    disp = displacement(c["box"], c["periodic"])
    r = [O.metrics_mse_mae(disp, p[:n], t[:n], active=("mse", "mae")) for p, t in zip(c["pred"], c["target"])]
    return {k: np.stack([x[k] for x in r]) for k in ("mse", "mae")}


def ekin_oracle(c, roll, stride):
    disp = displacement(c["box"], c["periodic"])
    return np.stack([O.e_kin(disp, r, stride, DT * WRITE_EVERY, float(c["md"]["dx"]), len(c["box"])) for r in roll])


# ---------------------------------------------------------------------------------------------------- the checks
def metric_miss(got, ref):
    """mse / mae / e_kin: rtol 1e-12 and nothing absolute - the fp64 bar of tests/test_gpu_parity.py."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    with np.errstate(all="ignore"):
        rel = np.abs(got - ref) / np.abs(ref)
    if not np.all(rel <= 1e-12):
        return f"relative error {np.nanmax(rel):.3e}" if np.isfinite(got).all() else "non-finite"
    return None


def sk_miss(out, iters, d, info):
    """What test_sinkhorn_engine_matches_oracle asserts: the iteration triple equal, |out - d| <= 1e-9 reg_xy + 1e-6 |d|."""
    if tuple(int(i) for i in iters) != tuple(info["iters"]):
        return f"iterations {tuple(int(i) for i in iters)} != {tuple(info['iters'])}"
    if not abs(out - d) <= 1e-9 * info["reg"][0] + 1e-6 * abs(d):
        return f"value {out!r} != {d!r}"
    return None


def pot_miss(out, info6, d, oi):
    """What test_sinkhorn_pot_engine_matches_oracle asserts: iterations and exits equal, the value within 3e-7 of the xy value,
    float32-representable and non-negative."""
    got = tuple(int(i) for i in info6)
    if got != tuple(oi["iters"]) + tuple(oi["how"]):
        return f"iterations / exits {got} != {tuple(oi['iters']) + tuple(oi['how'])}"
    if not abs(out - float(d)) <= 3e-7 * float(oi["values"][0]):
        return f"value {out!r} != {float(d)!r}"
    if not (out >= 0 and float(np.float32(out)) == out):
        return f"value {out!r} not a non-negative float32"
    return None


def trace_margin(info, threshold=1e-4):
    """Smallest relative distance of any traced error of a problem to the threshold."""
    e = np.array([x for tr in info["traces"] for x in tr])
    return float(np.min(np.abs(e - threshold) / threshold))


# ---------------------------------------------------------------------------------------------------- twins: shared walks
def _disp1(a, b, L, periodic):
    """lb_disp1 (lb_device.h) in fp64: fmod is exact, so np.fmod gives lb_mod's value on each of its three ranges."""
    d = a - b
    if not periodic:
        return d
    half = 0.5 * L
    r = np.fmod(d + half, L)
    r = np.where((r != 0.0) & (r < 0.0), r + L, r)
    return r - half


def _sum256(*arrays):
    """One 256-thread workgroup: thread i adds elements i, i + 256, ... of each array in turn, then the LDS tree."""
    acc = np.zeros(256)
    for x in arrays:
        x = np.asarray(x, np.float64)
        pad = np.zeros(-(-max(len(x), 1) // 256) * 256)
        pad[:len(x)] = x                      # the ragged last pass: threads past n add nothing (+0.0 is exact)
        for row in pad.reshape(-1, 256):
            acc = acc + row
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        acc[:o] = acc[:o] + acc[o:2 * o]
    return float(acc[0])


def _frame_elems(flat, b, T, t, N, dim):
    """the N * dim elements k -> flat[((b * T + t) * N + k / dim) * dim + k % dim]"""
    k = np.arange(N * dim)
    return flat[((b * T + t) * N + k // dim) * dim + k % dim], k % dim


def metrics_twin(pred, target, n_steps, box, periodic, mut=None):
    """k_metrics: one workgroup per (trajectory, step) -> {"mse", "mae"} (B, n_steps)."""
    B, pred_T, N, dim = pred.shape
    target_T = target.shape[1]
    pf, tf = pred.reshape(-1), target.reshape(-1)
    L = np.asarray(box, np.float64)
    mse, mae = np.empty((B, n_steps)), np.empty((B, n_steps))
    for b in range(B):
        for t in range(n_steps):
            p, d = _frame_elems(pf, b, pred_T, t, N, dim)
            q, _ = _frame_elems(tf, b, pred_T if mut == "pred_T_frames" else target_T, t, N, dim)
            dd = _disp1(p, q, L[0] if mut == "box0_every_axis" else L[d], periodic and mut != "skip_wrap")
            mse[b, t] = _sum256(dd * dd) / float(N * dim)
            mae[b, t] = _sum256(np.abs(dd)) / float(N * dim)
    return {"mse": mse, "mae": mae}


def ekin_twin(roll, stride, dt, dx, box, periodic, mut=None):
    """k_ekin: one workgroup per (trajectory, strided frame) -> (B, ceil((T - 1) / stride))."""
    B, T, N, dim = roll.shape
    n_out = (T - 1 + stride - 1) // stride
    rf = roll.reshape(-1)
    L = np.asarray(box, np.float64)
    inv_dt, vol = 1.0 / dt, 1.0
    for _ in range(dim):
        vol *= dx
    out = np.empty((B, n_out))
    for b in range(B):
        for k in range(n_out):
            p1, d = _frame_elems(rf, b, T, 1 + k * stride, N, dim)
            p0, _ = _frame_elems(rf, b, T, k * stride, N, dim)
            v = _disp1(p1, p0, L[0] if mut == "box0_every_axis" else L[d], periodic and mut != "skip_wrap") * inv_dt
            out[b, k] = _sum256(v * v) * vol
    return out


def cost_matrix(A, Bq, box, periodic, mut=None):
    """lb_sk_cost for every pair: C[p, q] = float32(sum_d lb_disp1(A[p, d], Bq[q, d])^2), axis after axis, held in fp64."""
    s = np.zeros((len(A), len(Bq)))
    for d in range(A.shape[1]):
        r = _disp1(A[:, None, d], Bq[None, :, d], box[0] if mut == "box0_every_axis" else box[d],
                   periodic and mut != "skip_wrap")
        s = s + r * r
    return s.astype(np.float32).astype(np.float64)


_LANES = np.arange(64)


def _tile(n_src, nq, mut):
    """The walk of k_sk_sweep / k_pot_sweep: (clamped output index of every (wave, k) slot, how many of them are stored,
    source index per (pass, lane), which of those lanes hold a source)."""
    slots = np.arange(-(-nq // 4) * 4)                         # waves with q0 >= nq leave early: no slot
    qidx = np.minimum(slots, nq - 1)
    n_store = nq - nq % 4 if mut == "drop_tail_outputs" else nq
    n_eff = n_src - n_src % 64 if mut == "drop_tail_sources" else n_src
    p = _LANES[None, :] + 64 * np.arange(-(-n_eff // 64))[:, None]
    return qidx, n_store, np.minimum(p, n_src - 1), p < n_eff


def _xor_sum(s):
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[_LANES ^ off]
    return s


def sk_sweep(mode, Cs, h, u, old, eps, logm, w, mut=None):
    """k_sk_sweep<MODE> on the cost Cs[source p, output q] -> out (nq,); an output that is not stored stays 0."""
    n_src, nq = Cs.shape
    qidx, n_store, P, live = _tile(n_src, nq, mut)
    Cq = Cs[:, qidx]
    with np.errstate(all="ignore"):                            # a mutant may hand over eps = 0: inf, as on the device
        inv = np.float64(1.0) / np.float64(1.0 if mode == 2 else eps)
    m, s =np.full((64, len(qidx)), -np.inf), np.zeros((64, len(qidx)))
    with np.errstate(all="ignore"):
        for p, lv in zip(P, live):
            c, lv = Cq[p], lv[:, None]
            if mode == 2:
                s = np.where(lv, s + c, s)
            elif mode == 1:
                s = np.where(lv, s + np.exp((h[p][:, None] + u[qidx][None, :] - c) * inv), s)
            else:
                z = (h[p][:, None] - c) * inv
                up = z > m
                s = np.where(lv, np.where(up, s * np.exp(m - z) + 1.0, s + np.exp(z - m)), s)
                m = np.where(lv & up, z, m)
        if mode != 0:
            s = _xor_sum(s)
        else:
            if mut == "idle_lane_zero":
                m[~live.any(axis=0) if len(live) else np.ones(64, bool)] = 0.0
            for off in (32, 16, 8, 4, 2, 1):                   # lb_lse_merge with the lane `off` away, both ways at once
                m2, s2 = m[_LANES ^ off], s[_LANES ^ off]
                c1 = m2 > m
                c2 = ~c1 & (s2 != 0.0)
                s = np.where(c1, s * np.exp(m - m2) + s2, np.where(c2, s + s2 * np.exp(m2 - m), s))
                m = np.where(c1, m2, m)
        out = np.zeros(nq)
        if mode == 0:
            nv = eps * logm - eps * (m[0] + np.log(s[0]))
            out[:n_store] = ((1.0 - w) * old[qidx] + w * nv)[:n_store]
        else:
            out[:n_store] = s[0, :n_store]
    return out


def _sk_err(marg, target, acc, scal):
    """k_sk_scalar op 1: scal[1] (+)= sum |v - target|, scal[2] = sum v"""
    scal[1] = (scal[1] if acc else 0.0) + _sum256(np.abs(marg - target))
    scal[2] = _sum256(marg)


def sk_solve_twin(C, eps, parallel, w, threshold, mut=None, max_it=2000):
    """sk_solve: one entropic problem on C[i, j] (n x m) -> (reg_ot_cost, iterations).  max_it is 2000 on the device; the
    mutation table lowers it to just past the oracle's count - a mutant still running there has missed the check already."""
    n, m = C.shape
    Ci, Cj = C, C.T                                             # over_i: sources i, outputs j; over_j (swap): the transpose
    f, g = np.zeros(n), np.zeros(m)
    la, lb, a, b = math.log(1.0 / n), math.log(1.0 / m), 1.0 / n, 1.0 / m
    scal = [eps, 0.0, 0.0, 0.0]
    it = 0
    while it < max_it:
        g2 = sk_sweep(0, Ci, f, None, g, eps, lb, w, mut)
        f2 = sk_sweep(0, Cj, g if parallel else g2, None, f, eps, la, w, mut)
        f, g = f2, g2
        it += 1
        if it % 10 == 0:
            _sk_err(sk_sweep(1, Ci, f, g, None, eps, 0.0, 0.0, mut), b, 0, scal)
            if parallel:
                _sk_err(sk_sweep(1, Cj, g, f, None, eps, 0.0, 0.0, mut), a, 1, scal)
            if not scal[1] >= threshold:
                break
    _sk_err(sk_sweep(1, Ci, f, g, None, eps, 0.0, 0.0, mut), b, 0, scal)
    with np.errstate(all="ignore"):                            # k_sk_scalar op 2
        reg = _sum256((f - eps * math.log(a)) * a, (g - eps * math.log(b)) * b) + eps * (1.0 - scal[2])
    return reg, it


def sinkhorn_twin(x, y, box, periodic, threshold=1e-4, mut=None, max_it=(2000, 2000, 2000)):
    """lbk_sinkhorn for one frame pair -> (divergence, (iterations xy, xx, yy))."""
    N = len(x)
    Cxy = cost_matrix(x, y, box, periodic, mut)
    eps = 0.05 * (_sum256(sk_sweep(2, Cxy, None, None, None, 1.0, 0.0, 0.0, mut)) / (float(N) * float(N)))
    rxy, ixy = sk_solve_twin(Cxy, eps, False, 1.0, threshold, mut, max_it[0])
    rxx, ixx = sk_solve_twin(cost_matrix(x, x, box, periodic, mut), eps, True, 0.5, threshold, mut, max_it[1])
    ryy, iyy = sk_solve_twin(cost_matrix(y, y, box, periodic, mut), eps, True, 0.5, threshold, mut, max_it[2])
    return rxy - 0.5 * (rxx + ryy), (ixy, ixx, iyy)


def pot_sweep(mode, Ks, Cs, st, num, mut=None):
    """k_pot_sweep<MODE> on K = exp(-C / reg) laid out [source p, output q]; st: u2, v2 (2, ld), marg, ctrl."""
    ctrl = st["ctrl"]
    if mode != 3 and ctrl["stopped"]:
        return
    cur = ctrl["cur"]
    n_src, nq = Ks.shape
    qidx, n_store, P, live = _tile(n_src, nq, mut)
    src2, dst2, scale2 = (st["v2"], st["u2"], None) if mode == 1 else (st["u2"], st["v2"], st["v2"])
    h = src2[cur ^ 1 if mode == 1 else cur]
    with np.errstate(all="ignore"):
        hK = h[:n_src, None] * Ks[:, qidx]                      # t = h[p] * exp(-c / reg)
        if mode == 3:
            hK = hK * Cs[:, qidx]
    s = np.zeros((64, len(qidx)))
    for p, lv in zip(P, live):
        s = np.where(lv[:, None], s + hK[p], s)
    s = _xor_sum(s)[0, :n_store]
    with np.errstate(all="ignore"):
        if mode == 0:
            v = num / s
            dst2[cur ^ 1, :n_store] = v
            if (s == 0.0).any() or not np.isfinite(v).all():
                ctrl["bad"] = 1
        elif mode == 1:
            u = 1.0 / (num * s)
            dst2[cur ^ 1, :n_store] = u
            if not np.isfinite(u).all():
                ctrl["bad"] = 1
        else:
            st["marg"][:n_store] = scale2[cur, :n_store] * s


def pot_solve_twin(C, reg=0.1, max_it=500, thr=1e-5, mut=None):
    """pot_solve on C[i, j] -> (float32 value, iterations, exit: 0 numItermax / 1 converged / 2 numerical stop)."""
    n, m = C.shape
    ld = max(n, m)
    st = dict(u2=np.zeros((2, ld)), v2=np.zeros((2, ld)), marg=np.zeros(ld),
              ctrl=dict(cur=0, stopped=0, bad=0, iters=0, err=0.0, loss=0.0))
    st["u2"][0, :n], st["v2"][0, :m] = 1.0 / n, 1.0 / m
    ctrl = st["ctrl"]
    a, b, inv_reg = 1.0 / n, 1.0 / m, 1.0 / reg
    Ki = np.exp(-C * inv_reg)
    Kj, Cj = Ki.T, C.T
    for ii in range(max_it):
        pot_sweep(0, Ki, C, st, b, mut)
        pot_sweep(1, Kj, Cj, st, 1.0 / a, mut)
        if not ctrl["stopped"]:                                 # k_pot_ctrl op 0
            if ctrl["bad"]:
                ctrl["stopped"] = 2
            else:
                ctrl["cur"] ^= 1
            ctrl["iters"] += 1
        if ii % 10 == 0:
            pot_sweep(2, Ki, C, st, 0.0, mut)
            if not ctrl["stopped"]:                             # k_pot_ctrl op 1
                ctrl["err"] = math.sqrt(_sum256((st["marg"][:m] - b) ** 2))
                if ctrl["err"] < thr:
                    ctrl["stopped"] = 1
            if ctrl["stopped"]:
                break
    pot_sweep(3, Ki, C, st, 0.0, mut)
    return np.float32(_sum256(st["marg"][:m])), ctrl["iters"], ctrl["stopped"]


def sinkhorn_pot_twin(x, y, box, periodic, mut=None):
    """lbk_sinkhorn_pot for one frame pair -> (value, (iterations x 3, exits x 3))."""
    r = [pot_solve_twin(cost_matrix(p, q, box, periodic, mut), mut=mut) for p, q in ((x, y), (x, x), (y, y))]
    d = np.float32(r[0][0] - np.float32(0.5) * np.float32(r[1][0] + r[2][0]))
    out = float(d) if d > 0 else (0.0 if d == d else float(d))
    return out, tuple(x[1] for x in r) + tuple(x[2] for x in r)
