"""RolloutEngine: thin Python handle over liblbhip.so (include/lbhip.h).

PyTorch is only plumbing here: tensors own the device memory that is handed to the C ABI as
raw pointers, and ``torch.cuda.current_stream()`` supplies the hipStream_t.  All arithmetic of
the hot path happens inside the HIP library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import CaseDesc, LbHipError, check, ptr


def _d3(v, fill=0.0):
    a = [fill, fill, fill]
    for i, x in enumerate(list(v)[:3]):
        a[i] = float(x)
    return _lib.D3(*a)


def _dev(t: torch.Tensor, dtype, device) -> torch.Tensor:
    return t.to(device=device, dtype=dtype).contiguous()


def _n_strided(n: int, stride: int) -> int:
    """len(range(0, n, stride)); 0 for a stride or length the library refuses, so that the refusal is the library's."""
    return (n + stride - 1) // stride if stride >= 1 and n >= 1 else 0


def _graph_ops():
    """The lb_graph_* entries (include/lbhip.h) as a table for RolloutEngine._graph_call - symbol: (library entry, inputs,
    outputs, sizes) in the entry's argument order.  An input is (shape, dtype): a shape entry is 1, "nodes" (B N), "slots" (B
    E_cap), a size the caller fixes, or the name of a free size >= 1 that the first input which has it binds; dtype None marks
    a data tensor - float32 or bfloat16, one dtype for the whole call, whose code the entry then takes last.  `sizes` names
    the free sizes the entry takes, in its order; a name the caller fixes may also stand for a scalar argument that is no size
    (aggregate's ops word and eps).  A trailing True says that an input may be None (a null pointer).  An output is (shape,
    dtype, like): like is the index, among the inputs followed by the earlier outputs, of a tensor of its shape and dtype, or
    -1."""
    nc, sc, sh, shd, nh, nhd, nkc, sk = ("nodes", "C"), ("slots", "C"), ("slots", "H"), ("slots", "H", "D"), ("nodes", "H"), \
        ("nodes", "H", "D"), ("nodes", "K", "C"), ("slots", "K")
    f32, i32 = torch.float32, torch.int32
    nac, npc = ("nodes", "A", "C"), ("nodes", "planes", "C")   # aggregate: A planes of out; the 2 planes of win and of stats
    ops = {
        "lb_graph_gather": ("lb_graph_gather_t", ((nc, None),), ((sc, None),), ("C",)),
        "lb_graph_segment_sum": ("lb_graph_segment_sum_t", ((sc, None),), ((nc, None),), ("C",)),
        "lb_graph_degree": ("lb_graph_degree", (), ((("nodes",), i32),), ()),
        "lb_graph_segment_max": ("lb_graph_segment_max_t", ((sc, None),), ((nc, None), (nc, i32)), ("C",)),
        "lb_graph_segment_min": ("lb_graph_segment_min_t", ((sc, None),), ((nc, None), (nc, i32)), ("C",)),
        "lb_graph_segment_max_backward": ("lb_graph_segment_max_backward_t", ((nc, None), (nc, i32)), ((sc, None),), ("C",)),
        "lb_graph_segment_softmax": ("lb_graph_segment_softmax_t", ((sc, None),), ((sc, None),), ("C",)),
        "lb_graph_segment_softmax_backward": ("lb_graph_segment_softmax_backward_t", ((sc, None), (sc, None)), ((sc, None),),
                                              ("C",)),
        "lb_graph_attend": ("lb_graph_attend_t", ((sh, None), (shd, None)), ((nhd, None), (nh, f32), (nh, f32)), ("H", "D")),
        "lb_graph_attend_backward": ("lb_graph_attend_backward_t", ((sh, None), (shd, None), (nh, f32), (nh, f32), (nhd, None)),
                                     ((sh, None), (shd, None)), ("H", "D")),
        "lb_graph_conv": ("lb_graph_conv", ((nkc, None), (sc, None)), ((nkc, None),), ("K", "C")),
        "lb_graph_pair_mul": ("lb_graph_pair_mul", ((nkc, None), (nkc, None)), ((sc, None),), ("K", "C")),
        "lb_graph_pair_add": ("lb_graph_pair_add", ((nc, None), (nc, None)), ((sc, None),), ("C",)),
        "lb_graph_reverse": ("lb_graph_reverse", (), ((("slots",), i32),), ()),
        "lb_graph_edge_pair": ("lb_graph_edge_pair_t", ((sc, None),), ((sc, None),), ("C",)),   # (`role` carries the mode)
        "lb_graph_conv_vec": ("lb_graph_conv_vec", ((nc, None), (sc, None), (sk, None)), ((nkc, None),), ("K", "C")),
        "lb_graph_conv_dot": ("lb_graph_conv_dot", ((nkc, None), (sc, None), (sk, None)), ((nc, None),), ("K", "C")),
        "lb_graph_conv_vec_edge_grad": ("lb_graph_conv_vec_edge_grad", ((nc, None), (nkc, None), (sc, None), (sk, None)),
                                        ((sc, None), (sk, None)), ("K", "C")),
        "lb_graph_filter_conv": ("lb_graph_filter_conv", ((nkc, None), (("slots", "R"), None), (("R", "C"), None)), ((nkc, None),),
                                 ("K", "R", "C")),
        "lb_graph_filter_conv_grad": ("lb_graph_filter_conv_grad",
                                      ((nkc, None), (nkc, None), (("slots", "R"), None), (("R", "C"), None)),
                                      ((("slots", "R"), None), (("R", "C"), None), (("partials",), f32)),
                                      ("partials", "K", "R", "C")),
        "lb_graph_aggregate": ("lb_graph_aggregate", ((sc, None),), ((nac, None), (npc, i32), (npc, f32)), ("C", "ops", "eps")),
        "lb_graph_aggregate_backward": ("lb_graph_aggregate_backward", ((nac, None), (sc, None), (npc, i32), (npc, f32)),
                                        ((sc, None),), ("C", "ops"), True),
        "lb_graph_features_backward": ("lb_graph_features_backward",
                                       ((("nodes", "isl", "dim"), f32), (("nodes", "vel"), f32), (("nodes", "mag"), f32),
                                        (("nodes", "bound"), f32), (("slots", "dim"), f32), (("slots", 1), f32)),
                                       ((("B", "N", "isl", "dim"), torch.float64),), (), True),
    }
    table = {}
    for symbol, (entry, ins, outs, sizes, *optional) in ops.items():
        known, liked = list(ins), []
        for spec in outs:
            liked.append(spec + (known.index(spec) if spec in known else -1,))
            known.append(spec)
        table[symbol] = (entry, ins, tuple(liked), sizes, bool(optional))
    return table


_GRAPH_OPS = _graph_ops()


class ForceSpec:
    """How external_force_fn(position) (features.py:105-107) is evaluated on the device.

    * ``ForceSpec.piecewise(axis, split, f_lo, f_hi)``: f = pos[axis] > split ? f_hi : f_lo -
      covers the RPF body force (``where(r[1] > 1.0, -1, 1) * g``) and constant gravity (DAM).
    * ``ForceSpec.callable(fn)``: arbitrary ``fn(pos (n,dim) tensor) -> (n,dim)`` evaluated with
      torch on the device each step and handed to the engine as a buffer.
    """

    def __init__(self, kind: int, axis=0, split=0.0, f_lo=(0, 0, 0), f_hi=(0, 0, 0), fn=None):
        self.kind, self.axis, self.split, self.f_lo, self.f_hi, self.fn = kind, axis, split, f_lo, f_hi, fn

    @staticmethod
    def piecewise(axis: int, split: float, f_lo: Sequence[float], f_hi: Sequence[float]):
        return ForceSpec(_lib.LB_FORCE_PIECEWISE, axis, split, tuple(f_lo), tuple(f_hi))

    @staticmethod
    def constant(f: Sequence[float]):
        return ForceSpec(_lib.LB_FORCE_PIECEWISE, 0, 0.0, tuple(f), tuple(f))

    @staticmethod
    def callable(fn):
        return ForceSpec(_lib.LB_FORCE_BUFFER, fn=fn)


class RolloutEngine:
    """One engine = one (case, batch size B, device)."""

    def __init__(
        self,
        *,
        dim: int,
        n_particles: int,
        batch: int,
        isl: int,
        box: Sequence[float],
        periodic: bool,
        r_cutoff: float,
        multiplier: float,
        vel_mean, vel_std, acc_mean, acc_std,
        bounds=None,
        has_bound: bool = False,
        has_vel_mag: bool = False,
        force: Optional[ForceSpec] = None,
        device: Optional[torch.device] = None,
        geometry_f32: bool = False,
    ):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise LbHipError("RolloutEngine needs a HIP device (torch.cuda.is_available() is False); "
                             "there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dim, self.N, self.B, self.isl = dim, n_particles, batch, isl
        self.force = force
        d = CaseDesc()
        d.dim, d.n_particles, d.batch, d.isl = dim, n_particles, batch, isl
        d.periodic = int(bool(periodic))
        d.geometry_f32 = int(bool(geometry_f32))
        self.geometry_f32 = bool(geometry_f32)
        d.has_bound = int(bool(has_bound))
        d.has_vel_mag = int(bool(has_vel_mag))
        d.force_kind = force.kind if force is not None else _lib.LB_FORCE_NONE
        d.force_axis = force.axis if force is not None else 0
        d.box = _d3(box, 1.0)
        d.r_cutoff = float(r_cutoff)
        d.capacity_multiplier = float(multiplier)
        d.vel_mean, d.vel_std = _d3(vel_mean), _d3(vel_std, 1.0)
        d.acc_mean, d.acc_std = _d3(acc_mean), _d3(acc_std, 1.0)
        if bounds is not None:
            b = np.asarray(bounds, dtype=np.float64)
            d.bound_lo, d.bound_hi = _d3(b[:, 0]), _d3(b[:, 1])
        if force is not None and force.kind == _lib.LB_FORCE_PIECEWISE:
            d.force_split = float(force.split)
            d.force_lo, d.force_hi = _d3(force.f_lo), _d3(force.f_hi)
        self.desc = d
        self.K = isl - 1
        self.node_in = (self.K * dim + (self.K if has_vel_mag else 0) + (2 * dim if has_bound else 0)
                        + (dim if d.force_kind != _lib.LB_FORCE_NONE else 0))
        self.has_bound, self.has_vel_mag = bool(has_bound), bool(has_vel_mag)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream(self.device)
            h = C.c_void_p()
            check(self.lib.lb_engine_create(C.byref(d), C.c_void_p(self.stream.cuda_stream), C.byref(h)),
                  "lb_engine_create")
        self._h = h
        self._keep: List[torch.Tensor] = []  # tensors the library may still read asynchronously
        self.cell_capacity = 0
        self.e_cap = 0
        self.version = 0  # bumped whenever window / list change: ties FeatureDicts to a state
        self.has_pads = False  # the current particle types hold NodeType.PAD_VALUE (set_particle_type)
        self.particle_type: Optional[torch.Tensor] = None  # the (B, N) int32 device tensor last handed to the engine

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            torch.cuda.synchronize(self.device)
            self.lib.lb_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _t(self, t: Optional[torch.Tensor], dtype) -> Optional[torch.Tensor]:
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        t = _dev(t, dtype, self.device)
        self._keep.append(t)
        if len(self._keep) > 64:
            self._keep = self._keep[-32:]
        return t

    # ------------------------------------------------------------------ state
    def set_particle_type(self, ptype) -> None:
        """(B, N) particle types.  NodeType.PAD_VALUE (-1) marks a particle that is not there (padded trajectories): the
        engine leaves it out of the neighbor search; `has_pads` tells the models (only GNS takes padded input)."""
        src = ptype if isinstance(ptype, torch.Tensor) else torch.as_tensor(np.asarray(ptype))
        self.has_pads = bool((src == -1).any())
        t = self._t(src, torch.int32).reshape(self.B, self.N)
        check(self.lib.lb_set_particle_type(self._h, ptr(t)), "lb_set_particle_type")
        self.particle_type = t

    def train_batch(self, dd, trajs: Sequence[int], t0s: Sequence[int], slots: Sequence[int], seed: int, step: int,
                    noise_std: float, unroll_steps: int = 0, want_normals: bool = False):
        """One launch of lb_train_batch (include/lbhip.h) on the DeviceDataset `dd`: sample b = frames [t0s[b], t0s[b] +
        dd.subseq_length) of trajectory trajs[b], global slot slots[b].  Returns (traj (B,N,T,dim) fp64, particle types
        (B,N) int32, {"acc", "vel", "pos"} (B,N,dim) fp64, the raw normal draws (B,N,isl-1,dim) or None), all on the
        device; the engine's state is not touched."""
        B, T = self.B, int(dd.subseq_length)
        if not (len(trajs) == len(t0s) == len(slots) == B):
            raise ValueError(f"train_batch: {len(trajs)} trajectories, {len(t0s)} offsets, {len(slots)} slots for B={B}")
        if dd.N != self.N or dd.dim != self.dim or dd.pos.device != self.device:
            raise ValueError(f"train_batch: dataset (N={dd.N}, dim={dd.dim}, {dd.pos.device}) does not match the engine "
                             f"(N={self.N}, dim={self.dim}, {self.device})")
        f64 = dict(dtype=torch.float64, device=self.device)
        traj = torch.empty((B, self.N, T, self.dim), **f64)
        ptype = torch.empty((B, self.N), dtype=torch.int32, device=self.device)
        tgt = torch.empty((3, B, self.N, self.dim), **f64)
        normals = torch.empty((B, self.N, self.isl - 1, self.dim), **f64) if want_normals and noise_std != 0 else None
        I32 = C.c_int32 * B
        check(self.lib.lb_train_batch(self._h, ptr(dd.pos), int(dd.pos_f64), ptr(dd.ptype), dd.n_traj, dd.sequence_length,
                                      I32(*[int(v) for v in trajs]), I32(*[int(v) for v in t0s]), I32(*[int(v) for v in slots]),
                                      C.c_uint64(int(seed) & (2**64 - 1)), int(step), float(noise_std), T, int(unroll_steps),
                                      ptr(traj), ptr(ptype), ptr(tgt[0]), ptr(tgt[1]), ptr(tgt[2]), ptr(normals)),
              "lb_train_batch")
        return traj, ptype, {"acc": tgt[0], "vel": tgt[1], "pos": tgt[2]}, normals

    def set_particle_type_device(self, ptype: torch.Tensor, has_pads: bool) -> None:
        """set_particle_type for (B, N) int32 types already on the device, with `has_pads` known to the caller (no
        read-back)."""
        if ptype.dtype != torch.int32 or ptype.device != self.device or tuple(ptype.shape) != (self.B, self.N):
            raise ValueError(f"set_particle_type_device: expected ({self.B}, {self.N}) int32 on {self.device}")
        self.has_pads = bool(has_pads)
        self._t(ptype, torch.int32)
        check(self.lib.lb_set_particle_type(self._h, ptr(ptype)), "lb_set_particle_type")
        self.particle_type = ptype

    def prepare_traj(self, pos) -> torch.Tensor:
        """(B,N,T,dim) or (N,T,dim) positions -> fp64 contiguous device tensor."""
        t = pos if isinstance(pos, torch.Tensor) else torch.as_tensor(np.asarray(pos))
        if t.dim() == 3:
            t = t[None]
        if t.shape[0] != self.B or t.shape[1] != self.N or t.shape[3] != self.dim:
            raise ValueError(f"trajectory shape {tuple(t.shape)} does not match engine "
                             f"(B={self.B}, N={self.N}, dim={self.dim})")
        return _dev(t, torch.float64, self.device)

    def load_window(self, traj: torch.Tensor, t0: int = 0, step: int = 0) -> None:
        traj = self.prepare_traj(traj)
        self._keep.append(traj)
        check(self.lib.lb_load_window(self._h, ptr(traj), traj.shape[2], t0, step), "lb_load_window")
        self.version += 1
        self._refresh_force()

    def read_window(self) -> torch.Tensor:
        out = torch.empty((self.B, self.N, self.isl, self.dim), dtype=torch.float64, device=self.device)
        check(self.lib.lb_read_window(self._h, ptr(out)), "lb_read_window")
        return out

    def _refresh_force(self) -> None:
        if self.force is not None and self.force.kind == _lib.LB_FORCE_BUFFER:
            newest = self.read_window()[:, :, -1].reshape(self.B * self.N, self.dim)
            if self.geometry_f32:  # dtype=float32: the callable sees float32 positions and its result is a float32 array
                f = self._t(self.force.fn(newest.to(torch.float32)), torch.float32)
            else:
                f = self.force.fn(newest)
            f = self._t(f, torch.float64).reshape(self.B, self.N, self.dim)
            check(self.lib.lb_set_force(self._h, ptr(f)), "lb_set_force")

    # ------------------------------------------------------------------ neighbor list
    def nl_allocate(self) -> Tuple[int, int, List[int]]:
        cc, ec = C.c_int32(), C.c_int32()
        occ = (C.c_int32 * self.B)()
        check(self.lib.lb_nl_allocate(self._h, C.byref(cc), C.byref(ec), occ), "lb_nl_allocate")
        self.cell_capacity, self.e_cap = cc.value, ec.value
        self.version += 1
        return cc.value, ec.value, list(occ)

    def nl_set_capacity(self, cell_capacity: int, e_cap: int) -> None:
        check(self.lib.lb_nl_set_capacity(self._h, int(cell_capacity), int(e_cap)), "lb_nl_set_capacity")
        self.cell_capacity, self.e_cap = int(cell_capacity), int(e_cap)

    def nl_update(self) -> None:
        check(self.lib.lb_nl_update(self._h), "lb_nl_update")
        self.version += 1

    def nl_flags(self) -> torch.Tensor:
        out = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        check(self.lib.lb_nl_read_flags(self._h, ptr(out)), "lb_nl_read_flags")
        return out

    def nl_idx(self) -> Tuple[torch.Tensor, torch.Tensor]:
        idx = torch.empty((self.B, 2, self.e_cap), dtype=torch.int32, device=self.device)
        ne = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        check(self.lib.lb_nl_read_idx(self._h, ptr(idx), ptr(ne)), "lb_nl_read_idx")
        return idx, ne

    def nl_route(self) -> dict:
        """What the most recent neighbor-list build launched (include/lbhip.h: lb_nl_route), e.g. {"build": "multi", "cells":
        "strided", "search": "k_nl", "cand": 256, "mode": "rows", "finish": "compact_scan", ...}; numbers come back as int."""
        buf = C.create_string_buffer(512)
        check(self.lib.lb_nl_route(self._h, buf, 512), "lb_nl_route")
        kv = dict(p.split("=", 1) for p in buf.value.decode().split(";") if "=" in p)
        return {k: int(v) if v.lstrip("-").isdigit() else v for k, v in kv.items()}

    def stats(self) -> Dict[str, int]:
        n, ec, cc = C.c_int64(), C.c_int32(), C.c_int32()
        check(self.lib.lb_stats(self._h, C.byref(n), C.byref(ec), C.byref(cc)), "lb_stats")
        return {"n_edges_total": n.value, "e_cap": ec.value, "cell_capacity": cc.value}

    def edge_accounting(self, reset: bool = False) -> Dict[str, float]:
        """Edge counts of the neighbor-list builds since the last reset (include/lbhip.h: lb_edge_accounting):
        mean / first / last real E over all B trajectories, and the number of builds."""
        s, n, f, l = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.lb_edge_accounting(self._h, C.byref(s), C.byref(n), C.byref(f), C.byref(l), int(bool(reset))),
              "lb_edge_accounting")
        return {"sum": s.value, "builds": n.value, "first": f.value, "last": l.value,
                "mean": s.value / n.value if n.value else float(l.value)}

    # ------------------------------------------------------------------ features

    def kernel_names(self) -> dict:
        """{"edge": ..., "node": ...}: the network kernels a GNS forward runs on at the current size."""
        buf = C.create_string_buffer(256)
        check(self.lib.lb_kernel_names(self._h, buf, 256), "lb_kernel_names")
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if "=" in kv)

    def node_features(self) -> Dict[str, torch.Tensor]:
        f64 = dict(dtype=torch.float64, device=self.device)
        out = {"vel_hist": torch.empty((self.B, self.N, self.K * self.dim), **f64)}
        vm = bd = fo = None
        if self.has_vel_mag:
            vm = out["vel_mag"] = torch.empty((self.B, self.N, self.K), **f64)
        if self.has_bound:
            bd = out["bound"] = torch.empty((self.B, self.N, 2 * self.dim), **f64)
        if self.desc.force_kind != _lib.LB_FORCE_NONE:
            fo = out["force"] = torch.empty((self.B, self.N, self.dim), **f64)
        check(self.lib.lb_node_features(self._h, ptr(out["vel_hist"]), ptr(vm), ptr(bd), ptr(fo)),
              "lb_node_features")
        return out

    def edge_features(self) -> Dict[str, torch.Tensor]:
        f64 = dict(dtype=torch.float64, device=self.device)
        rd = torch.empty((self.B, self.e_cap, self.dim), **f64)
        rr = torch.empty((self.B, self.e_cap, 1), **f64)
        check(self.lib.lb_edge_features(self._h, ptr(rd), ptr(rr)), "lb_edge_features")
        return {"rel_disp": rd, "rel_dist": rr}

    # ------------------------------------------------------------------ model
    def _new_handle(self, cls, symbol: str, desc, blob: np.ndarray, *extra):
        """A new `cls` handle from the C entry point `symbol`(engine, desc, blob, n_floats, [extra ...,] &handle): one
        model (models/*.py `_create`) or its training state (`_train_create`) on this engine."""
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        h = C.c_void_p()
        check(getattr(self.lib, symbol)(self._h, C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.c_int64(blob.size), *extra, C.byref(h)), symbol)
        return cls(self, h, desc, blob.size)

    def _forward(self, symbol: str, model, out: Optional[torch.Tensor], dtype) -> torch.Tensor:
        if out is None:
            out = torch.empty((self.B, self.N, self.dim), dtype=dtype, device=self.device)
        check(getattr(self.lib, symbol)(self._h, model._h, ptr(out)), symbol)
        return out

    def gns_forward(self, gns: "GnsHandle", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._forward("lb_gns_forward", gns, out, torch.float32)

    def segnn_forward(self, segnn: "SegnnHandle", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._forward("lb_segnn_forward", segnn, out, torch.float32)

    def egnn_forward(self, egnn: "EgnnHandle", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """EGNN positions (B, N, dim) fp64 holding the fp32 values of the network."""
        return self._forward("lb_egnn_forward", egnn, out, torch.float64)

    def painn_forward(self, painn: "PainnHandle", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """PaiNN normalised accelerations (B, N, dim) fp32."""
        return self._forward("lb_painn_forward", painn, out, torch.float32)

    def linear_forward(self, linear: "LinearHandle", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Linear normalised accelerations (B, N, dim) fp32."""
        return self._forward("lb_linear_forward", linear, out, torch.float32)

    def math_mode(self, set_mode: int = -1) -> Tuple[int, int]:
        """(mode, guard flags): 0 exact fp32 MFMA, 1 guarded f16x2 (default), 2 unguarded f16x2; flags: 1
        large operand, 2 tiny operand tile, 4 non-finite acceleration (include/lbhip.h: lb_math_mode)."""
        mode, flags = C.c_int32(), C.c_int32()
        check(self.lib.lb_math_mode(self._h, int(set_mode), C.byref(mode), C.byref(flags)), "lb_math_mode")
        return mode.value, flags.value

    def math_fallbacks(self) -> int:
        """Steps / stand-alone forwards the range guard has redone in exact fp32 on this engine (the engine returns
        to guarded f16x2 afterwards: include/lbhip.h: lb_math_fallbacks)."""
        return int(self.lib.lb_math_fallbacks(self._h))

    def debug_inject_guard(self, flags: int, step: int) -> None:
        """Test hook: the next rollout behaves as if the range guard had raised `flags` at rollout step `step`
        (include/lbhip.h: lb_debug_inject_guard)."""
        check(self.lib.lb_debug_inject_guard(self._h, int(flags), int(step)), "lb_debug_inject_guard")

    def set_fused_aggregation(self, on: bool) -> None:
        check(self.lib.lb_set_fused_aggregation(self._h, int(bool(on))), "lb_set_fused_aggregation")

    # ------------------------------------------------------------------ integrate / rollout
    def integrate(self, acc: Optional[torch.Tensor], target: torch.Tensor,
                  pred: Optional[torch.Tensor] = None) -> None:
        acc_t = self._t(acc, torch.float32) if acc is not None else None
        tgt = self._t(target, torch.float64)
        pred_T = pred.shape[1] if pred is not None else 0
        check(self.lib.lb_integrate(self._h, ptr(acc_t), ptr(tgt), ptr(pred), pred_T), "lb_integrate")
        self.version += 1
        self._refresh_force()

    def case_integrate(self, mode: int, pred: torch.Tensor, pos_seq: torch.Tensor) -> torch.Tensor:
        p = self._t(pred, torch.float32)
        ps = self.prepare_traj(pos_seq)
        out = torch.empty((self.B, self.N, self.dim), dtype=torch.float64, device=self.device)
        check(self.lib.lb_case_integrate(self._h, mode, ptr(p), ptr(ps), ps.shape[2], ptr(out)),
              "lb_case_integrate")
        return out

    def rollout(self, model, traj: torch.Tensor, n_steps: int) -> Tuple[torch.Tensor, int]:
        """model: a model handle; its class names the C rollout (GnsHandle: lb_rollout, SegnnHandle: lb_segnn_rollout,
        ...)."""
        traj = self.prepare_traj(traj)
        pred = torch.zeros((self.B, n_steps, self.N, self.dim), dtype=torch.float64, device=self.device)
        nre = C.c_int32(0)
        check(getattr(self.lib, model._ROLLOUT)(self._h, model._h, ptr(traj), traj.shape[2], n_steps, ptr(pred),
                                                C.byref(nre)), model._ROLLOUT)
        self.version += 1
        st = self.stats()
        self.e_cap, self.cell_capacity = st["e_cap"], st["cell_capacity"]
        return pred, nre.value

    def metrics(self, pred: torch.Tensor, target: torch.Tensor, n_steps: int,
                want=("mse",)) -> Dict[str, torch.Tensor]:
        """pred, target: (B,T,N,dim) (or (T,N,dim) when B == 1)."""
        pred = _dev(pred if pred.dim() == 4 else pred[None], torch.float64, self.device)
        target = _dev(target if target.dim() == 4 else target[None], torch.float64, self.device)
        mse = torch.empty((self.B, n_steps), dtype=torch.float64, device=self.device) if "mse" in want else None
        mae = torch.empty((self.B, n_steps), dtype=torch.float64, device=self.device) if "mae" in want else None
        check(self.lib.lb_metrics(self._h, ptr(pred), pred.shape[1], ptr(target), target.shape[1], n_steps,
                                  ptr(mse), ptr(mae)), "lb_metrics")
        out = {}
        if mse is not None:
            out["mse"] = mse
        if mae is not None:
            out["mae"] = mae
        return out

    def ekin(self, rollout: torch.Tensor, stride: int, dt: float, dx: float) -> torch.Tensor:
        """Kinetic energy of strided frames of (B,T,N,dim) (or (T,N,dim)) positions -> (B, n_out)."""
        r = _dev(rollout if rollout.dim() == 4 else rollout[None], torch.float64, self.device)
        T = r.shape[1]
        n_out = _n_strided(T - 1, stride)
        out = torch.empty((self.B, n_out), dtype=torch.float64, device=self.device)
        check(self.lib.lb_ekin(self._h, ptr(r), T, int(stride), float(dt), float(dx), ptr(out), n_out), "lb_ekin")
        return out

    def sinkhorn(self, pred: torch.Tensor, target: torch.Tensor, stride: int, threshold: float = 1e-4,
                 return_iters: bool = False):
        """Sinkhorn divergence of every stride-th frame pair of (B,T,N,dim) rollouts -> (B, n_out)."""
        p = _dev(pred if pred.dim() == 4 else pred[None], torch.float64, self.device)
        t = _dev(target if target.dim() == 4 else target[None], torch.float64, self.device)
        T = min(p.shape[1], t.shape[1])
        n_out = _n_strided(T, stride)
        out = torch.empty((self.B, n_out), dtype=torch.float64, device=self.device)
        iters = (C.c_int32 * (self.B * n_out * 3))()
        check(self.lib.lb_sinkhorn(self._h, ptr(p), p.shape[1], ptr(t), t.shape[1], int(stride), float(threshold),
                                   ptr(out), n_out, iters), "lb_sinkhorn")
        if return_iters:
            return out, np.frombuffer(iters, dtype=np.int32).reshape(self.B, n_out, 3).copy()
        return out

    def sinkhorn_pot(self, pred: torch.Tensor, target: torch.Tensor, stride: int, reg: float = 0.1,
                     num_iter_max: int = 500, stop_thr: float = 1e-5, return_info: bool = False):
        """ot_backend="pot" (metrics.py:178-196): clip(sinkhorn2_xy - 0.5 (sinkhorn2_xx + sinkhorn2_yy), 0) of every
        stride-th frame pair of (B,T,N,dim) rollouts -> (B, n_out)."""
        p = _dev(pred if pred.dim() == 4 else pred[None], torch.float64, self.device)
        t = _dev(target if target.dim() == 4 else target[None], torch.float64, self.device)
        T = min(p.shape[1], t.shape[1])
        n_out = _n_strided(T, stride)
        out = torch.empty((self.B, n_out), dtype=torch.float64, device=self.device)
        info = (C.c_int32 * (self.B * n_out * 6))()
        check(self.lib.lb_sinkhorn_pot(self._h, ptr(p), p.shape[1], ptr(t), t.shape[1], int(stride), float(reg),
                                       int(num_iter_max), float(stop_thr), ptr(out), n_out, info), "lb_sinkhorn_pot")
        if return_info:
            return out, np.frombuffer(info, dtype=np.int32).reshape(self.B, n_out, 6).copy()
        return out

    def blob_train_handle(self, blob: np.ndarray) -> "BlobTrainHandle":
        """A training handle that is only optimiser state - weights (from `blob`), gradients and the AdamW moments of
        blob.size floats - for a model the caller evaluates (include/lbhip.h: lb_blob_train_create)."""
        blob = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
        h = C.c_void_p()
        check(self.lib.lb_blob_train_create(self._h, blob.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(blob.size),
                                            C.byref(h)), "lb_blob_train_create")
        return BlobTrainHandle(self, h, None, blob.size)

    # The graph ops run on float32 or bfloat16 tensors - every data tensor of one call the same dtype (win stays int32, m and s
    # of attend float32), outputs in that dtype - through the typed entries (include/lbhip.h: lb_graph_*_t).  The bfloat16
    # contract: round_to_bf16(float32 op(upcast inputs)) bit for bit.
    _GRAPH_DTYPES = {torch.float32: 0, torch.bfloat16: 1}   # LB_DTYPE_F32, LB_DTYPE_BF16

    def _graph_call(self, symbol: str, role, tensors=(), want=None, **fixed):
        """The one way into the lb_graph_* entries (_GRAPH_OPS): check every input against its shape, dtype, device and
        contiguity, allocate the outputs, call, return the outputs.  Where the table allows it, None passes a null pointer;
        `fixed` gives the sizes of a shape that the caller sets (graph_features_backward).  `want`: one flag per output - an
        output not wanted is not allocated, the entry gets a null pointer and None is returned in its place."""
        entry, ins, outs, sizes, optional = _GRAPH_OPS[symbol]
        dims = {"nodes": self.B * self.N, "slots": self.B * self.e_cap, 1: 1}
        if fixed:
            dims.update(fixed)
        data, device, codes = None, self.device, self._GRAPH_DTYPES
        args = [self._h] if role is None else [self._h, int(role)]
        seen = []
        for t, (shape, dtype) in zip(tensors, ins):
            seen.append(t)
            if t is None and optional:
                args.append(None)
                continue
            ok = isinstance(t, torch.Tensor)
            if ok:
                got = t.shape
                ok = len(got) == len(shape)
                for d, n in zip(shape, got):
                    if dims.setdefault(d, n) != n or n < 1:   # (binds a free size at its first sight)
                        ok = False
                have = t.dtype
                if dtype is None:
                    if data is None and have in codes:
                        data, first = have, t
                    dtype = data
                ok = ok and have == dtype and t.device == device and t.is_contiguous()
            if not ok:
                text = ", ".join(str(dims[d]) if dims.get(d, 0) > 0 else f"{d} >= 1" for d in shape)
                raise ValueError(f"{symbol}: expected a contiguous ({text}) {dtype or data or 'float32 or bfloat16'} tensor on "
                                 f"{device}, got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))} on "
                                 f"{getattr(t, 'device', None)}")
            args.append(t.data_ptr())
        made = []
        # (the cheapest allocation that fits: a twin's, the data tensors', a plain one)
        for n, (shape, dtype, like) in enumerate(outs):
            if want is not None and not want[n]:
                seen.append(None)
                made.append(None)
                args.append(None)
                continue
            if like >= 0 and seen[like] is not None:
                o = torch.empty_like(seen[like])
            elif dtype is None:
                o = first.new_empty([dims[d] for d in shape])
            else:
                o = torch.empty([dims[d] for d in shape], dtype=dtype, device=device)
            seen.append(o)
            made.append(o)
            args.append(o.data_ptr())
        for s in sizes:
            args.append(dims[s])
        if data is not None:
            args.append(codes[data])
        check(getattr(self.lib, entry)(*args), symbol)
        return made[0] if len(made) == 1 else tuple(made)

    def _graph_op(self, symbol: str, role: int, src: torch.Tensor, rows_in: int, rows_out: int) -> torch.Tensor:
        """A one-tensor op on rows the caller counts: (rows_in, C) -> (rows_out, C).  Kept for one purpose: the test of the
        library's refusal on an engine without a list (e_cap == 0, so no output could be allocated otherwise) calls it.  No
        graph_* method does; with input and output both in slots (softmax) rows_out would stand for both."""
        _, ins, outs, _, _ = _GRAPH_OPS[symbol]
        return self._graph_call(symbol, role, (src,), **{ins[0][0][0]: rows_in, outs[0][0][0]: rows_out})

    def graph_gather(self, role: int, x: torch.Tensor) -> torch.Tensor:
        """x (B*N, C) float32 or bfloat16 -> (B*E_cap, C): the node row of every real edge slot of the current list in the
        padded layout of nl_idx(), +0.0 in the pad slots; a bit copy.  role: 0 receivers, 1 senders (include/lbhip.h:
        lb_graph_gather_t)."""
        return self._graph_call("lb_graph_gather", role, (x,))

    def graph_segment_sum(self, role: int, msg: torch.Tensor) -> torch.Tensor:
        """msg (B*E_cap, C) float32 or bfloat16 -> (B*N, C): per node the sum of its real edge slots in ascending slot order, one
        fp32 add after the other; no atomics.  bfloat16: the terms are widened, the fp32 sum is rounded once (include/lbhip.h:
        lb_graph_segment_sum_t)."""
        return self._graph_call("lb_graph_segment_sum", role, (msg,))

    def graph_degree(self, role: int) -> torch.Tensor:
        """-> (B*N,) int32: the real edge slots of the current list whose role index is the node (lb_graph_degree)."""
        return self._graph_call("lb_graph_degree", role)

    def graph_segment_max(self, role: int, msg: torch.Tensor, minimum: bool = False):
        """msg (B*E_cap, C) float32 or bfloat16 -> (out (B*N, C), win (B*N, C) int32): per node and column the first real slot's
        value, replaced in ascending slot order by a strictly greater (minimum: smaller) one, and the slot that won (-1 and +0.0
        for a node without edges) (include/lbhip.h: lb_graph_segment_max_t / _min_t)."""
        return self._graph_call("lb_graph_segment_min" if minimum else "lb_graph_segment_max", role, (msg,))

    def graph_segment_max_backward(self, role: int, d_out: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
        """d_out (B*N, C), win (B*N, C) int32 -> d_msg (B*E_cap, C) in d_out's dtype: d_out in the winning slots, +0.0 elsewhere."""
        return self._graph_call("lb_graph_segment_max_backward", role, (d_out, win))

    def graph_segment_softmax(self, role: int, logits: torch.Tensor) -> torch.Tensor:
        """logits (B*E_cap, C) float32 or bfloat16 -> (B*E_cap, C): per node and column the softmax over the node's real slots,
        shifted by their maximum, the denominator summed in ascending slot order; +0.0 in the pad slots
        (lb_graph_segment_softmax_t)."""
        return self._graph_call("lb_graph_segment_softmax", role, (logits,))

    def graph_segment_softmax_backward(self, role: int, y: torch.Tensor, d_y: torch.Tensor) -> torch.Tensor:
        """y, d_y (B*E_cap, C), one dtype -> d_logits (B*E_cap, C) = y (d_y - the node's ordered sum of d_y y)."""
        return self._graph_call("lb_graph_segment_softmax_backward", role, (y, d_y))

    def graph_attend(self, role: int, logits: torch.Tensor, values: torch.Tensor):
        """logits (B*E_cap, H), values (B*E_cap, H, D), both float32 or both bfloat16 -> (out (B*N, H, D) in that dtype,
        m (B*N, H), s (B*N, H) float32): the softmax of the logits over each node's slots times the values, summed per node in
        ascending slot order.  float32: the bits of graph_segment_sum(graph_segment_softmax(logits)[..., None] * values) in one
        launch.  bfloat16: that float32 result on the widened inputs, rounded once - the weights are not rounded to bfloat16
        on the way, as the composition's are.  m and s are the maximum and the denominator it used (include/lbhip.h:
        lb_graph_attend_t)."""
        return self._graph_call("lb_graph_attend", role, (logits, values))

    def graph_attend_backward(self, role: int, logits: torch.Tensor, values: torch.Tensor, m: torch.Tensor, s: torch.Tensor,
                              d_out: torch.Tensor):
        """-> (d_logits (B*E_cap, H), d_values (B*E_cap, H, D)) of graph_attend, in the dtype of logits, values and d_out
        (include/lbhip.h: lb_graph_attend_backward_t)."""
        return self._graph_call("lb_graph_attend_backward", role, (logits, values, m, s, d_out))

    def graph_conv(self, role: int, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """x (B*N, K, C), w (B*E_cap, C), both float32 or both bfloat16 -> (B*N, K, C): per node the sum over its real slots of
        `role`, in ascending slot order, of x[the slot's other node] * w[slot] - each product rounded to float32, one float32
        add after the other; no edge-shaped intermediate.  float32: the bits of graph_segment_sum(graph_gather(x) * w).
        bfloat16: the exact products summed in float32, rounded once (include/lbhip.h: lb_graph_conv)."""
        return self._graph_call("lb_graph_conv", role, (x, w))

    def graph_pair_mul(self, a_role: int, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b (B*N, K, C), one dtype -> (B*E_cap, C): per real slot the sum over k ascending of a[the slot's `a_role` node, k]
        * b[its other node, k], each product rounded to float32, the first starts the sum; +0.0 in the pad slots.  K = 1 is
        the plain product; with K > 1 it is graph_conv's gradient to w (include/lbhip.h: lb_graph_pair_mul)."""
        return self._graph_call("lb_graph_pair_mul", a_role, (a, b))

    def graph_pair_add(self, a_role: int, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b (B*N, C), one dtype -> (B*E_cap, C): a[the slot's `a_role` node] + b[its other node] in the real slots, one
        float32 add, +0.0 in the pad slots (include/lbhip.h: lb_graph_pair_add)."""
        return self._graph_call("lb_graph_pair_add", a_role, (a, b))

    def graph_reverse(self) -> torch.Tensor:
        """-> (B*E_cap,) int32: per padded slot of the current list the slot, within its trajectory, of the transposed edge
        (receiver and sender exchanged); a self-edge maps to itself; -1 where the list holds no such edge and in every pad slot.
        The engine builds the map once per list build, in one launch, and keeps it; this is a copy (include/lbhip.h:
        lb_graph_reverse)."""
        return self._graph_call("lb_graph_reverse", None)

    def graph_edge_pair(self, mode: int, msg: torch.Tensor) -> torch.Tensor:
        """msg (B*E_cap, C) float32 or bfloat16 -> (B*E_cap, C), with p the reverse map: mode 0 msg[p] (a bit copy), 1
        msg + msg[p], 2 msg - msg[p] - one float32 operation, bfloat16 rounded once; +0.0 in a slot without a partner and in
        the pad slots, which are never read (include/lbhip.h: lb_graph_edge_pair_t)."""
        return self._graph_call("lb_graph_edge_pair", mode, (msg,))

    def graph_conv_vec(self, role: int, x: torch.Tensor, w: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """x (B*N, C), w (B*E_cap, C), u (B*E_cap, K), 1 <= K <= 9, one dtype (float32 or bfloat16) -> (B*N, K, C): per node
        the sum over its real slots of `role`, in ascending slot order, of (x[the slot's other node] * w[slot]) * u[slot, k] -
        two rounded float32 products, one float32 add after the other, the first term starts the sum; nothing edge-shaped of K C
        columns exists.  float32: the bits of graph_segment_sum((graph_gather(x) * w)[:, None, :] * u[:, :, None]).  bfloat16:
        that float32 result on the widened inputs, rounded once (include/lbhip.h: lb_graph_conv_vec)."""
        return self._graph_call("lb_graph_conv_vec", role, (x, w, u))

    def graph_conv_dot(self, role: int, v: torch.Tensor, w: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """v (B*N, K, C), w (B*E_cap, C), u (B*E_cap, K), one dtype -> (B*N, C): per node the sum over its real slots of `role`,
        ascending, of w[slot] * t[slot], t = v[the slot's other node, 0] * u[slot, 0] + v[.., 1] * u[slot, 1] + ... (k
        ascending, every product rounded to float32, the first starts the sum).  The adjoint of graph_conv_vec over the other
        role (include/lbhip.h: lb_graph_conv_dot)."""
        return self._graph_call("lb_graph_conv_dot", role, (v, w, u))

    def graph_conv_vec_edge_grad(self, s_role: int, s: torch.Tensor, v: torch.Tensor, w: torch.Tensor, u: torch.Tensor,
                                 want_w: bool = True, want_u: bool = True):
        """s (B*N, C) read at the slot's `s_role` node, v (B*N, K, C) at its other node, w (B*E_cap, C), u (B*E_cap, K) -> (d_w
        (B*E_cap, C), d_u (B*E_cap, K)), the gradients of graph_conv_vec (s = x, v = the cotangent) and graph_conv_dot (s = the
        cotangent, v = v) to w and u, +0.0 in the pad slots: d_w = s * t with t as in graph_conv_dot; d_u[slot, k] = the sum over c
        of (s[c] * w[slot, c]) * v[k, c] in blocks of 16 columns - c ascending inside a block, the block sums added in ascending
        order.  One launch shares the loads; an output not wanted is neither computed nor allocated (None in its place)
        (include/lbhip.h: lb_graph_conv_vec_edge_grad)."""
        if not (want_w or want_u):
            return None, None
        return self._graph_call("lb_graph_conv_vec_edge_grad", s_role, (s, v, w, u), want=(want_w, want_u))

    def graph_filter_conv(self, role: int, x: torch.Tensor, f: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
        """x (B*N, K, C), f (B*E_cap, R), weight (R, C), 1 <= R <= 32, one dtype (float32 or bfloat16) -> (B*N, K, C): graph_conv
        with the filter wf[slot, c] = f[slot, 0] * weight[0, c] + f[slot, 1] * weight[1, c] + ... (r ascending, every product
        rounded to float32, the first starts the sum) formed in registers - wf never reaches memory.  float32: the bits of
        graph_conv(role, x, wf).  bfloat16: that float32 result on the widened inputs, rounded once (include/lbhip.h:
        lb_graph_filter_conv)."""
        return self._graph_call("lb_graph_filter_conv", role, (x, f, weight))

    def graph_filter_conv_grad(self, role: int, x: torch.Tensor, d: torch.Tensor, f: torch.Tensor, weight: torch.Tensor,
                               want_f: bool = True, want_weight: bool = True):
        """The gradients of graph_filter_conv over `role` to f and weight from x and the cotangent d (both (B*N, K, C)) -> (d_f
        (B*E_cap, R), d_weight (R, C)).  With g[slot, c] = the sum over k ascending of x[the slot's other node, k, c] * d[its
        `role` node, k, c] (never stored): d_f[slot, r] = the sum over c of weight[r, c] * g[slot, c] in blocks of 16 columns - c
        ascending inside a block, the block sums added in ascending order -, +0.0 in the pad slots; d_weight[r, c] = the sum over
        every real slot of f[slot, r] * g[slot, c]: per chunk of LB_GRAPH_FILTER_CHUNK flat padded slots a partial from +0.0 in
        ascending slot order, then the partials from +0.0 in ascending chunk order - no atomics.  An output not wanted is neither
        computed nor allocated (None in its place); the float32 partials (chunks, R, C) are the only scratch (include/lbhip.h:
        lb_graph_filter_conv_grad)."""
        if not (want_f or want_weight):
            return None, None
        n = int(self.lib.lb_graph_filter_partials(self._h, int(f.shape[-1]), int(weight.shape[-1]))) if want_weight else 1
        return self._graph_call("lb_graph_filter_conv_grad", role, (x, d, f, weight), want=(want_f, want_weight, want_weight),
                                partials=max(n, 1))[:2]

    def graph_aggregate(self, role: int, msg: torch.Tensor, ops: int, eps: float, planes: int):
        """msg (B*E_cap, C) float32 or bfloat16 -> (out (B*N, planes, C) in the dtype of msg, win (B*N, 2, C) int32 or None, stats
        (B*N, 2, C) float32 or None): the reductions the nibbles of `ops` name (1 sum, 2 mean, 3 max, 4 min, 5 std, 6 var; one per
        plane of out from the low end) over the real slots of each node, from one walk of its row and a second one for std /
        var.  win - the winning slots of max, then min - exists with max or min; stats - the float32 mean, then std - with std or
        var (include/lbhip.h: lb_graph_aggregate)."""
        codes = [(ops >> (4 * a)) & 15 for a in range(8)]
        return self._graph_call("lb_graph_aggregate", role, (msg,), want=(True, 3 in codes or 4 in codes, 5 in codes or 6 in codes),
                                A=int(planes), planes=2, ops=int(ops), eps=float(eps))

    def graph_aggregate_backward(self, role: int, d_out: torch.Tensor, msg, win, stats, ops: int) -> torch.Tensor:
        """-> d_msg (B*E_cap, C) of graph_aggregate in the dtype of d_out (B*N, A, C), +0.0 in the pad slots, from one
        edge-parallel launch; msg and stats may be None without std / var, win without max / min (include/lbhip.h:
        lb_graph_aggregate_backward)."""
        return self._graph_call("lb_graph_aggregate_backward", role, (d_out, msg, win, stats), planes=2, ops=int(ops))

    def graph_features_backward(self, d_abs_pos=None, d_vel_hist=None, d_vel_mag=None, d_bound=None, d_rel_disp=None,
                                d_rel_dist=None) -> torch.Tensor:
        """-> d loss / d window (B, N, isl, dim) float64 from the float32 cotangents of the features a TorchModel module
        receives, on the current window and list; None = zero.  Shapes: d_abs_pos (B*N, isl, dim), d_vel_hist (B*N, (isl-1)*dim),
        d_vel_mag (B*N, isl-1), d_bound (B*N, 2*dim), d_rel_disp (B*E_cap, dim), d_rel_dist (B*E_cap, 1); the pad slots of the
        last two are never read.  fp64 sums in a fixed order, no atomics (include/lbhip.h: lb_graph_features_backward)."""
        symbol = "lb_graph_features_backward"
        if d_vel_mag is not None and not self.has_vel_mag:
            raise ValueError(f"{symbol}: d_vel_mag given, but the engine has no vel_mag feature")
        if d_bound is not None and not self.has_bound:
            raise ValueError(f"{symbol}: d_bound given, but the engine has no bound feature")
        return self._graph_call(symbol, None, (d_abs_pos, d_vel_hist, d_vel_mag, d_bound, d_rel_disp, d_rel_dist), B=self.B,
                                N=self.N, isl=self.isl, dim=self.dim, vel=(self.isl - 1) * self.dim, mag=self.isl - 1,
                                bound=2 * self.dim)

    def graph_sender_sorts(self) -> int:
        """Sender-ordered views the graph ops built by the radix sort (a list with an edge in one direction only)."""
        return int(self.lib.lb_graph_sender_sorts(self._h))

    def segment_sum(self, msg: torch.Tensor) -> torch.Tensor:
        msg = _dev(msg, torch.float32, self.device)
        out = torch.empty((self.B * self.N, msg.shape[1]), dtype=torch.float32, device=self.device)
        check(self.lib.lb_segment_sum(self._h, ptr(msg), ptr(out), msg.shape[1]), "lb_segment_sum")
        return out

    # ------------------------------------------------------------------ timers
    def timers_enable(self, on: bool = True) -> None:
        check(self.lib.lb_timers_enable(self._h, int(on)))

    def timers_reset(self) -> None:
        check(self.lib.lb_timers_reset(self._h))

    def timers(self) -> Dict[str, Tuple[float, int]]:
        out = {}
        for c in range(self.lib.lb_timer_count()):
            ms, n = C.c_double(), C.c_int64()
            check(self.lib.lb_timer_get(self._h, c, C.byref(ms), C.byref(n)))
            out[self.lib.lb_timer_name(c).decode()] = (ms.value, n.value)
        return out


class _Handle:
    """An engine-side object (a model or its training state) made from a blob of n_floats weights on `engine`; the
    subclass names its destroy symbol (and a model handle its rollout symbol)."""
    _DESTROY = ""

    def __init__(self, engine: RolloutEngine, h, desc, n_floats: int):
        self.engine, self._h, self.desc, self.n_floats = engine, h, desc, int(n_floats)

    def close(self):
        if self._h:
            if self.engine._h:
                torch.cuda.synchronize(self.engine.device)
            getattr(self.engine.lib, self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GnsHandle(_Handle):
    _DESTROY, _ROLLOUT = "lb_gns_destroy", "lb_rollout"
    _tap = None

    def set_tap(self, on: bool = True) -> Optional[torch.Tensor]:
        e = self.engine
        if on:
            # the kernels work on 128-wide rows (narrower latents are zero-padded): the tap buffer is
            # 128 wide, the caller sees the first latent_size columns
            self._tap = torch.zeros((self.desc.num_mp_steps + 1, e.B * e.N, 128), dtype=torch.float32,
                                    device=e.device)
            check(e.lib.lb_gns_set_tap(self._h, ptr(self._tap)))
            return self._tap[:, :, :self.desc.latent_size]
        self._tap = None
        check(e.lib.lb_gns_set_tap(self._h, None))
        return None

    def image(self) -> np.ndarray:
        """The packed device blob of the model - every weight image, in packing order - as bytes (test support)."""
        lib = self.engine.lib
        out = np.empty(int(lib.lb_gns_image_bytes(self._h)), np.uint8)
        check(lib.lb_gns_image_read(self._h, out.ctypes.data_as(C.c_void_p), C.c_int64(out.size)), "lb_gns_image_read")
        return out


class _DeviceSpan:
    """n float32 at a device address owned by a training handle, in the form torch.as_tensor wraps without a copy
    (__cuda_array_interface__); the tensor keeps this object, and with it the handle, referenced."""

    def __init__(self, owner, addr: int, n: int):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(addr), False), "version": 2}


class GnsTrainHandle(_Handle):
    """trainer.py:35-89 on the device: value_and_grad of _mse summed over the batch + optax.adamw."""
    _DESTROY = "lb_gns_train_destroy"
    _dev_floats: Optional[int] = None

    def loss_grad(self, target: torch.Tensor, loss_weight: float = 1.0, want_pred: bool = False):
        """target (B, N, dim) normalised accelerations -> mean per-trajectory loss (float); gradients accumulate."""
        e = self.engine
        tgt = target.to(device=e.device, dtype=torch.float32).reshape(e.B * e.N, e.dim).contiguous()
        loss = C.c_double()
        pred = torch.empty((e.B, e.N, e.dim), dtype=torch.float32, device=e.device) if want_pred else None
        check(e.lib.lb_gns_train_loss_grad(self._h, ptr(tgt), C.c_float(float(loss_weight)), C.byref(loss),
                                           ptr(pred) if want_pred else None), "lb_gns_train_loss_grad")
        return (loss.value, pred) if want_pred else loss.value

    def forward(self) -> torch.Tensor:
        """The model's forward with saved activations on the engine's current window and neighbor list -> (B, N, dim)
        float32: the normalised accelerations (GNS, SEGNN) or the positions x^L (EGNN), the `pred` of loss_grad bit for
        bit.  The forward stays live - backward() may follow - until any other call on the handle but zero_grad
        (include/lbhip.h: lb_train_forward)."""
        e = self.engine
        pred = torch.empty((e.B, e.N, e.dim), dtype=torch.float32, device=e.device)
        check(e.lib.lb_train_forward(self._h, ptr(pred)), "lb_train_forward")
        return pred

    def backward(self, dpred: torch.Tensor, want_dpos: bool = False) -> Optional[torch.Tensor]:
        """The hand-written backward of the live forward from the caller's d loss / d pred (B, N, dim): the gradients
        accumulate into the gradient blob, as in loss_grad.  Rows of pad particles count as zero.  want_dpos (GNS only):
        also returns d loss / d window (B, N, isl, dim) float64 through the feature builder, with the neighbor list held
        fixed and the external force treated as constant in the positions (include/lbhip.h: lb_train_backward)."""
        e = self.engine
        if tuple(dpred.shape) not in ((e.B, e.N, e.dim), (e.B * e.N, e.dim)):
            raise ValueError(f"backward: dpred must be ({e.B}, {e.N}, {e.dim}), got {tuple(dpred.shape)}")
        d = dpred.detach().to(device=e.device, dtype=torch.float32).contiguous()
        dpos = torch.empty((e.B, e.N, e.isl, e.dim), dtype=torch.float64, device=e.device) if want_dpos else None
        check(e.lib.lb_train_backward(self._h, ptr(d), ptr(dpos) if want_dpos else None), "lb_train_backward")
        return dpos

    def exact_math(self, on: bool) -> None:
        """Exact-fp32 products from the next forward on (True), or the handle's default arithmetic (False): what
        LB_TRAIN_MATH=f32 selects at creation, per step (include/lbhip.h: lb_train_exact_math)."""
        check(self.engine.lib.lb_train_exact_math(self._h, int(bool(on))), "lb_train_exact_math")

    def zero_grad(self) -> None:
        check(self.engine.lib.lb_gns_train_zero_grad(self._h), "lb_gns_train_zero_grad")

    def adamw_step(self, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, weight_decay: float = 1e-8) -> None:
        check(self.engine.lib.lb_adamw_step(self._h, C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps),
                                            C.c_float(weight_decay)), "lb_adamw_step")

    def device_blob(self, which: str = "grads", keep_alive: bool = True) -> torch.Tensor:
        """The device memory of a blob as a 1-D float32 tensor - a view, no copy - in the DEVICE layout (latents padded
        to 128, so it can be longer than read(which); every rank of a data-parallel run has the same layout).  Valid
        until close().  keep_alive: the tensor references this handle; False is for a tensor the handle itself keeps
        (BlobTrainHandle.module), which must not hold its owner in a reference cycle."""
        idx = {"weights": 0, "grads": 1, "m": 2, "v": 3}[which]
        p, n = C.c_void_p(), C.c_int64()
        check(self.engine.lib.lb_gns_train_device_blob(self._h, idx, C.byref(p), C.byref(n)), "lb_gns_train_device_blob")
        self._dev_floats = n.value
        return torch.as_tensor(_DeviceSpan(self if keep_alive else None, p.value, n.value), device=self.engine.device)

    def device_floats(self) -> int:
        """Floats of a blob in the device layout (the length of device_blob)."""
        if self._dev_floats is None:
            self.device_blob("weights")
        return self._dev_floats

    def adamw_step_gathered(self, gathered: torch.Tensor, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
                            weight_decay: float = 1e-8, grad_scale: float = 1.0) -> None:
        """The data-parallel AdamW step: `gathered` (world, len(device_blob)) float32 on the engine's device, row r = the
        gradients of rank r.  One kernel sums the rows in rank order, keeps the sum (x grad_scale) as this handle's
        gradients and applies adamw_step's arithmetic (include/lbhip.h: lb_adamw_step_gathered)."""
        e, n = self.engine, self.device_floats()
        if gathered.dim() != 2 or gathered.shape[1] != n or not 1 <= gathered.shape[0] <= 16:
            raise ValueError(f"adamw_step_gathered: expected (1 ... 16, {n}) gradient rows, got {tuple(gathered.shape)}")
        if gathered.dtype != torch.float32 or gathered.device != e.device or not gathered.is_contiguous():
            raise ValueError(f"adamw_step_gathered: the rows must be contiguous float32 on {e.device} "
                             f"(got {gathered.dtype}, {gathered.device}, contiguous={gathered.is_contiguous()})")
        check(e.lib.lb_adamw_step_gathered(self._h, ptr(gathered), int(gathered.shape[0]), C.c_float(grad_scale), C.c_float(lr),
                                           C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(weight_decay)),
              "lb_adamw_step_gathered")

    def read(self, which: str = "weights") -> np.ndarray:
        idx = {"weights": 0, "grads": 1, "m": 2, "v": 3}[which]
        out = np.empty(self.n_floats, np.float32)
        check(self.engine.lib.lb_gns_train_read(self._h, idx, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                C.c_int64(out.size)), "lb_gns_train_read")
        return out

    def sync_model(self, handle: "GnsHandle") -> None:
        """Re-make the packed images of the inference model `handle` (same engine, same description) from this handle's
        CURRENT weights, on the device: afterwards it is the model lb_gns_create would make from read("weights"), bit for
        bit, without the weights leaving the device (include/lbhip.h: lb_gns_train_sync_model)."""
        check(self.engine.lib.lb_gns_train_sync_model(self._h, handle._h), "lb_gns_train_sync_model")

    def step_count(self) -> int:
        """AdamW steps taken on the device (optax's `count`)."""
        return int(self.engine.lib.lb_gns_train_step_count(self._h))

    def math_fallbacks(self) -> int:
        """Steps repeated because the X range guard of the f16x2 weight-gradient kernel fired: each ran again with the
        site's X scale re-centred, or scaled per chunk, in f16x2 (include/lbhip.h)."""
        return int(self.engine.lib.lb_gns_train_math_fallbacks(self._h))

    def sort_fallbacks(self) -> int:
        """Training steps repeated with the radix sort of the senders because an edge of the list had no transpose
        (include/lbhip.h: lb_gns_train_sort_fallbacks)."""
        return int(self.engine.lib.lb_gns_train_sort_fallbacks(self._h))

    def write(self, which: str, blob: np.ndarray, step: int = -1) -> None:
        idx = {"weights": 0, "grads": 1, "m": 2, "v": 3}[which]
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        check(self.engine.lib.lb_gns_train_write(self._h, idx, blob.ctypes.data_as(C.POINTER(C.c_float)),
                                                 C.c_int64(blob.size), C.c_int64(step)), "lb_gns_train_write")


class EgnnTrainHandle(GnsTrainHandle):
    """trainer.py:35-89 for EGNN: _mse over the model's three outputs pos / vel / acc (models/egnn.py:361-369)."""

    def loss_grad(self, targets: Dict[str, torch.Tensor], loss_weight: Dict[str, float], want_pred: bool = False):
        """targets: the case's {"pos", "vel", "acc"} (B, N, dim) (a missing one needs weight 0); loss_weight: {"pos", "vel",
        "acc"} -> mean per-trajectory loss (float); gradients accumulate.  want_pred: also the fp32 positions (B, N, dim)."""
        e = self.engine
        w = {k: float(loss_weight.get(k, 0.0)) for k in ("pos", "vel", "acc")}
        tg = {}
        for k in ("pos", "vel", "acc"):
            if w[k] != 0.0:
                if k not in targets or targets[k] is None:
                    raise ValueError(f"EGNN loss: loss_weight[{k!r}] = {w[k]} but there is no {k!r} target")
                tg[k] = torch.as_tensor(targets[k]).to(device=e.device, dtype=torch.float64).reshape(e.B * e.N, e.dim).contiguous()
        loss = C.c_double()
        pred = torch.empty((e.B, e.N, e.dim), dtype=torch.float32, device=e.device) if want_pred else None
        check(e.lib.lb_egnn_train_loss_grad(self._h, ptr(tg["pos"]) if "pos" in tg else None,
                                            ptr(tg["vel"]) if "vel" in tg else None, ptr(tg["acc"]) if "acc" in tg else None,
                                            C.c_float(w["pos"]), C.c_float(w["vel"]), C.c_float(w["acc"]), C.byref(loss),
                                            ptr(pred) if want_pred else None), "lb_egnn_train_loss_grad")
        return (loss.value, pred) if want_pred else loss.value

    _view: Optional["EgnnHandle"] = None

    def model_handle(self) -> "EgnnHandle":
        """The inference model of this handle: a view of its device weights, so engine.egnn_forward / rollout on it run on
        the CURRENT weights.  Borrowed - it is this handle's; closing it frees nothing, closing this handle ends it."""
        if self._view is None or not self._view._h:
            h = C.c_void_p()
            check(self.engine.lib.lb_egnn_train_model(self._h, C.byref(h)), "lb_egnn_train_model")
            self._view = _BorrowedEgnnHandle(self.engine, h, self.desc, self.n_floats)
        return self._view

    def close(self):
        if self._view is not None:
            self._view._h = None   # the view dies with the handle
        super().close()


class LinearTrainHandle(GnsTrainHandle):
    """trainer.py:35-89 for the Linear baseline (csrc/lb_train_linear.h): GnsTrainHandle's calls, one "acc" target."""

    _view: Optional["LinearHandle"] = None

    def model_handle(self) -> "LinearHandle":
        """The inference model of this handle: a view of its device weights, so engine.linear_forward / rollout on it run
        on the CURRENT weights.  Borrowed - it is this handle's; closing it frees nothing, closing this handle ends it."""
        if self._view is None or not self._view._h:
            h = C.c_void_p()
            check(self.engine.lib.lb_linear_train_model(self._h, C.byref(h)), "lb_linear_train_model")
            self._view = _BorrowedLinearHandle(self.engine, h, self.desc, self.n_floats)
        return self._view

    def close(self):
        if self._view is not None:
            self._view._h = None   # the view dies with the handle
        super().close()


class BlobTrainHandle(GnsTrainHandle):
    """Optimiser state with no model in it (include/lbhip.h: lb_blob_train_create): zero_grad, adamw_step(_gathered), read /
    write / device_blob and step_count are GnsTrainHandle's; loss_grad, forward, backward and sync_model are refused by the
    library.  models.TorchModel keeps its device module here: `module`, whose parameters and gradients alias the weight
    and gradient blobs, and `view`, the inference handle on that module.  Those aliases do not reference the handle (no
    cycle: dropping the last reference to the handle frees it at once, like the other handles); close() - also run by
    __del__ - empties the module's parameters before the blobs are freed, so a module kept beyond its handle holds no
    dangling memory."""

    module = None
    view = None

    def close(self):
        if self.module is not None:   # the parameters alias memory that is about to be freed: let go of it first
            for p in self.module.parameters():
                p.grad = None
                p.data = torch.empty(0, dtype=p.dtype, device=p.device)
        self.module = self.view = None
        super().close()


    def probe(self, op: str, **kw) -> Tuple[int, int]:
        """Test hook (include/lbhip.h: lb_train_probe): one gradient-reduction launcher of the training step on the
        caller's device tensors, accumulated into this handle's gradient blob at float offsets dst0 / dst1 / dst_b.
        Tensors are passed by pointer - keep them alive and synchronised.  Returns (guard word, site slot)."""
        from ._lib import PROBE_OPS, TrainProbeArgs
        a = TrainProbeArgs()
        a.dst0 = a.dst1 = a.dst_b = -1
        for k, v in kw.items():
            if not hasattr(a, k):
                raise TypeError(f"probe: no argument {k!r}")
            setattr(a, k, ptr(v) if isinstance(v, torch.Tensor) else v)
        torch.cuda.synchronize(self.engine.device)   # the launch runs on the engine's stream
        check(self.engine.lib.lb_train_probe(self._h, PROBE_OPS[op], C.byref(a)), "lb_train_probe")
        return int(a.guard), int(a.slot)


class PainnTrainHandle(GnsTrainHandle):
    """trainer.py:35-89 for PaiNN (csrc/lb_train_painn.h): GnsTrainHandle's calls, one "acc" target."""

    _view: Optional["PainnHandle"] = None

    def model_handle(self) -> "PainnHandle":
        """The inference model of this handle: a view of its device weights, so engine.painn_forward / rollout on it run
        on the CURRENT weights.  Borrowed - it is this handle's; closing it frees nothing, closing this handle ends it."""
        if self._view is None or not self._view._h:
            h = C.c_void_p()
            check(self.engine.lib.lb_painn_train_model(self._h, C.byref(h)), "lb_painn_train_model")
            self._view = _BorrowedPainnHandle(self.engine, h, self.desc, self.n_floats)
        return self._view

    def close(self):
        if self._view is not None:
            self._view._h = None   # the view dies with the handle
        super().close()


class SegnnHandle(_Handle):
    _DESTROY, _ROLLOUT = "lb_segnn_destroy", "lb_segnn_rollout"
    _tap = None

    def set_tap(self, on: bool = True) -> Optional[torch.Tensor]:
        e = self.engine
        if on:
            width = int(e.lib.lb_segnn_row_floats(self._h))   # 128, or the e3nn row of the general-irreps path
            self._tap = torch.zeros((self.desc.num_mp_steps + 1, e.B * e.N, width), dtype=torch.float32,
                                    device=e.device)
            check(e.lib.lb_segnn_set_tap(self._h, ptr(self._tap)))
        else:
            self._tap = None
            check(e.lib.lb_segnn_set_tap(self._h, None))
        return self._tap


class EgnnHandle(_Handle):
    _DESTROY, _ROLLOUT = "lb_egnn_destroy", "lb_egnn_rollout"
    _tap = None

    def set_tap(self, on: bool = True) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """Per-layer taps: (h (L+1, B*N, hidden), positions (L+1, B*N, dim)) fp32, filled by every forward."""
        e = self.engine
        if on:
            L = self.desc.num_mp_steps
            self._tap = (torch.zeros((L + 1, e.B * e.N, self.desc.hidden), dtype=torch.float32, device=e.device),
                         torch.zeros((L + 1, e.B * e.N, e.dim), dtype=torch.float32, device=e.device))
            check(e.lib.lb_egnn_set_tap(self._h, ptr(self._tap[0]), ptr(self._tap[1])), "lb_egnn_set_tap")
        else:
            self._tap = None
            check(e.lib.lb_egnn_set_tap(self._h, None, None), "lb_egnn_set_tap")
        return self._tap


class _BorrowedEgnnHandle(EgnnHandle):
    """An EgnnHandle whose lb_egnn belongs to a training handle (EgnnTrainHandle.model_handle): close() only lets go."""

    def close(self):
        self._h = None


class LinearHandle(_Handle):
    _DESTROY, _ROLLOUT = "lb_linear_destroy", "lb_linear_rollout"


class _BorrowedLinearHandle(LinearHandle):
    """A LinearHandle whose lb_linear belongs to a training handle (LinearTrainHandle.model_handle): close() only lets go."""

    def close(self):
        self._h = None


class PainnHandle(_Handle):
    _DESTROY, _ROLLOUT = "lb_painn_destroy", "lb_painn_rollout"
    _tap = None

    def set_tap(self, on: bool = True) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """Per-layer taps: (s (L+1, B*N, hidden), v (L+1, B*N, dim, hidden)) fp32, filled by every forward."""
        e = self.engine
        if on:
            L, H = self.desc.num_mp_steps, self.desc.hidden
            self._tap = (torch.zeros((L + 1, e.B * e.N, H), dtype=torch.float32, device=e.device),
                         torch.zeros((L + 1, e.B * e.N, e.dim, H), dtype=torch.float32, device=e.device))
            check(e.lib.lb_painn_set_tap(self._h, ptr(self._tap[0]), ptr(self._tap[1])), "lb_painn_set_tap")
        else:
            self._tap = None
            check(e.lib.lb_painn_set_tap(self._h, None, None), "lb_painn_set_tap")
        return self._tap


class _BorrowedPainnHandle(PainnHandle):
    """A PainnHandle whose lb_painn belongs to a training handle (PainnTrainHandle.model_handle): close() only lets go."""

    def close(self):
        self._h = None
