"""ctypes binding of liblbhip.so (include/lbhip.h).  There is NO CPU fallback: if the HIP
library is missing or fails to load, every entry point raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "liblbhip.so")

LB_OK = 0
LB_FORCE_NONE, LB_FORCE_PIECEWISE, LB_FORCE_BUFFER = 0, 1, 2
LB_TRAIN_BATCH_MAX = 128

D3 = C.c_double * 3


class CaseDesc(C.Structure):
    """lb_case_desc (include/lbhip.h)."""

    _fields_ = [
        ("dim", C.c_int32), ("n_particles", C.c_int32), ("batch", C.c_int32), ("isl", C.c_int32),
        ("periodic", C.c_int32), ("has_bound", C.c_int32), ("has_vel_mag", C.c_int32),
        ("force_kind", C.c_int32), ("force_axis", C.c_int32), ("geometry_f32", C.c_int32),
        ("box", D3), ("r_cutoff", C.c_double), ("capacity_multiplier", C.c_double),
        ("vel_mean", D3), ("vel_std", D3), ("acc_mean", D3), ("acc_std", D3),
        ("bound_lo", D3), ("bound_hi", D3),
        ("force_split", C.c_double), ("force_lo", D3), ("force_hi", D3),
    ]


class GnsDesc(C.Structure):
    """lb_gns_desc (include/lbhip.h)."""

    _fields_ = [
        ("latent_size", C.c_int32), ("blocks_per_step", C.c_int32), ("num_mp_steps", C.c_int32),
        ("embedding_size", C.c_int32), ("num_particle_types", C.c_int32), ("node_in", C.c_int32),
        ("edge_in", C.c_int32), ("out_dim", C.c_int32),
    ]


class SegnnDesc(C.Structure):
    """lb_segnn_desc (include/lbhip.h)."""

    _fields_ = [
        ("hidden", C.c_int32), ("blocks_per_step", C.c_int32), ("num_mp_steps", C.c_int32),
        ("homogeneous", C.c_int32), ("n_vels", C.c_int32), ("velocity_avg", C.c_int32),
        ("lmax_hidden", C.c_int32), ("lmax_attributes", C.c_int32), ("norm", C.c_int32), ("norm_eps", C.c_float),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "lmax_hidden" not in kw and len(args) < 7:
            self.lmax_hidden = 1
        if "lmax_attributes" not in kw and len(args) < 8:
            self.lmax_attributes = 1


class EgnnDesc(C.Structure):
    """lb_egnn_desc (include/lbhip.h)."""

    _fields_ = [
        ("hidden", C.c_int32), ("num_mp_steps", C.c_int32), ("n_vels", C.c_int32), ("homogeneous", C.c_int32),
        ("residual", C.c_int32), ("normalize", C.c_int32), ("tanh_pos", C.c_int32),
    ]


class PainnDesc(C.Structure):
    """lb_painn_desc (include/lbhip.h)."""

    _fields_ = [
        ("hidden", C.c_int32), ("num_mp_steps", C.c_int32), ("n_vels", C.c_int32), ("homogeneous", C.c_int32),
        ("shared_filters", C.c_int32), ("shared_interactions", C.c_int32), ("n_rbf", C.c_int32),
        ("has_cutoff", C.c_int32), ("cutoff", C.c_float),
    ]


class LinearDesc(C.Structure):
    """lb_linear_desc (include/lbhip.h)."""

    _fields_ = [("n_in", C.c_int32), ("out_dim", C.c_int32)]


class TrainProbeArgs(C.Structure):
    """lb_train_probe_args (include/lbhip.h): one call of the test hook lb_train_probe."""

    _fields_ = (
        [(k, C.c_void_p) for k in ("x", "dy", "dy_b", "tmax", "z", "b1", "scale", "gth", "dz", "idx")]
        + [(k, C.c_int64) for k in ("rows", "dst0", "dst1", "dst_b", "part_off", "stride")]
        + [(k, C.c_int32) for k in ("K", "ldx", "M", "ldy", "nb", "math", "xexp", "xdyn", "d", "G", "n0", "n1", "off1", "ld0",
                                    "skip", "col0", "emb", "ntypes", "guard", "slot")]
    )


PROBE_OPS = {"dw": 0, "dw_narrow": 1, "colsum": 2, "ln_bwd": 3, "reduce": 4, "embed_grad": 5}


def train_probe_plan(rows: int, K: int, math: int) -> dict:
    """Test hook (include/lbhip.h: lb_train_probe_plan): the row split and the kernel of a weight-gradient launch."""
    out = (C.c_int64 * 5)()
    check(load().lb_train_probe_plan(int(rows), int(K), int(math), out), "lb_train_probe_plan")
    return {"G": out[0], "chunk": out[1], "h": out[2], "NA": out[3], "DEPTH": out[4]}


# name -> (restype, argtypes).  Every symbol include/lbhip.h declares must be listed here;
# tests/test_abi.py checks the two against each other.
_P = C.c_void_p
_SIGS = {
    "lb_strerror": (C.c_char_p, [C.c_int]),
    "lb_last_error": (C.c_char_p, []),
    "lb_version": (C.c_int, []),
    "lb_engine_create": (C.c_int, [C.POINTER(CaseDesc), _P, C.POINTER(_P)]),
    "lb_engine_destroy": (None, [_P]),
    "lb_set_particle_type": (C.c_int, [_P, _P]),
    "lb_set_force": (C.c_int, [_P, _P]),
    "lb_load_window": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_train_batch": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.c_uint64, C.c_int64, C.c_double, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                 _P]),
    "lb_read_window": (C.c_int, [_P, _P]),
    "lb_nl_allocate": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lb_nl_set_capacity": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "lb_nl_update": (C.c_int, [_P]),
    "lb_nl_read_flags": (C.c_int, [_P, _P]),
    "lb_nl_read_idx": (C.c_int, [_P, _P, _P]),
    "lb_node_features": (C.c_int, [_P, _P, _P, _P, _P]),
    "lb_edge_features": (C.c_int, [_P, _P, _P]),
    "lb_gns_create": (C.c_int, [_P, C.POINTER(GnsDesc), _P, C.c_int64, C.POINTER(_P)]),
    "lb_gns_destroy": (None, [_P]),
    "lb_gns_forward": (C.c_int, [_P, _P, _P]),
    "lb_set_fused_aggregation": (C.c_int, [_P, C.c_int32]),
    "lb_gns_set_tap": (C.c_int, [_P, _P]),
    "lb_math_mode": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lb_math_fallbacks": (C.c_int32, [_P]),
    "lb_debug_inject_guard": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "lb_train_probe_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "lb_train_probe": (C.c_int, [_P, C.c_int32, C.POINTER(TrainProbeArgs)]),
    "lb_integrate": (C.c_int, [_P, _P, _P, _P, C.c_int32]),
    "lb_case_integrate": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P]),
    "lb_rollout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "lb_ekin": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32]),
    "lb_sinkhorn": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_double, _P, C.c_int32, _P]),
    "lb_sinkhorn_pot": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double, _P,
                                  C.c_int32, _P]),
    "lb_metrics": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    "lb_timers_enable": (C.c_int, [_P, C.c_int32]),
    "lb_timers_reset": (C.c_int, [_P]),
    "lb_timer_count": (C.c_int32, []),
    "lb_timer_name": (C.c_char_p, [C.c_int32]),
    "lb_timer_get": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "lb_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lb_edge_accounting": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.c_int32]),
    "lb_kernel_names": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "lb_nl_route": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "lb_gns_train_create": (C.c_int, [_P, C.POINTER(GnsDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_gns_train_destroy": (None, [_P]),
    "lb_gns_train_loss_grad": (C.c_int, [_P, _P, C.c_float, C.POINTER(C.c_double), _P]),
    "lb_gns_train_zero_grad": (C.c_int, [_P]),
    "lb_adamw_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "lb_gns_train_read": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float), C.c_int64]),
    "lb_gns_train_write": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float), C.c_int64, C.c_int64]),
    "lb_gns_train_step_count": (C.c_int64, [_P]),
    "lb_gns_train_device_blob": (C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "lb_adamw_step_gathered": (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_float]),
    "lb_gns_train_math_fallbacks": (C.c_int32, [_P]),
    "lb_gns_train_sort_fallbacks": (C.c_int32, [_P]),
    "lb_train_forward": (C.c_int, [_P, _P]),
    "lb_train_backward": (C.c_int, [_P, _P, _P]),
    "lb_train_exact_math": (C.c_int, [_P, C.c_int32]),
    "lb_gns_train_sync_model": (C.c_int, [_P, _P]),
    "lb_gns_image_bytes": (C.c_int64, [_P]),
    "lb_gns_image_read": (C.c_int, [_P, _P, C.c_int64]),
    "lb_gns_pack_selftest": (C.c_int64, [C.POINTER(GnsDesc), C.c_int32, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "lb_segnn_train_create": (C.c_int, [_P, C.POINTER(SegnnDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_segnn_train_loss_grad": (C.c_int, [_P, _P, C.c_float, C.POINTER(C.c_double), _P]),
    "lb_segment_sum": (C.c_int, [_P, _P, _P, C.c_int32]),
    "lb_segnn_create": (C.c_int, [_P, C.POINTER(SegnnDesc), _P, C.c_int64, C.POINTER(_P)]),
    "lb_segnn_destroy": (None, [_P]),
    "lb_segnn_forward": (C.c_int, [_P, _P, _P]),
    "lb_segnn_row_floats": (C.c_int32, [_P]),
    "lb_segnn_set_tap": (C.c_int, [_P, _P]),
    "lb_segnn_rollout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "lb_egnn_create": (C.c_int, [_P, C.POINTER(EgnnDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_egnn_destroy": (None, [_P]),
    "lb_egnn_forward": (C.c_int, [_P, _P, _P]),
    "lb_egnn_set_tap": (C.c_int, [_P, _P, _P]),
    "lb_egnn_rollout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "lb_egnn_train_create": (C.c_int, [_P, C.POINTER(EgnnDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_egnn_train_loss_grad": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double), _P]),
    "lb_egnn_train_model": (C.c_int, [_P, C.POINTER(_P)]),
    "lb_painn_create": (C.c_int, [_P, C.POINTER(PainnDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_painn_destroy": (None, [_P]),
    "lb_painn_forward": (C.c_int, [_P, _P, _P]),
    "lb_painn_set_tap": (C.c_int, [_P, _P, _P]),
    "lb_painn_rollout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "lb_painn_train_create": (C.c_int, [_P, C.POINTER(PainnDesc), C.POINTER(C.c_float), C.c_int64, C.c_int32, C.POINTER(_P)]),
    "lb_painn_train_model": (C.c_int, [_P, C.POINTER(_P)]),
    "lb_linear_create": (C.c_int, [_P, C.POINTER(LinearDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_linear_destroy": (None, [_P]),
    "lb_linear_forward": (C.c_int, [_P, _P, _P]),
    "lb_linear_rollout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "lb_linear_train_create": (C.c_int, [_P, C.POINTER(LinearDesc), C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_linear_train_model": (C.c_int, [_P, C.POINTER(_P)]),
    "lb_blob_train_create": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int64, C.POINTER(_P)]),
    "lb_graph_gather": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32]),
    "lb_graph_segment_sum": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32]),
    "lb_graph_sender_sorts": (C.c_int32, [_P]),
    "lb_graph_degree": (C.c_int, [_P, C.c_int32, _P]),
    "lb_graph_segment_max": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32]),
    "lb_graph_segment_min": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32]),
    "lb_graph_segment_max_backward": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32]),
    "lb_graph_segment_softmax": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32]),
    "lb_graph_segment_softmax_backward": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32]),
    "lb_graph_attend": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_attend_backward": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_features_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    # the same ops on float32 or bfloat16 tensors: the float32 entry's arguments and a trailing dtype (0 float32, 1 bfloat16)
    "lb_graph_gather_t": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_sum_t": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_max_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_min_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_max_backward_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_softmax_t": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_segment_softmax_backward_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "lb_graph_attend_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_attend_backward_t": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    # edge messages (float32 or bfloat16 by the trailing dtype)
    "lb_graph_conv": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_pair_mul": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_pair_add": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    # edge pairs: the reverse map (out (B E_cap) int32); swap / symmetrize / antisymmetrize (mode, msg, out, C, dtype)
    "lb_graph_reverse": (C.c_int, [_P, _P]),
    "lb_graph_edge_pair_t": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    # equivariant vector messages: (x | v, w, u, out); the edge gradients (S, V, w, u, d_w or null, d_u or null)
    "lb_graph_conv_vec": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_conv_dot": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_conv_vec_edge_grad": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    # filter_conv: (x, f, weight, out, K, R, C); its edge gradients (x, d, f, weight, d_f or null, d_weight or null, partials,
    # partials_len, K, R, C)
    "lb_graph_filter_conv": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lb_graph_filter_conv_grad": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32]),
    "lb_graph_filter_partials": (C.c_int64, [_P, C.c_int32, C.c_int32]),
    # the multi-aggregator: (msg, out, win or null, stats or null, C, ops, eps); backward (d_out, msg, win, stats, d_msg, C, ops)
    "lb_graph_aggregate": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32]),
    "lb_graph_aggregate_backward": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
}

_lib: Optional[C.CDLL] = None


class LbHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load liblbhip.so and bind the prototypes.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbHipError(
            f"{LIB_PATH} not found: the HIP engine is not built. Run "
            "`python -m lagrangebench_amd.build` (needs hipcc). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != LB_OK:
        lib = load()
        msg = lib.lb_last_error().decode() or lib.lb_strerror(rc).decode()
        raise LbHipError(f"{what or 'liblbhip'} failed ({rc}: {lib.lb_strerror(rc).decode()}): {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (or None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()
