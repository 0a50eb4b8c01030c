#!/usr/bin/env python
"""bench.py - rollout throughput of the MI355X engine on BASELINE.json's metric.

    python bench.py --gpus N --steps K --warmup W [--workload tgv3d] [--batch B] [--dump-outputs DIR] [--full]

A "step" is ONE rollout step (neighbor-list rebuild -> features -> GNS-10-128 -> integrator ->
prediction store) over one batch of B synthetic trajectories per GPU.  Inputs are resident in
HBM before the timed region.  Workload of `value` (config.workload): TGV3D-8k x 8 trajectories whose
neighbour count is stationary over the rollout (--vel-amp 0.03, round 6); the drifting trajectories
rounds 1 - 5 quoted `value` on are other_configs[tag = "tgv3d_drifting"].  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, allocation pass, warm-up, the timed repeats, the MSE
gather, --dump-outputs, and a line with metric / value / unit / higher_is_better / dtype / ms_per_step, the
repeats, dist and config objects and mse20_mean.  --full appends everything below; each object takes runs of
its own after the timed region (--no-f32, --no-other-configs, --no-cpu-baseline trim them, --pmc adds to them):

  metric/value : rollout particle-steps/s, whole job = n_gpus * B * N_particles * K / max-rank time
                 (median of --repeats timed regions of exactly K steps)
  roofline     : (--full) the dominant kernel (processor edge MLP with the fused aggregation), timed with HIP
                 events bound to its dispatches inside this run; algorithmic bytes from the mean real
                 edge count of the timed steps.  `bound` "hbm" in the default f16x2 arithmetic (edge
                 latents stream once in, once out per layer), `limiter` says what actually holds the
                 launch: the package power cap (`power`: hwmon sclk / W at 100 Hz over 1.5 s of the
                 same rollout).  `traffic`: committed rocprofv3 FETCH_SIZE / WRITE_SIZE passes
                 (profiles/pmc_traffic.json; --pmc re-measures with two nested passes).
                 With LB_MATH=f32 the kernel is bound by the fp32 MFMA pipe and the object says so.
  roofline_aggregate : the stand-alone jraph.segment_sum kernel (HBM bound) north_star singles out
  breakdown_ms_per_step, power : per-kernel-class HIP-event times of the same K steps; hwmon clock / power
  f32_exact    : the same K steps in exact-fp32 MFMA arithmetic (N=1, unless --no-f32)
  other_configs, stationary, train_step : short runs of the other BASELINE.json configs (N=1, unless --no-other-configs)
  cpu_baseline : the CPU restatement of the reference's algorithm (oracle/: torch-CPU network + NumPy
                 neighbor list, padded E_cap rows, unfused ops; kind "port", NOT JAX-CPU) timed on this
                 host's cores on a bounded sample after all GPU work (rank 0, N=1 only, unless --no-cpu-baseline)

--dump-outputs DIR: after the timed region, rank 0 writes what the last timed repeat of the K-step rollout returned as
DIR/<name>.npy (float64, at most DUMP_BUDGET_BYTES in all, see dump_outputs); the inputs depend on the arguments only
(seeded synthetic trajectories and weights), so two builds run with the same arguments compare output for output.

Multi-GPU: launched by torch.distributed.run, one rank per GPU; trajectories are independent, so
there is no data-path collective - RCCL only gathers the per-trajectory MSE vectors and the max
wall time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STATIONARY_VEL_AMP = 0.03  # lagrangebench_amd/data/synthetic.py: the ballistic rollout stays within half a spacing of the lattice
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_F32_PEAK_TF = 157.3   # MI355X_MICROARCH.md: fp32-input MFMA, dense
MFMA_F16_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: bf16/fp16 MFMA, dense (2:1-sparse figure is 2x)
D = 128
DUMP_BUDGET_BYTES = 64 << 20


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def pmc_traffic(kernel_substr: str, workload: str, batch: int, stationary: bool = False):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json,
    produced by tools/pmc_traffic.py from separate FETCH_SIZE / WRITE_SIZE runs of this command;
    FETCH_SIZE doubled per the gfx950 note in MI355X_MICROARCH.md).  None if not measured."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            tab = json.load(f)
        keys = (f"{workload}_b{batch}", f"{workload}_b{batch}_r01")   # _r01: kernels only profiled in round 1
        if stationary:   # round 6: the headline's stationary trajectories have their own passes
            keys = (f"{workload}_b{batch}_st",) + keys
        for key in keys:
            for k, v in sorted(tab.get(key, {}).items()):
                if kernel_substr in k:
                    return v["hbm_bytes_per_launch"]
    except Exception:
        pass
    return None


def dump_outputs(path, arrays):
    """Write the (name, array) pairs to path/<name>.npy as float64, in order, within DUMP_BUDGET_BYTES in all.  An array
    that does not fit into what is left is replaced by a fixed sample of its flattened elements (seed 0, ascending
    index order), so that the same arguments always dump the same elements."""
    os.makedirs(path, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    for name, a in arrays:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        cap = max(left - 4096, 0) // a.itemsize   # 4 KiB per file for the .npy header
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=cap, replace=False))
            log(f"[bench] --dump-outputs: {name} {a.shape} sampled to {cap} elements")
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes + 4096


def hip_case(ds):
    """case_builder for a synthetic dataset (product code only: nothing under oracle/ or tests/ is
    imported on the measured path)."""
    from lagrangebench_amd.case_setup import case_builder
    return case_builder(
        ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"multiplier": ds.multiplier},
        cfg_model={"isotropic_norm": ds.isotropic_norm, "magnitude_features": getattr(ds, "magnitude_features", False)},
        noise_std=ds.noise_std, external_force_fn=ds.force)


def sg_msg_flops(n_edges, dim):
    """fp16 MFMA products k_sg_msg issues per launch: block 0: S 128x64, T 64x32, V dim x 64x32; block 1: S 64x64,
    T 32x32, V dim x 32x32; x 3 split passes (lo*hi + hi*lo + hi*hi), 2 flop per product."""
    return n_edges * 2 * 3 * (128 * 64 + 64 * 32 + dim * 64 * 32 + 64 * 64 + 32 * 32 + dim * 32 * 32)


def gns_widths(ds):
    dim, K = len(ds.box), ds.input_seq_length - 1
    node_in = K * dim + (K if getattr(ds, "magnitude_features", False) else 0)
    if not any(ds.metadata["periodic_boundary_conditions"]):
        node_in += 2 * dim
    if ds.external_force_fn is not None:
        node_in += dim
    return node_in, dim + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="tgv3d", choices=["tgv2d", "rpf2d", "tgv3d", "ldc3d", "dam2d"])
    ap.add_argument("--batch", type=int, default=8, help="trajectories advanced together per GPU")
    ap.add_argument("--mp-steps", type=int, default=10)
    ap.add_argument("--model", default="gns", choices=["gns", "segnn"],
                    help="gns: BASELINE.json's headline config; segnn: configs[4] (SEGNN-10-64)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure what takes runs of its own: roofline objects and per-kernel "
                         "breakdown, power, the fp32 sub-run, the other configs, training steps and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="(--full) skip the short sub-runs of the other BASELINE.json configs appended as `other_configs`")
    ap.add_argument("--pmc", action="store_true",
                    help="(--full) re-measure roofline.traffic with two nested rocprofv3 PMC passes of this command (FETCH_SIZE, WRITE_SIZE; "
                         "~10 s); default (round 6): the committed profiles/pmc_traffic.json value, `traffic_source` names it")
    ap.add_argument("--no-pmc", action="store_true", help="(accepted for older scripts; the nested passes are opt-in now: --pmc)")
    ap.add_argument("--shuffle", action="store_true",
                    help="randomly permute the particle ids (memory-locality ablation; default: lattice order)")
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15,
                    help="the K-step timed region is repeated this many times; value / ms_per_step = the median")
    ap.add_argument("--cpu-baseline-only", default=None, metavar="WORKLOAD",
                    help="(internal) run only the CPU baseline leg of WORKLOAD and print its JSON object")
    ap.add_argument("--no-f32", action="store_true", help="(--full) skip the exact-fp32 (LB_MATH=f32 arithmetic) sub-run")
    ap.add_argument("--vel-amp", type=float, default=STATIONARY_VEL_AMP,
                    help="velocity scale of the synthetic trajectories: 0.03 (default, round 6) keeps the neighbour count of "
                         "the untrained rollout stationary (TGV3D ~14.4 per particle, SURVEY 8d: 13.1); 1.0 = the drifting "
                         "workload rounds 1-5 quoted `value` on (13.6 -> 18.5 -> 17.1, mean 16.2)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed rollout returned (rank 0) as DIR/<name>.npy: pred_last_step (B, N, dim) = "
                         "the positions of the last timed step, mse (world*B, K) (GNS only), pred (B, K, N, dim); float64, "
                         "<= 64 MB in all (a seeded sample of pred beyond that)")
    args = ap.parse_args()
    if args.pmc and not args.full:
        ap.error("--pmc re-measures the roofline objects of --full: give both")
    if args.cpu_baseline_only:   # legs one after the other in this process: they must not compete for the cores
        print(json.dumps({w: cpu_baseline_leg(w, args.mp_steps, args.vel_amp) for w in args.cpu_baseline_only.split(",")}), flush=True)
        return

    t_start = time.perf_counter()
    from lagrangebench_amd import dist as lbdist
    rank, local_rank, world = lbdist.init()
    cpu_jobs = None
    if world != args.gpus:
        log(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: using WORLD_SIZE")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    device = lbdist.local_device(local_rank)
    torch.cuda.set_device(device)

    if args.model == "segnn":
        return run_segnn(args, rank, world, device)

    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS

    B, K, W, L = args.batch, args.steps, args.warmup, args.mp_steps
    math_mode = "f32" if os.environ.get("LB_MATH") == "f32" else "f16x2"
    ds = make_case(args.workload, n_trajs=world * B, extra_seq_length=max(K, W, 1), vel_amp=args.vel_amp)
    dim = len(ds.box)
    model = GNS(dim, D, 2, L, 16)
    node_in, edge_in = gns_widths(ds)
    params = model.init_params(1234, node_in, edge_in, decoder_scale=0.01)  # haiku-default init, decoder x0.01
    case = hip_case(ds)
    mine = [rank * B + i for i in range(B)]  # weak scaling: B trajectories per GPU
    pos = np.stack([ds[i][0] for i in mine])
    pt = np.stack([ds[i][1] for i in mine])
    N = pos.shape[1]
    if args.shuffle:  # particle order of real SPH output is not lattice order: same physics, random ids
        perm = np.random.default_rng(7).permutation(N)
        pos, pt = pos[:, perm], pt[:, perm]
    eng = case.engine(B)
    eng.set_particle_type(pt)
    traj = eng.prepare_traj(pos)  # fp64, resident in HBM
    handle = model.handle(eng, params)

    # allocation pass (not the warm-up): one untimed run of the K-step rollout grows the neighbor-list
    # capacities to what it needs, as they have in the steady state of eval_rollout's loop over trajectory
    # batches (the reference's `allocate` + recompile happen outside its step loop too) - so that a small W
    # does not put re-allocations into the timed region; n_realloc of the timed region is reported
    if W < K:
        eng.rollout(handle, traj, K)
    # warm-up: W steps of the same rollout
    eng.rollout(handle, traj, max(W, 1))
    # timed region: EXACTLY K steps between barrier + synchronize on both sides, max over ranks; repeated
    # `--repeats` times (same rollout, same inputs) - value / ms_per_step are the MEDIAN repeat, all repeats listed
    dts, n_realloc = [], 0
    eng.edge_accounting(reset=True)   # every neighbor-list build from here on adds its real edge count (device side)
    for _ in range(max(1, args.repeats)):
        lbdist.barrier(device)
        t0 = time.perf_counter()
        pred, nr = eng.rollout(handle, traj, K)  # host-synchronous at the end
        lbdist.barrier(device)
        dts.append(lbdist.max_over_ranks(time.perf_counter() - t0, device))
        n_realloc += nr
    dt = float(np.median(dts))
    dist_info = lbdist.group_info(device)
    acct = eng.edge_accounting(reset=True)   # edges of the builds of the timed repeats (every repeat = the same K steps)
    st = eng.stats()
    E_last = st["n_edges_total"]             # the LAST step's list (what the engine still holds)
    fallbacks_timed = eng.math_fallbacks()

    # gather the per-trajectory MSE vectors over RCCL (the only collective of the job)
    tgt = traj[:, :, ds.input_seq_length:ds.input_seq_length + K].permute(0, 2, 1, 3).contiguous()
    mse = eng.metrics(pred, tgt, K, want=("mse",))["mse"]
    merged = lbdist.gather_metrics({mine[i]: mse[i] for i in range(B)}, world * B, K, device)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [("pred_last_step", pred[:, -1].cpu().numpy()),
                                         ("mse", np.stack([merged[i].cpu().numpy() for i in range(world * B)])),
                                         ("pred", pred.cpu().numpy())])

    def headline(a):
        """The line of a plain run; `a`: the edge accounting its edge figures come from (--full: the HIP-event pass)."""
        return {
            "metric": "rollout particle-steps/sec",
            "value": world * B * N * K / dt,
            "unit": "particle-steps/s",
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": 1e3 * dt / K,
            "repeats": {"n": len(dts), "ms_per_step_all": [round(1e3 * x / K, 4) for x in dts],
                        "ms_per_step_min": 1e3 * min(dts) / K, "ms_per_step_max": 1e3 * max(dts) / K,
                        "note": "value / ms_per_step = the median repeat of the K-step timed region"},
            "dist": dist_info,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if math_mode == "f32" else "f32 (GEMMs as fp16 hi/lo split products, fp32 accumulate)",
            "data": "synthetic",
            "config": {
                "workload": f"{args.workload} GNS-{L}-{D} inference rollout, neighbor list rebuilt every step",
                "n_particles": int(N), "batch_per_gpu": B, "edges_per_traj": int(round(a["mean"] / B)),
                "edges_per_traj_first": int(a["first"] // B), "edges_per_traj_mean": round(a["mean"] / B, 1),
                "edges_per_traj_last": int(E_last // B), "edges_per_traj_mean_timed_repeats": round(acct["mean"] / B, 1),
                "vel_amp": args.vel_amp,
                "edges_note": ("per-launch bytes / flops of every roofline object use the MEAN real E of the K steps the HIP-event "
                               "timers cover (device-side sum over the neighbor-list builds, lb_edge_accounting); round 6: `value` "
                               "is quoted on trajectories whose neighbour count is stationary (vel_amp 0.03, ~14.4 per particle; "
                               "SURVEY 8d: 13.1) - the drifting workload of rounds 1 - 5 is other_configs[tag = tgv3d_drifting]"),
                "math_fallbacks": int(fallbacks_timed),
                "input_seq_length": ds.input_seq_length, "geometry_dtype": "f64", "network_math": math_mode,
                "weights": "haiku-default init (seed 1234), decoder x0.01", "n_realloc": int(n_realloc),
            },
            "steps_per_s_per_traj": K / dt,
            "mse20_mean": float(np.mean([float(v.mean()) for v in merged.values()])),
            "mse_note": ("untrained (random-init) weights against synthetic trajectories: exercises the metric kernel "
                         "and the RCCL gather, NOT an accuracy figure; parity of the rollout with the reference "
                         "arithmetic (MSE within 1e-5 of the oracle) is asserted by tests/test_gpu_parity.py"),
        }

    if not args.full:
        if rank == 0:
            out = headline(acct)
            out["bench_wall_s"] = round(time.perf_counter() - t_start, 1)
            log(f"[bench] done at {out['bench_wall_s']} s (--full for roofline, breakdown, sub-runs and CPU baseline)")
            print(json.dumps(out), flush=True)
        return

    # second pass with per-kernel-class HIP events (same K steps) for the roofline objects
    eng.timers_enable(True)
    eng.timers_reset()
    eng.rollout(handle, traj, K)
    tm = eng.timers()
    acct_tm = eng.edge_accounting(reset=True)
    # E of a launch AVERAGED over the K steps the timers cover (the rollout's E drifts, the launch times are
    # averages over all K steps - bytes and flops per launch must use the mean E of those steps, not the last step's)
    E_tot = acct_tm["mean"]
    fused = tm["aggregate"][1] == 0
    if fused:
        # aggregation is fused into the edge kernel on the hot path: time the stand-alone
        # jraph.segment_sum kernel (lb_segment_sum) on the same receiver-sorted list separately
        # (that list is the LAST step's: its bytes use E_last)
        msg = torch.randn((E_last, D), dtype=torch.float32, device=device)
        eng.segment_sum(msg)
        eng.timers_reset()
        for _ in range(20):
            eng.segment_sum(msg)
        tm["aggregate"] = eng.timers()["aggregate"]
        del msg
    eng.timers_enable(False)

    if rank != 0:
        return
    # power pass (round 6): the same rollout repeated for ~1.5 s while a thread samples the card's hwmon
    # node (shader clock, package power) at 100 Hz: mean clock / power of the headline workload, joules per rollout step
    power = None
    if world == 1:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import power_probe as PP
            with PP.PowerProbe(hz=100.0, pci=PP.hip_pci_address()) as probe:
                eng.rollout(handle, traj, K)   # clocks settle
                torch.cuda.synchronize(device)
                tp0 = time.perf_counter()
                n_pw = 0
                while time.perf_counter() - tp0 < 1.5:
                    eng.rollout(handle, traj, K)
                    n_pw += K
                torch.cuda.synchronize(device)
                tp1 = time.perf_counter()
            power = probe.summary(units=n_pw, t0=tp0, t1=tp1)
            if power:
                power["joules_per_step"] = power.pop("joules_per_unit", None)
                power["steps_in_window"] = n_pw
        except Exception as exc:
            power = {"error": repr(exc)[:200]}
    ms_edge, n_edge = tm["edge_mlp"]
    ms_last, n_last = tm.get("edge_mlp_last", (0.0, 0))   # last layer: no edge-latent store (its own timer class)
    if n_edge == 0 and n_last > 0:                         # (one MP layer: the no-store variant is the only launch)
        ms_edge, n_edge, ms_last, n_last = ms_last, n_last, 0.0, 0
    if n_edge == 0 and tm.get("processor", (0, 0))[1] > 0:   # all layers in one persistent launch: per-layer share
        ms_edge, n_edge = tm["processor"][0], tm["processor"][1] * L
    ms_agg, n_agg = tm["aggregate"]
    us_edge = 1e3 * ms_edge / max(n_edge, 1)
    us_agg = 1e3 * ms_agg / max(n_agg, 1)
    BN = B * N
    # ---- dominant kernel: processor edge MLP (+ fused aggregation), one launch = one MP layer.
    # Algorithmic HBM bytes (SURVEY 8d "edge latents round-trip HBM" + node-side rows):
    #   read e (E*512) + write e (E*512) + sender/receiver ids (E*8) + projections read once (N*1024)
    #   + aggregated messages written once (N*512)
    # SURVEY 8d counts E*(2*D*4+8) + N*2*D*4 (= E*1032 + N*1024); the N*512 of aggregated messages the
    # kernel also writes are left out of `achieved` (conservative) and listed under bytes_incl_agg
    edge_bytes = int(round(E_tot * (2 * D * 4 + 8))) + BN * (2 * D * 4)
    edge_bytes_incl_agg = edge_bytes + BN * D * 4
    gbs_edge = edge_bytes / (us_edge * 1e-6) / 1e9
    # flops: algorithmic (reference formulation) 2*4*D*D per edge; executed products
    # 2*2*D*D per edge (sender/receiver part projected per node), x3 MFMA passes in f16x2
    flop_algo = int(round(E_tot * 2 * 4 * D * D))
    flop_prod = int(round(E_tot * 2 * 2 * D * D))
    if math_mode == "f16x2":
        mfma = {"dtype": "f16 (x3 split passes)", "achieved": 3 * flop_prod / (us_edge * 1e-6) / 1e12,
                "peak": MFMA_F16_PEAK_TF, "unit": "TFLOP/s"}
    else:
        mfma = {"dtype": "f32", "achieved": flop_prod / (us_edge * 1e-6) / 1e12, "peak": MFMA_F32_PEAK_TF,
                "unit": "TFLOP/s"}
    mfma["frac"] = mfma["achieved"] / mfma["peak"]
    mfma["fp32_equivalent_algorithmic_tflops"] = flop_algo / (us_edge * 1e-6) / 1e12
    kern = eng.kernel_names()["edge"]  # the library names the kernel family it picked for this size / arithmetic
    pmc_key = kern.split("<")[0].split(" ")[0]
    # the LAST layer's launch writes no edge latents (nobody reads them): E*520 + N*1024 algorithmic bytes, timed as
    # its own class so that the dominant kernel above is not credited bytes that variant does not move
    last_variant = None
    if n_last > 0:
        us_last = 1e3 * ms_last / n_last
        last_bytes = int(round(E_tot * (D * 4 + 8))) + BN * (2 * D * 4)
        last_variant = {"kernel": kern + " [last layer: SKIP = no edge-latent store]", "us_per_launch": us_last,
                        "launches": int(n_last), "bytes_per_launch": last_bytes,
                        "achieved": last_bytes / (us_last * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": last_bytes / (us_last * 1e-6) / 1e9 / HBM_PEAK_GBS,
                        "note": "half the bytes, nearly the same time: this launch is bound by instruction issue / LDS "
                                "weight reads, not by HBM (DESIGN.md section 4.3)"}
    if math_mode == "f16x2":
        roof = {"kernel": kern, "bound": "hbm", "achieved": gbs_edge, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": gbs_edge / HBM_PEAK_GBS, "last_layer_variant": last_variant,
                "traffic": pmc_traffic(pmc_key, args.workload, B, args.vel_amp != 1.0),
                "traffic_source": "profiles/pmc_traffic.json (separate rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this command, committed; not re-measured by this run - `--pmc` does)",
                "us_per_launch": us_edge, "launches": int(n_edge), "bytes_per_launch": edge_bytes,
                "edges_per_launch_mean": round(E_tot, 1), "tiles_per_launch_mean": round(E_tot / 16, 1),
                "bytes_formula": "E_mean * (2*128*4 + 8) + B*N * 2*128*4  (SURVEY 8d; E_mean = mean real E of the timed steps)",
                "bytes_incl_agg": edge_bytes_incl_agg, "mfma": mfma, "node_kernel": eng.kernel_names()["node"]}
    else:
        roof = {"kernel": kern, "bound": "mfma", "achieved": mfma["achieved"], "peak": mfma["peak"],
                "unit": "TFLOP/s", "frac": mfma["frac"],
                "traffic": pmc_traffic("k_edge16<true, false", args.workload, B),
                "node_kernel": eng.kernel_names()["node"],
                "us_per_launch": us_edge, "launches": int(n_edge), "flop_per_launch_executed": flop_prod,
                "hbm": {"achieved": gbs_edge, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs_edge / HBM_PEAK_GBS}}
    agg_bytes = E_last * (D * 4 + 4) + BN * D * 4  # E*516 + N*512 (the stand-alone kernel ran on the last step's list)
    gbs_agg = agg_bytes / (us_agg * 1e-6) / 1e9
    breakdown = {k: round(v[0] / K, 4) for k, v in tm.items() if v[1] > 0 and not (fused and k == "aggregate")}

    out = headline(acct_tm)
    out.update({
        "roofline": roof,
        "roofline_aggregate": {
            "kernel": "k_segment_sum", "bound": "hbm", "achieved": gbs_agg, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": gbs_agg / HBM_PEAK_GBS, "traffic": pmc_traffic("k_segment_sum", args.workload, B),
            "us_per_launch": us_agg, "launches": int(n_agg), "bytes_per_launch": agg_bytes,
            "on_hot_path": not fused,
            "note": ("stand-alone jraph.segment_sum kernel timed on the same receiver-sorted list; the hot path "
                     "fuses the aggregation into the edge-MLP epilogue (no message round trip)") if fused else "",
        },
        "breakdown_ms_per_step": breakdown,
        "power": power,
    })
    if power and power.get("power_w_mean") and power.get("power_cap_w"):
        at_cap = power["power_w_mean"] >= 0.93 * power["power_cap_w"]
        roof["sclk_mhz"] = power["sclk_mhz_mean"]
        roof["power_w"] = power["power_w_mean"]
        roof["joules_per_launch"] = power["power_w_mean"] * us_edge * 1e-6
        roof["limiter"] = ("power: the package sits at its cap while this workload runs (hwmon, 100 Hz) and the shader clock "
                           f"falls from 2400 to {power['sclk_mhz_mean']:.0f} MHz - only removing work moves the launch, overlap does not"
                           ) if at_cap else "not at the power cap while this workload runs"

    if world == 1 and math_mode == "f16x2" and not args.no_f32:
        # the same K steps in exact-fp32 MFMA arithmetic (what LB_MATH=f32 selects and what the range guard falls
        # back to): recorded so that the driver's line carries both arithmetics
        try:
            eng.math_mode(0)
            eng.rollout(handle, traj, K)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            eng.rollout(handle, traj, K)
            torch.cuda.synchronize(device)
            dt32 = time.perf_counter() - t0
            out["f32_exact"] = {"ms_per_step": 1e3 * dt32 / K, "value": B * N * K / dt32, "unit": "particle-steps/s",
                                "kernels": eng.kernel_names(), "note": "LB_MATH=f32 arithmetic, same inputs / weights"}
        except Exception as exc:
            out["f32_exact"] = {"error": repr(exc)[:200]}
        finally:
            eng.math_mode(1)
    log(f"[bench] headline + f32 sub-run done at {time.perf_counter() - t_start:.1f} s")
    if world == 1 and not args.no_other_configs:
        del pred, traj, handle, eng
        out["other_configs"] = other_configs(device)
        log(f"[bench] other_configs done at {time.perf_counter() - t_start:.1f} s")
        out["stationary"] = {"lines": other_configs(device, STATIONARY_PLAN, repeats=3),
                             "note": ("more lines on trajectories whose neighbour count does not drift over the rollout "
                                      "(vel_amp 0.03, as the headline since round 6: TGV3D holds ~14.4 neighbours per particle, "
                                      "SURVEY 8d quotes 13.1 for the dataset)")}
        log(f"[bench] stationary lines done at {time.perf_counter() - t_start:.1f} s")
        out["train_step"] = train_step_lines(device)
        log(f"[bench] train_step done at {time.perf_counter() - t_start:.1f} s")
    # Everything TIMED on the GPU is done.  The CPU-baseline legs run NOW, one after the other, with nothing else on the
    # host (run beside the nested rocprofv3 passes their step times spread 3x); the PMC passes follow.
    # Everything TIMED on the GPU is done.  The CPU-baseline legs run NOW, one after the other, with nothing else on the
    # host (beside the GPU sub-runs - tried in round 6 with disjoint core sets - the sub-runs' host side stalls: a
    # launch-bound B = 1 line read 12x slow); the opt-in PMC passes follow.
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_jobs = cpu_baseline_start(args)
        out["cpu_baseline"] = cpu_baseline_collect(cpu_jobs)
        cpu_jobs = None
        log(f"[bench] cpu_baseline done at {time.perf_counter() - t_start:.1f} s")
    # roofline.traffic measured by THIS run: two nested rocprofv3 passes of the same command (FETCH_SIZE, WRITE_SIZE:
    # the counters do not fit one pass; --kernel-trace + --pmc only), after the timed region; any failure or a
    # missing rocprofv3 falls back to the committed table above
    if world == 1 and args.pmc and not args.no_pmc:
        live = measure_traffic(args)
        if live:
            for key, dst in ((pmc_key, out["roofline"]), ("k_segment_sum", out["roofline_aggregate"])):
                hit = [v for k, v in sorted(live.items()) if key in k]
                if hit:
                    dst["traffic"] = hit[0]
                    dst["traffic_source"] = ("measured by this run: nested rocprofv3 --kernel-trace --pmc FETCH_SIZE / "
                                             "WRITE_SIZE passes (separate), (2*FETCH + WRITE) * 1 KiB per launch")
    if cpu_jobs is not None:
        out["cpu_baseline"] = cpu_baseline_collect(cpu_jobs)
    out["bench_wall_s"] = round(time.perf_counter() - t_start, 1)
    log(f"[bench] done at {out['bench_wall_s']} s")
    print(json.dumps(out), flush=True)


def measure_traffic(args, timeout_s=240):
    """HBM bytes per launch of every kernel of this workload from two nested rocprofv3 PMC passes
    (tools/pmc_traffic.py: averages over the real launches; FETCH_SIZE doubled per MI355X_MICROARCH.md).
    Returns {kernel name: bytes} or None.  Bounded: each pass runs in its own process group under a timeout."""
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    if not shutil.which("rocprofv3"):
        return None
    # already running under a profiler (e.g. the driver wraps this command in rocprofv3): no nested tracing
    if any(k.startswith(("ROCP_", "ROCPROF", "ROCTRACER")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import pmc_traffic as PT
        per = {}
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="lbpmc_", dir="/tmp")
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", ctr, "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--full", "--no-cpu-baseline", "--no-other-configs", "--no-pmc", "--no-f32", "--repeats", "1",
                   "--steps", str(args.steps), "--warmup", str(args.warmup),   # the SAME steps as the timed region: same mean E
                   "--workload", args.workload, "--batch", str(args.batch), "--mp-steps", str(args.mp_steps),
                   "--model", args.model, "--vel-amp", str(args.vel_amp)]
            p = subprocess.Popen(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                                 stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                p.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                shutil.rmtree(d, ignore_errors=True)
                return None
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if p.returncode != 0 or not dbs:
                shutil.rmtree(d, ignore_errors=True)
                return None
            per[ctr] = PT.per_kernel(dbs[0], ctr)
            shutil.rmtree(d, ignore_errors=True)
        return {k: int((2 * f + per["WRITE_SIZE"].get(k, 0.0)) * 1024) for k, f in per["FETCH_SIZE"].items()}
    except Exception as ex:  # measurement extra: never let it take the bench line down
        log(f"[bench] PMC traffic pass failed ({ex}); using profiles/pmc_traffic.json")
        return None


def _train_dtype():
    """LB_TRAIN_MATH=f32: exact-fp32 MFMA products; default: fp16 hi/lo split products with power-of-two row / matrix scaling."""
    return "f32" if os.environ.get("LB_TRAIN_MATH", "").startswith("f3") else \
        "f32 (products as fp16 hi/lo splits under power-of-two row / matrix scaling, fp32 accumulate)"


def _train_kernels():
    if os.environ.get("LB_TRAIN_MATH", "").startswith("f3"):
        return "k_lin32f (Y = XW, dX = dY W^T) + k_dw_part (dW += X^T dY): v_mfma_f32_16x16x4_f32, no library GEMM"
    return "k_lin32h (Y = XW, dX = dY W^T) + k_dw_part_h (dW += X^T dY): v_mfma_f32_16x16x32_f16 x 3 split products, no library GEMM"


def train_step_lines(device):
    """SURVEY section 8 row N4, the training step (trainer.py:35-89: value_and_grad of the masked MSE over the batch +
    optax.adamw), timed like the reference runs it: batch 1 (defaults.py train.batch_size), loss fetched every step.
    One line per workload: ms per step, particle-steps/s, and the rate of fp32-EQUIVALENT flops against the fp32 MFMA peak
    (forward 1x + backward 2x the forward's GEMM flops).  Default arithmetic: Y = XW and dX = dY W^T on k_lin32h, dW += X^T dY
    on k_dw_part_h - fp16 hi / lo split products under power-of-two scaling, fp32 accumulate, a range guard on dW's
    activation operand (include/lbhip.h); LB_TRAIN_MATH=f32 selects the exact-fp32 MFMA kernels k_lin32f / k_dw_part.
    Everything else - LayerNorm, gathers and their deterministic transposes, AdamW - is hand-written HIP; no library GEMM."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    res = []
    for workload, K in (("tgv2d", 10), ("tgv3d", 5)):
        try:
            ds = make_case(workload, n_trajs=1, extra_seq_length=2)
            dim, isl = len(ds.box), ds.input_seq_length
            model = GNS(dim, D, 2, 10, 16)
            node_in, edge_in = gns_widths(ds)
            params = model.init_params(1234, node_in, edge_in, decoder_scale=1.0)
            case = hip_case(ds)
            pos, pt = ds[0]
            feats, _ = case.allocate_eval((pos[None, :, :isl], pt[None]))
            eng = feats.engine
            E = eng.stats()["n_edges_total"]
            N = len(pt)
            th = model.train_handle(eng, params)
            target = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(5)).to(device)
            for _ in range(2):
                th.zero_grad()
                th.loss_grad(target, 1.0)
                th.adamw_step(1e-4)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(K):
                th.zero_grad()
                loss = th.loss_grad(target, 1.0)
                th.adamw_step(1e-4)
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / K
            # flops EXECUTED (the edge block's first Linear is split: e W_e per edge, n [W_s | W_r] per node)
            fwd = 10 * (E * 2 * (D * D + D * D) + N * 2 * (2 * D * D) + N * 2 * (2 * D * D + D * D)) + E * 2 * (8 * D + D * D) \
                + N * 2 * (eng.node_in + 16 + D) * D + N * 2 * (D * D + D * dim)
            tf = 3 * fwd / dt / 1e12
            res.append({"workload": f"{workload} GNS-10-128 training step (B = 1)", "n_particles": int(N), "edges": int(E),
                        "steps": K, "ms_per_step": 1e3 * dt, "value": N / dt, "unit": "particle-steps/s",
                        "loss": float(loss), "dtype": _train_dtype(),
                        "roofline": {"kernel": _train_kernels(), "bound": "mfma",
                                     "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                                     "flop_per_step": int(3 * fwd),
                                     "note": "whole-step rate (GEMMs + everything else) of fp32-equivalent flops against the fp32 MFMA peak"}})
            th.close()
            del eng, feats
        except Exception as exc:
            res.append({"workload": workload, "error": repr(exc)[:200]})
    # config 5's model (round 5: lb_segnn_train_loss_grad, csrc/lb_train_segnn.h): SEGNN-10-64 on DAM2D, B = 1
    try:
        from lagrangebench_amd.models import SEGNN, node_irreps
        ds = make_case("dam2d", n_trajs=1, extra_seq_length=2)
        ds.magnitude_features = True
        dim, isl = len(ds.box), ds.input_seq_length
        homog = bool((ds[0][1] == 0).all())
        model = SEGNN(node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog), "1x1o+1x0e", 64, 1, 1, "1x1o",
                      num_mp_steps=10, n_vels=isl - 1, homogeneous_particles=homog)
        params = model.init_params(1234)
        case = hip_case(ds)
        pos, pt = ds[0]
        feats, _ = case.allocate_eval((pos[None, :, :isl], pt[None]))
        eng = feats.engine
        E, N, K = eng.stats()["n_edges_total"], len(pt), 10
        th = model.train_handle(eng, params)
        target = torch.randn((1, N, dim), generator=torch.Generator().manual_seed(5)).to(device)
        for _ in range(2):
            th.zero_grad()
            th.loss_grad(target, 1.0)
            th.adamw_step(1e-4)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(K):
            th.zero_grad()
            loss = th.loss_grad(target, 1.0)
            th.adamw_step(1e-4)
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t0) / K
        # flops EXECUTED: every tensor product is a (4 rows per row) x Kp x 128 product, forward + dW + dZ
        fwd = sum(2 * 4 * (E if name.split("/")[-1].startswith("message") else N) * ((Kb + 15) // 16 * 16) * 128
                  for name, Kb, _, _ in model.block_shapes())
        tf = 3 * fwd / dt / 1e12
        res.append({"workload": "dam2d SEGNN-10-64 training step (B = 1)", "n_particles": int(N), "edges": int(E), "steps": K,
                    "ms_per_step": 1e3 * dt, "value": N / dt, "unit": "particle-steps/s", "loss": float(loss), "dtype": _train_dtype(),
                    "roofline": {"kernel": "k_lin32 / k_lin32h + k_dw_part / k_dw_part_h on the stacked tensor-product operands (lb_train_segnn.h)", "bound": "mfma",
                                 "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                                 "flop_per_step": int(3 * fwd),
                                 "note": "executed flops (2x the necessary ones: cross terms of the side-by-side operand), whole step against the fp32 MFMA peak"}})
        th.close()
        del eng, feats
    except Exception as exc:
        res.append({"workload": "dam2d segnn", "error": repr(exc)[:200]})
    return res


OTHER_PLAN = [("tgv3d", "gns", 8, 20, 1.0, "tgv3d_drifting"),
              ("tgv2d", "gns", 1, 20, 1.0), ("tgv2d", "gns", 8, 20, 1.0), ("rpf2d", "gns", 1, 400, 1.0),
              ("tgv3d", "gns", 1, 20, 1.0), ("ldc3d", "gns", 1, 20, 1.0), ("ldc3d", "gns", 8, 20, 1.0),
              ("dam2d", "segnn", 1, 20, 1.0), ("dam2d", "segnn", 8, 20, 1.0)]
# `value` of rounds 1 - 5 was quoted on the DRIFTING TGV3D x 8 workload (vel_amp 1.0: 13.6 -> 18.5 -> 17.1 neighbours per
# particle over the rollout, mean 16.2); round 6 moves `value` to the stationary trajectories and keeps
# the drifting run as other_configs[tag == "tgv3d_drifting"], the driver's round-5 figure beside it
ROUND5_DRIFTING = {"value": 19249472.69, "ms_per_step": 3.3248, "source": "BENCH_r05.json (driver run, round 5)"}
# the headline workload (and config 5) on trajectories whose neighbour count does NOT drift over the rollout: velocities
# scaled down so that the ballistic rollout of untrained weights stays within half a spacing of the lattice
# (lagrangebench_amd/data/synthetic.py: vel_amp); TGV3D then holds 14.4 neighbours per particle over all steps
STATIONARY_PLAN = [("tgv3d", "gns", 1, 20, 0.03), ("dam2d", "segnn", 8, 20, 0.03)]


def other_configs(device, plan=None, repeats=1):
    """Short runs of the other BASELINE.json configs (configs[0], [1], [3], [4]) so that the driver's
    single bench line carries them too: same step definition and timing (barrier + synchronize on both
    sides of K steps, inputs resident), one line per (workload, batch).  Also used for the `stationary` lines
    (STATIONARY_PLAN; `repeats` timed regions, the median reported)."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS, SEGNN, node_irreps
    res = []
    for item in (plan or OTHER_PLAN):
        workload, kind, B, K, vel_amp = item[:5]
        tag = item[5] if len(item) > 5 else None
        try:
            ds = make_case(workload, n_trajs=B, extra_seq_length=K, vel_amp=vel_amp)
            dim, isl = len(ds.box), ds.input_seq_length
            if kind == "gns":
                model = GNS(dim, D, 2, 10, 16)
                node_in, edge_in = gns_widths(ds)
                params = model.init_params(1234, node_in, edge_in, decoder_scale=0.01)
            else:
                ds.magnitude_features = True
                homog = bool(np.all(ds[0][1] == 0))
                irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog)
                model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=10, n_vels=isl - 1,
                              homogeneous_particles=homog)
                params = model.init_params(1234)
                params["output"]["wv"] = (params["output"]["wv"] * 0.01).astype(np.float32)
            case = hip_case(ds)
            pos = np.stack([ds[i][0] for i in range(B)])
            pt = np.stack([ds[i][1] for i in range(B)])
            eng = case.engine(B)
            eng.set_particle_type(pt)
            traj = eng.prepare_traj(pos)
            handle = model.handle(eng, params)
            eng.rollout(handle, traj, K)  # warm-up: same rollout (capacities grown)
            dts = []
            for _ in range(max(1, repeats)):
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                _, n_realloc = eng.rollout(handle, traj, K)
                torch.cuda.synchronize(device)
                dts.append(time.perf_counter() - t0)
            dt = float(np.median(dts))
            N = pos.shape[1]
            entry = {"workload": f"{workload} {'GNS-10-128' if kind == 'gns' else 'SEGNN-10-64'}", "n_particles": int(N),
                     "batch": B, "steps": K, "ms_per_step": round(1e3 * dt / K, 4),
                     "value": B * N * K / dt, "unit": "particle-steps/s", "n_realloc": int(n_realloc),
                     "math_fallbacks": int(eng.math_fallbacks())}
            if vel_amp != 1.0:
                entry["vel_amp"] = vel_amp
            if tag:
                entry["tag"] = tag
            if tag == "tgv3d_drifting":
                entry["round5"] = ROUND5_DRIFTING
                entry["note"] = ("the workload `value` was quoted on in rounds 1 - 5: untrained weights at the datasets' velocity "
                                 "scale compress the lattice, the neighbour count drifts")
            if repeats > 1:
                entry["ms_per_step_all"] = [round(1e3 * x / K, 4) for x in dts]
            # this entry's own roofline: the processor edge (GNS) / message (SEGNN) kernel on the engine's HIP-event
            # timers over min(K, 20) more steps
            try:
                Kt = min(K, 20)
                eng.timers_enable(True)
                eng.timers_reset()
                eng.edge_accounting(reset=True)
                eng.rollout(handle, traj, Kt)
                tm = eng.timers()
                eng.timers_enable(False)
                acct = eng.edge_accounting(reset=True)
                E_tot = acct["mean"]   # mean real E of the Kt steps the timers cover (not the last step's)
                entry["edges_per_traj"] = {"first": int(acct["first"] // B), "mean": round(E_tot / B, 1),
                                           "last": int(acct["last"] // B)}
                ms_e, n_e = tm["edge_mlp"]
                if n_e == 0 and tm.get("processor", (0, 0))[1] > 0:  # persistent launch: one layer's share (edge + node)
                    ms_e, n_e = tm["processor"][0], tm["processor"][1] * 10
                us = 1e3 * ms_e / max(n_e, 1)
                if kind == "gns":
                    byts = int(round(E_tot * (2 * D * 4 + 8))) + B * N * (2 * D * 4)
                    entry["roofline"] = {"kernel": eng.kernel_names()["edge"], "node_kernel": eng.kernel_names()["node"],
                                         "bound": "hbm", "us_per_launch": round(us, 2), "bytes_per_launch": int(byts),
                                         "achieved": byts / (us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": byts / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                         "note": ("B = 1 graphs are launch-latency bound, not bandwidth bound" if B == 1 else
                                                  "bytes from the mean real E of the timed steps")}
                    ms_l, n_l = tm.get("edge_mlp_last", (0.0, 0))
                    if n_l > 0:
                        us_l = 1e3 * ms_l / n_l
                        byts_l = int(round(E_tot * (D * 4 + 8))) + B * N * (2 * D * 4)
                        entry["roofline"]["last_layer_variant"] = {
                            "us_per_launch": round(us_l, 2), "bytes_per_launch": byts_l,
                            "frac": byts_l / (us_l * 1e-6) / 1e9 / HBM_PEAK_GBS}
                else:
                    fl = int(round(sg_msg_flops(E_tot, len(ds.box))))
                    entry["roofline"] = {"kernel": "k_sg_msg (gather + 2 gated TP blocks + segment_sum, f16x2)",
                                         "bound": "mfma", "us_per_launch": round(us, 2),
                                         "achieved": fl / (us * 1e-6) / 1e12, "peak": MFMA_F16_PEAK_TF,
                                         "unit": "TFLOP/s", "frac": fl / (us * 1e-6) / 1e12 / MFMA_F16_PEAK_TF}
                entry["breakdown_ms_per_step"] = {k: round(v[0] / Kt, 4) for k, v in tm.items() if v[1] > 0}
            except Exception as exc:
                entry["roofline"] = {"error": repr(exc)[:200]}
            res.append(entry)
            del eng, traj, handle
        except Exception as exc:  # a sub-run must never take the headline line down
            res.append({"workload": workload, "batch": B, "error": repr(exc)[:200]})
    return res


def run_segnn(args, rank, world, device):
    """configs[4]: SEGNN-10-64 (lmax 1) rollout.  Same step definition and timing contract as the
    GNS line; the dominant kernel is the message tensor-product block pair (fp32 MFMA bound)."""
    from lagrangebench_amd import dist as lbdist
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import SEGNN, node_irreps

    B, K, W, L = args.batch, args.steps, args.warmup, args.mp_steps
    ds = make_case(args.workload, n_trajs=world * B, extra_seq_length=max(K, W, 1))
    ds.magnitude_features = True  # configs/*/segnn.yaml
    isl = ds.input_seq_length
    homog = bool(np.all(ds[0][1] == 0))
    irr = node_irreps(ds.metadata, isl, ds.external_force_fn is not None, True, homog)
    model = SEGNN(irr, "1x1o+1x0e", 64, 1, 1, "1x1o", num_mp_steps=L, n_vels=isl - 1, homogeneous_particles=homog)
    params = model.init_params(1234)  # U(-1,1) under e3nn's "element" normalisation (segnn.py:30-41)
    params["output"]["wv"] = (params["output"]["wv"] * 0.01).astype(np.float32)
    case = hip_case(ds)
    mine = [rank * B + i for i in range(B)]
    pos = np.stack([ds[i][0] for i in mine])
    pt = np.stack([ds[i][1] for i in mine])
    N = pos.shape[1]
    eng = case.engine(B)
    eng.set_particle_type(pt)
    traj = eng.prepare_traj(pos)
    handle = model.handle(eng, params)
    if W < K:
        eng.rollout(handle, traj, K)  # allocation pass, see the GNS path
    eng.rollout(handle, traj, max(W, 1))
    lbdist.barrier(device)
    t0 = time.perf_counter()
    pred, n_realloc = eng.rollout(handle, traj, K)
    lbdist.barrier(device)
    dt = lbdist.max_over_ranks(time.perf_counter() - t0, device)
    E_last = eng.stats()["n_edges_total"]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [("pred_last_step", pred[:, -1].cpu().numpy()), ("pred", pred.cpu().numpy())])

    def headline(edges):
        """The line of a plain run; `edges`: the config's edge figures (--full: those of the HIP-event pass)."""
        return {
            "metric": "rollout particle-steps/sec", "value": world * B * N * K / dt, "unit": "particle-steps/s",
            "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": 1e3 * dt / K, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.workload} SEGNN-{L}-64 (lmax 1) inference rollout, neighbor list rebuilt every step",
                       "n_particles": int(N), "batch_per_gpu": B, **edges,
                       "input_seq_length": isl, "geometry_dtype": "f64", "network_math": "f32",
                       "weights": "U(-1,1) e3nn-style init (seed 1234), output x0.01", "n_realloc": int(n_realloc)},
            "steps_per_s_per_traj": K / dt,
        }

    if not args.full:
        if rank == 0:
            print(json.dumps(headline({"edges_per_traj_last": int(E_last // B)})), flush=True)
        return
    eng.timers_enable(True)
    eng.timers_reset()
    eng.edge_accounting(reset=True)
    eng.rollout(handle, traj, K)
    tm = eng.timers()
    eng.timers_enable(False)
    acct_tm = eng.edge_accounting(reset=True)
    E_tot = acct_tm["mean"]   # mean real E of the K steps the timers cover
    if rank != 0:
        return
    ms_msg, n_msg = tm["edge_mlp"]  # one record per layer = the two gated message blocks
    us_msg = 1e3 * ms_msg / max(n_msg, 1)
    C = 32
    fused = tm["aggregate"][1] == 0
    flop_algo = int(round(E_tot * 2 * (130 + 64) * (2 * C + 3 * C)))   # reference formulation: TP + Linear, two blocks
    if fused:
        # k_sg_msg (f16x2): products actually executed per edge (s W_v^s computed once instead of 3x):
        # block 0: 128x64 + 64x32 + 3*64x32, block 1: 64x64 + 32x32 + 3*32x32; x3 split passes
        # (round 4: the vector products run on `dim` components - in 2D the z component is identically zero in the
        # reference too and is skipped: 126 instead of 144 MFMAs per 16-edge tile)
        flop_exec = int(round(sg_msg_flops(E_tot, len(ds.box))))
        peak, kname = MFMA_F16_PEAK_TF, "k_sg_msg (gather + 2 gated TP blocks + segment_sum, f16x2)"
        msg_bytes = int(round(E_tot * (2 * 512 + 40))) + B * N * 512   # two node rows per edge (L2/MALL), one row per receiver
    else:
        flop_exec = int(round(E_tot * 2 * (136 + 64) * (2 * C + 3 * C)))    # K padded to 136 / 64, fp32 MFMA
        peak, kname = MFMA_F32_PEAK_TF, "k_sg_tp<GATE> x2 (message blocks of one layer, fp32 MFMA)"
        msg_bytes = int(round(E_tot * (2 * 512 + 512 + 512 + 512 + 16 + 64 + 8)))
    tf = flop_exec / (us_msg * 1e-6) / 1e12
    out = headline({"edges_per_traj": int(round(E_tot / B)), "edges_per_traj_first": int(acct_tm["first"] // B),
                    "edges_per_traj_mean": round(E_tot / B, 1), "edges_per_traj_last": int(E_last // B)})
    out.update({
        "roofline": {"kernel": kname, "bound": "mfma", "achieved": tf,
                     "peak": peak, "unit": "TFLOP/s", "frac": tf / peak,
                     "traffic": pmc_traffic("k_sg_msg", "segnn_" + args.workload, B),
                     "us_per_launch": us_msg, "launches": int(n_msg), "flop_per_launch_executed": flop_exec,
                     "flop_per_launch_algorithmic": flop_algo,
                     "fp32_equivalent_algorithmic_tflops": flop_algo / (us_msg * 1e-6) / 1e12,
                     "gather": {"achieved": msg_bytes / (us_msg * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "note": "node rows gathered per edge (mostly L2/MALL hits) + rows written"}},
        "breakdown_ms_per_step": {k: round(v[0] / K, 4) for k, v in tm.items() if v[1] > 0},
    })
    print(json.dumps(out), flush=True)


CPU_PLAN = {
    # config 1 (TGV2D-2.5k, 20 steps) is mandatory; TGV3D-8k (the config the >= 5x target is quoted on)
    # costs ~1.8 s per step on this host: a bounded sample.  One rollout of warm + steps steps, every step timed
    # (the reference's step loop is host driven, rollout.py:125-169); the reported figure is the MEDIAN step.
    # (round 6: 8 + 3 timed steps instead of 20 + 5, one warm-up step each: ~12 s of CPU work incl. the leg process's start-up
    # and list allocation, bench wall <= 20 s)
    "tgv2d": {"steps": 8, "warm": 1},
    "tgv3d": {"steps": 3, "warm": 1},
}


def cpu_model_string():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline_leg(workload, L, vel_amp=1.0):
    """One CPU-baseline leg (own process, `--cpu-baseline-only`): the CPU restatement in the reference's algorithmic
    shape (dense candidate matrix -> mask -> compaction; MLPs over all E_cap padded rows; unfused
    gather / GEMM / LayerNorm / scatter-add; fp64 geometry, fp32 network; batch 1): torch-CPU for the network
    (oracle/lb_oracle_torch.py), NumPy for the neighbor list / features / integrator."""
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import GNS
    from oracle import lb_oracle as O
    from oracle import lb_oracle_torch as OT
    from tests._common import oracle_case
    plan = CPU_PLAN[workload]
    # threads: torch-CPU on the MI355X host (256 hardware threads) is fastest at 32 threads and collapses when
    # oversubscribed (tools/cpu_threads_probe.py: 4/8/16/32/64/256 threads -> 2.6/2.0/1.8/1.6/2.5/47 s per TGV3D
    # forward); "cores" reports the threads actually used
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    n_warm, n_steps = plan["warm"], plan["steps"]
    ds = make_case(workload, n_trajs=1, extra_seq_length=n_warm + n_steps, vel_amp=vel_amp)
    node_in, edge_in = gns_widths(ds)
    params = GNS(len(ds.box), D, 2, L, 16).init_params(1234, node_in, edge_in, decoder_scale=0.01)
    ocase = oracle_case(ds)
    isl = ds.input_seq_length
    pos, pt = ds[0]
    pos = pos.astype(np.float64)
    pt_params = OT.params_to_torch(params)
    stamps = []

    def apply(p, s, sample):
        stamps.append(time.perf_counter())  # one call per rollout step, after that step's neighbor list / features
        return OT.gns_apply(pt_params, sample[0], sample[1], num_mp_steps=L), s

    _, nbrs = ocase.allocate_eval((pos[:, :isl], pt))
    t_begin = time.perf_counter()
    O.eval_batched_rollout(apply, ocase, params, {}, (pos[None, :, :isl + n_warm + n_steps], pt[None]), nbrs,
                           n_warm + n_steps, isl)
    t_end = time.perf_counter()
    # step i runs from (roughly) stamp[i] - its preprocessing to stamp[i+1] - the next one's: consecutive stamp
    # differences are whole steps (network of step i + integrator + neighbor list / features of step i+1)
    edges = stamps + [t_end]
    steps = np.diff(np.asarray(edges))[n_warm:]
    dt = float(np.median(steps))
    return {
        "workload": workload, "value": len(pt) / dt, "unit": "particle-steps/s", "cores": cores,
        "cpu_model": cpu_model_string(), "host_threads": os.cpu_count(), "kind": "port",
        "ms_per_step": 1e3 * dt, "ms_per_step_all": [round(1e3 * float(t), 1) for t in steps],
        "ms_per_step_min": round(1e3 * float(steps.min()), 1), "ms_per_step_max": round(1e3 * float(steps.max()), 1),
        "total_s": round(t_end - t_begin, 2),
        "sample": f"median step of a {n_steps}-step rollout of 1 {ds.name} trajectory (N={len(pt)}) after {n_warm} warm-up "
                  f"steps; torch-CPU network + NumPy neighbor list in the reference's padded/unfused shape",
    }


def cpu_baseline_start(args):
    """Start the CPU-baseline legs as ONE background process (host cores only; meanwhile the nested rocprofv3 passes -
    byte counters, nothing timed - re-run the GPU workload)."""
    import subprocess
    legs = ["tgv2d"] + ([args.workload] if args.workload in CPU_PLAN and args.workload != "tgv2d" else ["tgv3d"])
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", ",".join(legs), "--mp-steps", str(args.mp_steps),
           "--vel-amp", str(args.vel_amp)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    return legs, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True,
                                  start_new_session=True)


def cpu_baseline_collect(job, timeout_s=240):
    """cpu_baseline object of the bench line: the headline workload's leg on top, every leg under `configs`."""
    import signal
    names, p = job
    try:
        out, _ = p.communicate(timeout=timeout_s)
        legs = json.loads(out.strip().splitlines()[-1])
    except Exception as exc:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except Exception:
            pass
        legs = {w: {"workload": w, "error": repr(exc)[:200]} for w in names}
    head = next((legs[w] for w in ("tgv3d", "ldc3d", "rpf2d", "tgv2d") if w in legs and "value" in legs[w]), None)
    res = dict(head) if head else {"value": None, "unit": "particle-steps/s", "cores": None, "kind": "port", "sample": "failed"}
    res["configs"] = legs
    res["note"] = ("JAX is not installable here: this is the reference-shaped CPU restatement, not JAX-CPU; the legs "
                   "run one after the other in their own process with nothing else on the host (the GPU work of this "
                   "command is finished, the opt-in PMC passes have not started); spread in ms_per_step_min / _max")
    return res


if __name__ == "__main__":
    main()
