"""Every build route of csrc/lb_neighbor.hip (lbk_nl_build, lb_launch_nl) on the point clouds of tests/_nl_clouds.py: genuine
fp64 positions, pairs within two ulps of the cutoff, particles on cell faces.  Each case asserts WHICH route it reached
(Engine.nl_route) and compares the list, the edge features, the flags and the capacities with the all-pairs reference and the
oracle, bit for bit.  tests/test_nl_routes.py holds the premises (CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from tests import _nl_clouds as C  # noqa: E402
from tests._common import hip_case  # noqa: E402
from tests._nl_route_table import FUSED_OFF_CLOUDS, ROUTES, ROUTES_UNFUSED, SWEEP_CAPS, _fmt, _knl_cand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = os.environ.get("LB_SMALL_FUSED", "1") != "0"


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


CASES = [(cid, f32, B) for cid in C.SPECS for f32 in (False, True) for B in C.BATCHES[cid]]
IDS = [f"{cid}-{'f32' if f32 else 'f64'}-B{B}" for cid, f32, B in CASES]


def _check_build(R, f32, feats, nbrs, t, what):
    """List, padding, edge count, edge features and flags of one build against the reference of window t, per trajectory."""
    idx_all, ne_all = _np(nbrs.idx), _np(nbrs.n_edges)
    rd, rdist = _np(feats["rel_disp"]), _np(feats["rel_dist"])
    flags = _np(nbrs.did_buffer_overflow)
    cast = (lambda x: x.astype(np.float32)) if f32 else (lambda x: x)
    for b in range(R.B):
        want = R.edges[b, t]
        ne = want.shape[1]
        assert int(ne_all[b]) == ne, (what, b, int(ne_all[b]), ne)
        assert np.array_equal(idx_all[b][:, :ne], want), (what, b, "edge list")
        assert (idx_all[b][:, ne:] == R.N).all(), (what, b, "padding")
        assert np.array_equal(cast(rd[b][:ne]), R.feats[b, t]["rel_disp"]), (what, b, "rel_disp")
        assert np.array_equal(cast(rdist[b][:ne]), R.feats[b, t]["rel_dist"]), (what, b, "rel_dist")
        if f32:
            assert np.array_equal(rd[b][:ne], cast(rd[b][:ne]).astype(np.float64))
        assert (rd[b][ne:] == 0).all() and (rdist[b][ne:] == 0).all(), (what, b, "feature padding")
        assert not bool(flags[b]) and not R.overflow[b, t], (what, b, "did_buffer_overflow")


@pytest.mark.parametrize("cid,f32,B", CASES, ids=IDS)
def test_route_and_list_bitexact(cid, f32, B):
    """allocate_eval, then two preprocess_eval updates on later frames: after each build the route is the table's, and
    n_edges, the edge list with its == N padding, rel_disp, rel_dist and did_buffer_overflow equal the reference bit for bit
    in every trajectory; cell_capacity and e_cap of the allocation equal the oracle's."""
    R = C.reference(cid, f32, B)
    g = R.g
    hcase = hip_case(R.ds, dtype="float32" if f32 else "float64")
    sample = lambda t: (R.pos[:, :, t:t + C.ISL], R.pt)
    feats, nbrs = hcase.allocate_eval(sample(0))
    eng = hcase.engine(B)
    routes = [eng.nl_route()]
    _check_build(R, f32, feats, nbrs, 0, "allocate")
    assert nbrs.cell_capacity == R.batch_cell_capacity, (nbrs.cell_capacity, R.batch_cell_capacity)
    assert nbrs.max_occupancy == R.batch_e_cap, (nbrs.max_occupancy, R.e_cap)
    for t in C.FRAMES[1:]:
        feats, nbrs = hcase.preprocess_eval(sample(t), nbrs)
        routes.append(eng.nl_route())
        _check_build(R, f32, feats, nbrs, t, f"update {t}")
    got = (_fmt(routes[0]), _fmt(routes[1]))
    print(f"ROUTE {cid} {'f32' if f32 else 'f64'} B={B} fused={int(FUSED)}: {got[0]} || {got[1]}")
    for r in routes:
        assert (r["f32"], r["dim"], r["cell_list"]) == (int(f32), g.dim, int(g.use_cells)), r
        assert r["dense"] == int(bool(C.SPECS[cid].get("clump") or C.SPECS[cid].get("dense"))), r
    assert _fmt(routes[2]) == got[1], "both updates take one route"
    assert got == (ROUTES if FUSED else ROUTES_UNFUSED)[cid, "f32" if f32 else "f64", B]


CELL_CASES = [c for c in CASES if C.geometry(c[0]).use_cells]


@pytest.mark.parametrize("cid,f32,B", CELL_CASES, ids=[i for c, i in zip(CASES, IDS) if c in CELL_CASES])
def test_cell_overflow_flag_per_trajectory(cid, f32, B):
    """The frozen cell capacity set to the oracle's largest occupancy on the last window: no overflow.  One below it:
    did_buffer_overflow in every trajectory the oracle flags and in no other (the list is unspecified then: flags only).

    The engine keeps one largest occupancy per batch (lb_ctrl.max_cell_occ); when that exceeds the capacity the finish kernels
    re-count every trajectory's own from the bins (lb_traj_cell_occ)."""
    R = C.reference(cid, f32, B)
    hcase = hip_case(R.ds, dtype="float32" if f32 else "float64")
    t = C.FRAMES[-1]
    _, nbrs = hcase.allocate_eval((R.pos[:, :, t:t + C.ISL], R.pt))
    eng = hcase.engine(B)
    occ = [R.occ[b, t] for b in range(B)]
    for cap in (max(occ), max(occ) - 1):     # (in this order: an overflow stops the engine until the next allocation)
        eng.nl_set_capacity(cap, eng.e_cap)
        eng.nl_update()
        flags = [int(v) for v in _np(eng.nl_flags())]
        print(f"FLAGS {cid} {'f32' if f32 else 'f64'} B={B} capacity {cap} occupancies {occ}: {flags}")
        assert flags == [int(o > cap) for o in occ], (cap, occ)


def _sweep(cid, B, caps, expect):
    """Updates of one window under every frozen cell capacity of `caps` (e_cap unchanged; none is below a trajectory's fullest
    cell): no flag, the list and the features of the update at the allocation's own capacity every time, and the route
    `expect(cap)`."""
    R = C.reference(cid, False, B)
    hcase = hip_case(R.ds)
    t = C.FRAMES[-1]
    _, nbrs = hcase.allocate_eval((R.pos[:, :, :C.ISL], R.pt))
    eng = hcase.engine(B)
    e_cap = eng.e_cap
    feats, nbrs = hcase.preprocess_eval((R.pos[:, :, t:t + C.ISL], R.pt), nbrs)
    _check_build(R, False, feats, nbrs, t, "native capacity")
    base = (_np(nbrs.idx), _np(nbrs.n_edges), _np(feats["rel_disp"]), _np(feats["rel_dist"]))
    assert max(R.occ[b, t] for b in range(B)) <= min(caps)
    seen = []
    for cap in caps:
        eng.nl_set_capacity(cap, e_cap)
        eng.nl_update()
        seen.append(_fmt(eng.nl_route()))
        assert not _np(eng.nl_flags()).any(), cap
        idx, ne = eng.nl_idx()
        ef = eng.edge_features()
        for b in range(B):
            assert int(_np(ne)[b]) == int(base[1][b]) and np.array_equal(_np(idx)[b], base[0][b]), (cap, b)
            assert np.array_equal(_np(ef["rel_disp"])[b], base[2][b]) and np.array_equal(_np(ef["rel_dist"])[b][:, 0:1], base[3][b]), (cap, b)
    print(f"SWEEP {cid} B={B}: {list(zip(caps, seen))}")
    assert seen == [expect(c) for c in caps]


def test_capacity_sweep_reaches_every_staged_capacity_of_k_nl():
    """`small2d`, fp64, B = 3: cell capacities 14 .. 120 walk k_nl<NL_ROWS, 64, C> through C = 128, 256, .., 1024 and on to
    the 256-thread 2048-candidate variant; the list and the features never change."""
    assert FUSED
    _sweep("small2d", 3, SWEEP_CAPS, lambda c: f"strided > rows k_nl[{_knl_cand(c)}] > compact_scan")
    assert [_knl_cand(c) for c in SWEEP_CAPS] == [128, 256, 384, 512, 640, 768, 896, 1024, 2048]


def test_capacity_sweep_hands_the_single_launch_build_over():
    """B = 1: k_nl_small takes the build while capacity * 9 <= 512 candidates fit its row buffer; beyond that the multi-launch
    route (fixed-stride bins, k_nl, fused scan + compaction) does.  3D: beyond 512 / 27 the hand-over is to k_nlc."""
    assert FUSED
    _sweep("small2d", 1, SWEEP_CAPS,
           lambda c: "k_nl_small" if c * 9 <= 512 else f"strided > rows k_nl[{_knl_cand(c)}] > compact_scan")
    _sweep("small3d", 1, (18, 19, 40), lambda c: "k_nl_small" if c * 27 <= 512 else "strided > rows k_nlc > compact_scan")


def test_routes_without_the_fused_launches():
    """LB_SMALL_FUSED=0 (read once per process): the tiny, small and all-pairs cases in a fresh process - no single-launch
    build, counting-sort bins, separate scan / finish / compaction - against the table's second column."""
    sel = "test_route_and_list_bitexact and (" + " or ".join(f"{c}-" for c in FUSED_OFF_CLOUDS) + ")"
    n = sum(1 for cid, _, _ in CASES if cid in FUSED_OFF_CLOUDS)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_nl_routes_gpu.py", "-m", "gpu", "-q", "-k", sel,
                        "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, LB_SMALL_FUSED="0"), capture_output=True,
                       text=True, timeout=300)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    assert r.returncode == 0, tail
    assert f"{n} passed" in r.stdout and "failed" not in r.stdout, tail
