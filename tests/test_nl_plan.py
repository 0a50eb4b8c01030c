"""The routing of the neighbor-list build (csrc/lb_nl_plan.h) without a GPU: tools/nl_plan_check.cpp, a host-only program,
prints the route lb_nl_route would report for the inputs it is given.  (a) every row of the route table that
tests/test_nl_routes_gpu.py asserts of the engine, from what tests/_nl_clouds.py computes on the CPU; (b) its capacity
sweeps; (c) every hand-over threshold from both sides, on synthetic inputs.  The thresholds are written out here as numbers:
a changed threshold in the header must fail (c), not move its case along."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _nl_clouds as C
from tests._nl_route_table import FUSED_OFF_CLOUDS, ROUTES, ROUTES_UNFUSED, SWEEP_CAPS, _fmt, _knl_cand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("B N dim f32 use_cell_list ncell0 ncell1 ncell2 ncells nstencil cell_capacity e_cap nl_dense nl_one_off wg_sum maxd "
          "tmp_send tmp_feat64 want_efeat64 fused max_stencil max_deg").split()
SEEN = set()   # every route any test of this module got


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """routes(cases) -> [_fmt route, its dict] per case, through one run of the check program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("nl_plan") / "nl_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "nl_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def routes(cases):
        text = "".join(" ".join(str(int(c[f])) for f in FIELDS) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases), r.stdout
        out = []
        for line in lines:   # (as Engine.nl_route reads the same text)
            kv = dict(p.split("=", 1) for p in line.split(";") if "=" in p)
            d = {k: int(v) if v.lstrip("-").isdigit() else v for k, v in kv.items()}
            out.append((_fmt(d), d))
            SEEN.add(out[-1][0])
        return out

    return routes


def _engine(dim, use_cells, ncell, N, B, f32, fused=1):
    """The geometry part of lb_nl_in as lb_engine_create sets it: without a cell list one "cell" per trajectory, a stencil of
    one, and the dense fall-back from the start above 2048 particles."""
    c = dict.fromkeys(FIELDS, 0)
    c.update(B=B, N=N, dim=dim, f32=f32, use_cell_list=use_cells, wg_sum=1, want_efeat64=1, fused=fused)
    nc = [int(v) for v in ncell] + [1] * (3 - len(ncell)) if use_cells else [1, 1, 1]
    c.update(ncell0=nc[0], ncell1=nc[1], ncell2=nc[2], ncells=int(np.prod(nc)), nstencil=(3 ** dim if use_cells else 1),
             nl_dense=int(not use_cells and N > 2048))
    return c


def _frozen(c, cell_capacity, e_cap, max_deg, dense):
    """c after lb_nl_allocate: capacities frozen, per-node slots (twice the largest degree, at least 16) and row buffers there."""
    maxd = min(max(16, (2 * max_deg + 7) // 8 * 8), 4096 if dense else 256)
    return dict(c, cell_capacity=cell_capacity, e_cap=e_cap, nl_dense=dense, maxd=maxd, tmp_send=1, tmp_feat64=1)


def _cloud_case(cid, f32, B, fused=1):
    """The allocation on window 0 of the first B trajectories of a cloud, and what its count sweep reads back."""
    R = C.reference(cid, f32, max(C.BATCHES[cid]))
    g = R.g
    c = _engine(g.dim, g.use_cells, g.ncell if g.use_cells else (), R.N, B, int(f32), fused)
    max_deg = max(int(np.bincount(R.edges[b, 0][0]).max()) for b in range(B))
    if g.use_cells:   # the fullest stencil of a non-empty cell (the stencil wraps, periodic box or not)
        max_stencil = 0
        for b in range(B):
            x = R.pos[b][:R.n_real[b], C.ISL - 1].astype(g.dt)
            occ = np.bincount(g.hashes(x), minlength=g.ncells).reshape([int(v) for v in g.ncell[::-1]])
            sten = sum(np.roll(occ, [s - 1 for s in sh], axis=tuple(range(g.dim))) for sh in np.ndindex(*(3,) * g.dim))
            max_stencil = max(max_stencil, int(sten[occ > 0].max()))
    else:
        max_stencil = max(R.n_real[:B])
    cap = int(max(R.occ[b, 0] for b in range(B)) * R.ds.multiplier) if g.use_cells else 0
    return dict(c, max_stencil=max_stencil, max_deg=max_deg), cap, max(R.e_cap[:B]), max_deg


CASES = [(cid, f32, B) for cid in C.SPECS for f32 in (False, True) for B in C.BATCHES[cid]]


def test_route_table(plan):
    """(a) allocation and update route of every (cloud, dtype, B) equal the table's, fused and under LB_SMALL_FUSED=0."""
    assert set(ROUTES) == {(cid, "f32" if f32 else "f64", B) for cid, f32, B in CASES}
    for fused, table in ((1, ROUTES), (0, ROUTES_UNFUSED)):
        todo = [c for c in CASES if fused or c[0] in FUSED_OFF_CLOUDS]
        assert len(todo) == len(table)
        allocs = [_cloud_case(cid, f32, B, fused) for cid, f32, B in todo]
        got_a = plan([a[0] for a in allocs])
        updates = [_frozen(a[0], a[1], a[2], a[3], ga[1]["dense"]) for a, ga in zip(allocs, got_a)]
        got_u = plan(updates)
        for (cid, f32, B), a, ga, gu in zip(todo, allocs, got_a, got_u):
            spec = C.SPECS[cid]
            if spec.get("clump"):
                assert a[0]["max_deg"] > 256 and a[0]["max_stencil"] <= 2048
            else:
                assert (a[0]["max_stencil"] > 2048) == bool(spec.get("dense")), (cid, a[0]["max_stencil"])
            assert ga[1]["dense"] == gu[1]["dense"] == int(bool(spec.get("clump") or spec.get("dense"))), (cid, f32, B)
            for r in (ga[1], gu[1]):
                assert (r["f32"], r["dim"], r["cell_list"]) == (int(f32), spec["dim"], a[0]["use_cell_list"])
            assert (ga[0], gu[0]) == table[cid, "f32" if f32 else "f64", B], (cid, f32, B, fused)


def test_capacity_sweeps(plan):
    """(b) the sweeps of test_nl_routes_gpu.py: small2d at B = 3 walks k_nl's staged capacities, at B = 1 hands the build over
    from k_nl_small beyond 512 candidates; small3d at B = 1 hands it over to k_nlc."""
    def sweep(cid, B, caps):
        c, _, e_cap, max_deg = _cloud_case(cid, False, B)
        return [r[0] for r in plan([_frozen(c, cap, e_cap, max_deg, 0) for cap in caps])]

    multi = lambda c: f"strided > rows k_nl[{_knl_cand(c)}] > compact_scan"
    assert sweep("small2d", 3, SWEEP_CAPS) == [multi(c) for c in SWEEP_CAPS]
    assert [_knl_cand(c) for c in SWEEP_CAPS] == [128, 256, 384, 512, 640, 768, 896, 1024, 2048]
    assert sweep("small2d", 1, SWEEP_CAPS) == ["k_nl_small" if c * 9 <= 512 else multi(c) for c in SWEEP_CAPS]
    assert sweep("small3d", 1, (18, 19, 40)) == ["k_nl_small", "strided > rows k_nlc > compact_scan",
                                                 "strided > rows k_nlc > compact_scan"]


def _upd(**kw):
    """An update of a 2D fp64 batch with a 10 x 10 cell list: 2 x 1000 particles, 20 * 9 = 180 candidates per stencil."""
    c = _frozen(_engine(2, 1, (10, 10), 1000, 2, 0), 20, 100, 16, 0)
    return dict(c, **kw)


def _alloc(**kw):
    return dict(_engine(2, 1, (10, 10), 1000, 1, 0), **kw)


U = "strided > rows k_nl[256] > compact_scan"
A_SMALL, A_SORT = "cells_small > count {k} > rows_small > fill {k}", "sort > count {k} > scan+finish > fill {k}"
K = "k_nl[2048]"
# name: (the threshold, the case at it, its route, the case one past it, its route)
BOUNDARIES = {
    "LB_SMALL_N nodes, allocation": (_alloc(N=4096), A_SMALL.format(k=K), _alloc(N=4097), A_SORT.format(k=K)),
    "LB_SMALL_N cells, allocation": (_alloc(ncells=4096), A_SMALL.format(k=K),
                                     _alloc(ncells=4097), "sort > count k_nl[2048] > rows_small > fill k_nl[2048]"),
    "LB_SMALL_N nodes, dense update": (_upd(N=2048, nl_dense=1), "cells_small > rows k_nlw > compact_scan",
                                       _upd(N=2049, nl_dense=1), "cells_traj > rows k_nlw > compact_scan"),
    "LB_SMALL_N nodes, rows_small": (_upd(N=2048, maxd=0), "strided > count k_nl[256] > rows_small > fill k_nl[256]",
                                     _upd(N=2049, maxd=0), "strided > count k_nl[256] > scan+finish > fill k_nl[256]"),
    "LB_SMALL_N, one trajectory": (_upd(B=1, N=4096), "k_nl_small", _upd(B=1, N=4097), "k_nl_mid"),
    "LB_CSCAN_N": (_upd(B=1, N=16384), U, _upd(B=1, N=16385), "strided > rows k_nl[256] > scan+finish+compact"),
    "64 trajectories": (_upd(B=64, N=100), U, _upd(B=65, N=100), "strided > rows k_nl[256] > scan+finish+compact"),
    "NLM_N": (_upd(B=1, N=8192), "k_nl_mid", _upd(B=1, N=8193), U),
    "6144 particles a trajectory": (_upd(N=6144, nl_dense=1), "cells_traj > rows k_nlw > compact_scan",
                                    _upd(N=6145, nl_dense=1), "sort > rows k_nlw > compact_scan"),
    "LB_CELLS1_NCELL, batch": (_upd(N=3000, nl_dense=1, ncells=32768), "cells_traj > rows k_nlw > compact_scan",
                               _upd(N=3000, nl_dense=1, ncells=32769), "sort > rows k_nlw > compact_scan"),
    "LB_CELLS1_NCELL, one trajectory": (_upd(B=1, N=5000, nl_dense=1, ncells=32768), "cells_mid > rows k_nlw > compact_scan",
                                        _upd(B=1, N=5000, nl_dense=1, ncells=32769), "sort > rows k_nlw > compact_scan"),
    "LB_CELLS1_N": (_upd(B=1, N=8192, nl_dense=1), "cells_mid > rows k_nlw > compact_scan",
                    _upd(B=1, N=8193, nl_dense=1), "sort > rows k_nlw > compact_scan"),
    # (a stencil of one cell: the plan reads the product alone, and 512 and 1024 are no multiples of 9 or 27)
    "NLS_CAND": (_upd(B=1, N=300, nstencil=1, cell_capacity=512), "k_nl_small",
                 _upd(B=1, N=300, nstencil=1, cell_capacity=513), "strided > rows k_nl[640] > compact_scan"),
    "NLM_ROWBUF - LB_MAX_ROW": (_upd(B=1, N=8000, nstencil=1, cell_capacity=768), "k_nl_mid",
                                _upd(B=1, N=8000, nstencil=1, cell_capacity=769), "strided > rows k_nl[896] > compact_scan"),
    "NL_SMALL_MAXC": (_upd(nstencil=1, cell_capacity=1024), "strided > rows k_nl[1024] > compact_scan",
                      _upd(nstencil=1, cell_capacity=1025), "strided > rows k_nl[2048] > compact_scan"),
    "2^30 cell slots": (_upd(nstencil=1, cell_capacity=1023, ncells=1 << 19), "strided > rows k_nl[1024] > compact_scan",
                        _upd(nstencil=1, cell_capacity=1024, ncells=1 << 19), "sort > rows k_nl[1024] > compact_scan"),
    "2048 cells along x": (_upd(B=1, N=300, ncell0=2047), "k_nl_small", _upd(B=1, N=300, ncell0=2048), U),
    "1024 cells along z": (_upd(B=1, N=300, dim=3, nstencil=27, cell_capacity=10, ncell2=1023), "k_nl_small",
                           _upd(B=1, N=300, dim=3, nstencil=27, cell_capacity=10, ncell2=1024),
                           "strided > rows k_nlc > compact_scan"),
    "nl_one_off": (_upd(B=1, N=300), "k_nl_small", _upd(B=1, N=300, nl_one_off=1), U),
    "nl_dense": (_upd(B=1, N=300), "k_nl_small", _upd(B=1, N=300, nl_dense=1), "cells_small > rows k_nlw > compact_scan"),
    "fused": (_upd(B=1, N=300), "k_nl_small", _upd(B=1, N=300, fused=0), "sort > rows k_nl[256] > scan+finish+compact"),
    "fused, batch": (_upd(), U, _upd(fused=0), "sort > rows k_nl[256] > scan+finish+compact"),
    "LB_MAX_ROW at the read-back": (_alloc(max_deg=256), A_SMALL.format(k=K),
                                    _alloc(max_deg=257), "cells_small > count k_nl[2048] > rows_small > fill k_nlw"),
    "LB_MAX_STENCIL_CAND at the read-back": (_alloc(max_stencil=2048), A_SMALL.format(k=K), _alloc(max_stencil=2049),
                                             A_SMALL.format(k="k_nlw") + " (again after k_nl)"),
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_threshold_from_both_sides(plan, name):
    """(c) the route at a threshold and the route one past it."""
    at, want_at, past, want_past = BOUNDARIES[name]
    got = [r[0] for r in plan([at, past])]
    assert got == [want_at, want_past], name
    assert want_at != want_past


def test_every_name_is_reached(plan):
    """Every binning, search kernel, single-launch build and finish that lb_nl_route can name came out of some case above."""
    plan([c for b in BOUNDARIES.values() for c in (b[0], b[2])])
    test_route_table(plan)
    words = " ".join(SEEN).replace("[", " ").replace(">", " ").split()
    for name in ("k_nl_small", "k_nl_mid", "strided", "cells_small", "cells_traj", "cells_mid", "sort", "k_nl", "k_nlw", "k_nlc",
                 "compact_scan", "rows_small", "scan+finish", "scan+finish+compact"):
        assert name in words, name
