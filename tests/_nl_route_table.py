"""The routes the neighbor-list build takes on the clouds of tests/_nl_clouds.py, as one-line strings: what
tests/test_nl_routes_gpu.py asserts of the engine (Engine.nl_route) and tests/test_nl_plan.py of the host-only plan
(csrc/lb_nl_plan.h through tools/nl_plan_check.cpp)."""


def _fmt(r):
    """A route (Engine.nl_route) in one line: the single-launch kernel, or binning > search > finish."""
    k = lambda name, cand: f"{name}[{cand}]" if cand else name
    if r["build"] != "multi":
        return r["build"]
    if r["mode"] == "rows":
        return f"{r['cells']} > rows {k(r['search'], r['cand'])} > {r['finish']}"
    s = f"{r['cells']} > count {k(r['count'], r['count_cand'])} > {r['finish']} > fill {k(r['search'], r['cand'])}"
    return s + (f" (again after {r['reentry']})" if r["reentry"] != "none" else "")


# (cloud, dtype, B) -> (allocation, update) as _fmt writes them, and under LB_SMALL_FUSED=0 for the clouds that
# test_routes_without_the_fused_launches runs.  Template instances follow from the case (f32, dim are asserted from the
# probe's own fields).
A_SMALL = "cells_small > count {k} > rows_small > fill {k}"   # allocation of <= LB_SMALL_N particles and cells
A_WIDE = "sort > count {k} > rows_small > fill {k}"           # ... of more cells than that
A_SORT = "sort > count {k} > scan+finish > fill {k}"          # ... of more particles; every allocation under LB_SMALL_FUSED=0
A_DENSE = "{c} > count {k} > {f} > fill k_nlw"                # the count sees a degree above 256: the fill runs the dense kernel
U_SCAN = "{c} > rows {k} > compact_scan"
U_UNFUSED = "sort > rows {k} > scan+finish+compact"           # LB_SMALL_FUSED=0: counting sort, separate scan / finish / compaction
FUSED_OFF_CLOUDS = ("tiny", "small2d", "small3d", "small3d_walls", "allpairs2d", "allpairs3d")
ROUTES, ROUTES_UNFUSED = {}, {}


def _row(cid, f32, B, alloc, update, k_alloc=None, k_update=None):
    """k_alloc, k_update: the search kernels of the row, for its LB_SMALL_FUSED=0 twin."""
    key = cid, "f32" if f32 else "f64", B
    ROUTES[key] = (alloc, update)
    if cid in FUSED_OFF_CLOUDS:
        ROUTES_UNFUSED[key] = (A_SORT.format(k=k_alloc), U_UNFUSED.format(k=k_update))


def _fill_table():
    for f32 in (False, True):
        # all pairs: fp64 stages the one "cell" in k_nl, float32 geometry walks it with k_nlw
        k = "k_nlw" if f32 else "k_nl[2048]"
        for cid in ("allpairs2d", "allpairs3d"):
            _row(cid, f32, 1, A_SMALL.format(k=k), "k_nl_small", k, k)
            _row(cid, f32, 3, A_SMALL.format(k=k), U_SCAN.format(c="cells_small", k=k), k, k)
        # 2D with a cell list: k_nl (fp64; the update stages cell_capacity * 9 candidates), k_nlc (float32)
        for cid, cand, alloc in (("tiny", 128, A_SMALL), ("small2d", 256, A_SMALL), ("wide", 128, A_WIDE)):
            ka, ku = ("k_nlc", "k_nlc") if f32 else ("k_nl[2048]", f"k_nl[{cand}]")
            _row(cid, f32, 1, alloc.format(k=ka), "k_nl_small", ka, ku)
            _row(cid, f32, 3, alloc.format(k=ka), U_SCAN.format(c="strided", k=ku), ka, ku)
        for cid in ("small3d", "small3d_walls"):
            _row(cid, f32, 1, A_SMALL.format(k="k_nlc"), "k_nl_small", "k_nlc", "k_nlc")
            _row(cid, f32, 3, A_SMALL.format(k="k_nlc"), U_SCAN.format(c="strided", k="k_nlc"), "k_nlc", "k_nlc")
        # one mid-size trajectory: counting sort + scan + k_row_finish at allocation, k_nl_mid on the update path
        ka = "k_nlc" if f32 else "k_nl[2048]"
        _row("mid2d", f32, 1, A_SORT.format(k=ka), "k_nl_mid")
        _row("mid2d", f32, 3, A_SORT.format(k=ka), U_SCAN.format(c="strided", k="k_nlc" if f32 else "k_nl[256]"))
        _row("mid3d", f32, 1, A_SORT.format(k="k_nlc"), "k_nl_mid")
        _row("mid3d", f32, 3, A_SORT.format(k="k_nlc"), U_SCAN.format(c="strided", k="k_nlc"))
        # a clump: every build after the count is dense, and a dense build bins with the CSR kernels
        small, large = dict(c="cells_small", k=ka, f="rows_small"), dict(c="sort", k=ka, f="scan+finish")
        _row("clump", f32, 1, A_DENSE.format(**small), U_SCAN.format(c="cells_small", k="k_nlw"))
        _row("clump", f32, 3, A_DENSE.format(**small), U_SCAN.format(c="cells_small", k="k_nlw"))
        _row("clump_batch", f32, 2, A_DENSE.format(**large), U_SCAN.format(c="cells_traj", k="k_nlw"))
        _row("clump_mid", f32, 1, A_DENSE.format(**large), U_SCAN.format(c="cells_mid", k="k_nlw"))
        # every stencil above 2048 candidates: the staged k_nl's count flags it and the allocation runs again, dense (k_nlc
        # has no such limit: the float32 count sees degrees above 256 and only the fill changes kernel)
        _row("reentry", f32, 1, A_DENSE.format(c="cells_small", k="k_nlc", f="rows_small") if f32 else
             A_SMALL.format(k="k_nlw") + " (again after k_nl)", U_SCAN.format(c="cells_small", k="k_nlw"))
        # more than LB_CSCAN_N nodes: scan, finish and compaction as launches of their own
        _row("big_batch", f32, 6, A_SORT.format(k=ka), f"strided > rows {'k_nlc' if f32 else 'k_nl[256]'} > scan+finish+compact")


_fill_table()

SWEEP_CAPS = (14, 28, 42, 56, 71, 85, 99, 113, 120)


def _knl_cand(cap):
    return 128 * ((cap * 9 + 127) // 128) if cap * 9 <= 1024 else 2048
