"""The premises of tests/test_nl_routes_gpu.py, checked without a GPU for every cloud of tests/_nl_clouds.py in both geometry
dtypes: the all-pairs reference is the oracle's list, the crafted particles really are hard, and what the current suite
could not see (positions that do not survive a rounding to float32) is really there."""
import numpy as np
import pytest

from oracle import lb_oracle as O
from tests import _nl_clouds as C

CASES = [(cid, f32) for cid in C.SPECS for f32 in (False, True)]
IDS = [f"{cid}-{'f32' if f32 else 'f64'}" for cid, f32 in CASES]


def _ref(cid, f32):
    return C.reference(cid, f32, max(C.BATCHES[cid]))


def _newest(R, b, t):
    return R.pos[b][:R.n_real[b], t + C.ISL - 1].astype(R.g.dt)


@pytest.mark.parametrize("cid,f32", CASES, ids=IDS)
def test_all_pairs_reference_is_the_oracles_list(cid, f32):
    """On the allocation frame and on both update frames, for every trajectory: the all-pairs list equals the list of
    O.neighbor_list (allocate, then update with the frozen capacities), nothing overflows, the capacities are those of an
    allocation on the frame, and every frame has another list than the one before."""
    R = _ref(cid, f32)
    g = R.g
    for b in range(R.B):
        n = R.n_real[b]
        nf = O.neighbor_list(g.disp, np.asarray(R.ds.box), C.SPECS[cid]["rc"], capacity_multiplier=R.ds.multiplier)
        for t in C.FRAMES:
            assert not R.overflow[b, t], (b, t)
            assert np.array_equal(R.edges[b, t], R.oracle_edges[b, t]), (b, t)
            x = _newest(R, b, t)
            assert R.pos[b].dtype == np.float64 and np.array_equal(x.astype(np.float64), R.pos[b][:n, t + C.ISL - 1])
            if g.use_cells:
                assert (g.cells(x) < g.ncell).all() and (x >= 0).all() and (x < g.box).all()
            fresh = nf.allocate(x)
            assert np.array_equal(O.canonical_edges(fresh.idx, n), R.edges[b, t]) and not fresh.did_buffer_overflow
            if g.use_cells:
                assert fresh.cell_capacity == int(R.occ[b, t] * R.ds.multiplier)
            if t:
                assert not np.array_equal(R.edges[b, t], R.edges[b, t - 1]), "an update must see another list"
        assert (R.pt[b][:n] == 0).all() and (R.pt[b][n:] == -1).all() and (R.pos[b][n:] == 0).all()
    if "pads" in C.SPECS[cid]:
        assert sorted(set(R.N - np.array(R.n_real))) == [0, 7]


@pytest.mark.parametrize("cid,f32", CASES, ids=IDS)
def test_cutoff_pairs_straddle_the_cutoff(cid, f32):
    """Of the 40 crafted pairs of a trajectory at least a quarter are edges and a quarter are not; in a periodic box some
    cross a face; they stand still.  In an fp64 cloud, rounding the positions to float32 and evaluating the same fp64
    predicate flips at least 5 of the 40 decisions: an engine fed float32 values never meets these inputs."""
    R = _ref(cid, f32)
    g = R.g
    one_dir = 0
    for b in range(R.B):
        pairs = R.ds.info[b]["pairs"]
        assert len(pairs) == C.N_CUT
        i, j = np.array(pairs).T
        x = _newest(R, b, 0)
        for t in C.FRAMES[1:]:
            assert np.array_equal(_newest(R, b, t)[i], x[i]) and np.array_equal(_newest(R, b, t)[j], x[j])
        fwd = g.metric_sq(x[j], x[i]) < g.cut          # edge (receiver i, sender j)
        bwd = g.metric_sq(x[i], x[j]) < g.cut
        have = set(zip(R.edges[b, 0][0].tolist(), R.edges[b, 0][1].tolist()))
        assert [(r, s) in have for r, s in zip(i.tolist(), j.tolist())] == fwd.tolist()
        assert [(r, s) in have for r, s in zip(j.tolist(), i.tolist())] == bwd.tolist()
        assert fwd.sum() >= C.N_CUT // 4 and (~fwd).sum() >= C.N_CUT // 4, (b, int(fwd.sum()))
        one_dir += int((fwd != bwd).sum())
        if g.pbc:
            assert (np.abs(x[j].astype(np.float64) - x[i]) > 0.5 * g.box64).any(), "no pair crosses a periodic face"
        # one nextafter step of the walked coordinate away from the decision: within 3 steps the predicate changes
        if not f32:
            x32 = x.astype(np.float32).astype(np.float64)
            flipped = (g.metric_sq(x32[j], x32[i]) < g.cut) != fwd
            assert flipped.sum() >= 5, (b, int(flipped.sum()))
    print(f"[{cid} {'f32' if f32 else 'f64'}] one-directional crafted pairs: {one_dir} of {R.B * C.N_CUT}")


@pytest.mark.parametrize("cid,f32", [c for c in CASES if C.SPECS[c[0]]["faces"]],
                         ids=[i for c, i in zip(CASES, IDS) if C.SPECS[c[0]]["faces"]])
def test_face_particles_decide_the_largest_occupancy(cid, f32):
    """On every frame: the cells on either side of every crafted face all hold T particles and no other cell holds as many
    (one particle binned on the wrong side of one face gives T + 1 somewhere), the face particles sit at k * cell_size, at
    its nextafter neighbours and within ten steps of it, both cells of a face hold one, and without them the largest
    occupancy is another."""
    R = _ref(cid, f32)
    g = R.g
    dt = g.dt
    for b in range(R.B):
        info = R.ds.info[b]
        T = info["target"]
        fh = np.array([int(np.dot(c, g.mult)) for c in info["face_cells"]])
        assert len(fh) >= 2 * g.dim and len(info["face"]) >= 3 * 3 * g.dim - 3
        for t in C.FRAMES:
            x = _newest(R, b, t)
            occ = np.bincount(g.hashes(x), minlength=g.ncells)
            assert (occ[fh] == T).all() and R.occ[b, t] == T, (b, t, occ[fh], T)
            rest = np.delete(occ, fh)
            assert rest.max() < T
            assert g.occupancy(np.delete(x, info["face"], axis=0)) != T
            assert set(fh.tolist()) <= set(g.hashes(x[info["face"]]).tolist())
        # the crafted coordinates: q = x / cell_size is within one ulp of an integer k on some axis
        x = _newest(R, b, 0)[info["face"]]
        cs = g.cell_size.astype(dt)
        k = np.rint(x.astype(np.float64) / cs.astype(np.float64))
        edge = (k.astype(dt) * cs).astype(dt)
        on_face = np.abs(x - edge) <= 10 * np.spacing(np.maximum(edge, cs))
        for a in range(g.dim):      # the face itself and both nextafter neighbours are there
            for e in np.unique(edge[on_face[:, a] & (k[:, a] < g.ncell[a]), a]):   # (k = cells per side: the box's top)
                have = set(x[on_face[:, a] & (edge[:, a] == e), a].tolist())
                want = {e, np.nextafter(e, dt.type(np.inf))} | ({np.nextafter(e, dt.type(-np.inf))} if e > 0 else set())
                assert {float(v) for v in want} <= have, (a, e)
        top = g.pbc & (x >= g.into_grid(np.nextafter(g.box, dt.type(0))[None])[0])
        assert (on_face | top).any(axis=1).all()
        ks = {(a, int(k[r, a])) for r in range(len(x)) for a in range(g.dim) if (on_face | top)[r, a]}
        for a in range(g.dim):
            n = int(g.ncell[a])
            assert {(a, 0), (a, n // 2), (a, n - 1)} <= ks, (a, sorted(ks))


@pytest.mark.parametrize("cid", [c for c in C.SPECS if C.SPECS[c].get("clump")])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_clump_has_a_degree_above_256(cid, f32):
    R = _ref(cid, f32)
    for b in range(R.B):
        for t in C.FRAMES:
            deg = np.bincount(R.edges[b, t][0], minlength=R.n_real[b])
            assert deg.max() > 256 and (deg[R.ds.info[b]["clump"]] > 256).sum() >= 200, (b, t, int(deg.max()))
            assert deg.max() <= 4096


@pytest.mark.parametrize("cid", ["small2d", "mid2d", "big_batch"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_batch_trajectories_differ_in_their_largest_occupancy(cid, f32):
    """test_cell_overflow_flag_per_trajectory bites only where one trajectory of a batch overflows a capacity that another
    holds: on the window it uses, the fullest trajectory is fuller than some other one.  small2d and mid2d finish in
    k_nl_compact_scan, big_batch (more than LB_CSCAN_N nodes) in k_row_finish."""
    R = _ref(cid, f32)
    occ = [R.occ[b, C.FRAMES[-1]] for b in range(R.B)]
    assert R.B > 1 and min(occ) < max(occ), occ


def test_sweep_cloud_fits_the_smallest_capacity_of_the_sweep():
    """The capacity sweep of test_nl_routes_gpu.py starts at 14 on small2d (fp64): no trajectory's fullest cell holds more,
    on the window it uses, so every capacity of the sweep compares its list."""
    R = _ref("small2d", False)
    assert max(R.occ[b, C.FRAMES[-1]] for b in range(R.B)) <= 14


def test_wide_grid_sits_near_the_float_quotient_limit():
    """`wide`: 1500 cells along x, so x / cell_size runs up to 1500 of the 2000 the float quotient of the cell coordinate is
    budgeted for, with crafted particles at cells 0, 750 and 1499."""
    g = C.geometry("wide")
    assert g.ncell.tolist() == [1500, 3]
    R = _ref("wide", False)
    x = _newest(R, 0, 0)
    assert (x[:, 0] / g.cell_size[0]).max() > 1400


def test_cell_grids_are_those_of_the_table():
    want = {"tiny": [5, 4], "small2d": [7, 5], "small3d": [4, 5, 3], "small3d_walls": [4, 5, 3], "wide": [1500, 3]}
    for cid, nc in want.items():
        assert C.geometry(cid).ncell.tolist() == nc == C.geometry(cid, True).ncell.tolist()
    for cid in ("allpairs2d", "allpairs3d"):
        assert not C.geometry(cid).use_cells and not C.geometry(cid, True).use_cells
