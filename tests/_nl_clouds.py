"""Point clouds for the neighbor search, and a reference that knows nothing about cells.

The datasets of `make_case` are float32 lattices: every position converts to float exactly, no particle sits within an ulp
of the cutoff or of a cell face, and which search route a test reaches is an accident of its size.  The clouds here are
built for the routes of csrc/lb_neighbor.hip (lbk_nl_build):

* positions uniform in [0, box) with full fp64 mantissas (float32 geometry: the same cloud rounded to float32, everything
  below then done in float32 with float32 predicates, as tests/_asym.py does); every later frame is the last one plus a
  small random drift, wrapped (periodic) or clamped (walls) into the box, so an update sees another list than the allocation;
* crafted particles that stand still in every frame:
  - cutoff pairs: x_j = wrap(x_i + r_c u) for an oblique unit vector u, then ONE coordinate of x_j is walked by nextafter
    until the oracle's own metric_sq(x_j, x_i) < cutoff_sq changes, and left -2 .. +2 steps from that crossing;
  - cell-face particles: at k * cell_size exactly and at its nextafter neighbours, for the first, a middle and the last
    cell of every axis; the two cells on either side of each such face are then topped up to ONE common occupancy T above
    every other cell's, so a single particle binned on the wrong side of any face makes some cell hold T + 1: the largest
    occupancy - cell_capacity at allocation, did_buffer_overflow at an update - changes.  Particles in those cells stand
    still and no drifting particle may enter them.

`all_pairs_edges` evaluates the oracle's displacement and strict < on all N^2 ordered pairs, in the geometry dtype; its only
shortcut is a one-coordinate fp64 band filter (a pair further apart than 1.01 r_c along x alone is no edge) that is two
orders of magnitude wider than any rounding.  tests/test_nl_routes.py asserts on the CPU that it equals the oracle's list and
that the crafted premises hold; tests/test_nl_routes_gpu.py compares the engine with it.
"""
import functools

import numpy as np

from lagrangebench_amd.data.synthetic import PAD_VALUE, SyntheticDataset, _meta
from oracle import lb_oracle as O
from tests._common import oracle_case

ISL, EXTRA = 2, 2            # four frames: the allocation window [0, 2) and the update windows [1, 3), [2, 4)
FRAMES = (0, 1, 2)           # window starts; the newest frame of window t is t + ISL - 1
N_CUT = 40                   # crafted cutoff pairs per trajectory

# id -> geometry.  r_c and the boxes are chosen so that box / r_c is no integer (cell_size > r_c) and no cell count is a power
# of two.  anchors: background particles the cutoff pairs hang on; faces: (axis, which) cell faces that get particles
# ("all": first, middle and last cell of every axis); clump: particles inside a disc of radius r_c / 2; pads: {trajectory:
# PAD_VALUE particles at its end}; drift: another per-frame drift than DRIFT; targets: the largest occupancy T of trajectory
# i (small2d: at most 14, the smallest capacity of the sweep in test_nl_routes_gpu.py, and not the same in every trajectory).
SPECS = {
    "allpairs2d": dict(dim=2, N=130, box=(0.9, 1.3), rc=0.31, pbc=True, faces=()),
    "allpairs3d": dict(dim=3, N=130, box=(0.9, 1.3, 1.1), rc=0.31, pbc=True, faces=()),
    "tiny": dict(dim=2, N=65, box=(0.53, 0.43), rc=0.1, pbc=True, anchors=10, faces=(), drift=0.2),
    "small2d": dict(dim=2, N=300, box=(0.73, 0.53), rc=0.1, pbc=True, faces="all", pads={1: 7}, targets=(14, 13, 14)),
    "small3d": dict(dim=3, N=300, box=(0.43, 0.53, 0.33), rc=0.1, pbc=True, faces="all"),
    "small3d_walls": dict(dim=3, N=300, box=(0.43, 0.53, 0.33), rc=0.1, pbc=False, faces="all"),
    "wide": dict(dim=2, N=300, box=(15.004, 0.0312), rc=0.01, pbc=True, faces="all", drift=0.3),
    "mid2d": dict(dim=2, N=4200, box=(2.13, 1.93), rc=0.1, pbc=True, faces="all", margin=4),
    "mid3d": dict(dim=3, N=4200, box=(1.23, 1.13, 1.03), rc=0.1, pbc=True, faces="all"),
    "clump": dict(dim=2, N=600, box=(0.83, 0.73), rc=0.1, pbc=True, faces=(), clump=300),
    "clump_batch": dict(dim=2, N=2100, box=(1.53, 1.43), rc=0.1, pbc=True, faces=(), clump=300),
    "clump_mid": dict(dim=2, N=4200, box=(2.13, 1.93), rc=0.1, pbc=True, faces=(), clump=300),
    # 3 x 3 cells: every stencil is the whole cloud, more than the 2048 candidates the staged k_nl holds
    "reentry": dict(dim=2, N=2300, box=(0.33, 0.34), rc=0.1, pbc=True, faces=(), dense=True),
    "big_batch": dict(dim=2, N=2800, box=(1.83, 1.63), rc=0.1, pbc=True, faces="all"),
}
# the batch sizes each cloud is searched at (every trajectory of a batch is another cloud); B = 1 is trajectory 0
BATCHES = {"allpairs2d": (1, 3), "allpairs3d": (1, 3), "tiny": (1, 3), "small2d": (1, 3), "small3d": (1, 3),
           "small3d_walls": (1, 3), "wide": (1, 3), "mid2d": (1, 3), "mid3d": (1, 3), "clump": (1, 3), "clump_batch": (2,),
           "clump_mid": (1,), "reentry": (1,), "big_batch": (6,)}
SEEDS = {}                   # id -> seed (default 0): fixed where the default does not meet the premises of test_nl_routes.py
DRIFT = 0.03                 # per-frame drift, standard deviation in units of r_c


class Geometry:
    """The oracle's arithmetic for one cloud in one dtype: displacement, cutoff predicate, cell coordinates."""

    def __init__(self, box, rc, pbc, dtype):
        self.dt = np.dtype(dtype)
        self.box64 = np.asarray(box, np.float64)
        self.box = self.box64.astype(self.dt)
        self.rc, self.pbc, self.dim = float(rc), bool(pbc), len(box)
        self.disp, self.shift = O.space_periodic(self.box) if pbc else O.space_free()
        self.cut = self.dt.type(self.rc ** 2)                      # neighbor_list: dR < position.dtype.type(cutoff_sq)
        box32 = np.asarray(box, np.float32)                        # partition.py: box and cell_size are float32
        self.use_cells = bool(np.all(np.float32(rc) < box32 / np.float32(3.0)))
        if self.use_cells:
            cps = np.floor(box32 / np.float32(rc))
            self.cell_size = (box32 / cps).astype(np.float32)
            self.ncell = cps.astype(np.int64)
            self.mult = np.concatenate([[1], np.cumprod(self.ncell[:-1])]).astype(np.int64)
            self.ncells = int(np.prod(self.ncell))

    def metric_sq(self, a, b):
        d = self.disp(a, b)
        return np.sum(d ** 2, axis=-1)

    def cells(self, p):
        return (p / self.cell_size.astype(p.dtype)).astype(np.int32).astype(np.int64)

    def hashes(self, p):
        return np.sum(self.cells(p) * self.mult, axis=-1)

    def occupancy(self, p):
        """Largest cell occupancy as the oracle counts it (0 without a cell list)."""
        return int(np.bincount(self.hashes(p), minlength=self.ncells).max()) if self.use_cells else 0

    def into_grid(self, p):
        """p in [0, box] -> below the box and, with a cell list, inside the grid (int(p / cell_size) < cells per side)."""
        p = np.minimum(np.maximum(p, self.dt.type(0)), np.nextafter(self.box, self.dt.type(0)))
        if self.use_cells:
            # (cell_size is a rounded float32: cells_per_side * cell_size may lie below the box by 1e-8 of it, and the
            # reference does not clamp the coordinate of a particle in that sliver - the clouds stay out of it)
            p = np.minimum(p, (self.ncell * self.cell_size.astype(np.float64)).astype(self.dt))
            for _ in range(64):
                bad = self.cells(p) >= self.ncell
                if not bad.any():
                    break
                p = np.where(bad, np.nextafter(p, self.dt.type(0)), p)
            assert not (self.cells(p) >= self.ncell).any()
        return p.astype(self.dt)


def geometry(cid, f32=False):
    s = SPECS[cid]
    return Geometry(s["box"], s["rc"], s["pbc"], np.float32 if f32 else np.float64)


def _step(x, axis, direction, n=1):
    x = x.copy()
    for _ in range(n):
        x[axis] = np.nextafter(x[axis], x.dtype.type(np.inf if direction > 0 else -np.inf))
    return x


def _cutoff_partner(g, rng, xi, offset, through=None):
    """x_j next to the cutoff sphere of xi: one coordinate is walked by nextafter to where metric_sq(x_j, x_i) < cutoff_sq
    changes; offset 0 is the first position outside, offset > 0 that many steps further out, offset < 0 that many steps
    inwards (-1: the last position inside).  None if the walk leaves the box or finds no crossing."""
    dt = g.dt
    u = rng.standard_normal(g.dim)
    u /= np.linalg.norm(u)
    if np.abs(u).min() < 0.15:          # oblique: every coordinate takes part
        return None
    if through is not None and u[through[0]] * through[1] < 0.5:   # (axis, sign): the pair must reach through that face
        return None
    dr = (g.rc * u).astype(dt)
    xj = np.asarray(g.shift(xi, dr), dt)
    axis = int(rng.integers(g.dim))

    def ok(x):
        return bool((x >= 0).all() and (x < g.box).all() and (not g.use_cells or (g.cells(x) < g.ncell).all()))

    def inside(x):
        return bool(g.metric_sq(x, xi) < g.cut)

    if not ok(xj):
        return None
    s0 = inside(xj)
    away = 1 if g.disp(xj, xi)[axis] > 0 else -1
    direction = away if s0 else -away   # inside: walk away from x_i, outside: towards it
    x = xj
    for _ in range(4096):
        x = _step(x, axis, direction)
        if not ok(x):
            return None
        if inside(x) != s0:
            break
    else:
        return None
    if not s0:
        x = _step(x, axis, away)        # walked inwards: the position before the change is the first one outside
    x = _step(x, axis, away if offset >= 0 else -away, abs(offset))
    return x if ok(x) else None


def _cell_interior(g, rng, cell, n):
    """n points in the middle half of cell `cell` (a vector of cell coordinates)."""
    cs = g.cell_size.astype(np.float64)
    return ((np.asarray(cell, np.float64) + 0.25 + 0.5 * rng.random((n, g.dim))) * cs).astype(g.dt)


def _face_particles(g, rng, faces, per_face):
    """Particles on cell faces: for face k of `axis`, coordinate k * cell_size exactly, its upper and its lower nextafter
    neighbour (k = 0: the lower one is the last value below the box when the box is periodic), and further nextafter steps
    on a side until the oracle bins one of them into the cell of that side.  Returns the points and the
    cells (coordinate vectors) on either side of each face."""
    dt = g.dt
    pts, cells = [], []
    if faces == "all":
        faces = [(a, w) for a in range(g.dim) for w in ("first", "mid", "last")]
    for axis, which in faces:
        n = int(g.ncell[axis])
        k = {"first": 0, "mid": n // 2, "last": n - 1}[which]
        other = [int(rng.integers(g.ncell[d])) for d in range(g.dim)]
        edge = dt.type(k) * g.cell_size[axis].astype(dt)
        cell_of = lambda v: int(v / g.cell_size[axis].astype(dt))
        vals = [edge, np.nextafter(edge, dt.type(np.inf))]
        while cell_of(vals[-1]) < k:        # (the quotient of a value above the face may still round below k: go on until
            vals.append(np.nextafter(vals[-1], dt.type(np.inf)))   # one lands in cell k, so both sides hold a face particle)
        if k > 0:
            vals.append(np.nextafter(edge, dt.type(-np.inf)))
            while cell_of(vals[-1]) >= k:
                vals.append(np.nextafter(vals[-1], dt.type(-np.inf)))
        elif g.pbc:
            vals.append(np.nextafter(g.box[axis], dt.type(0)))
        assert len(vals) <= 12
        for _ in range(per_face):
            base = _cell_interior(g, rng, other, 1)[0]
            for v in vals:
                p = base.copy()
                p[axis] = v
                pts.append(p)
        for kk in ([k - 1, k] if k > 0 else ([n - 1, 0] if g.pbc else [0])):
            c = list(other)
            c[axis] = kk
            cells.append(tuple(c))
    pts = g.into_grid(np.array(pts, dt).reshape(-1, g.dim))
    return pts, sorted(set(cells))


def _make_traj(cid, f32, i):
    s = SPECS[cid]
    g = geometry(cid, f32)
    dt, dim, rc = g.dt, g.dim, g.rc
    n_real = s["N"] - s.get("pads", {}).get(i, 0)
    rng = np.random.default_rng([SEEDS.get(cid, 0), i])
    T = ISL + EXTRA
    n_anchor = s.get("anchors", N_CUT)

    # anchors first: the same fp64 draws in both dtypes
    anchors = (rng.random((n_anchor, dim)) * g.box64).astype(dt)
    through = {}
    if g.pbc:   # the first 2 dim anchors sit a quarter r_c inside a face each, and their partners on its other side
        for a in range(dim):
            anchors[a, a] = dt.type(0.25 * rc)
            anchors[dim + a, a] = dt.type(g.box64[a] - 0.25 * rc)
            through[a], through[dim + a] = (a, -1), (a, 1)
    anchors = g.into_grid(anchors)
    parts, still = [anchors], [np.ones(n_anchor, bool)]
    pairs = []
    q, tries = 0, 0
    partners = []
    while q < N_CUT:
        tries += 1
        assert tries < 4000, f"{cid}: no cutoff placement"
        xj = _cutoff_partner(g, rng, anchors[q % n_anchor], q % 5 - 2, through.get(q))
        if xj is None:
            continue
        partners.append(xj)
        pairs.append((q % n_anchor, n_anchor + q))      # (i, j): metric_sq(x_j, x_i) decides the edge (receiver i, sender j)
        q += 1
    parts.append(np.array(partners, dt))
    still.append(np.ones(N_CUT, bool))

    n_clump = s.get("clump", 0)
    if n_clump:
        c = (0.3 + 0.4 * rng.random(dim)) * g.box64
        r = 0.5 * rc * np.sqrt(rng.random(n_clump))
        th = 2 * np.pi * rng.random(n_clump)
        parts.append(g.into_grid((c + np.stack([r * np.cos(th), r * np.sin(th)], axis=-1)).astype(dt)))
        still.append(np.ones(n_clump, bool))

    face_cells, target = [], 0
    n_face = 0
    if s["faces"]:
        fp, face_cells = _face_particles(g, rng, s["faces"], s.get("per_face", 1))
        parts.append(fp)
        still.append(np.ones(len(fp), bool))
        n_face = len(fp)
    placed = np.concatenate(parts)
    budget = n_real - len(placed)
    assert budget >= 0, (cid, budget)
    if face_cells:
        # background: as much of what is left as still lets every face cell be topped up to T = largest occupancy + margin
        bg_all = g.into_grid((rng.random((budget, dim)) * g.box64).astype(dt))
        fh = np.array([int(np.dot(c, g.mult)) for c in face_cells])
        for n_bg in range((2 * budget) // 3, -1, -max(1, budget // 40)):
            occ = np.bincount(g.hashes(np.concatenate([placed, bg_all[:n_bg]])), minlength=g.ncells)
            target = int(occ.max()) + s.get("margin", 2)
            if "targets" in s:      # T fixed per trajectory: fewer background particles until it leaves the margin
                if target > s["targets"][i % len(s["targets"])]:
                    continue
                target = s["targets"][i % len(s["targets"])]
            if int((target - occ[fh]).sum()) <= budget - n_bg:
                break
        else:
            raise AssertionError(f"{cid}: the face cells cannot be topped up")
        placed = np.concatenate([placed, bg_all[:n_bg]])
        still.append(np.zeros(n_bg, bool))
        tops = [_cell_interior(g, rng, c, target - int(occ[h])) for c, h in zip(face_cells, fh)]
        tops = np.concatenate(tops).reshape(-1, dim)
        assert len(tops) <= budget - n_bg, f"{cid}: {len(tops)} top-ups for {budget - n_bg} free particles"
        placed = np.concatenate([placed, tops])
        still.append(np.ones(len(tops), bool))
        # the rest: anywhere outside the face cells, in cells that stay two below T
        occ = np.bincount(g.hashes(placed), minlength=g.ncells)
        rest = []
        for _ in range(200 * n_real):
            if len(placed) + len(rest) == n_real:
                break
            p = g.into_grid((rng.random((1, dim)) * g.box64).astype(dt))
            h = int(g.hashes(p)[0])
            if h in fh or occ[h] >= target - 2:
                continue
            occ[h] += 1
            rest.append(p[0])
        assert len(placed) + len(rest) == n_real, f"{cid}: no room outside the face cells"
        if rest:
            placed = np.concatenate([placed, np.array(rest, dt)])
            still.append(np.zeros(len(rest), bool))
    else:
        bg = g.into_grid((rng.random((budget, dim)) * g.box64).astype(dt))
        placed = np.concatenate([placed, bg])
        still.append(np.zeros(budget, bool))
        fh = np.zeros(0, np.int64)
    still = np.concatenate(still)
    assert len(placed) == n_real == len(still)
    if len(fh):
        still |= np.isin(g.hashes(placed), fh)

    frames = [placed]
    for _ in range(1, T):
        p = frames[-1]
        new = p.astype(np.float64) + rng.normal(0.0, s.get("drift", DRIFT) * rc, size=p.shape)
        new = np.mod(new, g.box64) if g.pbc else np.clip(new, 0.0, g.box64)
        new = g.into_grid(new.astype(dt))
        keep = still.copy()
        if len(fh):
            keep |= np.isin(g.hashes(new), fh)
        new[keep] = p[keep]
        if len(fh):   # no other cell may drift up to the face cells' occupancy: particles that entered such a cell stay put
            for _ in range(32):
                hn = g.hashes(new)
                full = np.bincount(hn, minlength=g.ncells) > target - 2
                full[fh] = False
                back = full[hn] & (hn != g.hashes(p))
                if not back.any():
                    break
                new[back] = p[back]
            else:
                new = p.copy()
        frames.append(new)
    pos = np.stack(frames, axis=1).astype(np.float64)          # (n_real, T, dim): float64 holding `dt` values
    pt = np.zeros(n_real, np.int32)
    k = s["N"] - n_real
    if k:
        pos = np.pad(pos, ((0, k), (0, 0), (0, 0)))
        pt = np.pad(pt, (0, k), constant_values=PAD_VALUE).astype(np.int32)
    first_face = n_anchor + N_CUT + n_clump
    info = dict(n_real=n_real, pairs=pairs, face=np.arange(first_face, first_face + n_face), face_cells=face_cells,
                target=target, clump=np.arange(n_anchor + N_CUT, n_anchor + N_CUT + n_clump))
    return pos, pt, info


@functools.lru_cache(maxsize=None)
def cloud(cid, f32=False, n_trajs=6):
    """The dataset of cloud `cid`: ds[i] -> (pos (N, T, dim) float64 - float32 values when f32 -, particle types (N,));
    ds.info[i]: what was crafted into trajectory i (filled when ds[i] is made)."""
    s = SPECS[cid]
    md = _meta(s["dim"], s["N"], s["box"], [s["pbc"]] * s["dim"], s["rc"], s["rc"] / 1.45, 0.05 * s["rc"], 0.01 * s["rc"],
               ISL + EXTRA, cid)
    info = {}

    def make(i):
        pos, pt, info[i] = _make_traj(cid, f32, i)
        return pos, pt

    ds = SyntheticDataset(cid, md, ISL, EXTRA, n_trajs, make)
    ds.info = info
    return ds


def all_pairs_edges(g, pos, chunk=512):
    """Every ordered pair (receiver r, sender s) with metric_sq(pos[s], pos[r]) < cutoff_sq, evaluated as the oracle does in
    g's dtype, as canonical_edges gives them: (2, E) int32 sorted by (receiver, sender)."""
    pos = np.ascontiguousarray(pos, g.dt)
    n = len(pos)
    x = pos[:, 0].astype(np.float64)
    band = 1.01 * g.rc
    recv, send = [], []
    for r0 in range(0, n, chunk):
        dx = np.abs(x[None, :] - x[r0:r0 + chunk, None])
        if g.pbc:
            dx = np.minimum(dx, g.box64[0] - dx)
        r, s = np.nonzero(dx < band)
        r += r0
        hit = g.metric_sq(pos[s], pos[r]) < g.cut
        recv.append(r[hit])
        send.append(s[hit])
    return np.stack([np.concatenate(recv), np.concatenate(send)]).astype(np.int32)


class Reference:
    """Everything the GPU tests compare with, for the first B trajectories of a cloud: per trajectory and window the
    all-pairs list, the oracle's edge features in that order, its overflow flag and the largest cell occupancy; the
    capacities of the allocation."""

    def __init__(self, cid, f32, B):
        self.ds = ds = cloud(cid, f32)
        self.g = g = geometry(cid, f32)
        self.B, self.N = B, SPECS[cid]["N"]
        dt = g.dt
        ocase = oracle_case(ds, dtype=dt)
        self.pos = np.stack([ds[b][0] for b in range(B)])
        self.pt = np.stack([ds[b][1] for b in range(B)])
        self.n_real = [ds.info[b]["n_real"] for b in range(B)]
        self.edges, self.feats, self.overflow, self.occ, self.oracle_edges = {}, {}, {}, {}, {}
        self.cell_capacity, self.e_cap = [], []
        for b in range(B):
            n = self.n_real[b]
            nb = None
            for t in FRAMES:
                win = self.pos[b][:n, t:t + ISL].astype(dt)
                if nb is None:
                    of, nb = ocase.allocate_eval((win, self.pt[b][:n]))
                    self.cell_capacity.append(nb.cell_capacity or 0)
                    self.e_cap.append(nb.max_occupancy)
                else:
                    of, nb = ocase.preprocess_eval((win, self.pt[b][:n]), nb)
                real = nb.idx[0] < n
                order = np.lexsort((nb.idx[1][real], nb.idx[0][real]))
                self.oracle_edges[b, t] = O.canonical_edges(nb.idx, n)
                self.feats[b, t] = {k: of[k][real][order] for k in ("rel_disp", "rel_dist")}
                self.overflow[b, t] = bool(nb.did_buffer_overflow)
                newest = win[:, ISL - 1]
                self.edges[b, t] = all_pairs_edges(g, newest)
                self.occ[b, t] = g.occupancy(newest)
        # a batch freezes the capacities of its fullest trajectory (the engine's and the reference's vmap alike)
        self.batch_cell_capacity = int(max(self.occ[b, 0] for b in range(B)) * ds.multiplier) if g.use_cells else 0
        self.batch_e_cap = max(self.e_cap)   # (int(occupancy * multiplier) is monotonic, and its clamps do not bind here)


@functools.lru_cache(maxsize=None)
def reference(cid, f32=False, B=1):
    return Reference(cid, f32, B)
