"""graph.Graph on the device (csrc/lb_graph.hip): gather and the ordered segment sum over receivers and senders, forward
and backward, against numpy - bit for bit: the order of the sum is part of the contract, so there is no tolerance here.

Cases - the smallest that reach every path:
  rpf2d_b1 / _b2  make_case("rpf2d", scale=0.25): N = 200, periodic; with B = 2 the second trajectory's slots start at E_cap,
                  not at n_edges[0]
  ldc3d           make_case("ldc3d", scale=0.5) in free space: N = 1020, 3-D - more than one workgroup of rows, a row tail
  lj              the LJ fixture with input_seq_length 3: N = 3 - rows shorter than a wave, nearly every slot a pad
  asym            tests._asym.asym_case("tgv2d", B=2): edges without a transpose, the sender view comes from the radix sort
Columns: 1 (narrowest row), 5 (the row ends inside a 16-byte access: the scalar kernels), 64 (16 lanes of 16 bytes), 130 (past
128 and no multiple of 4: a lane owns several columns), 260 (65 units of 16 bytes: one more than the 64 lanes of a row, so the
second pass over the row has one live lane).
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._common import hip_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
LJ = os.path.join(ROOT, "golden", "3D_LJ_3_1214every1")
CASES = ["rpf2d_b1", "rpf2d_b2", "ldc3d", "lj", "asym"]
COLUMNS = [1, 5, 64, 130, 260]
ROLES = ("receivers", "senders")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _build(cid):
    """(features (batched), engine, {"receivers", "senders"}: (B, E_cap) int, n_edges (B,), pairs or None)."""
    pairs = None
    if cid == "lj":
        from lagrangebench_amd.case_setup import case_builder
        from lagrangebench_amd.data import H5Dataset
        isl = 3
        ds = H5Dataset("valid", LJ, name="lj3d", input_seq_length=isl, extra_seq_length=2)
        md = ds.metadata
        bounds = np.array(md["bounds"])
        hcase = case_builder(bounds[:, 1] - bounds[:, 0], md, isl, noise_std=0.0)
        pos, pt = ds[0][0][None].astype(np.float64), ds[0][1][None]
    elif cid == "asym":
        from tests._asym import asym_case
        ds, pos, pt, pairs = asym_case("tgv2d", B=2)
        isl = ds.input_seq_length
        hcase = hip_case(ds)
    else:
        from lagrangebench_amd.data import make_case
        name, scale, B = {"rpf2d_b1": ("rpf2d", 0.25, 1), "rpf2d_b2": ("rpf2d", 0.25, 2), "ldc3d": ("ldc3d", 0.5, 1)}[cid]
        isl = 6
        ds = make_case(name, n_trajs=B, extra_seq_length=2, input_seq_length=isl, scale=scale)
        if name == "ldc3d":
            ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
        hcase = hip_case(ds)
        pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
        pt = np.stack([ds[b][1] for b in range(B)])
    feats, _ = hcase.allocate_eval((pos[:, :, :isl], pt))
    eng = feats.engine
    idx, ne = eng.nl_idx()
    idx, ne = _np(idx), _np(ne)
    return feats, eng, {"receivers": idx[:, 0], "senders": idx[:, 1]}, ne, pairs, hcase


@functools.lru_cache(maxsize=None)
def _setup(cid):
    return _build(cid)


def np_gather(x, idx, ne):
    """x (B, N, C) -> (B, E_cap, C): numpy indexing in the real slots, +0.0 in the pads."""
    B, E = idx.shape
    out = np.zeros((B, E, x.shape[2]), np.float32)
    for b in range(B):
        out[b, :ne[b]] = x[b, idx[b, :ne[b]]]
    return out


def np_segment_sum(msg, idx, ne, N):
    """msg (B, E_cap, C) -> (B, N, C): a float32 loop over the real slots in ascending order; the first term starts the
    sum.  The pad slots are not read."""
    B, E = idx.shape
    out = np.zeros((B, N, msg.shape[2]), np.float32)
    seen = np.zeros((B, N), bool)
    for b in range(B):
        for j in range(int(ne[b])):
            i = idx[b, j]
            if seen[b, i]:
                out[b, i] += msg[b, j]
            else:
                out[b, i] = msg[b, j]
                seen[b, i] = True
    return out


def test_cases_are_what_they_claim():
    _need_gpu()
    from tests._asym import check_premise
    sizes = {}
    for cid in CASES:
        feats, eng, idx, ne, pairs, _ = _setup(cid)
        sizes[cid] = (eng.B, eng.N, eng.e_cap, ne.tolist())
        assert (ne <= eng.e_cap).all() and (ne > 0).all()
        for b in range(eng.B):   # real slots hold node ids, pad slots N; canonical (receiver, sender) order
            r, s = idx["receivers"][b], idx["senders"][b]
            assert (r[ne[b]:] == eng.N).all() and (s[ne[b]:] == eng.N).all() and r[:ne[b]].max() < eng.N
            key = r[:ne[b]].astype(np.int64) * eng.N + s[:ne[b]]
            assert (np.diff(key) > 0).all()
        if pairs is not None:
            for b in range(eng.B):
                edges = np.stack([idx["receivers"][b, :ne[b]], idx["senders"][b, :ne[b]]])
                assert check_premise(edges, pairs, b)
    print(f"[graph ops] (B, N, E_cap, n_edges): {sizes}")
    assert sizes["rpf2d_b1"][1] == 200 and sizes["ldc3d"][1] == 1020 and sizes["lj"][1] == 3
    assert sizes["rpf2d_b2"][0] == 2 and sizes["rpf2d_b2"][3][0] < sizes["rpf2d_b2"][2]   # trajectory 1 starts behind pads
    assert sizes["lj"][3][0] <= 9


@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_ops_equal_numpy_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, pairs, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    assert np.array_equal(_np(g.n_edges), ne) and np.array_equal(_np(g.senders), idx["senders"])
    rng = np.random.default_rng(100 * C + len(cid))
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    msg = (rng.standard_normal((B, E, C)) * 10.0 ** rng.integers(-3, 4, (B, E, 1))).astype(np.float32)
    w = rng.standard_normal((B, N, C)).astype(np.float32)
    msg_nan = msg.copy()
    for b in range(B):
        msg_nan[b, ne[b]:] = np.nan
    sorts0 = eng.graph_sender_sorts()
    for role in ROLES:
        xd = torch.tensor(x, device=eng.device, requires_grad=True)
        # ---- gather: numpy indexing exactly, +0.0 in the pad slots
        got = g.gather(xd, role)
        assert got.shape == (B, E, C) and got.dtype == torch.float32
        assert np.array_equal(_bits(_np(got)), _bits(np_gather(x, idx[role], ne))), (cid, role, C)
        # ---- segment sum: the float32 loop, bit for bit; NaN in the pad slots does not reach the output
        want = np_segment_sum(msg, idx[role], ne, N)
        got_s = _np(g.segment_sum(torch.tensor(msg_nan, device=eng.device), role))
        assert np.isfinite(got_s).all()
        assert np.array_equal(_bits(got_s), _bits(want)), (cid, role, C, np.abs(got_s - want).max())
        # ---- backward of (segment_sum(gather(x)) * w).sum(): the two adjoints, restated in numpy float32
        y = g.segment_sum(g.gather(xd, role), role)
        (y * torch.tensor(w, device=eng.device)).sum().backward()
        want_dx = np_segment_sum(np_gather(w, idx[role], ne), idx[role], ne, N)
        assert np.array_equal(_bits(_np(xd.grad)), _bits(want_dx)), (cid, role, C)
        assert np.array_equal(_bits(_np(y)), _bits(np_segment_sum(np_gather(x, idx[role], ne), idx[role], ne, N)))
        # ---- two runs: identical bits
        again = _np(g.segment_sum(torch.tensor(msg_nan, device=eng.device), role))
        assert np.array_equal(_bits(again), _bits(got_s))
    # the sender view of a list with one-directional edges came from the sort - once per list, not per call
    if pairs is not None:
        assert eng.graph_sender_sorts() >= 1 and eng.graph_sender_sorts() - sorts0 <= 1


def test_unbatched_features_and_trailing_dimensions():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    _, _, _, _, _, hcase = _setup("rpf2d_b1")
    from lagrangebench_amd.data import make_case
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=6, scale=0.25)
    feats, _ = hcase.allocate_eval((ds[0][0][:, :6], ds[0][1]))   # one un-batched sample
    assert not feats.batched
    eng = feats.engine
    g = Graph(feats)
    idx, ne = eng.nl_idx()
    idx, ne = _np(idx), _np(ne)
    x = np.random.default_rng(1).standard_normal((eng.N, 3, 4)).astype(np.float32)
    got = g.gather(torch.tensor(x, device=eng.device), "senders")
    assert got.shape == (eng.e_cap, 3, 4) and g.senders.shape == (eng.e_cap,) and g.n_edges.dim() == 0
    want = np_gather(x.reshape(1, eng.N, 12), idx[:, 1], ne)
    assert np.array_equal(_bits(_np(got)), _bits(want.reshape(eng.e_cap, 3, 4)))
    back = g.segment_sum(got, "senders")
    assert back.shape == (eng.N, 3, 4)
    assert np.array_equal(_bits(_np(back)), _bits(np_segment_sum(want, idx[:, 1], ne, eng.N).reshape(eng.N, 3, 4)))
    # a non-contiguous input is made contiguous; a CPU tensor is refused
    xt = torch.tensor(np.ascontiguousarray(x.reshape(eng.N, 12).T), device=eng.device).T
    assert not xt.is_contiguous()
    assert np.array_equal(_bits(_np(g.gather(xt, "senders"))), _bits(want[0]))
    with pytest.raises(TypeError, match="engine on"):
        g.gather(torch.zeros((eng.N, 2)), "senders")
    with pytest.raises(ValueError, match="expected"):
        g.gather(torch.zeros((eng.N + 1, 2), device=eng.device), "senders")


def test_ops_after_the_list_moved_on_raise():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, hcase = _build("rpf2d_b1")
    g = Graph(feats)
    x = torch.randn((1, eng.N, 4), device=eng.device, requires_grad=True)
    y = g.gather(x, "receivers")
    z = g.segment_sum(y, "senders")
    eng.nl_update()
    for op, t in ((g.gather, x), (g.segment_sum, y)):
        with pytest.raises(RuntimeError, match="stale"):
            op(t.detach(), "senders")
    with pytest.raises(RuntimeError, match="stale"):   # ... and so does a backward of the graph made before
        z.sum().backward()
    # the library's own refusals: an overflowed list, and no list at all
    flat = torch.zeros((eng.N, 4), device=eng.device)
    eng.nl_set_capacity(eng.cell_capacity, int(ne[0]) - 5)
    eng.nl_update()
    assert bool(eng.nl_flags().any())
    with pytest.raises(LbHipError, match="-3.*overflowed"):
        eng.graph_gather(1, flat)
    with pytest.raises(LbHipError, match="-3.*overflowed"):
        eng.graph_segment_sum(1, torch.zeros((eng.e_cap, 4), device=eng.device))
    eng.nl_allocate()
    assert eng.graph_gather(1, flat).shape == (eng.e_cap, 4)
    from lagrangebench_amd.data import make_case
    ds = make_case("rpf2d", n_trajs=3, extra_seq_length=2, input_seq_length=6, scale=0.25)
    fresh = hip_case(ds).engine(3)
    assert fresh.e_cap == 0
    with pytest.raises(LbHipError, match="-3.*before lb_nl_allocate"):
        fresh._graph_op("lb_graph_gather", 0, torch.zeros((3 * fresh.N, 2), device=fresh.device), 3 * fresh.N, 1)
