"""The edge-pair ops of graph.Graph (reverse, swap, symmetrize, antisymmetrize) without a device: the public surface, the C
ABI, and the yardsticks themselves - the numpy twins of tests/_graph_reverse.py - on the oracle's own lists and on hand-made
ones.  Each property the device tests lean on has its own check function here, and each check is shown to catch the mutated
twin it is meant for (tests/test_train_kernels.py does the same for its twins).

Lists (receiver, sender per real slot, sorted by (receiver, sender) as every list of the engine is; pad slots hold N):
  three     N = 3, B = 1: rows of 3, 3 and 2 slots - shorter than a wave -, every node with its self-edge, and the edge (0, 2)
            without its transpose
  empty     B = 2: `three`, then a trajectory without edges
  uneven    B = 2 with different n_edges: `three` (8 slots), then 3 slots with a self-edge
  asym      the oracle's lists of tests._asym.asym_case("tgv2d", B=2): the one-directional pairs it returns
"""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_bf16 as GB  # noqa: E402
from tests import _graph_reverse as GR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ("swap", "symmetrize", "antisymmetrize")
NEW_SYMBOLS = ("lb_graph_reverse", "lb_graph_edge_pair_t")

THREE = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
SMALL = [(0, 1), (1, 0), (2, 2)]


def _padded(trajs, N, e_cap):
    """[[(receiver, sender), ...] per trajectory] -> (receivers, senders (B, E_cap) with N in the pads, n_edges (B,))."""
    B = len(trajs)
    r, s = np.full((B, e_cap), N, np.int64), np.full((B, e_cap), N, np.int64)
    for b, edges in enumerate(trajs):
        edges = sorted(edges)
        r[b, :len(edges)] = [e[0] for e in edges]
        s[b, :len(edges)] = [e[1] for e in edges]
    return r, s, np.array([len(t) for t in trajs], np.int64)


@functools.lru_cache(maxsize=None)
def _lists(name):
    """-> (receivers, senders, n_edges, N, the set of (b, receiver, sender) that must be unpaired)"""
    if name == "three":
        return _padded([THREE], 3, 11) + (3, {(0, 0, 2)})
    if name == "empty":
        return _padded([THREE, []], 3, 10) + (3, {(0, 0, 2)})
    if name == "uneven":
        return _padded([THREE, SMALL], 3, 9) + (3, {(0, 0, 2)})
    assert name == "asym"
    from tests._asym import asym_case, check_premise, one_directional_edges, oracle_edges
    ds, pos, pt, pairs = asym_case("tgv2d", B=2)
    isl, N = ds.input_seq_length, pos.shape[1]
    trajs, one = [], set()
    for b in range(2):
        edges = oracle_edges(ds, pos[b], pt[b], isl)
        found = check_premise(edges, pairs, b)
        assert found == one_directional_edges(edges)
        one |= {(b, r, s) for r, s in found}
        trajs.append(list(zip(edges[0].tolist(), edges[1].tolist())))
    assert one == set(pairs)          # exactly the crafted pairs: the list holds no other one-directional edge
    return _padded(trajs, N, max(len(t) for t in trajs) + 7) + (N, one)


NAMES = ("three", "empty", "uneven", "asym")


def _msg(ne, e_cap, C_, seed, ints=False):
    """(B, E_cap, C) float32 with NaN in every pad slot; `ints`: small integers (every sum and product below is exact)."""
    rng = np.random.default_rng(seed)
    B = len(ne)
    m = rng.integers(-8, 9, (B, e_cap, C_)).astype(np.float32) if ints else \
        (rng.standard_normal((B, e_cap, C_)) * 10.0 ** rng.integers(-3, 4, (B, e_cap, 1))).astype(np.float32)
    for b in range(B):
        m[b, int(ne[b]):] = np.nan
    return m


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the checks
def check_map(rev, r, s, ne, unpaired):
    """involution; self-edges map to themselves; exactly `unpaired` are -1 among the real slots; every pad slot is -1; a partner
    is a real slot of the same trajectory holding the transposed edge."""
    B, E = r.shape
    assert rev.shape == (B, E) and rev.dtype == np.int32
    got = set()
    for b in range(B):
        n = int(ne[b])
        assert (rev[b, n:] == -1).all()
        for j in range(n):
            p = int(rev[b, j])
            if p < 0:
                got.add((b, int(r[b, j]), int(s[b, j])))
                continue
            assert 0 <= p < n and (r[b, p], s[b, p]) == (s[b, j], r[b, j])
            assert rev[b, p] == j                                   # involution
            if r[b, j] == s[b, j]:
                assert p == j                                       # a self-edge is its own partner
    assert got == set(unpaired), (sorted(got), sorted(unpaired))


def check_zeros(out, rev, ne):
    """unpaired and pad slots are +0.0 (all bits zero)"""
    for b in range(out.shape[0]):
        n = int(ne[b])
        assert (_u32(out[b, n:]) == 0).all(), "a pad slot is not +0.0"
        assert (_u32(out[b, :n][rev[b, :n] < 0]) == 0).all(), "an unpaired slot is not +0.0"


def check_symmetry(mode, out, msg, rev, ne):
    """swap(msg)[j] is msg[rev j] in bits; symmetrize(msg)[rev] == symmetrize(msg) in bits; antisymmetrize(msg)[rev] ==
    -antisymmetrize(msg) as values; a self-edge gives fl32(m + m) under symmetrize and +0.0 under antisymmetrize (finite m)."""
    for b in range(out.shape[0]):
        for j in range(int(ne[b])):
            p = int(rev[b, j])
            if p < 0:
                continue
            if mode == "swap":
                assert np.array_equal(_u32(out[b, j]), _u32(msg[b, p]))
            elif mode == "symmetrize":
                assert np.array_equal(_u32(out[b, p]), _u32(out[b, j]))
                if p == j:
                    assert np.array_equal(_u32(out[b, j]), _u32(msg[b, j] + msg[b, j])), "self-edge: fl32(m + m)"
            else:
                assert np.array_equal(out[b, p], -out[b, j])
                if p == j:
                    assert (_u32(out[b, j]) == 0).all(), "self-edge: +0.0"
                else:
                    assert np.array_equal(_u32(out[b, j]), _u32(msg[b, j] - msg[b, p]))


def check_adjoint(op, rev, ne, e_cap, C_=3, grad=None):
    """<op(a), b> == <a, grad(b)> with grad = op unless given, orbit by orbit of the map - {j, rev j}, a self-edge or an unpaired
    slot alone - on integer data, where every term is exact: the self-adjointness the backward rests on (the backward of op is
    op on the cotangent).  The two signs of antisymmetrize cancel: (I - P)^T = I - P for the involution P."""
    a, b_ = _msg(ne, e_cap, C_, 40, ints=True), _msg(ne, e_cap, C_, 41, ints=True)
    oa, ob = op(a), (grad or op)(b_)
    for t in range(a.shape[0]):
        for j in range(int(ne[t])):
            orbit = sorted({j, int(rev[t, j])} - {-1})
            lhs = sum(oa[t, q].astype(np.float64) * b_[t, q] for q in orbit)
            rhs = sum(a[t, q].astype(np.float64) * ob[t, q] for q in orbit)
            assert np.array_equal(lhs, rhs), (t, j)


# ------------------------------------------------------------------------------------------------ the twins on the lists
@pytest.mark.parametrize("name", NAMES)
def test_the_map_twin_on_hand_made_and_oracle_lists(name):
    r, s, ne, N, unpaired = _lists(name)
    rev = GR.np_reverse(r, s, ne)
    check_map(rev, r, s, ne, unpaired)
    if name == "empty":
        assert ne[1] == 0 and (rev[1] == -1).all()
    if name == "uneven":
        assert ne[0] != ne[1] and rev[1, :3].tolist() == [1, 0, 2]        # slots local to the trajectory, not to the batch
    if name == "three":
        assert rev[0, :8].tolist() == [0, 3, -1, 1, 4, 6, 5, 7]
    if name == "asym":
        assert len(unpaired) == 6 and (rev >= 0).sum() == ne.sum() - 6
    # a map that sends an unpaired slot to itself, and one that is not local to the trajectory, are told apart
    bad = rev.copy()
    for b in range(len(ne)):
        lone = np.flatnonzero(rev[b, :ne[b]] < 0)
        bad[b, lone] = lone
    with pytest.raises(AssertionError):
        check_map(bad, r, s, ne, unpaired)


@pytest.mark.parametrize("C_", [1, 5])
@pytest.mark.parametrize("name", NAMES)
def test_the_op_twins_are_symmetric_antisymmetric_zero_where_unpaired_and_self_adjoint(name, C_):
    r, s, ne, N, unpaired = _lists(name)
    rev = GR.np_reverse(r, s, ne)
    e_cap = r.shape[1]
    msg = _msg(ne, e_cap, C_, 7 + C_)
    for mode in GR.MODES:
        out = GR.np_edge_pair(mode, msg, rev, ne)
        assert out.dtype == np.float32 and np.isfinite(out).all()            # NaN in the pads of msg was never read
        check_zeros(out, rev, ne)
        check_symmetry(mode, out, msg, rev, ne)
        check_adjoint(lambda a: GR.np_edge_pair(mode, a, rev, ne), rev, ne, e_cap)
        assert GR.same_bits(GR.np_edge_pair_grad(mode, msg, rev, ne), out)
        # bfloat16: widen, the float32 loop, one rounding; swap copies the bits
        bits = GB.round_bf16(np.nan_to_num(msg))
        got = GR.np_edge_pair_bf16(mode, bits, rev, ne)
        assert got.dtype == np.uint16 and GB.same_bits(got, GB.round_bf16(GR.np_edge_pair(mode, GB.widen(bits), rev, ne)))
        # the torch composition over the map is the same float32 operation
        comp = GR.torch_edge_pair(mode, torch.tensor(np.nan_to_num(msg)), torch.tensor(rev)).numpy()
        assert GR.same_bits(comp, out)


def test_each_check_catches_the_mutated_twin_it_is_meant_for():
    r, s, ne, N, unpaired = _lists("uneven")
    rev = GR.np_reverse(r, s, ne)
    e_cap = r.shape[1]
    msg = _msg(ne, e_cap, 4, 3)
    assert set(GR.MUTANTS) == {"unpaired_pass_through", "self_edge_skipped", "antisymmetrize_adds", "pads_copied"}

    def twin(mode, mutant):
        return GR.np_edge_pair(mode, msg, rev, ne, mutant=mutant)

    for mode in GR.MODES:                                     # an unpaired slot passes msg[j] through: the zero check
        check_symmetry(mode, twin(mode, "unpaired_pass_through"), msg, rev, ne)
        with pytest.raises(AssertionError, match="unpaired"):
            check_zeros(twin(mode, "unpaired_pass_through"), rev, ne)
        with pytest.raises(AssertionError, match="pad"):      # the pads of msg copied out: the zero check
            check_zeros(twin(mode, "pads_copied"), rev, ne)
    check_zeros(twin("symmetrize", "self_edge_skipped"), rev, ne)
    with pytest.raises(AssertionError, match="self-edge"):    # a self-edge treated as unpaired: the self-edge rule
        check_symmetry("symmetrize", twin("symmetrize", "self_edge_skipped"), msg, rev, ne)
    with pytest.raises(AssertionError):                       # ... and swap must copy it
        check_symmetry("swap", twin("swap", "self_edge_skipped"), msg, rev, ne)
    check_zeros(twin("antisymmetrize", "antisymmetrize_adds"), rev, ne)
    with pytest.raises(AssertionError):                       # the wrong sign: out[rev] == -out
        check_symmetry("antisymmetrize", twin("antisymmetrize", "antisymmetrize_adds"), msg, rev, ne)
    # a backward that is not the op itself - an antisymmetrize whose backward carries a sign, a symmetrize whose backward is swap -
    # fails the adjoint check, and so does a map that is no involution
    with pytest.raises(AssertionError):
        check_adjoint(lambda a: GR.np_edge_pair("antisymmetrize", a, rev, ne), rev, ne, e_cap,
                      grad=lambda d: -GR.np_edge_pair("antisymmetrize", d, rev, ne))
    with pytest.raises(AssertionError):
        check_adjoint(lambda a: GR.np_edge_pair("symmetrize", a, rev, ne), rev, ne, e_cap,
                      grad=lambda d: GR.np_edge_pair("swap", d, rev, ne))
    half = rev.copy()
    half[0, 1] = -1                                           # a map that is no involution: slot 3 still points at slot 1
    with pytest.raises(AssertionError):
        check_adjoint(lambda a: GR.np_edge_pair("symmetrize", a, half, ne), half, ne, e_cap)


# ------------------------------------------------------------------------------------------------ the surface and the ABI
def test_graph_and_engine_have_the_new_ops():
    from lagrangebench_amd.engine import RolloutEngine, _GRAPH_OPS
    from lagrangebench_amd.graph import Graph
    for name in NEW_OPS:
        assert callable(getattr(Graph, name, None)), name
    assert isinstance(Graph.reverse, property)
    assert callable(RolloutEngine.graph_reverse) and callable(RolloutEngine.graph_edge_pair)
    assert _GRAPH_OPS["lb_graph_reverse"][0] == "lb_graph_reverse" and _GRAPH_OPS["lb_graph_edge_pair"][0] == "lb_graph_edge_pair_t"


@pytest.fixture(scope="module")
def lib():
    from lagrangebench_amd import build
    build.build()
    from lagrangebench_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from lagrangebench_amd import _lib
    text = open(os.path.join(ROOT, "include", "lbhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lb_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGS and hasattr(lib, name), name
    assert _lib._SIGS["lb_graph_edge_pair_t"][1][-1] is C.c_int32              # the trailing dtype
    modes = dict(re.findall(r"#define (LB_GRAPH_PAIR_[A-Z]+) (\d+)", header))
    assert modes == {"LB_GRAPH_PAIR_SWAP": "0", "LB_GRAPH_PAIR_SYM": "1", "LB_GRAPH_PAIR_ANTISYM": "2"}


def test_new_entries_refuse_a_null_engine(lib):
    from lagrangebench_amd import _lib
    for name in NEW_SYMBOLS:
        args = [None] + [1 if t is C.c_int32 else None for t in _lib._SIGS[name][1][1:]]
        assert getattr(lib, name)(*args) == -1, name
        assert b"null" in lib.lb_last_error()


def test_dtype_device_and_staleness_refusals_come_before_any_device_call():
    """A Graph over a stub engine without a library: every refusal below is raised from the shapes and dtypes alone."""
    from lagrangebench_amd.graph import Graph
    N, E = 3, 9
    engine = types.SimpleNamespace(B=2, N=N, e_cap=E, device=torch.device("cpu"), version=3)
    g = Graph(types.SimpleNamespace(engine=engine, version=3, batched=True))
    m = torch.zeros((2, E, 5))
    for op in (g.swap, g.symmetrize, g.antisymmetrize):
        for dt in (torch.float16, torch.float64, torch.int32):
            with pytest.raises(TypeError, match="float32 or bfloat16"):
                op(m.to(dt))
        with pytest.raises(ValueError, match="expected"):
            op(torch.zeros((2, E + 1, 5)))
        with pytest.raises(ValueError, match="expected"):
            op(torch.zeros((2, E)))
        with pytest.raises(TypeError, match="engine on"):
            op(m.to("meta"))
    engine.version = 4                                        # the list moved on: the staleness rule, before any launch
    for op in (g.swap, g.symmetrize, g.antisymmetrize):
        with pytest.raises(RuntimeError, match="stale"):
            op(m)
    with pytest.raises(RuntimeError, match="stale"):
        g.reverse
