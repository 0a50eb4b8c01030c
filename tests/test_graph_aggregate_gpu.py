"""graph.Graph.aggregate on the device (csrc/lb_graph.hip: k_graph_aggregate, k_graph_aggregate_bwd), over receivers and senders,
forward and backward.

Cases and columns are those of tests/test_graph_ops_gpu.py (its docstring says which path each reaches: both unit widths, a
row tail, more units than lanes, the radix-sorted sender view).  The planted rows of tests/_graph_aggregate.py are written into
the real slots of chosen nodes of each role; every pad slot holds NaN.

  1  forward and d_msg against the numpy float32 twin, bit for bit (a NaN matches a NaN), for each of the six single ops and
     three op sets: all six in another order, ("mean", "std") without winners, ("max", "min") without stats
  2  the sum / mean / max / min planes and their single-op gradients against this library's own segment_sum / segment_mean /
     segment_max / segment_min, bit for bit
  3  bfloat16: forward and backward equal the float32 op on the widened tensors, rounded once, bit for bit
  4  against the float64 restatement on random inputs: forward within 1e-5 max|msg|, d_msg within 1e-5 max|d_out| - the bound
     tests/test_graph_attention_gpu.py holds segment_softmax to.  It runs at eps = 1e-2: the std term t / (d std) amplifies the
     rounding of the mean (2^-24 |m|) by 1 / std <= 1 / sqrt(eps), 10 there; at 1e-5 that factor is 316 and a row of two nearly
     equal values would decide the outcome, not the kernel.  The measured deviations are printed.
  5  two calls give the same bits; the pad slots of d_msg are +0.0 with NaN in the pads of msg
  6  a storage one element off alignment takes the scalar path and gives the aligned call's bits
  7  a TorchModel with a PNA layer trains through Trainer in float32 and under autocast=torch.bfloat16; the loss goes down
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _graph_aggregate as AG  # noqa: E402
from tests import _graph_attention as GA  # noqa: E402
from tests import _graph_bf16 as GB  # noqa: E402
from tests.test_graph_ops_gpu import CASES, COLUMNS, ROLES, _bits, _build, _np  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
SETS = [(op,) for op in AG.OPS] + [("std", "max", "sum", "min", "mean", "var"), ("mean", "std"), ("max", "min")]
BF = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _setup(cid):
    """The cases of tests/test_graph_ops_gpu.py, built once for this file (that module's cached copies move on when a later
    test allocates another sample on their engine)."""
    return _build(cid)


def _dev(a, eng, grad=False):
    return torch.tensor(a, device=eng.device, requires_grad=grad)


def _pads_are_plus_zero(a, ne):
    return all((_bits(a[b, ne[b]:]) == 0).all() for b in range(a.shape[0]))


def _planted_input(rng, idx, ne, N, E, C):
    B = idx.shape[0]
    msg = (rng.standard_normal((B, E, C)) * 10.0 ** rng.integers(-2, 3, (B, E, 1))).astype(np.float32)
    return msg, AG.plant_rows(msg, idx, ne, N)


def _run(g, msg_t, role, ops, d_out_t, eps=EPS):
    """forward and backward of one aggregate -> (out, d_msg) as tensors"""
    leaf = msg_t.detach().clone().requires_grad_()
    out = g.aggregate(leaf, role, ops, eps)
    out.backward(d_out_t)
    return out.detach(), leaf.grad


# ------------------------------------------------------------------------------------------------ 1, 2, 5: the bits
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_aggregate_equals_the_twin_and_the_separate_ops_bit_for_bit(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(17 * C + len(cid))
    for role in ROLES:
        msg, placed = _planted_input(rng, idx[role], ne, N, E, C)
        assert {"tie", "zeros", "equal", "big", "nan"} <= set(placed) or cid == "lj", (cid, role, sorted(placed))
        md = _dev(msg, eng)
        full, win, stats = AG.np_aggregate(msg, idx[role], ne, N, AG.OPS, EPS)
        d_full = rng.standard_normal((B, N, 6, C)).astype(np.float32)
        for ops in SETS:
            planes = [AG.OPS.index(o) for o in ops]
            d_out = np.ascontiguousarray(d_full[:, :, planes])
            out, d_msg = _run(g, md, role, ops, _dev(d_out, eng))
            assert out.shape == (B, N, len(ops), C) and out.dtype == torch.float32 and d_msg.shape == (B, E, C)
            # ---- 1: the twin
            assert AG.same_bits(_np(out), full[:, :, planes]), (cid, role, C, ops)
            want = AG.np_aggregate_backward(d_out, msg, win, stats, idx[role], ne, ops)
            assert AG.same_bits(_np(d_msg), want), (cid, role, C, ops)
            # ---- 5: the pads of d_msg, a second call
            assert _pads_are_plus_zero(_np(d_msg), ne)
            out2, d_msg2 = _run(g, md, role, ops, _dev(d_out, eng))
            assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
            assert torch.equal(d_msg2.view(torch.int32), d_msg.view(torch.int32))
            # ---- 2: the library's own separate ops, forward and gradient
            if len(ops) == 1 and ops[0] in ("sum", "mean", "max", "min"):
                leaf = md.detach().clone().requires_grad_()
                own = getattr(g, "segment_" + ops[0])(leaf, role)
                own.backward(_dev(d_out[:, :, 0], eng))
                assert AG.same_bits(_np(out[:, :, 0]), _np(own)), (cid, role, C, ops)
                assert AG.same_bits(_np(d_msg), _np(leaf.grad)), (cid, role, C, ops)
        # segment_std / segment_var are the one-plane forms
        assert AG.same_bits(_np(g.segment_std(md, role, EPS)), full[:, :, 4]) and AG.same_bits(_np(g.segment_var(md, role)), full[:, :, 5])
        # what the planted rows are there for, read from the device result
        out = _np(g.aggregate(md, role, AG.OPS, EPS))
        if "equal" in placed:
            b, i, s = placed["equal"]
            assert not _bits(out[b, i, 5]).any() and (out[b, i, 4] == np.sqrt(np.float32(EPS))).all()
        empty = GA.np_degree(idx[role], ne, N) == 0
        assert not _bits(out[empty]).any()
        assert np.isnan(out).sum() == (6 * C if "nan" in placed else 0)          # the NaN of the pads reached nothing


# ------------------------------------------------------------------------------------------------ 3: bfloat16
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_bfloat16_is_the_float32_op_on_the_widened_tensors_rounded_once(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(19 * C + len(cid))
    for role in ROLES:
        msg, _ = _planted_input(rng, idx[role], ne, N, E, C)
        mb = _dev(msg, eng).to(BF)                                   # (the planted values are bfloat16 numbers but 4096 + j / 4)
        for ops in SETS[6:]:
            d_out = _dev(rng.standard_normal((B, N, len(ops), C)).astype(np.float32), eng).to(BF)
            out, d_msg = _run(g, mb, role, ops, d_out)
            assert out.dtype == BF and d_msg.dtype == BF
            out32, d32 = _run(g, mb.float(), role, ops, d_out.float())
            assert GB.same_bits(GB.torch_bits(out), GB.torch_bits(out32.to(BF))), (cid, role, C, ops)
            assert GB.same_bits(GB.torch_bits(d_msg), GB.torch_bits(d32.to(BF))), (cid, role, C, ops)
            assert all((GB.torch_bits(d_msg)[b, ne[b]:] == 0).all() for b in range(B))


# ------------------------------------------------------------------------------------------------ 4: float64
@pytest.mark.parametrize("C", COLUMNS)
@pytest.mark.parametrize("cid", CASES)
def test_aggregate_against_the_float64_restatement(cid, C):
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup(cid)
    B, N, E = eng.B, eng.N, eng.e_cap
    g = Graph(feats)
    rng = np.random.default_rng(23 * C + len(cid))
    eps, ops = 1e-2, ("std", "max", "sum", "min", "mean", "var")
    real = np.arange(E)[None, :] < ne[:, None]
    for role in ROLES:
        msg = rng.standard_normal((B, E, C)).astype(np.float32)
        d_out = rng.standard_normal((B, N, len(ops), C)).astype(np.float32)
        nan = msg.copy()
        nan[~real] = np.nan
        out, d_msg = _run(g, _dev(nan, eng), role, ops, _dev(d_out, eng), eps)
        cg = AG.CpuAggGraph(idx[role], idx[role], ne, N)
        x64 = torch.tensor(msg, dtype=torch.float64, requires_grad=True)
        o64 = cg.aggregate(x64, "senders", ops, eps)
        (o64 * torch.tensor(d_out, dtype=torch.float64)).sum().backward()
        fwd = np.abs(_np(out) - o64.detach().numpy()).max() / np.abs(msg).max()
        bwd = np.abs(_np(d_msg)[real] - x64.grad.numpy()[real]).max() / np.abs(d_out).max()
        print(f"[aggregate {cid} {role} C={C}] forward {fwd:.2e} of max|msg|; d_msg {bwd:.2e} of max|d_out|")
        assert fwd <= 1e-5, (cid, role, C, fwd)
        assert bwd <= 1e-5 and _pads_are_plus_zero(_np(d_msg), ne), (cid, role, C, bwd)


# ------------------------------------------------------------------------------------------------ 6: alignment
def test_a_storage_one_element_off_alignment_gives_the_same_bits():
    _need_gpu()
    from lagrangebench_amd.graph import Graph
    feats, eng, idx, ne, _, _ = _setup("rpf2d_b2")
    B, N, E, C = eng.B, eng.N, eng.e_cap, 64
    g = Graph(feats)
    rng = np.random.default_rng(29)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=eng.device)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
        return out

    ops = ("std", "max", "sum", "min", "mean", "var")
    for role in ROLES:
        msg, _ = _planted_input(rng, idx[role], ne, N, E, C)
        for dtype in (torch.float32, BF):
            md = _dev(msg, eng).to(dtype)
            d_out = _dev(rng.standard_normal((B, N, len(ops), C)).astype(np.float32), eng).to(dtype)
            out, d_msg = _run(g, md, role, ops, d_out)
            for m2, d2 in ((shifted(md), d_out), (md, shifted(d_out))):
                leaf = m2.requires_grad_()
                o2 = g.aggregate(leaf, role, ops, EPS)
                o2.backward(d2)
                same = AG.same_bits if dtype == torch.float32 else (lambda a, b: GB.same_bits(GB.torch_bits(a), GB.torch_bits(b)))
                cast = _np if dtype == torch.float32 else (lambda t: t)
                assert same(cast(o2.detach()), cast(out)) and same(cast(leaf.grad), cast(d_msg)), (role, dtype)


# ------------------------------------------------------------------------------------------------ shapes and refusals
def test_unbatched_features_trailing_dimensions_and_refusals():
    _need_gpu()
    from lagrangebench_amd._lib import LbHipError
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.graph import Graph
    from tests._common import hip_case
    ds = make_case("rpf2d", n_trajs=1, extra_seq_length=2, input_seq_length=6, scale=0.25)
    feats, _ = hip_case(ds).allocate_eval((ds[0][0][:, :6], ds[0][1]))
    assert not feats.batched
    eng = feats.engine
    g = Graph(feats)
    idx, ne = eng.nl_idx()
    idx, ne = _np(idx), _np(ne)
    N, E = eng.N, eng.e_cap
    msg = np.random.default_rng(2).standard_normal((E, 3, 4)).astype(np.float32)
    md = _dev(msg, eng, True)
    out = g.aggregate(md, "senders")
    assert out.shape == (N, 5, 3, 4) and g.segment_std(md, "senders").shape == (N, 3, 4) and g.segment_var(md, "senders").shape == (N, 3, 4)
    want, _, _ = AG.np_aggregate(msg.reshape(1, E, 12), idx[:, 1], ne, N, AG.OPS[:5], EPS)
    assert AG.same_bits(_np(out), want.reshape(N, 5, 3, 4))
    out.sum().backward()
    assert md.grad.shape == (E, 3, 4)
    with pytest.raises(RuntimeError):                      # once differentiable
        x = _dev(msg, eng, True)
        (d,) = torch.autograd.grad(g.segment_var(x, "senders").sum(), x, create_graph=True)
        d.sum().backward()
    # ---- the library's own refusals: a bad ops word, a missing side output
    flat = torch.zeros((E, 4), device=eng.device)
    for word in (0, 0x11, 0x7, 0x102, -1):
        with pytest.raises(LbHipError, match="-1.*ops"):
            eng.graph_aggregate(0, flat, word, 1e-5, 1)
    with pytest.raises(LbHipError, match="-1.*eps"):
        eng.graph_aggregate(0, flat, 0x5, 0.0, 1)
    with pytest.raises(LbHipError, match="-1.*null"):      # std in ops: msg and stats are required
        eng.graph_aggregate_backward(0, torch.zeros((N, 1, 4), device=eng.device), None, None, None, 0x5)
    # ---- a stale list
    leaf = _dev(msg, eng, True)
    res = g.aggregate(leaf, "receivers")
    eng.nl_update()
    with pytest.raises(RuntimeError, match="stale"):
        g.aggregate(_dev(msg, eng), "receivers")
    with pytest.raises(RuntimeError, match="stale"):
        res.sum().backward()


# ------------------------------------------------------------------------------------------------ 7: through the model path
@pytest.mark.parametrize("autocast", [None, BF], ids=["float32", "bfloat16"])
def test_a_pna_model_trains_through_the_trainer(autocast):
    _need_gpu()
    from lagrangebench_amd.data import make_case
    from lagrangebench_amd.models import TorchModel
    from lagrangebench_amd.train import Trainer
    from tests import _torch_models as TM
    from tests._common import hip_case
    isl = 6
    data_train = make_case("rpf2d", n_trajs=2, extra_seq_length=2, input_seq_length=isl, scale=0.25)
    data_valid = make_case("rpf2d", n_trajs=2, extra_seq_length=6, input_seq_length=isl, scale=0.25)
    case = hip_case(data_train)
    model = TorchModel(AG.TinyPNA(TM.node_in_of(case.engine(1)), 2, 32), autocast=autocast)
    cfg_train = {"batch_size": 2, "noise_std": 0.0, "pushforward": {"steps": [-1], "unrolls": [0], "probs": [1]},
                 "optimizer": {"lr_start": 1e-3, "lr_final": 1e-5, "lr_decay_rate": 0.1, "lr_decay_steps": 200}}
    trainer = Trainer(model, case, data_train, data_valid, cfg_train=cfg_train,
                      cfg_eval={"n_rollout_steps": 4, "train": {"n_trajs": 2, "metrics": ["mse"]}},
                      cfg_logging={"log_steps": 1, "eval_steps": 100}, input_seq_length=isl, seed=0)
    trainer.train(step_max=3)
    losses = [l for _, l in trainer.loss_log]
    print(f"[pna trainer {autocast}] losses {['%.5e' % l for l in losses]}")
    assert len(losses) >= 3 and np.isfinite(losses).all() and losses[-1] < losses[0]
