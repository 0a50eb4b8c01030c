"""Device side of the rollout-metric tests off the 64-multiple: k_metrics / k_ekin (lb_state.hip) and lb_sinkhorn /
lb_sinkhorn_pot (lb_sinkhorn.hip) against their oracles at N in {3, 5, 61, 67, 190, 257} in free space, in the periodic unit
cube and in a periodic (1, 2) box, with B > 1, pred_T != target_T and n_steps < T, on a padded batch, and through every exit of
the POT loop.  Inputs, oracle results and checks come from tests/_metrics_twins.py; tests/test_metrics.py shows on the CPU that
these inputs meet the premises of the checks and that the checks catch a wrong walk of the tiles."""
import numpy as np
import pytest
import torch

from tests import _metrics_twins as MT

pytestmark = pytest.mark.gpu

_CASES = {}


def _np(t):
    return t.detach().cpu().numpy()


def _hip(c):
    """One CaseSetupFn (and through it one engine per batch size) per particle count and geometry."""
    key = (int(c["md"]["num_particles_max"]), tuple(float(b) for b in c["box"]), bool(c["periodic"]))
    if key not in _CASES:
        _CASES[key] = MT.hip_case_of(c["md"])
    return _CASES[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_np(a).view(np.int64), _np(b).view(np.int64))


# ---------------------------------------------------------------------------------------------- mse / mae
@pytest.mark.parametrize("cid", MT.METRIC_CASES)
def test_mse_mae_match_oracle(cid):
    """B = 3 distinct trajectories, pred_T = 9, target_T = 12, n_steps = 7, per trajectory at rtol 1e-12; mse alone and mae
    alone (the other output pointer null) give the bits of the joint call."""
    c = MT.metric_case(cid)
    eng = _hip(c).engine(3)
    pred, target = _t(c["pred"]), _t(c["target"])
    m = eng.metrics(pred, target, MT.N_STEPS, want=("mse", "mae"))
    ref = MT.mse_mae_oracle(c, MT.N_STEPS)
    for k in ("mse", "mae"):
        miss = MT.metric_miss(_np(m[k]), ref[k])
        print(f"{cid} {k}: max relative error {np.max(np.abs(_np(m[k]) - ref[k]) / ref[k]):.2e}")
        assert miss is None, (k, miss)
        alone = eng.metrics(pred, target, MT.N_STEPS, want=(k,))
        assert set(alone) == {k} and _same_bits(alone[k], m[k])


@pytest.mark.parametrize("cid", ["free2d-257", "per3d-67", "per2d_1x2-5"])
def test_metrics_computer_cuts_a_longer_target(cid):
    """MetricsComputer hands the engine the non-contiguous slice tgt[:, :T] of a target longer than the prediction (B = 2): the
    same bits as the calls on a contiguous, truncated copy."""
    from lagrangebench_amd.evaluate import MetricsComputer
    c = MT.metric_case(cid)
    hcase = _hip(c)
    eng = hcase.engine(2)
    pred, target = _t(c["pred"][:2]), _t(c["target"][:2])
    assert target.shape[1] > pred.shape[1] and not target[:, :MT.PRED_T].is_contiguous()
    mc = MetricsComputer(["mse", "mae", "e_kin"], hcase.displacement, c["md"], 6, stride=3, case=hcase)
    got = mc(pred, target)
    cut = _t(c["target"][:2, :MT.PRED_T])
    want = eng.metrics(pred, cut, MT.PRED_T, want=("mse", "mae"))
    assert _same_bits(got["mse"], want["mse"]) and _same_bits(got["mae"], want["mae"])
    assert _same_bits(got["e_kin"]["target"], eng.ekin(cut, 3, MT.DT * MT.WRITE_EVERY, MT.DX))
    assert _same_bits(got["e_kin"]["predicted"], eng.ekin(pred, 3, MT.DT * MT.WRITE_EVERY, MT.DX))
    ref = MT.mse_mae_oracle(dict(c, pred=c["pred"][:2], target=c["target"][:2]), MT.PRED_T)
    assert MT.metric_miss(_np(got["mse"]), ref["mse"]) is None and MT.metric_miss(_np(got["mae"]), ref["mae"]) is None


# ---------------------------------------------------------------------------------------------- e_kin
@pytest.mark.parametrize("cid", MT.GRID)
def test_ekin_matches_oracle(cid):
    """T = 24 at strides 1, 3, 10 (T - 1 = 23 is a multiple of neither 3 nor 10), dt * write_every = 0.01, B = 3."""
    c = MT.ekin_case(cid)
    eng = _hip(c).engine(3)
    roll = _t(c["roll"])
    for stride in MT.EKIN_STRIDES:
        got = _np(eng.ekin(roll, stride, MT.DT * MT.WRITE_EVERY, MT.DX))
        ref = MT.ekin_oracle(c, c["roll"], stride)
        assert got.shape == (3, -(-(MT.EKIN_T - 1) // stride))
        print(f"{cid} stride {stride}: max relative error {np.max(np.abs(got - ref) / ref):.2e}")
        assert MT.metric_miss(got, ref) is None, (stride, MT.metric_miss(got, ref))


def test_metric_entry_points_refuse_bad_shapes():
    from lagrangebench_amd._lib import LbHipError
    c = MT.metric_case("free2d-5")
    eng = _hip(c).engine(3)
    pred, target = _t(c["pred"]), _t(c["target"])
    with pytest.raises(LbHipError, match="T >= 2"):
        eng.ekin(pred[:, :1], 1, 0.01, MT.DX)
    for stride in (0, -1):
        with pytest.raises(LbHipError, match="stride >= 1"):
            eng.ekin(pred, stride, 0.01, MT.DX)
        with pytest.raises(LbHipError, match="stride >= 1"):
            eng.sinkhorn(pred, target, stride)
        with pytest.raises(LbHipError, match="stride >= 1"):
            eng.sinkhorn_pot(pred, target, stride)
    with pytest.raises(LbHipError, match="n_steps exceeds"):
        eng.metrics(pred, target, MT.PRED_T + 1)                       # n_steps > pred_T
    with pytest.raises(LbHipError, match="n_steps exceeds"):
        eng.metrics(target, pred, MT.PRED_T + 1)                       # n_steps > target_T
    assert eng.metrics(pred, target, MT.PRED_T)["mse"].shape == (3, MT.PRED_T)


# ---------------------------------------------------------------------------------------------- sinkhorn
def _sinkhorn_checks(cid, c, eng):
    out, iters = eng.sinkhorn(_t(c["pred"][:, :MT.SK_T]), _t(c["target"][:, :MT.SK_T]), MT.SK_STRIDE, return_iters=True)
    out = _np(out)
    assert out.shape == (MT.SK_B, 2) and iters.shape == (MT.SK_B, 2, 3)
    for (b, k, _, _), (d, info) in zip(MT.sk_frames(c), MT.sk_oracle(cid)):
        print(f"{cid} [{b},{k}]: iterations {tuple(iters[b, k])} / {info['iters']}, value off by {abs(out[b, k] - d):.2e} "
              f"(allowed {1e-9 * info['reg'][0] + 1e-6 * abs(d):.2e})")
        miss = MT.sk_miss(out[b, k], iters[b, k], d, info)
        assert miss is None, (b, k, miss)


def _pot_checks(cid, c, eng):
    out, info = eng.sinkhorn_pot(_t(c["pred"][:, :MT.SK_T]), _t(c["target"][:, :MT.SK_T]), MT.SK_STRIDE, return_info=True)
    out = _np(out)
    assert out.shape == (MT.SK_B, 2) and info.shape == (MT.SK_B, 2, 6)
    for (b, k, _, _), (d, oi) in zip(MT.sk_frames(c), MT.pot_oracle(cid)):
        print(f"{cid} [{b},{k}]: iterations, exits {tuple(info[b, k])} / {oi['iters'] + oi['how']}, value off by "
              f"{abs(out[b, k] - float(d)):.2e} (allowed {3e-7 * float(oi['values'][0]):.2e})")
        miss = MT.pot_miss(out[b, k], info[b, k], d, oi)
        assert miss is None, (b, k, miss)
    return info


@pytest.mark.parametrize("cid", MT.SK_CASES)
def test_sinkhorn_matches_oracle(cid):
    """B = 2, T = 3, stride 2: four problems a case, every output slot and iteration triple against the OTT restatement."""
    c = MT.sk_case(cid)
    _sinkhorn_checks(cid, c, _hip(c).engine(MT.SK_B))


@pytest.mark.parametrize("cid", MT.SK_CASES)
def test_sinkhorn_pot_matches_oracle(cid):
    """The same problems against the POT restatement; the grid holds all three exits of the loop: N = 3 in the (1, 2) box ends
    at numItermax (500 iterations, exit 0), the stray particle with a numerical stop, the rest converged."""
    c = MT.sk_case(cid)
    info = _pot_checks(cid, c, _hip(c).engine(MT.SK_B))
    if cid == "per2d_1x2-3":
        assert info[0, 0, 0] == 500 and info[0, 0, 3] == 0
    if cid == "free2d-61-stray":
        assert (info[:, :, 0] == 1).all() and (info[:, :, 3] == 2).all()


# ---------------------------------------------------------------------------------------------- padded batch
def test_padded_batch_all_four_metrics():
    """waterdrop2d, 190 and 61 real particles padded to 257, B = 2, pads at position 0 in both clouds as the reference pads them:
    the four metrics equal the oracles on the same padded arrays - divisor N * dim and uniform weights 1 / N with the pads
    counted, which is what the reference computes on padded data (pinned, not proposed)."""
    c = MT.padded_case()
    from tests._common import hip_case
    hcase = hip_case(c["ds"])
    eng = hcase.engine(2)
    assert eng.N == 257
    pred, target = _t(c["pred"]), _t(c["target"])
    T = pred.shape[1]
    m = eng.metrics(pred, target, T, want=("mse", "mae"))
    ref = MT.mse_mae_oracle(c)
    assert MT.metric_miss(_np(m["mse"]), ref["mse"]) is None and MT.metric_miss(_np(m["mae"]), ref["mae"]) is None
    # the pads add nothing to the sums and count in the divisor: the mean over the real particles alone is N / n_b larger
    disp = MT.displacement(c["box"], False)
    for b, n in enumerate(MT.PADDED[1]):
        real = MT.O.metrics_mse_mae(disp, c["pred"][b][:, :n], c["target"][b][:, :n])["mse"]
        assert np.allclose(_np(m["mse"])[b] * 257 / n, real, rtol=1e-12, atol=0)
    dx = float(c["md"]["dx"])
    for roll, a in ((pred, c["pred"]), (target, c["target"])):
        got = _np(eng.ekin(roll, 2, MT.DT * MT.WRITE_EVERY, dx))
        assert MT.metric_miss(got, MT.ekin_oracle(c, a, 2)) is None
    _sinkhorn_checks("padded", c, eng)
    _pot_checks("padded", c, eng)
