"""CPU side of the rollout-metric tests off the 64-multiple (tests/_metrics_twins.py; the device side is
tests/test_metrics_gpu.py): the premises the device test's inputs must meet, the NumPy twins of the device tiling against the
checks the device is held to, and the mutation table - wrong variants of the twins that those checks must catch on the grid."""
import numpy as np
import pytest

from tests import _metrics_twins as MT


# ---------------------------------------------------------------------------------------------- premises on the inputs
@pytest.mark.parametrize("cid", MT.SK_CASES + ["padded"])
def test_no_error_check_lands_on_the_threshold(cid):
    """Equal iteration counts are a fair demand only if no error the solver looks at sits on the threshold: every traced error
    of every problem of the case is more than 1e-6 relative away from 1e-4.  A condition on the inputs (seeds
    default_rng(N + dim), none had to be changed), not a tolerance on the device."""
    margins = [MT.trace_margin(info) for _, info in MT.sk_oracle(cid)]
    print(f"{cid}: iterations {[info['iters'] for _, info in MT.sk_oracle(cid)]}, nearest error {min(margins):.2e} of the threshold away")
    assert min(margins) > 1e-6
    assert all(len(tr) == it // 10 for _, info in MT.sk_oracle(cid) for tr, it in zip(info["traces"], info["iters"]))


def test_sinkhorn_trace_is_optional():
    x, y = MT.sk_frames(MT.sk_case("per3d-5"))[0][2:]
    disp = MT.displacement(*MT.GEOMS["per3d"])
    C = MT.SK.distance_matrix(disp, x, y)
    a = np.ones(5) / 5
    tr = []
    assert MT.SK.sinkhorn_solve(C, a, a, 0.01, trace=tr) == MT.SK.sinkhorn_solve(C, a, a, 0.01)
    assert len(tr) >= 1 and tr[-1] < 1e-4 and all(e >= 1e-4 for e in tr[:-1])
    assert np.isscalar(MT.SK.sinkhorn_divergence(disp, x, y))


def test_pot_reaches_every_exit_on_the_grid():
    """N = 3 in the periodic (1, 2) box runs xy to numItermax (exit 0); the stray particle ends xy with a numerical stop
    (exit 2); everything else converges (exit 1)."""
    _, oi = MT.pot_oracle("per2d_1x2-3")[0]
    assert oi["iters"][0] == 500 and oi["how"][0] == 0
    assert all(oi["how"][0] == 2 and oi["iters"][0] == 1 for _, oi in MT.pot_oracle("free2d-61-stray"))
    hows = {h for cid in MT.SK_CASES for _, oi in MT.pot_oracle(cid) for h in oi["how"]}
    assert hows == {0, 1, 2}


def test_iteration_counts_vary_over_the_grid():
    its = {info["iters"][0] for cid in MT.SK_CASES for _, info in MT.sk_oracle(cid)}
    assert len(its) >= 15 and min(its) == 10 and max(its) > 500


# ---------------------------------------------------------------------------------------------- twins against the checks
@pytest.mark.parametrize("cid", MT.METRIC_CASES)
def test_mse_mae_twin(cid):
    c = MT.metric_case(cid)
    assert c["pred"].shape[:2] == (3, MT.PRED_T) and c["target"].shape[:2] == (3, MT.TARGET_T)
    ref = MT.mse_mae_oracle(c, MT.N_STEPS)
    tw = MT.metrics_twin(c["pred"], c["target"], MT.N_STEPS, c["box"], c["periodic"])
    assert MT.metric_miss(tw["mse"], ref["mse"]) is None and MT.metric_miss(tw["mae"], ref["mae"]) is None
    assert len({float(v) for v in ref["mse"].ravel()}) == 3 * MT.N_STEPS       # distinct trajectories and frames


@pytest.mark.parametrize("cid", MT.GRID)
def test_ekin_twin(cid):
    c = MT.ekin_case(cid)
    for stride in MT.EKIN_STRIDES:
        ref = MT.ekin_oracle(c, c["roll"], stride)
        assert ref.shape == (3, -(-(MT.EKIN_T - 1) // stride))
        assert MT.metric_miss(MT.ekin_twin(c["roll"], stride, MT.DT * MT.WRITE_EVERY, MT.DX, c["box"], c["periodic"]), ref) is None


@pytest.mark.parametrize("cid", MT.SK_CASES + ["padded"])
def test_sinkhorn_twins(cid):
    c = MT._case_of(cid)
    for (b, k, x, y), (d, info), (pd, poi) in zip(MT.sk_frames(c), MT.sk_oracle(cid), MT.pot_oracle(cid)):
        out, iters = MT.sinkhorn_twin(x, y, c["box"], c["periodic"])
        assert MT.sk_miss(out, iters, d, info) is None, (b, k, MT.sk_miss(out, iters, d, info))
        out, info6 = MT.sinkhorn_pot_twin(x, y, c["box"], c["periodic"])
        assert MT.pot_miss(out, info6, pd, poi) is None, (b, k, MT.pot_miss(out, info6, pd, poi))


def test_padded_metric_twins():
    c = MT.padded_case()
    ref = MT.mse_mae_oracle(c)
    tw = MT.metrics_twin(c["pred"], c["target"], c["pred"].shape[1], c["box"], False)
    assert MT.metric_miss(tw["mse"], ref["mse"]) is None and MT.metric_miss(tw["mae"], ref["mae"]) is None
    dx = float(c["md"]["dx"])
    assert MT.metric_miss(MT.ekin_twin(c["pred"], 2, MT.DT * MT.WRITE_EVERY, dx, c["box"], False), MT.ekin_oracle(c, c["pred"], 2)) is None


# ---------------------------------------------------------------------------------------------- mutation table
# the Sinkhorn mutants run on the first problem of the cases up to N = 67 and of the stray-particle case: every tail they cut
# exists there (N = 67: np % 64 = 3, nq % 4 = 3); a mutant is stopped ten iterations past the oracle's count, where it has
# missed the check whatever it would go on to do
_SK_MUT_CASES = [c for c in MT.SK_CASES if MT._parse(c)[1] <= 67]


def _catches(mut):
    hit = []
    if mut in ("box0_every_axis", "skip_wrap", "pred_T_frames"):
        for cid in MT.METRIC_CASES:
            c = MT.metric_case(cid)
            ref = MT.mse_mae_oracle(c, MT.N_STEPS)
            tw = MT.metrics_twin(c["pred"], c["target"], MT.N_STEPS, c["box"], c["periodic"], mut)
            hit += [f"{k}:{cid}" for k in ("mse", "mae") if MT.metric_miss(tw[k], ref[k])]
    if mut in ("box0_every_axis", "skip_wrap"):
        for cid in MT.GRID:
            c = MT.ekin_case(cid)
            tw = MT.ekin_twin(c["roll"], 3, MT.DT * MT.WRITE_EVERY, MT.DX, c["box"], c["periodic"], mut)
            hit += [f"e_kin:{cid}"] if MT.metric_miss(tw, MT.ekin_oracle(c, c["roll"], 3)) else []
    if mut != "pred_T_frames":
        for cid in _SK_MUT_CASES:
            c = MT.sk_case(cid)
            _, _, x, y = MT.sk_frames(c)[0]
            d, info = MT.sk_oracle(cid)[0]
            out, iters = MT.sinkhorn_twin(x, y, c["box"], c["periodic"], mut=mut, max_it=tuple(i + 10 for i in info["iters"]))
            hit += [f"sinkhorn:{cid}"] if MT.sk_miss(out, iters, d, info) else []
            if mut != "idle_lane_zero":                        # the POT sweeps are plain sums: an idle lane holds 0 either way
                out, info6 = MT.sinkhorn_pot_twin(x, y, c["box"], c["periodic"], mut=mut)
                hit += [f"sinkhorn_pot:{cid}"] if MT.pot_miss(out, info6, *MT.pot_oracle(cid)[0]) else []
    return hit


@pytest.mark.parametrize("mut", MT.MUTATIONS)
def test_mutation_is_caught(mut):
    hit = _catches(mut)
    print(f"{mut}: caught by {len(hit)} checks: {' '.join(hit)}")
    assert hit, f"{mut} survives the grid"
    if mut == "idle_lane_zero":
        # lb_lse_merge rescales by exp(m - m2): an idle lane read as (0, 0) changes the result only where that factor underflows,
        # which the uniform clouds never reach (|z| <~ 100) - the stray-particle case is in the grid for this mutation
        assert hit == ["sinkhorn:free2d-61-stray"]
    if mut == "box0_every_axis":
        assert all("per2d_1x2" in h for h in hit)
    if mut == "skip_wrap":
        assert not any("free2d" in h or "ldc3d" in h for h in hit)
    if mut == "drop_tail_sources":
        assert {f"sinkhorn:{g}-67" for g in MT.GEOMS} <= set(hit) and {f"sinkhorn_pot:{g}-67" for g in MT.GEOMS} <= set(hit)
    if mut == "drop_tail_outputs":
        assert {f"sinkhorn:{g}-{n}" for g in MT.GEOMS for n in (3, 5, 61, 67)} <= set(hit)
    if mut == "pred_T_frames":
        assert len(hit) == 2 * len(MT.METRIC_CASES)
