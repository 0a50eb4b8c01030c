"""The window gradient of a user's torch network: ``lb_graph_features_backward`` (the transpose of the feature builder as a graph
op), ``graph.differentiable_features``, ``autograd.TorchModule`` and ``autograd.advance_window`` on the device.

Cases (the smallest synthetic ones): rpf2d at scale 0.25, B = 1 and B = 2 (200 particles, periodic, an external force); ldc3d at
scale 0.3 in free space (walls: the bound feature, kinematic particles of types 1 and 2, dim 3); rpf2d with magnitude
features; and a list with one-directional edges from ``tests/_asym.py`` (B = 2), whose sender view goes through the radix sort.

Yardsticks: ``tests/_features_torch.py`` (the feature builder restated from the reference, float64 autograd) and
``tests/_torch_models.py`` (``TinyMP``, ``CpuGraph``) on the engine's own edge lists.
Bars - the project's for the same quantities (tests/test_torch_model_gpu.py, tests/test_autograd_gpu.py): forward and loss
within 1e-5 of the largest entry; d loss / d window and every gradient leaf within 1e-4 of its largest entry against float64;
a parameter leaf past that bar is held to 3x the float32 restatement's own deviation and printed.  Every test prints its
measured maximum.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _torch_models as TM  # noqa: E402
from tests._common import hip_case  # noqa: E402
from tests._features_torch import case_constants, displacement_torch, features_torch  # noqa: E402

pytestmark = pytest.mark.gpu

ISL = 6
#        name, scale, B, free space (-> bound feature), magnitude features, one-directional edges
CASES = {"rpf2d_b1": ("rpf2d", 0.25, 1, False, False, False),
         "rpf2d_b2": ("rpf2d", 0.25, 2, False, False, False),
         "ldc3d": ("ldc3d", 0.3, 1, True, False, False),
         "rpf2d_mag": ("rpf2d", 0.25, 1, False, True, False),
         "asym_b2": ("rpf2d", 0.5, 2, False, False, True)}
EDGE_KEYS = ("rel_disp", "rel_dist")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _setup(cid):
    """(dataset, engine case, pos (B, N, T, dim) float64, particle types (B, N), the feature builder's constants)."""
    from lagrangebench_amd.data import make_case
    name, scale, B, free, mag, asym = CASES[cid]
    if asym:
        from tests._asym import asym_case
        ds, pos, pt, _ = asym_case(name, B=B, scale=scale, isl=ISL)
    else:
        ds = make_case(name, n_trajs=B, extra_seq_length=4, input_seq_length=ISL, scale=scale)
        if free:
            ds.metadata["periodic_boundary_conditions"] = [False] * len(ds.box)
        if mag:
            ds.magnitude_features = True
        pos = np.stack([ds[b][0] for b in range(B)]).astype(np.float64)
        pt = np.stack([ds[b][1] for b in range(B)])
    return ds, hip_case(ds), pos, pt, case_constants(ds)


def _allocate(cid):
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, _ = hcase.allocate_eval((pos[:, :, :ISL], pt))
    return feats, feats.engine


def _list(eng):
    """The engine's current list: (idx (B, 2, E_cap) int64 host, n_edges (B,) host, [(receivers, senders)] of the real slots)."""
    idx, ne = eng.nl_idx()
    idx, ne = idx.cpu().long(), ne.cpu().long()
    return idx, ne, [(idx[b, 0, :int(ne[b])], idx[b, 1, :int(ne[b])]) for b in range(eng.B)]


def _force(eng):
    f = eng.node_features().get("force")
    return None if f is None else f.cpu()


def _model(cid, eng):
    from lagrangebench_amd.models import TorchModel
    model = TorchModel(TM.TinyMP(TM.node_in_of(eng), eng.dim, 32))
    params, state = model.init(np.array([7]), None)
    rng = np.random.default_rng(3)   # the defaults (gain 1, in_scale 1) would leave those two paths unseen
    params["~"]["gain"] = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32)
    state["~"]["in_scale"] = (1.0 + 0.1 * rng.standard_normal(state["~"]["in_scale"].shape)).astype(np.float32)
    model.set_state(state)
    return model, params, state


class _Cpu:
    device = torch.device("cpu")


def _mse(pred, target, mask):
    """The reference's _mse summed over the batch (trainer.py:35-60): squared error over dim, mean over the non-kinematic."""
    per = torch.where(mask, ((pred - target) ** 2).sum(-1), torch.zeros((), dtype=pred.dtype, device=pred.device))
    return (per.sum(1) / mask.sum(1)).sum()


def _mask(pt, device="cpu"):
    pt = torch.as_tensor(np.asarray(pt))
    return (~((pt == 1) | (pt == 2) | (pt == -1))).to(device)


def _restate(module, dtype, windows, edges, force, pt, consts, idx, ne):
    """TinyMP in `dtype` on the CPU: features (float64, tests/_features_torch.py) of every trajectory's window on its edge
    list, cast to `dtype`, the graph ops of CpuGraph in the padded layout of `idx`.  -> prediction (B, N, dim)."""
    B, E_cap, N = idx.shape[0], idx.shape[2], windows[0].shape[0]
    per = [features_torch(windows[b], edges[b][0], edges[b][1], force=None if force is None else force[b], **consts)
           for b in range(B)]
    fd = {}
    for k in per[0]:
        if k in ("node", "edge"):
            continue
        rows = []
        for b in range(B):
            v = per[b][k]
            if k in EDGE_KEYS:
                v = torch.cat([v, v.new_zeros((E_cap - v.shape[0], v.shape[1]))])
            rows.append(v)
        fd[k] = torch.stack(rows).to(dtype)
    g = TM.CpuGraph(idx[:, 1], idx[:, 0], ne, N)
    return module(fd, torch.as_tensor(pt).long(), g)


def _leaf_report(tag, dev, r64, r32):
    """dev, r64, r32: {leaf name: gradient}.  Every leaf within 1e-4 of its largest float64 entry, or - printed - within 3x the
    float32 restatement's own deviation."""
    worst, loose = 0.0, []
    for name, ref in r64.items():
        ref = np.asarray(ref, np.float64)
        scale = max(np.abs(ref).max(), 1e-30)
        d = np.abs(np.asarray(dev[name], np.float64) - ref).max()
        if d / scale <= 1e-4:
            worst = max(worst, d / scale)
            continue
        d32 = np.abs(np.asarray(r32[name], np.float64) - ref).max()
        assert d <= 3 * d32, (tag, name, d / scale, d32 / scale)
        loose.append(f"{name} ({d / scale:.2e}, fp32 {d32 / scale:.2e})")
    print(f"[torch window grad {tag}] worst relative gradient leaf {worst:.2e}; held to the fp32 restatement: {loose or 'none'}")


def _grads(module):
    return {n: _np(p.grad) for n, p in module.named_parameters()}


# ------------------------------------------------------------------------------------------------ 1. the op alone
@pytest.mark.parametrize("cid", list(CASES))
def test_features_backward_matches_float64_autograd_of_the_feature_builder(cid):
    """Random float32 cotangents for every feature of the case, NaN in every pad slot of the edge-shaped ones:
    graph_features_backward against d / d window of sum_k <c_k, f_k(window)> by float64 autograd of features_torch on the
    engine's own list - all cotangents at once, then each alone.

    Measured on an MI355X, deviation / largest entry: all cotangents 1.4e-8 - 3.0e-8 in the five cases; alone, abs_pos, rel_disp and
    bound 0 - 3e-16, vel_hist 1.7e-16, rel_dist 3.0e-8 - 4.1e-8, vel_mag 4.5e-8 (the two that divide by a float32 forward value)."""
    _need_gpu()
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, eng = _allocate(cid)
    B, N, dim, E_cap = eng.B, eng.N, eng.dim, eng.e_cap
    idx, ne, edges = _list(eng)
    if CASES[cid][5]:
        from tests._asym import one_directional_edges
        for b in range(B):
            assert one_directional_edges(np.stack([_np(edges[b][0]), _np(edges[b][1])]))
        sorts0 = eng.graph_sender_sorts()
    force = _force(eng)
    gen = torch.Generator().manual_seed(11)
    shapes = {"abs_pos": (B * N, ISL, dim), "vel_hist": (B * N, (ISL - 1) * dim), "rel_disp": (B * E_cap, dim),
              "rel_dist": (B * E_cap, 1)}
    if eng.has_vel_mag:
        shapes["vel_mag"] = (B * N, ISL - 1)
    if eng.has_bound:
        shapes["bound"] = (B * N, 2 * dim)
    assert eng.has_vel_mag == CASES[cid][4] and eng.has_bound == CASES[cid][3]
    cot = {k: torch.randn(s, generator=gen, dtype=torch.float32) for k, s in shapes.items()}
    real = (torch.arange(E_cap)[None, :] < ne[:, None]).reshape(-1)
    assert int((~real).sum()) > 0
    for k in EDGE_KEYS:
        cot[k][~real] = float("nan")
    dev = {k: v.to(eng.device) for k, v in cot.items()}

    # the reference: one gradient per cotangent, shared by every comparison below
    ref = {k: np.zeros((B, N, ISL, dim)) for k in cot}
    for b in range(B):
        w = torch.as_tensor(pos[b, :, :ISL]).clone().requires_grad_(True)
        f = features_torch(w, edges[b][0], edges[b][1], force=None if force is None else force[b], **consts)
        f["abs_pos"] = w
        E = int(ne[b])
        for k in cot:
            rows = E_cap if k in EDGE_KEYS else N
            c = cot[k].reshape((B, rows) + shapes[k][1:])[b].double()
            c = c[:E] if k in EDGE_KEYS else c
            (g,) = torch.autograd.grad((c * f[k].reshape(c.shape)).sum(), w, retain_graph=True)
            ref[k][b] = g.numpy()

    def check(tag, got, want):
        assert got.dtype == torch.float64 and tuple(got.shape) == (B, N, ISL, dim)
        got = _np(got)
        assert np.isfinite(got).all()           # no pad slot (NaN) was read
        scale = np.abs(want).max()
        assert scale > 0
        err = np.abs(got - want).max() / scale
        print(f"[features_backward {cid} {tag}] largest entry {scale:.3e}, relative error {err:.2e}")
        assert err < 1e-4, (cid, tag, err)
        return got

    all_got = eng.graph_features_backward(**{"d_" + k: v for k, v in dev.items()})
    all_np = check("all", all_got, sum(ref.values()))
    again = eng.graph_features_backward(**{"d_" + k: v for k, v in dev.items()})
    assert torch.equal(all_got.view(torch.int64), again.view(torch.int64))          # two calls: the same bits
    for k in cot:
        check(k, eng.graph_features_backward(**{"d_" + k: dev[k]}), ref[k])
    zero = eng.graph_features_backward()
    assert int(zero.view(torch.int64).abs().max()) == 0                             # every entry is +0.0
    # older frames and the newest one both carry gradient; kinematic rows are whatever the mathematics says
    assert np.abs(all_np[:, :, :-1]).max() > 0 and np.abs(all_np[:, :, -1]).max() > 0
    kin = (pt == 1) | (pt == 2)
    if cid == "ldc3d":
        assert kin.any() and np.abs(all_np[kin]).max() > 0
    if CASES[cid][5]:
        assert eng.graph_sender_sorts() > sorts0                                    # the one-directional path was taken
    # the refusals of the binding
    with pytest.raises(ValueError, match="lb_graph_features_backward"):
        eng.graph_features_backward(d_vel_hist=dev["vel_hist"][:-1])
    with pytest.raises(ValueError, match="lb_graph_features_backward"):
        eng.graph_features_backward(d_vel_hist=dev["vel_hist"].double())
    with pytest.raises(ValueError, match="lb_graph_features_backward"):
        eng.graph_features_backward(d_rel_disp=dev["rel_disp"].cpu())
    if not eng.has_vel_mag:
        with pytest.raises(ValueError, match="vel_mag"):
            eng.graph_features_backward(d_vel_mag=torch.zeros((B * N, ISL - 1), device=eng.device))
    if not eng.has_bound:
        with pytest.raises(ValueError, match="bound"):
            eng.graph_features_backward(d_bound=torch.zeros((B * N, 2 * dim), device=eng.device))


# ------------------------------------------------------------------------------------------------ 2. differentiable_features
@pytest.mark.parametrize("cid", ["rpf2d_b2", "ldc3d"])
def test_differentiable_features_bits_and_rules(cid):
    _need_gpu()
    from lagrangebench_amd.graph import differentiable_features
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, eng = _allocate(cid)
    w = torch.as_tensor(pos[:, :, :ISL], device=eng.device).requires_grad_(True)
    fd = differentiable_features(feats, w)
    assert list(fd) == feats.keys()
    for k in feats.keys():
        want = feats[k].to(torch.int64 if k in ("senders", "receivers") else torch.float32)
        assert fd[k].dtype == want.dtype and torch.equal(fd[k], want), k
        assert fd[k].requires_grad == (k not in ("senders", "receivers", "force")), k
    # the backward is the op: the same bits as a direct call with the same cotangents
    gen = torch.Generator().manual_seed(2)
    c_v = torch.randn(fd["vel_hist"].shape, generator=gen).to(eng.device)
    c_d = torch.randn(fd["rel_dist"].shape, generator=gen).to(eng.device)
    ((fd["vel_hist"] * c_v).sum() + (fd["rel_dist"] * c_d).sum()).backward()
    direct = eng.graph_features_backward(d_vel_hist=c_v.reshape(eng.B * eng.N, -1), d_rel_dist=c_d.reshape(-1, 1))
    assert torch.equal(w.grad.view(torch.int64), direct.view(torch.int64))
    # once differentiable
    fd = differentiable_features(feats, w)
    (g,) = torch.autograd.grad((fd["rel_disp"] ** 2).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated"):
        g.sum().backward()
    # the staleness rule, in the backward and in the forward
    fd = differentiable_features(feats, w)
    eng.nl_update()
    with pytest.raises(RuntimeError, match="stale"):
        fd["vel_hist"].sum().backward()
    with pytest.raises(RuntimeError, match="stale"):
        differentiable_features(feats, w)


# ------------------------------------------------------------------------------------------------ 3. one step
@pytest.mark.parametrize("cid", list(CASES))
def test_one_step_through_torch_module_matches_the_float64_restatement(cid):
    """TinyMP (hidden 32) through TorchModule: the prediction against TorchModel.apply, the loss, d loss / d window and every
    parameter's gradient against float64 TinyMP on CpuGraph + features_torch; with handle= the gradients land in the handle's
    blob.  Measured on an MI355X (rpf2d B = 1 / B = 2 / ldc3d / magnitude / one-directional): bit-equal to TorchModel.apply;
    forward 4.1e-7 / 4.0e-7 / 2.3e-7 / 2.7e-7 / 4.3e-7; loss 2.5e-8 / 3.3e-8 / 2.1e-8 / 1.0e-7 / 6.9e-8; d loss / d window 1.8e-7 /
    1.4e-7 / 1.7e-7 / 2.4e-7 / 2.1e-7; worst parameter leaf 1.0e-6 / 1.9e-6 / 2.2e-6 / 8.9e-7 / 2.4e-6; no leaf needed the allowance."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, eng = _allocate(cid)
    B, N, dim = eng.B, eng.N, eng.dim
    model, params, state = _model(cid, eng)
    applied = model.apply(params, state, (feats, pt))[0]["acc"]
    mod = TorchModule(model, hcase, params, B, state=state)
    assert mod.engine is eng and len(list(mod.parameters())) == len(model._names)
    window = torch.as_tensor(pos[:, :, :ISL], device=eng.device).requires_grad_(True)
    target = torch.randn((B, N, dim), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    pred = mod(window, pt)["acc"]
    assert pred.dtype == torch.float32 and pred.grad_fn is not None and tuple(pred.shape) == (B, N, dim)
    e_apply = float((pred.detach() - applied).abs().max() / applied.abs().max())
    assert e_apply <= 1e-5, e_apply
    loss = _mse(pred, target.to(eng.device).float(), _mask(pt, eng.device))
    loss.backward()
    assert mod.restored == 0
    idx, ne, edges = _list(eng)
    force = _force(eng)
    got_w, got_p = _np(window.grad), _grads(mod.module)

    refs = {}
    for dt in (torch.float64, torch.float32):
        m = model._device_module(_Cpu(), params, state).to(dt)
        ws = [torch.as_tensor(pos[b, :, :ISL]).clone().requires_grad_(True) for b in range(B)]
        pr = _restate(m, dt, ws, edges, force, pt, consts, idx, ne)
        ls = _mse(pr, target.to(dt), _mask(pt))
        ls.backward()
        refs[dt] = (pr.detach().double().numpy(), float(ls.detach()), np.stack([w.grad.numpy() for w in ws]), _grads(m))
    p64, l64, w64, g64 = refs[torch.float64]
    e_fwd = np.abs(_np(pred).astype(np.float64) - p64).max() / np.abs(p64).max()
    e_loss = abs(float(loss.detach()) - l64) / abs(l64)
    e_win = np.abs(got_w - w64).max() / np.abs(w64).max()
    print(f"[torch window grad one step {cid}] vs TorchModel.apply {e_apply:.2e}; forward {e_fwd:.2e}; loss {e_loss:.2e}; "
          f"d loss / d window {e_win:.2e} (largest entry {np.abs(w64).max():.3e}; the fp32 restatement "
          f"{np.abs(refs[torch.float32][2] - w64).max() / np.abs(w64).max():.2e})")
    assert e_fwd <= 1e-5 and e_loss <= 1e-5, (e_fwd, e_loss)
    assert got_w.dtype == np.float64 and np.abs(w64[:, :, :-1]).max() > 0 and e_win < 1e-4, e_win
    _leaf_report(f"one step {cid}", got_p, g64, refs[torch.float32][3])

    # a handle's module: the gradients land in the handle's blob
    th = model.train_handle(eng, params)
    th.zero_grad()
    mod_h = TorchModule(model, hcase, params, B, handle=th)
    assert mod_h.module is th.module
    w2 = torch.as_tensor(pos[:, :, :ISL], device=eng.device).requires_grad_(True)
    _mse(mod_h(w2, pt)["acc"], target.to(eng.device).float(), _mask(pt, eng.device)).backward()
    blob = model.unflatten(th.read("grads"))
    in_blob = {n: blob[n.rpartition(".")[0] or "~"][n.rpartition(".")[2]] for n in g64}
    _leaf_report(f"one step {cid}, handle", in_blob, g64, refs[torch.float32][3])
    assert np.abs(_np(w2.grad) - w64).max() / np.abs(w64).max() < 1e-4
    th.close()


# ------------------------------------------------------------------------------------------------ 4. two-step unroll
def _step_window(w, pred, consts, pt=None, target_pos=None):
    """integrate_fn for "acc" (case.py:230-259) and the window shift, float64 torch, written with the yardstick's displacement."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=torch.float64, device=w.device)
    acc = pred.double() * t(consts["acc_std"]) + t(consts["acc_mean"])
    vel = displacement_torch(w[..., -1, :], w[..., -2, :], consts["box"], consts["periodic"])
    new = w[..., -1, :] + (vel + acc)
    if consts["periodic"]:
        new = torch.remainder(new, t(consts["box"]))
    if target_pos is not None:
        new = torch.where((~_mask(pt))[..., None].to(w.device), t(target_pos), new)
    return torch.cat([w[..., 1:, :], new[..., None, :]], dim=-2)


def _unroll_loss(p1, p2, t1, t2, mask):
    return _mse(p1, t1, mask) + _mse(p2, t2, mask)


@pytest.mark.parametrize("cid", ["rpf2d_b1", "ldc3d"])
def test_two_step_unroll_is_differentiable_end_to_end(cid):
    """p1 = mod(w1), w2 = advance_window(w1, p1), p2 = mod(w2); the loss reads both.  The first step's backward finds the engine on
    the second step's list: it reloads w1, rebuilds the list and goes on (restored == 1).  Weights and d loss / d w1 against
    the float64 restatement on the engine's two lists.  ldc3d: the kinematic particles take their target positions.
    Measured on an MI355X (rpf2d / ldc3d): forward 4.1e-7 and 3.8e-7 / 2.3e-7 and 2.2e-7; loss 4.1e-8 / 4.9e-8; d loss / d first
    window 1.2e-7 / 1.5e-7; worst parameter leaf 6.5e-7 / 7.1e-7."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule, advance_window
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, eng = _allocate(cid)
    B, N, dim = eng.B, eng.N, eng.dim
    model, params, state = _model(cid, eng)
    kin = bool(((pt == 1) | (pt == 2)).any())
    assert kin == (cid == "ldc3d")
    tgt_pos = pos[:, :, ISL] if kin else None
    gen = torch.Generator().manual_seed(9)
    t1 = torch.randn((B, N, dim), generator=gen, dtype=torch.float64)
    t2 = torch.randn((B, N, dim), generator=gen, dtype=torch.float64)

    w1_dev = torch.as_tensor(pos[:, :, :ISL], device=eng.device)
    mod = TorchModule(model, hcase, params, B, state=state)
    w1 = w1_dev.clone().requires_grad_(True)
    p1 = mod(w1, pt)["acc"]
    idx1, ne1, e1 = _list(eng)
    f1 = _force(eng)
    w2 = advance_window(hcase, w1, p1, "acc", particle_type=pt if kin else None, target_pos=tgt_pos)
    p2 = mod(w2)["acc"]
    idx2, ne2, e2 = _list(eng)
    f2 = _force(eng)
    mask = _mask(pt, eng.device)
    loss = _unroll_loss(p1, p2, t1.to(eng.device).float(), t2.to(eng.device).float(), mask)
    assert mod.restored == 0
    loss.backward()
    assert mod.restored == 1
    got_w, got_p = _np(w1.grad), _grads(mod.module)

    refs = {}
    for dt in (torch.float64, torch.float32):
        m = model._device_module(_Cpu(), params, state).to(dt)
        r1 = torch.as_tensor(pos[:, :, :ISL]).clone().requires_grad_(True)
        q1 = _restate(m, dt, [r1[b] for b in range(B)], e1, f1, pt, consts, idx1, ne1)
        r2 = _step_window(r1, q1, consts, pt, tgt_pos)
        q2 = _restate(m, dt, [r2[b] for b in range(B)], e2, f2, pt, consts, idx2, ne2)
        ls = _unroll_loss(q1, q2, t1.to(dt), t2.to(dt), _mask(pt))
        ls.backward()
        refs[dt] = (q1.detach().double().numpy(), q2.detach().double().numpy(), float(ls.detach()), r1.grad.numpy(), _grads(m),
                    r2.detach().numpy())
    q1, q2, l64, w64, g64, r2 = refs[torch.float64]
    e1_, e2_ = (np.abs(_np(p).astype(np.float64) - q).max() / np.abs(q).max() for p, q in ((p1, q1), (p2, q2)))
    e_w2 = np.abs(_np(w2) - r2).max() / float(np.max(consts["box"]))
    e_loss = abs(float(loss.detach()) - l64) / abs(l64)
    e_win = np.abs(got_w - w64).max() / np.abs(w64).max()
    print(f"[torch window grad unroll {cid}] forward step 1 {e1_:.2e}, step 2 {e2_:.2e}; second window / box {e_w2:.2e}; loss "
          f"{e_loss:.2e}; d loss / d first window {e_win:.2e} (the fp32 restatement "
          f"{np.abs(refs[torch.float32][3] - w64).max() / np.abs(w64).max():.2e})")
    assert e1_ <= 1e-5 and e2_ <= 1e-5 and e_loss <= 1e-5, (e1_, e2_, e_loss)
    assert e_win < 1e-4, e_win
    _leaf_report(f"unroll {cid}", got_p, g64, refs[torch.float32][4])
    # separately, the premise of the restore: the same window under frozen capacities gives the same list, to the bit
    lists = []
    for w in (w1_dev, w2.detach(), w1_dev):
        eng.load_window(w)
        eng.nl_update()
        lists.append(eng.nl_idx())
    assert torch.equal(lists[0][0], lists[2][0]) and torch.equal(lists[0][1], lists[2][1])
    assert torch.equal(lists[0][0].cpu().long(), idx1) and not torch.equal(lists[1][0], lists[0][0])
    # a second backward of a graph whose window was forgotten says so
    p3 = mod(w1, pt)["acc"]
    mod.reset()
    with pytest.raises(RuntimeError, match="window is gone"):
        p3.sum().backward()


# ------------------------------------------------------------------------------------------------ 5. training through time
def test_three_adamw_steps_of_a_two_step_unroll_loss():
    """torch.optim.AdamW on mod.parameters(), the loss of a two-step unroll against the dataset's own (noise-free) accelerations:
    finite and falling."""
    _need_gpu()
    from lagrangebench_amd.autograd import TorchModule, advance_window
    cid = "rpf2d_b2"
    ds, hcase, pos, pt, consts = _setup(cid)
    feats, eng = _allocate(cid)
    B = eng.B
    model, params, state = _model(cid, eng)
    mod = TorchModule(model, hcase, params, B, state=state)
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-3)
    p3 = torch.as_tensor(pos, device=eng.device)
    t1 = hcase._compute_target(p3[:, :, ISL - 2:ISL + 1], True)["acc"].float()
    t2 = hcase._compute_target(p3[:, :, ISL - 1:ISL + 2], True)["acc"].float()
    mask = _mask(pt, eng.device)
    w1 = p3[:, :, :ISL].contiguous()
    before = _grads_free_copy(mod)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        a1 = mod(w1, pt)["acc"]
        a2 = mod(advance_window(hcase, w1, a1, "acc"))["acc"]
        loss = _unroll_loss(a1, a2, t1, t2, mask)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"[torch window grad adamw] losses {losses}; restored {mod.restored}")
    assert np.isfinite(losses).all() and losses[0] > losses[1] > losses[2], losses
    assert mod.restored == 3
    after = mod.params()
    assert any(np.abs(after[m][k] - before[m][k]).max() > 0 for m in after for k in after[m])


def _grads_free_copy(mod):
    return {m: {k: v.copy() for k, v in lv.items()} for m, lv in mod.params().items()}
