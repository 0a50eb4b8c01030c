"""The training step's gradient-reduction kernels one by one on the device (csrc/lb_train.hip: k_dw_part<NA, DEPTH>,
k_dw_part_h, k_dw_narrow, k_colsum_part, k_ln_bwd2<GATHER>, k_part_reduce, k_embed_grad), each run by the production
launcher through the lb_train_probe hook on a blob handle and compared with a float64 reference of the plain operation.

Exact inputs (small integers) must come back bit for bit in either arithmetic; accuracy inputs within the bounds of
tests/_train_kernels.py, which were derived from the operations and checked against CPU twins (tests/test_train_kernels.py),
never fitted to a device result.  Every case first asserts, through lb_train_probe_plan, that it reaches the path it is
named for.  The worst error / bound ratio of every case is printed.

Layout of every call: inputs carry 64 further rows of NaN behind `rows` and NaN in X's padding columns; the gradient blob is
a sentinel everywhere except the destinations, so a write outside them - or a read of a row or column that is not there -
shows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _train_kernels as TK  # noqa: E402
from tests._common import hip_case  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -12345.0
BAND = 256
NBLOB = 140_000
NAN = float("nan")


class Rig:
    def __init__(self):
        from lagrangebench_amd.data import make_case
        ds = make_case("small2d", n_trajs=1, extra_seq_length=2)
        self.eng = hip_case(ds).engine(1)
        self.dev = self.eng.device
        self.th = self.eng.blob_train_handle(np.zeros(NBLOB, np.float32))
        self.g = self.th.device_blob("grads")
        self.mask = torch.zeros(NBLOB, dtype=torch.bool, device=self.dev)

    def place(self, lens, prefill, seed=0, idx=None):
        """sentinel everywhere, destinations of `lens` floats between guard bands: (offsets, their prefill as CPU float64).
        prefill "int": integers in [-8, 8]; "zero": zeros (the accuracy bounds have no term for a previous value).
        idx[i]: the positions inside destination i that belong to it (default: all of it)."""
        gen = TK.gen(977 + seed)
        self.g.fill_(SENT)
        self.mask.zero_()
        offs, pre, o = [], [], BAND
        for i, L in enumerate(lens):
            p = torch.randint(-8, 9, (L,), generator=gen).float() if prefill == "int" else torch.zeros(L)
            if idx is not None and idx[i] is not None:
                keep = torch.zeros(L, dtype=torch.bool)
                keep[idx[i]] = True
                p = torch.where(keep, p, torch.tensor(SENT))
                self.mask[o:o + L] = keep.to(self.dev)
            else:
                self.mask[o:o + L] = True
            self.g[o:o + L] = p.to(self.dev)
            offs.append(o)
            pre.append(p.double())
            o += L + BAND
        assert o <= NBLOB
        return offs, pre

    def bands_ok(self):
        return bool((self.g[~self.mask] == SENT).all())

    def get(self, off, L):
        return self.g[off:off + L].detach().cpu()

    def dev_rows(self, a, rows_extra=64, cols=None):
        """a (rows x c) on the device inside a NaN frame: 64 rows behind, columns up to `cols`"""
        rows, c = a.shape
        out = torch.full((rows + rows_extra, cols or c), NAN, device=self.dev)
        out[:rows, :c] = a.to(self.dev)
        return out


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = Rig()
    yield r
    r.th.close()


def _check_plan(rows, K, math_):
    pl = TK.plan(rows, K, math_)
    if rows in TK.DW_ROWS_PLAN:
        assert (pl["chunk"], pl["G"], rows - (pl["G"] - 1) * pl["chunk"]) == TK.DW_ROWS_PLAN[rows]
    deep = pl["chunk"] >= 192
    want = (1, 0, 0) if math_ and K >= 32 else (0, 1, 12 if deep else 6) if K <= 128 else (0, 2, 8 if deep else 6) if K <= 256 else (0, 3, 4)
    assert (pl["h"], pl["NA"], pl["DEPTH"]) == want
    return pl


def _run_dw(rig, X, dY, rows, K, ldx, math_, prefill, nb=128, bias=True, dY_b=None, tmax=None, xexp=0, xdyn=0, seed=0):
    """one dw launch in the poison layout: (dW, db, dW_b, their prefills, guard, slot, the device X / dY)"""
    Xd = X if X.is_cuda else rig.dev_rows(X[:, :K], cols=ldx)
    Yd = dY if dY.is_cuda else rig.dev_rows(dY)
    Bd = None if dY_b is None else dY_b if dY_b.is_cuda else rig.dev_rows(dY_b)
    offs, pre = rig.place([K * 128, 128, K * 128], prefill, seed)
    guard, slot = rig.th.probe("dw", x=Xd, dy=Yd, rows=rows, K=K, ldx=ldx, dst0=offs[0], dst1=offs[1] if bias else -1, nb=nb,
                               math=math_, tmax=tmax, dy_b=Bd, dst_b=offs[2] if Bd is not None else -1, xexp=xexp, xdyn=xdyn)
    out = [rig.get(o, L) for o, L in zip(offs, (K * 128, 128, K * 128))]
    assert rig.bands_ok(), "a write outside the destinations"
    return out, pre, guard, slot, (Xd, Yd)


def _tile_max(Yd, rows):
    a = Yd[:rows].abs().amax(1)
    t = torch.zeros((rows + 15) // 16 + 64, device=Yd.device)
    return t.scatter_reduce_(0, torch.arange(rows, device=Yd.device) // 16, a, "amax")


# ---------------------------------------------------------------------------------------------- dw
@pytest.mark.parametrize("rows,K,ldx,math_", TK.dw_cases())
def test_dw(rig, rows, K, ldx, math_):
    pl = _check_plan(rows, K, math_)
    # exact inputs: prefill + the integer reference, bit for bit, db included; nothing outside the destinations
    X, dY = TK.dw_case_data("exact", rows, K, ldx)
    (w, b, wb), pre, guard, _, (Xd, Yd) = _run_dw(rig, X, dY, rows, K, ldx, math_, "int")
    rw, rb = TK.dw_reference(Xd, Yd, rows, K)
    assert guard == 0 and torch.isfinite(w).all() and torch.isfinite(b).all()
    assert np.array_equal(TK.bits(w), TK.bits(pre[0] + rw.cpu().reshape(-1))), "dW differs from the integer reference"
    assert np.array_equal(TK.bits(b), TK.bits(pre[1] + rb.cpu())), "db differs from the integer reference"
    assert np.array_equal(TK.bits(wb), TK.bits(pre[2]))
    # accuracy inputs: within the bound
    X, dY = TK.dw_case_data("accuracy", rows, K, ldx)
    (w, b, _), _, guard, _, (Xd, Yd) = _run_dw(rig, X, dY, rows, K, ldx, math_, "zero")
    rw, rb = TK.dw_reference(Xd, Yd, rows, K)
    bw, bb = TK.dw_bound(Xd, Yd, rows, K, pl, math_)
    qw = TK.worst_ratio(w.reshape(K, 128), rw.cpu(), bw.cpu())
    qb = TK.worst_ratio(b, rb.cpu(), bb.cpu())
    print(f"dw rows={rows} K={K} ldx={ldx} math={math_} chunk={pl['chunk']} G={pl['G']}: dW {qw:.3f} db {qb:.3f} of the bound")
    assert guard == 0 and qw <= 1.0 and qb <= 1.0


@pytest.mark.parametrize("math_", (0, 1))
@pytest.mark.parametrize("nb", (128, 5, 0))
def test_dw_bias_columns(rig, nb, math_):
    for rows in (65, 24577):
        X, dY = TK.dw_case_data("exact", rows, 128, 128)
        (w, b, _), pre, _, _, (Xd, Yd) = _run_dw(rig, X, dY, rows, 128, 128, math_, "int", nb=nb)
        rw, rb = TK.dw_reference(Xd, Yd, rows, 128)
        want = pre[1].clone()
        want[:nb] += rb.cpu()[:nb]
        assert np.array_equal(TK.bits(b), TK.bits(want))
        assert np.array_equal(TK.bits(w), TK.bits(pre[0] + rw.cpu().reshape(-1)))
    (w, b, _), pre, _, _, _ = _run_dw(rig, X, dY, rows, 128, 128, math_, "int", bias=False)   # no db at all
    assert np.array_equal(TK.bits(b), TK.bits(pre[1]))


@pytest.mark.parametrize("family", ("exact", "accuracy"))
@pytest.mark.parametrize("rows,K", [(65, 128), (24577, 128), (48897, 256), (33, 144)])
def test_dw_pair_equals_two_single_launches(rig, rows, K, family):
    assert _check_plan(rows, K, 1)["h"] == 1
    X, dY = TK.dw_case_data(family, rows, K, K)
    _, dYb = TK.dw_inputs(family, rows, K, seed=3)
    Xd, Yd, Bd = rig.dev_rows(X), rig.dev_rows(dY), rig.dev_rows(dYb)
    pf = "int" if family == "exact" else "zero"   # (a prefill enters the last rounding: the two B destinations get the same one)
    (wa, _, wb), pre, guard, _, _ = _run_dw(rig, Xd, Yd, rows, K, K, 1, pf, bias=False, dY_b=Bd)
    (sa, _, _), pa, ga, _, _ = _run_dw(rig, Xd, Yd, rows, K, K, 1, pf, bias=False)
    (sb, _, _), pb, gb, _, _ = _run_dw(rig, Xd, Bd, rows, K, K, 1, pf, bias=False)
    assert guard == ga == gb == 0 and torch.equal(pre[0], pa[0]) and torch.equal(pa[0], pb[0])
    assert np.array_equal(TK.bits(wa), TK.bits(sa))
    assert np.array_equal(TK.bits(wb - pre[2].float()), TK.bits(sb - pb[0].float()))   # (integers: the differences are exact)
    if family == "exact":
        assert np.array_equal(TK.bits(wb), TK.bits(pre[2] + TK.dw_reference(Xd, Bd, rows, K)[0].cpu().reshape(-1)))


@pytest.mark.parametrize("rows", (33, 65, 24577, 48897))
def test_dw_tile_maxima(rig, rows):
    """tmax given as the true 16-row tile maxima of dY against tmax absent"""
    pl = _check_plan(rows, 128, 1)
    X, dY = TK.dw_case_data("exact", rows, 128, 128)
    (w0, b0, _), _, _, _, (Xd, Yd) = _run_dw(rig, X, dY, rows, 128, 128, 1, "int")
    (w1, b1, _), _, _, _, _ = _run_dw(rig, Xd, Yd, rows, 128, 128, 1, "int", tmax=_tile_max(Yd, rows))
    assert np.array_equal(TK.bits(w0), TK.bits(w1)) and np.array_equal(TK.bits(b0), TK.bits(b1))
    X, dY = TK.dw_case_data("accuracy", rows, 128, 128)
    Xd, Yd = rig.dev_rows(X), rig.dev_rows(dY)
    rw, _ = TK.dw_reference(Xd, Yd, rows, 128)
    for tm in (None, _tile_max(Yd, rows)):
        (w, _, _), _, guard, _, _ = _run_dw(rig, Xd, Yd, rows, 128, 128, 1, "zero", tmax=tm)
        bw, _ = TK.dw_bound(Xd, Yd, rows, 128, pl, 1, tmax=tm is not None)
        q = TK.worst_ratio(w.reshape(128, 128), rw.cpu(), bw.cpu())
        print(f"dw tmax={'given' if tm is not None else 'absent'} rows={rows}: {q:.3f} of the bound")
        assert guard == 0 and q <= 1.0


@pytest.mark.parametrize("rows,K,ldx,math_", [(65, 3, 8, 0), (24577, 30, 32, 0), (48897, 128, 136, 0), (65, 144, 160, 1),
                                              (24577, 64, 128, 1), (48897, 256, 264, 1)])
def test_dw_poison_and_repeat(rig, rows, K, ldx, math_):
    """NaN behind the rows and in X's padding columns never reaches the result; a second identical call on a re-filled blob
    gives the same bits"""
    _check_plan(rows, K, math_)
    for family in ("exact", "accuracy"):
        X, dY = TK.dw_inputs(family, rows, K)
        (w, b, _), pre, guard, _, (Xd, Yd) = _run_dw(rig, X, dY, rows, K, ldx, math_, "int")
        assert torch.isnan(Xd[:, K:]).all() and torch.isnan(Xd[rows:]).all() and torch.isnan(Yd[rows:]).all()
        assert guard == 0 and torch.isfinite(w).all() and torch.isfinite(b).all()
        if family == "exact":
            rw, rb = TK.dw_reference(Xd, Yd, rows, K)
            assert np.array_equal(TK.bits(w), TK.bits(pre[0] + rw.cpu().reshape(-1)))
            assert np.array_equal(TK.bits(b), TK.bits(pre[1] + rb.cpu()))
        (w2, b2, _), _, _, _, _ = _run_dw(rig, Xd, Yd, rows, K, ldx, math_, "int")
        assert np.array_equal(TK.bits(w), TK.bits(w2)) and np.array_equal(TK.bits(b), TK.bits(b2))


@pytest.mark.parametrize("rows", (65, 24577))
@pytest.mark.parametrize("shift,bit", ((18, 1), (-14, 2)))
def test_dw_range_guard(rig, rows, shift, bit):
    """k_dw_part_h's X range guard: X outside the fp16 window raises the guard, leaves the largest raw |X| and adds nothing;
    with the site's exponent re-centred the same call passes"""
    pl = _check_plan(rows, 128, 1)
    mul = 2.0 ** shift
    X, dY = TK.dw_case_data("accuracy", rows, 128, 128)
    Xd, Yd = rig.dev_rows(X * mul), rig.dev_rows(dY)
    (w, b, wb), pre, guard, slot, _ = _run_dw(rig, Xd, Yd, rows, 128, 128, 1, "int")
    assert guard == bit
    assert np.uint32(slot) == TK.bits(Xd[:rows].abs().max().reshape(1))[0]
    assert np.array_equal(TK.bits(w), TK.bits(pre[0])) and np.array_equal(TK.bits(b), TK.bits(pre[1]))   # k_part_reduce skipped
    (w, _, _), _, guard, slot, _ = _run_dw(rig, Xd, Yd, rows, 128, 128, 1, "zero", xexp=-shift)
    rw, _ = TK.dw_reference(Xd, Yd, rows, 128)
    bw, _ = TK.dw_bound(Xd, Yd, rows, 128, pl, 1, xexp=-shift)
    q = TK.worst_ratio(w.reshape(128, 128), rw.cpu(), bw.cpu())
    print(f"dw X x 2^{shift} with xexp {-shift} rows={rows}: {q:.3f} of the bound")
    assert guard == 0 and slot == 0 and q <= 1.0
    X, dY = TK.dw_case_data("exact", rows, 128, 128)
    (w0, _, _), _, _, _, (Xe, Ye) = _run_dw(rig, X, dY, rows, 128, 128, 1, "zero")
    (w1, _, _), _, guard, _, _ = _run_dw(rig, Xe * mul, Ye, rows, 128, 128, 1, "zero", xexp=-shift)
    assert guard == 0 and np.array_equal(TK.bits(w1), TK.bits(w0 * mul))


@pytest.mark.parametrize("rows,K", ((200, 128), (24577, 128), (24577, 144)))
def test_dw_per_chunk_x_scale(rig, rows, K):
    """xdyn: chunks whose |X| lie 2^30 apart fit no single exponent; scaled per chunk they raise nothing"""
    pl = _check_plan(rows, K, 1)
    X, dY = TK.dw_case_data("accuracy", rows, K, K)
    Xd, Yd = rig.dev_rows(X * TK.xdyn_row_scale(rows, pl["chunk"])[:, None]), rig.dev_rows(dY)
    _, _, guard, _, _ = _run_dw(rig, Xd, Yd, rows, K, K, 1, "zero")
    assert guard & 1                                            # (without it the large chunks leave the window)
    (w, _, _), _, guard, _, _ = _run_dw(rig, Xd, Yd, rows, K, K, 1, "zero", xdyn=1)
    rw, _ = TK.dw_reference(Xd, Yd, rows, K)
    bw, _ = TK.dw_bound(Xd, Yd, rows, K, pl, 1, xdyn=True)
    q = TK.worst_ratio(w.reshape(K, 128), rw.cpu(), bw.cpu())
    print(f"dw xdyn rows={rows} K={K}: {q:.3f} of the bound")
    assert guard == 0 and q <= 1.0


# ---------------------------------------------------------------------------------------------- dw_narrow, colsum
@pytest.mark.parametrize("K,M,ldx,ldy", TK.NARROW_SHAPES)
def test_dw_narrow(rig, K, M, ldx, ldy):
    for rows in TK.NARROW_ROWS:
        pl = TK.plan(rows, K, 0)   # (k_dw_narrow's chunk is the plan's before its rounding to 4 rows: n_add covers it)
        for family in ("exact", "accuracy"):
            X, dY = TK.dw_inputs(family, rows, K, M)
            Xd, Yd = rig.dev_rows(X, cols=ldx), rig.dev_rows(dY, cols=ldy)
            offs, pre = rig.place([K * M], "int" if family == "exact" else "zero")
            rig.th.probe("dw_narrow", x=Xd, dy=Yd, rows=rows, K=K, ldx=ldx, M=M, ldy=ldy, dst0=offs[0])
            w = rig.get(offs[0], K * M)
            assert rig.bands_ok()
            rw = (Xd[:rows, :K].double().T @ Yd[:rows, :M].double()).cpu()
            if family == "exact":
                assert np.array_equal(TK.bits(w), TK.bits(pre[0] + rw.reshape(-1))), (rows, family)
            else:
                bw, _ = TK.dw_bound(Xd, Yd[:, :M], rows, K, pl, 0)
                q = TK.worst_ratio(w.reshape(K, M), rw, bw.cpu())
                print(f"dw_narrow K={K} M={M} rows={rows}: {q:.3f} of the bound")
                assert q <= 1.0


@pytest.mark.parametrize("cols,ld", TK.COLSUM_COLS)
def test_colsum(rig, cols, ld):
    for rows in TK.COLSUM_ROWS:
        for family in ("exact", "accuracy"):
            _, x = TK.dw_inputs(family, rows, 4, cols)
            xd = rig.dev_rows(x, cols=ld)
            offs, pre = rig.place([cols], "int" if family == "exact" else "zero")
            rig.th.probe("colsum", x=xd, rows=rows, M=cols, ldx=ld, dst0=offs[0])
            got = rig.get(offs[0], cols)
            assert rig.bands_ok()
            ref = xd[:rows, :cols].double().sum(0).cpu()
            if family == "exact":
                assert np.array_equal(TK.bits(got), TK.bits(pre[0] + ref)), rows
            else:
                q = TK.worst_ratio(got, ref, TK.colsum_bound(xd, rows, cols).cpu())
                print(f"colsum cols={cols} rows={rows}: {q:.3f} of the bound")
                assert q <= 1.0


# ---------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("gather", (False, True))
@pytest.mark.parametrize("d", TK.LN_D)
def test_ln_bwd(rig, d, gather):
    n_gth = 37
    for rows in TK.LN_ROWS:
        z, b1, sc, dy, gth, gidx = TK.ln_inputs("accuracy", rows, d, n_gth)
        assert int(gidx.min()) == 0 and (rows == 1 or int(gidx.max()) == n_gth - 1)
        assert rows < 4 or len(set(gidx.tolist())) < rows
        assert not z[:, d:].any() and not b1[d:].any() and not sc[d:].any()
        zd, dyd = rig.dev_rows(z), rig.dev_rows(dy)
        b1d, scd, gthd, gid = b1.to(rig.dev), sc.to(rig.dev), gth.to(rig.dev), gidx.to(rig.dev)
        dz = torch.full((rows + 64, 128), SENT, device=rig.dev)
        offs, pre = rig.place([128, 128], "zero")
        rig.g[offs[0] + d:offs[0] + 128] = 7.0      # the padded entries of the parameter gradients: left as they are
        rig.g[offs[1] + d:offs[1] + 128] = -3.0
        rig.th.probe("ln_bwd", z=zd, b1=b1d, scale=scd, dy=dyd, dz=dz, rows=rows, d=d, gth=gthd if gather else None,
                     idx=gid if gather else None, dst0=offs[0], dst1=offs[1])
        ds, do = rig.get(offs[0], 128), rig.get(offs[1], 128)
        assert rig.bands_ok()
        ga = (gthd, gid) if gather else (None, None)
        rz, rs_, ro = TK.ln_reference(zd[:rows], b1d, scd, dyd[:rows], d, *ga)
        bz, bs, bo = TK.ln_bound(zd[:rows], b1d, scd, dyd[:rows], d, *ga)
        q = (TK.worst_ratio(dz[:rows, :d], rz, bz), TK.worst_ratio(ds[:d], rs_.cpu(), bs.cpu()), TK.worst_ratio(do[:d], ro.cpu(), bo.cpu()))
        print(f"ln_bwd d={d} gather={gather} rows={rows}: dz {q[0]:.3f} scale {q[1]:.3f} offset {q[2]:.3f} of the bound")
        assert max(q) <= 1.0, (rows, q)
        assert not dz[:rows, d:].cpu().numpy().view(np.uint32).any(), "a padded column of dz is not +0.0"
        assert (dz[rows:] == SENT).all(), "rows past the end of dz were written"
        assert (ds[d:] == 7.0).all() and (do[d:] == -3.0).all(), "a padded parameter gradient changed"


# ---------------------------------------------------------------------------------------------- the ordered reduce
REDUCE_SHAPES = {   # n0, n1, off1, stride, part_off, ld0
    "dw": (128 * 128, 128, 128 * 128, 129 * 128, 0, 0),
    "ln": (128, 128, 128, 256, 64, 0),
    "scalar": (130, 0, 0, 130, 77, 0),                  # odd stride and offset: no 16-byte loads
    "straddle": (254, 5, 256, 512, 0, 0),               # a quad across n0
    "colblock": (128 * 64, 128, 128 * 64, 65 * 128, 128, 192),
}


@pytest.mark.parametrize("shape", sorted(REDUCE_SHAPES))
def test_reduce(rig, shape):
    n0, n1, off1, stride, part_off, ld0 = REDUCE_SHAPES[shape]
    for G in TK.REDUCE_G:
        part = torch.randint(-8, 9, (G, stride), generator=TK.gen(G)).float().to(rig.dev)
        len0 = (n0 // 128 - 1) * ld0 + 128 if ld0 else n0
        idx0 = (torch.arange(n0) // 128 * ld0 + torch.arange(n0) % 128) if ld0 else None
        for skip in (0, 1):
            offs, pre = rig.place([len0, max(n1, 1)], "int", seed=G, idx=[idx0, None])
            rig.th.probe("reduce", x=part, G=G, stride=stride, n0=n0, n1=n1, off1=off1, ld0=ld0, part_off=part_off,
                         dst0=offs[0], dst1=offs[1] if n1 else -1, skip=skip)
            got0, got1 = rig.get(offs[0], len0), rig.get(offs[1], max(n1, 1))
            assert rig.bands_ok()
            s = part.double().sum(0).cpu() * (0 if skip else 1)
            want0 = pre[0].clone()
            if ld0:
                want0[idx0] += s[:n0]
            else:
                want0 += s[:n0]
            want1 = pre[1].clone()
            want1[:n1] += s[off1:off1 + n1]
            assert np.array_equal(TK.bits(got0), TK.bits(want0)), (shape, G, skip)
            assert np.array_equal(TK.bits(got1), TK.bits(want1)), (shape, G, skip)


# ---------------------------------------------------------------------------------------------- embedding gradient
@pytest.mark.parametrize("BN", TK.EMBED_BN)
def test_embed_grad(rig, BN):
    emb, ntypes, col0, ld, absent = 16, 9, 5, 24, 3
    for family in ("exact", "accuracy"):
        x, pt = TK.embed_inputs(family, BN, emb, ntypes, absent, ld, col0)
        assert BN == 1 or int(pt.min()) == -1
        xd, ptd = rig.dev_rows(x), torch.cat([pt, torch.full((64,), 2, dtype=torch.int32)]).to(rig.dev)
        ref = TK.embed_reference(xd[:BN], ptd[:BN], col0, emb, ntypes).cpu()
        for skip in (0, 1):
            offs, pre = rig.place([ntypes * emb], "int" if family == "exact" or skip else "zero")
            rig.th.probe("embed_grad", x=xd, idx=ptd, rows=BN, ldx=ld, col0=col0, emb=emb, ntypes=ntypes, dst0=offs[0], skip=skip)
            got = rig.get(offs[0], ntypes * emb)
            assert rig.bands_ok()
            if skip:
                assert np.array_equal(TK.bits(got), TK.bits(pre[0]))
            elif family == "exact":
                assert np.array_equal(TK.bits(got), TK.bits(pre[0] + ref.reshape(-1)))
                assert np.array_equal(TK.bits(got.reshape(ntypes, emb)[absent]), TK.bits(pre[0].reshape(ntypes, emb)[absent]))
            else:
                q = TK.worst_ratio(got.reshape(ntypes, emb), ref, TK.embed_bound(xd[:BN], ptd[:BN], col0, emb, ntypes).cpu())
                print(f"embed_grad BN={BN}: {q:.3f} of the bound")
                assert q <= 1.0 and not got.reshape(ntypes, emb)[absent].any()
