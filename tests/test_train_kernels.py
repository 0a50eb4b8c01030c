"""CPU side of the kernel-by-kernel test of the training step's gradient reductions (tests/_train_kernels.py): the CPU twins
against the bounds the device is held to, the mutation checks - wrong variants of the twins that the exact check and the
bounds must catch - the sweep of the launcher's plan (lb_train_probe_plan) and lb_train_probe's refusals that need no device.
The device side is tests/test_train_kernels_gpu.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _train_kernels as TK  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from lagrangebench_amd import build
    build.build()
    from lagrangebench_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------- twins against the bounds
@pytest.mark.parametrize("rows,K,ldx,math_", TK.dw_cases())
def test_dw_twin_within_a_quarter_of_the_bound(lib, rows, K, ldx, math_):
    pl = TK.plan(rows, K, math_)
    X, dY = TK.dw_case_data("accuracy", rows, K, ldx)
    rw, rb = TK.dw_reference(X, dY, rows, K)
    bw, bb = TK.dw_bound(X, dY, rows, K, pl, math_)
    tw, tb = TK.dw_twin(X, dY, rows, K, pl, math_)
    qw, qb = TK.worst_ratio(tw, rw, bw), TK.worst_ratio(tb, rb, bb)
    print(f"dw twin rows={rows} K={K} math={math_}: dW {qw:.3f} db {qb:.3f} of the bound")
    assert qw <= 0.25 and qb <= 0.25
    Xe, dYe = TK.dw_case_data("exact", rows, K, ldx)
    rw, rb = TK.dw_reference(Xe, dYe, rows, K)
    tw, tb = TK.dw_twin(Xe, dYe, rows, K, pl, math_)
    assert np.array_equal(TK.bits(tw), TK.bits(rw)) and np.array_equal(TK.bits(tb), TK.bits(rb))


SCALE_CASES = ([(r, 128, dict(xexp=-18, mul=2.0 ** 18)) for r in (65, 24577)] + [(r, 128, dict(xexp=14, mul=2.0 ** -14)) for r in (65, 24577)]
               + [(200, 128, dict(xdyn=True)), (24577, 128, dict(xdyn=True)), (24577, 144, dict(xdyn=True))]
               + [(r, 128, dict(tmax=True)) for r in (33, 65, 24577, 48897)])


@pytest.mark.parametrize("rows,K,kw", SCALE_CASES)
def test_dw_twin_f16x2_scales(lib, rows, K, kw):
    """the device test's cases of the X exponent, per-chunk X scaling (chunks 2^30 apart) and the row-tile maxima: the twin
    within a quarter of their bounds"""
    kw = dict(kw)
    mul = kw.pop("mul", 1.0)
    pl = TK.plan(rows, K, 1)
    X, dY = TK.dw_case_data("accuracy", rows, K, K)
    X = X * mul
    if kw.get("xdyn"):
        X = X * TK.xdyn_row_scale(rows, pl["chunk"])[:, None]
    rw, _ = TK.dw_reference(X, dY, rows, K)
    bw, _ = TK.dw_bound(X, dY, rows, K, pl, 1, **kw)
    tw, _ = TK.dw_twin(X, dY, rows, K, pl, 1, **kw)
    q = TK.worst_ratio(tw, rw, bw)
    print(f"dw twin rows={rows} K={K} {kw}: {q:.3f} of the bound")
    assert q <= 0.25


@pytest.mark.parametrize("rows", TK.NARROW_ROWS)
@pytest.mark.parametrize("K,M,ldx,ldy", TK.NARROW_SHAPES)
def test_narrow_twin(lib, K, M, ldx, ldy, rows):
    pl = TK.plan(rows, K, 0)
    X, dY = TK.dw_inputs("accuracy", rows, K, M)
    rw, _ = TK.dw_reference(X, dY, rows, K)
    bw, _ = TK.dw_bound(X, dY, rows, K, pl, 0)
    assert TK.worst_ratio(TK.narrow_twin(X, dY, rows, K, M, pl["chunk"]), rw, bw) <= 0.25
    X, dY = TK.dw_inputs("exact", rows, K, M)
    assert np.array_equal(TK.bits(TK.narrow_twin(X, dY, rows, K, M, pl["chunk"])), TK.bits(TK.dw_reference(X, dY, rows, K)[0]))


@pytest.mark.parametrize("rows", TK.COLSUM_ROWS)
@pytest.mark.parametrize("cols,ld", TK.COLSUM_COLS)
def test_colsum_twin(cols, ld, rows):
    _, x = TK.dw_inputs("accuracy", rows, 4, ld)
    ref = x[:, :cols].double().sum(0)
    assert TK.worst_ratio(TK.colsum_twin(x, rows, cols), ref, TK.colsum_bound(x, rows, cols)) <= 0.25


@pytest.mark.parametrize("gather", (False, True))
@pytest.mark.parametrize("d", TK.LN_D)
@pytest.mark.parametrize("rows", TK.LN_ROWS)
def test_ln_twin(rows, d, gather):
    z, b1, sc, dy, gth, gidx = TK.ln_inputs("accuracy", rows, d, 37)
    ga = (gth, gidx) if gather else (None, None)
    rz, rs_, ro = TK.ln_reference(z, b1, sc, dy, d, *ga)
    bz, bs, bo = TK.ln_bound(z, b1, sc, dy, d, *ga)
    tz, ts, to = TK.ln_twin(z, b1, sc, dy, d, *ga)
    q = (TK.worst_ratio(tz[:, :d], rz, bz), TK.worst_ratio(ts[:d], rs_, bs), TK.worst_ratio(to[:d], ro, bo))
    print(f"ln twin rows={rows} d={d} gather={gather}: dz {q[0]:.3f} scale {q[1]:.3f} offset {q[2]:.3f} of the bound")
    assert max(q) <= 0.25
    assert not tz[:, d:].any()


@pytest.mark.parametrize("BN", TK.EMBED_BN)
def test_embed_twin(BN):
    x, pt = TK.embed_inputs("accuracy", BN)
    ref = TK.embed_reference(x, pt, 5, 16, 9)
    assert TK.worst_ratio(TK.embed_twin(x, pt, 5, 16, 9), ref, TK.embed_bound(x, pt, 5, 16, 9)) <= 0.25
    assert not ref[3].any() and (BN == 1 or ref[8].any())   # the absent type; -1 wrapped to the last row


# ---------------------------------------------------------------------------------------------- mutation checks
@pytest.mark.parametrize("math_", (0, 1))
@pytest.mark.parametrize("mutate", TK.MUTATIONS)
def test_mutations_fail_the_exact_check_and_the_bound(lib, mutate, math_):
    """A subtly wrong kernel - modelled on the twin - fails the bit-for-bit check on the exact inputs at the largest shape,
    and the bound on the accuracy inputs (taken at the chunk that holds the largest gradient rows: against a chunk 2^-30
    below the others no bound can see one row)."""
    rows, K = 24577, 128
    pl = TK.plan(rows, K, math_)
    g = TK.gen(5)
    pw, pb = torch.randint(-8, 9, (K, 128), generator=g).float(), torch.randint(-8, 9, (128,), generator=g).float()
    X, dY = TK.dw_inputs("exact", rows, K, extra_rows=1)
    rw, rb = TK.dw_reference(X, dY, rows, K)
    good = TK.dw_twin(X, dY, rows, K, pl, math_, pw, pb)
    assert np.array_equal(TK.bits(good[0]), TK.bits(pw + rw)) and np.array_equal(TK.bits(good[1]), TK.bits(pb + rb))
    bad = TK.dw_twin(X, dY, rows, K, pl, math_, pw, pb, mutate=mutate, mutate_chunk=3)
    if mutate == "db_rows_plus_1":
        assert not np.array_equal(TK.bits(bad[1]), TK.bits(pb + rb))
    else:
        assert not np.array_equal(TK.bits(bad[0]), TK.bits(pw + rw))
    # the bound (no prefill: it has no term for the destination's previous value - so `=` for `+=` is the exact check's)
    if mutate == "overwrite":
        return
    rows = 4099
    pl = TK.plan(rows, K, math_)
    X, dY = TK.dw_inputs("accuracy", rows, K, extra_rows=1)
    top = int(dY[:rows].abs().amax(1).argmax()) // pl["chunk"]
    if mutate == "db_rows_plus_1":
        dY[rows] = dY[:rows].abs().max()
    rw, rb = TK.dw_reference(X, dY, rows, K)
    bw, bb = TK.dw_bound(X, dY, rows, K, pl, math_)
    bad = TK.dw_twin(X, dY, rows, K, pl, math_, mutate=mutate, mutate_chunk=top)
    q = TK.worst_ratio(bad[1], rb, bb) if mutate == "db_rows_plus_1" else TK.worst_ratio(bad[0], rw, bw)
    assert q > 1.0, q


def test_mutation_unmasked_layernorm_padding():
    for fam in ("exact", "accuracy"):
        z, b1, sc, dy, gth, gidx = TK.ln_inputs(fam, 65, 48, 9)
        assert TK.ln_twin(z, b1, sc, dy, 48, gth, gidx, zero_pad=False)[0][:, 48:].any()
        assert not TK.ln_twin(z, b1, sc, dy, 48, gth, gidx)[0][:, 48:].any()


# ---------------------------------------------------------------------------------------------- the launcher's plan
PLAN_K = (3, 4, 8, 30, 32, 64, 128, 144, 256, 384)


def test_plan_sweep(lib):
    """rows 1 ... 70 000: the row split, dw_groups_max's claim and the variant table of dw_acc"""
    out = (C.c_int64 * 5)()
    gmax_run = 0
    seen = {}
    for rows in range(1, 70001):
        assert lib.lb_train_probe_plan(rows, 128, 0, out) == 0
        G, chunk = out[0], out[1]
        assert chunk % 4 == 0 and chunk >= 64 and 1 <= G <= 256 and G * chunk >= rows and (G - 1) * chunk < rows
        gmax_run = max(gmax_run, G)
        assert gmax_run <= min(256, (rows + 63) // 64 + 1)          # every rows' <= this cap stays under the cap's bound
        ks = PLAN_K if rows % 997 == 0 or rows < 70 or chunk in (188, 192) else (30, 128, 256)
        for K in ks:
            for m in (0, 1):
                assert lib.lb_train_probe_plan(rows, K, m, out) == 0
                assert (out[0], out[1]) == (G, chunk)
                h, NA, DEPTH = out[2], out[3], out[4]
                assert h == (1 if m == 1 and K >= 32 else 0)
                if h:
                    assert (NA, DEPTH) == (0, 0)
                else:
                    assert NA == (1 if K <= 128 else 2 if K <= 256 else 3)
                    deep = chunk >= 192
                    assert DEPTH == {1: 12 if deep else 6, 2: 8 if deep else 6, 3: 4}[NA]
                seen.setdefault((h, NA, DEPTH), rows)
    assert set(seen) == {(1, 0, 0), (0, 1, 6), (0, 1, 12), (0, 2, 6), (0, 2, 8), (0, 3, 4)}
    for rows, want in TK.DW_ROWS_PLAN.items():
        pl = TK.plan(rows, 128, 1)
        assert (pl["chunk"], pl["G"], rows - (pl["G"] - 1) * pl["chunk"]) == want
    print("first rows of each variant (h, NA, DEPTH):", seen)
    # what the whole-network gradient tests reach (tests/test_train.py: at most ~20 k rows in any product)
    for rows in (256, 512, 900, 20000):
        pl = TK.plan(rows, 128, 1)
        print(f"rows {rows}: chunk {pl['chunk']} G {pl['G']} full steps {pl['chunk'] // 32}")
        assert pl["chunk"] < 96 and TK.plan(rows, 128, 0)["DEPTH"] == 6


def test_plan_refuses(lib):
    out = (C.c_int64 * 5)()
    assert lib.lb_train_probe_plan(0, 128, 0, out) == -1
    assert lib.lb_train_probe_plan(10, 385, 0, out) == -1 and b"384" in lib.lb_last_error()
    assert lib.lb_train_probe_plan(10, 128, 0, None) == -1


# ---------------------------------------------------------------------------------------------- refusals without a device
def _args(**kw):
    from lagrangebench_amd._lib import TrainProbeArgs
    a = TrainProbeArgs()
    a.dst0 = a.dst1 = a.dst_b = -1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_probe_refusals_without_a_device(lib):
    """the arguments are checked before the handle is looked at: every refusal leaves its reason in lb_last_error"""
    P = 4096   # (a non-null, aligned pointer value: never dereferenced)
    assert lib.lb_train_probe(None, 0, None) == -1
    ok = dict(x=P, dy=P, rows=65, K=128, ldx=128, dst0=0, nb=128, math=1)
    for kw, word in ((dict(ok, x=None), b"null"), (dict(ok, dy=None), b"null"), (dict(ok, K=385, ldx=385), b"384"),
                     (dict(ok, K=33, ldx=33), b"odd K"), (dict(ok, math=0, dy_b=P, dst_b=0), b"f16x2"),
                     (dict(ok, K=30, ldx=32, dy_b=P, dst_b=0), b"f16x2"), (dict(ok, dy_b=P), b"together"),
                     (dict(ok, rows=0), b"rows"), (dict(ok, nb=129), b"nb"), (dict(ok), b"null handle")):
        assert lib.lb_train_probe(None, 0, C.byref(_args(**kw))) == -1
        assert word in lib.lb_last_error(), (kw, lib.lb_last_error())
    for op, kw, word in ((1, dict(x=P, dy=P, rows=5, K=128, ldx=128, M=5, ldy=5, dst0=0), b"dw_narrow"),
                         (1, dict(x=P, dy=None, rows=5, K=128, ldx=128, M=2, ldy=2, dst0=0), b"null"),
                         (2, dict(x=P, rows=5, M=129, ldx=129, dst0=0), b"colsum"),
                         (3, dict(z=P, b1=P, scale=P, dy=P, dz=None, rows=5, d=128, dst0=0, dst1=128), b"null"),
                         (3, dict(z=P, b1=P, scale=P, dy=P, dz=P, gth=P, rows=5, d=128, dst0=0, dst1=128), b"together"),
                         (4, dict(x=P, G=0, stride=128, n0=128, dst0=0), b"reduce"),
                         (4, dict(x=P, G=2, stride=128, n0=100, ld0=192, dst0=0), b"ld0"),
                         (5, dict(x=P, idx=None, rows=5, emb=16, ntypes=9, ldx=24, dst0=0), b"null"),
                         (9, dict(rows=1), b"op")):
        assert lib.lb_train_probe(None, op, C.byref(_args(**kw))) == -1
        assert word in lib.lb_last_error(), (op, kw, lib.lb_last_error())
