"""References, error bounds and CPU twins of the training step's gradient-reduction kernels (csrc/lb_train.hip:
k_dw_part, k_dw_part_h, k_dw_narrow, k_colsum_part, k_ln_bwd2, k_part_reduce, k_embed_grad), shared by
tests/test_train_kernels.py (CPU) and tests/test_train_kernels_gpu.py (device, through the lb_train_probe hook).

Everything here is torch on whatever device the inputs live on: the float64 references are the plain operations
(X^T dY, column sums, torch autograd through layer_norm, index_add_), the bounds are float64 formulas of the inputs and of
the geometry lb_train_probe_plan reports, and the twins are float32 / float16 restatements in another summation order.
No constant below was fitted to a device result: a twin has to sit at or below a QUARTER of its bound on every case the
device test runs (test_train_kernels.py), and the device is then held to the whole bound.

Two input families, both seeded:
  exact     X, dY small integers (dY in quarters), half of X zero: every product and partial sum is an integer multiple of
            1/4 below 2^24, exact in fp32 and - under power-of-two scales - in fp16 hi/lo halves, so either arithmetic has to
            return the integer reference bit for bit.  A dropped, doubled or misplaced row or column cannot hide.
  accuracy  X = relu(N(0, 1)), dY = N(0, 1) x 2^e with one e in [-20, 10] per 64 rows (the chunk scale of k_dw_part_h matters).
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32
LNB_ROWS = 64           # rows per workgroup of k_ln_bwd2
F64 = torch.float64

# ---------------------------------------------------------------------------------------------- the cases of the device test
DW_ROWS = (1, 31, 32, 33, 63, 64, 65, 24577, 32768, 40960, 48128, 48897)
DW_K_F32 = ((3, 8), (4, 8), (30, 32), (128, 128), (144, 144), (256, 256), (384, 384))     # (K, ldx), exact fp32
DW_K_H = ((32, 32), (64, 64), (128, 128), (144, 144), (256, 256), (384, 384))            # f16x2
# what each rows value is there for: (chunk, G, rows of the last chunk)
DW_ROWS_PLAN = {1: (64, 1, 1), 31: (64, 1, 31), 32: (64, 1, 32), 33: (64, 1, 33), 63: (64, 1, 63), 64: (64, 1, 64), 65: (64, 2, 1),
                24577: (100, 246, 77), 32768: (128, 256, 128), 40960: (160, 256, 160), 48128: (188, 256, 188),
                48897: (192, 255, 129)}


def dw_cases():
    """(rows, K, ldx, math): every rows value with K = 128 in both arithmetics, every K with rows 65 and 48 897."""
    out = []
    for math_, ks in ((0, DW_K_F32), (1, DW_K_H)):
        for rows in DW_ROWS:
            out.append((rows, 128, 128, math_))
        for K, ldx in ks:
            for rows in (65, 48897):
                if (rows, K, ldx, math_) not in out:
                    out.append((rows, K, ldx, math_))
    return out


NARROW_SHAPES = ((128, 2, 128, 2), (128, 3, 128, 3), (65, 2, 68, 2), (128, 1, 128, 1))   # (K, M, ldx, ldy)
NARROW_ROWS = (1, 64, 65, 16385, 40000)
COLSUM_COLS = ((2, 2), (3, 4), (20, 24), (128, 128))                                       # (cols, ld)
COLSUM_ROWS = (1, 127, 128, 129, 20011)
LN_ROWS = (1, 3, 63, 64, 65, 257, 20011)
LN_D = (128, 112, 64, 48, 40)
EMBED_BN = (1, 63, 64, 513, 8191)
REDUCE_G = (1, 2, 15, 16, 17, 255, 256)


def plan(rows, K, math_):
    from lagrangebench_amd import _lib
    return _lib.train_probe_plan(rows, K, math_)


def n_add(chunk, G):
    """The longest addition chain of one output through producer (chunk rows), k_part_reduce (ceil(G / 16) partials per range,
    16 ranges) and the final +=."""
    return chunk + (G + 15) // 16 + 17


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- inputs (CPU tensors, float32)
def dw_inputs(family, rows, K, M=128, seed=0, extra_rows=0):
    """X (rows + extra_rows, K), dY (rows + extra_rows, M) float32 of one family."""
    g = gen(1000003 * seed + 7919 * rows + 31 * K + M + (0 if family == "exact" else 1))
    n = rows + extra_rows
    if family == "exact":
        X = torch.randint(-4, 5, (n, K), generator=g).float() * (torch.rand((n, K), generator=g) < 0.5).float()
        dY = torch.randint(-4, 5, (n, M), generator=g).float() * 0.25
    else:
        X = torch.relu(torch.randn((n, K), generator=g))
        e = torch.randint(-20, 11, ((n + 63) // 64,), generator=g).repeat_interleave(64)[:n]
        dY = torch.randn((n, M), generator=g) * torch.exp2(e.float())[:, None]
    return X, dY


def ln_inputs(family, rows, d, n_gth, seed=0):
    """z, b1, scale, dy (rows x 128), gth (n_gth x 128), gidx (rows): zero beyond column d (what a latent narrower than 128
    leaves there: the padded columns of every activation and of every gradient that reaches this kernel are zero).  Rows
    have a mean of z + b1 within one standard deviation."""
    g = gen(7 * seed + 13 * rows + d + (0 if family == "exact" else 5))
    keep = (torch.arange(128) < d).float()
    if family == "exact":
        z = torch.randint(-4, 5, (rows, 128), generator=g).float()
        b1 = torch.randint(-2, 3, (128,), generator=g).float()
        scale = torch.randint(-3, 4, (128,), generator=g).float()
        dy = torch.randint(-4, 5, (rows, 128), generator=g).float() * 0.25
        gth = torch.randint(-4, 5, (n_gth, 128), generator=g).float() * 0.25
    else:
        rs = torch.exp2(torch.randint(-3, 4, (rows, 1), generator=g).float())
        z = (torch.randn((rows, 128), generator=g) + 0.5 * (2 * torch.rand((rows, 1), generator=g) - 1)) * rs
        b1 = 0.05 * torch.randn((128,), generator=g)
        scale = 1.0 + 0.3 * torch.randn((128,), generator=g)
        dy = torch.randn((rows, 128), generator=g) * torch.exp2(torch.randint(-8, 5, (rows, 1), generator=g).float())
        gth = torch.randn((n_gth, 128), generator=g)
    gidx = torch.randint(0, n_gth, (rows,), generator=g).int()
    gidx[0] = 0                                   # an index of 0, the largest row and a repeat are always there
    gidx[-1] = n_gth - 1 if rows > 1 else 0
    if rows > 3:
        gidx[1] = n_gth - 1
        gidx[2] = gidx[rows // 2]
    return z * keep, b1 * keep, scale * keep, dy * keep, gth * keep, gidx


def embed_inputs(family, BN, emb=16, ntypes=9, absent=3, ld=24, col0=5, seed=0):
    g = gen(11 * seed + BN + (0 if family == "exact" else 3))
    pt = torch.randint(-1, ntypes - 1, (BN,), generator=g).int()   # -1 wraps to the last row
    pt[pt == absent] = absent + 1
    if BN > 1:
        pt[BN // 2] = -1
    x = torch.randint(-4, 5, (BN, ld), generator=g).float() if family == "exact" else torch.randn((BN, ld), generator=g)
    return x, pt


def xdyn_row_scale(rows, chunk):
    """per row: 2^15 in the even chunks, 2^-15 in the odd ones - no single X exponent fits a site whose chunks lie 2^30 apart"""
    return torch.where((torch.arange(rows) // chunk) % 2 == 0, torch.tensor(2.0 ** 15), torch.tensor(2.0 ** -15))


# ---------------------------------------------------------------------------------------------- float64 references
def dw_reference(X, dY, rows, K):
    """(X[:rows, :K]^T dY[:rows], column sums of dY[:rows]) in float64."""
    x, y = X[:rows, :K].to(F64), dY[:rows].to(F64)
    return x.T @ y, y.sum(0)


def ln_reference(z, b1, scale, dy, d, gth=None, gidx=None):
    """(dz, d scale, d offset) of y = layer_norm(z + b1)[:, :d] * scale + offset from torch autograd in float64."""
    g = dy.to(F64)
    if gth is not None:
        g = g + gth.to(F64)[gidx.long()]
    zz = z.to(F64)[:, :d].clone().requires_grad_(True)
    sc = scale.to(F64)[:d].clone().requires_grad_(True)
    of = torch.zeros(d, dtype=F64, device=z.device, requires_grad=True)
    y = torch.nn.functional.layer_norm(zz + b1.to(F64)[:d], (d,), eps=1e-5) * sc + of
    (y * g[:, :d]).sum().backward()
    return zz.grad, sc.grad, of.grad


def embed_reference(x, pt, col0, emb, ntypes):
    q = torch.where(pt < 0, pt + ntypes, pt).long()
    return torch.zeros((ntypes, emb), dtype=F64, device=x.device).index_add_(0, q, x[:, col0:col0 + emb].to(F64))


# ---------------------------------------------------------------------------------------------- bounds
def _chunk_ids(rows, chunk, device):
    return torch.arange(rows, device=device) // chunk


def _chunk_max(v, rows, chunk):
    """per row: the largest entry of v (rows,) over the row's chunk"""
    ids = _chunk_ids(rows, chunk, v.device)
    G = (rows + chunk - 1) // chunk
    m = torch.zeros(G, dtype=v.dtype, device=v.device).scatter_reduce_(0, ids, v, "amax", include_self=True)
    return m[ids]


def dw_scale_max(dY, rows, chunk, tmax=False):
    """m(r): the largest |dY| of the chunk of row r; with tmax the largest over the 16-row tiles that chunk touches."""
    a = dY[:rows].to(F64).abs().amax(1)
    if not tmax:
        return _chunk_max(a, rows, chunk)
    nt = (rows + 15) // 16
    t = torch.zeros(nt, dtype=F64, device=a.device).scatter_reduce_(0, torch.arange(rows, device=a.device) // 16, a, "amax")
    G = (rows + chunk - 1) // chunk
    m = torch.zeros(G, dtype=F64, device=a.device)
    for gi in range(G):   # (the tmax cases are few and G <= 256)
        r0, r1 = gi * chunk, min(rows, (gi + 1) * chunk)
        m[gi] = t[r0 // 16:(r1 + 15) // 16].max()
    return m[_chunk_ids(rows, chunk, a.device)]


def dw_bound(X, dY, rows, K, pl, math_, xexp=0, xdyn=False, tmax=False):
    """(bound on dW (K x M), bound on db (M)) for the accuracy inputs.
    fp32: |err_kj| <= 2 n_add u sum_r |x_rk dy_rj| (2: the MFMA's four-term sum need not round once per add), db without X.
    f16x2 adds sum_r (3 2^-22 |x_rk| + 2^-25 2^-xexp) m(r): 2^-22 of split error per operand and the dropped lo x lo term,
    and the 2^-25 absolute floor of a subnormal lo half of the scaled X (k_dw_part_h's header).  xdyn: |x_rk| becomes the
    largest |X| of the chunk's 128-column slice and 2^-xexp the power of two that kernel scales it by."""
    x, y = X[:rows, :K].to(F64).abs(), dY[:rows].to(F64).abs()
    na = n_add(pl["chunk"], pl["G"])
    bw = 2 * na * U * (x.T @ y)
    bb = 2 * na * U * y.sum(0)
    if math_ and K >= 32:
        m = dw_scale_max(dY, rows, pl["chunk"], tmax)
        if xdyn:
            xs = torch.zeros_like(x)
            fl = torch.zeros_like(x)
            for c0 in range(0, K, 128):
                mx = _chunk_max(x[:, c0:c0 + 128].amax(1), rows, pl["chunk"])
                xs[:, c0:c0 + 128] = mx[:, None]
                fl[:, c0:c0 + 128] = torch.exp2(torch.floor(torch.log2(mx.clamp_min(2.0 ** -126))))[:, None]
            extra = ((3 * 2.0 ** -22 * xs + 2.0 ** -25 * fl) * m[:, None]).sum(0)
        else:
            extra = ((3 * 2.0 ** -22 * x + 2.0 ** -25 * 2.0 ** -xexp) * m[:, None]).sum(0)
        bw = bw + extra[:, None]
    return bw, bb


def colsum_bound(x, rows, cols):
    """128 adds in a block, ceil(nb / 16) + 16 in the reduce, the +=: one rounding each"""
    nb = (rows + 127) // 128
    return (128 + (nb + 15) // 16 + 17) * U * x[:rows, :cols].to(F64).abs().sum(0)


def ln_terms(z, b1, scale, dy, d, gth=None, gidx=None):
    """float64 (g, h, rs, u) of the LayerNorm backward over the first d columns"""
    g = dy.to(F64)
    if gth is not None:
        g = g + gth.to(F64)[gidx.long()]
    g = g[:, :d]
    x = (z.to(F64) + b1.to(F64))[:, :d]
    mean = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    return g, (x - mean) * rs, rs, g * scale.to(F64)[:d]


def ln_bound(z, b1, scale, dy, d, gth=None, gidx=None):
    """(bound on dz (rows x d), on d scale (d), on d offset (d)).
    dz = rs (u - a - h b), a = mean u, b = mean (u h):  |err_rj| <= 48 u rs_r (|u_rj| + A_r + (1 + |h_rj|) B_r) with
    A_r = mean_j |u_rj|, B_r = mean_j |u_rj h_rj|, for rows whose mean is within one standard deviation (the centring then
    loses no more than one bit).  48 counts the roundings on the longest path of an output: the four row sums (mean, variance,
    a, b) are seven levels deep (three adds inside a lane, four DPP steps over its 16 lanes) = 28; plus z + b1, x - mean, the
    mean's 1/d, the square, the variance's padding correction, its 1/d, + eps, the square root, the reciprocal, h = d rs,
    u = g scale, (+ the gathered term), u h, a's and b's 1/d, h b, the two subtractions, the final rs and the keep mask = 20.
    Parameter gradients: n_add u sum_r |g| for the offset, n_add = 64 + ceil(nb / 16) + 17, and for the scale
        u sum_r |g_rj| ((n_add + 12) |h_rj| + rs_r (|x_rj| + 8 M_r)),   x = z + b1, M_r = mean_j |x_rj|.
    The first term alone - (n_add + 12) u sum_r |g h|, 12 for the roundings inside h - treats the error of h as RELATIVE to
    h.  It is not: h = (x - mean) rs cancels where x is close to the row's mean, and what is left of the roundings of x (u |x|)
    and of the mean (seven levels and the 1/d: 8 u M_r) is absolute, rs_r (|x_rj| + 8 M_r) u whatever h_rj is.  With many rows
    the other rows' |g h| cover it; with one row and an entry at h = 8e-4 they do not: the float32 twin - not the device - sits
    at 9.2 x the first term alone for rows = 1, d = 112 (test_train_kernels.py runs every case), the device at 5.1 x."""
    g, h, rs, u = ln_terms(z, b1, scale, dy, d, gth, gidx)
    x = (z.to(F64) + b1.to(F64))[:, :d].abs()
    A = u.abs().mean(1, keepdim=True)
    B = (u * h).abs().mean(1, keepdim=True)
    bz = 48 * U * rs * (u.abs() + A + (1 + h.abs()) * B)
    nb = (z.shape[0] + LNB_ROWS - 1) // LNB_ROWS
    na = LNB_ROWS + (nb + 15) // 16 + 17
    bs = U * (g.abs() * ((na + 12) * h.abs() + rs * (x + 8 * x.mean(1, keepdim=True)))).sum(0)
    return bz, bs, na * U * g.abs().sum(0)


def embed_bound(x, pt, col0, emb, ntypes):
    """(BN / 64 + 64) u sum |v| per (type, column): BN / S terms per slice with S = 1024 / emb = 64 slices, added in order"""
    BN = x.shape[0]
    q = torch.where(pt < 0, pt + ntypes, pt).long()
    s = torch.zeros((ntypes, emb), dtype=F64, device=x.device).index_add_(0, q, x[:, col0:col0 + emb].to(F64).abs())
    return (BN / 64 + 64) * U * s


# ---------------------------------------------------------------------------------------------- CPU twins
MUTATIONS = ("drop_last_row", "drop_chunk", "shift_cols", "overwrite", "db_rows_plus_1")


def _split16(v):
    hi = v.to(torch.float16)
    lo = (v - hi.to(v.dtype)).to(torch.float16)
    return hi.to(F64), lo.to(F64)


def _pow2_scale(m):
    """(sc, inv) of k_dw_part_h for a chunk maximum m: sc m in [1, 2)"""
    if m == 0:
        return 1.0, 1.0
    e = min(max(math.floor(math.log2(m)), -126), 126)
    return 2.0 ** -e, 2.0 ** e


def dw_twin(X, dY, rows, K, pl, math_, prefill_w=None, prefill_b=None, xexp=0, xdyn=False, tmax=False, mutate=None,
            mutate_chunk=0):
    """dW, db as a float32 restatement with the launcher's row chunks: a chunk's partial is one float32 matrix product (the
    library's order, not the kernel's), the partials are added in float32 in chunk order.  f16x2: hi = float16(s x),
    lo = float16(s x - hi) for both operands under the kernel's power-of-two scales and the three products hi hi + hi lo +
    lo hi in float64, rounded to float32 per chunk.  mutate: one of MUTATIONS - a deliberately wrong variant."""
    chunk, G = pl["chunk"], pl["G"]
    h = bool(math_) and K >= 32
    M = dY.shape[1]
    w = torch.zeros((K, M), dtype=torch.float32) if prefill_w is None or mutate == "overwrite" else prefill_w.clone().float()
    b = torch.zeros(M, dtype=torch.float32) if prefill_b is None or mutate == "overwrite" else prefill_b.clone().float()
    x, y = X[:, :K].float(), dY.float()
    if mutate == "shift_cols":
        y = torch.roll(y, 1, dims=1)
    if tmax:
        mrow = dw_scale_max(dY, rows, chunk, True)
    accw = torch.zeros((K, M), dtype=torch.float32)
    accb = torch.zeros(M, dtype=torch.float32)
    for gi in range(G):
        r0, r1 = gi * chunk, min(rows, (gi + 1) * chunk)
        if mutate == "drop_chunk" and gi == mutate_chunk:
            continue
        r1w = r1 - 1 if mutate == "drop_last_row" and gi == mutate_chunk else r1
        xc, yc = x[r0:r1w], y[r0:r1w]
        if h:
            m = float(mrow[r0]) if tmax else float(yc.abs().max()) if r1w > r0 else 0.0
            sc, inv = _pow2_scale(m)
            yh, yl = _split16(yc.to(F64) * sc)
            p = torch.zeros((K, M), dtype=F64)
            for c0 in range(0, K, 128):
                xs = xc[:, c0:c0 + 128].to(F64)
                scx, invx = (_pow2_scale(float(xs.abs().max())) if r1w > r0 else (1.0, 1.0)) if xdyn else (2.0 ** xexp, 2.0 ** -xexp)
                xh, xl = _split16(xs * scx)
                p[c0:c0 + 128] = (xh.T @ yh + xh.T @ yl + xl.T @ yh) * inv * invx
            accw += p.float()
        else:
            accw += xc.T @ yc
        r1b = r1 + 1 if mutate == "db_rows_plus_1" and gi == G - 1 else r1
        accb += y[r0:r1b].sum(0)
    return w + accw, b + accb


def narrow_twin(X, dY, rows, K, M, chunk):
    acc = torch.zeros((K, M), dtype=torch.float32)
    for r0 in range(0, rows, chunk):
        acc += X[r0:min(rows, r0 + chunk), :K].float().T @ dY[r0:min(rows, r0 + chunk), :M].float()
    return acc


def colsum_twin(x, rows, cols):
    acc = torch.zeros(cols, dtype=torch.float32)
    for r0 in range(0, rows, 128):
        acc += x[r0:min(rows, r0 + 128), :cols].float().sum(0)
    return acc


def ln_twin(z, b1, scale, dy, d, gth=None, gidx=None, zero_pad=True):
    """float32 restatement of k_ln_bwd2 over 128-wide rows (torch's summation order): (dz (rows x 128), d scale (128),
    d offset (128)).  zero_pad = False is the wrong variant that leaves the padded columns of dz unmasked."""
    g = dy.float()
    if gth is not None:
        g = g + gth.float()[gidx.long()]
    x = z.float() + b1.float()
    mean = x.sum(1, keepdim=True) / d
    dv = x - mean
    q = (dv * dv).sum(1, keepdim=True) - (128 - d) * mean * mean
    rs = 1.0 / torch.sqrt(q / d + 1e-5)
    h = dv * rs
    u = g * scale.float()
    a = u.sum(1, keepdim=True) / d
    b = (u * h).sum(1, keepdim=True) / d
    dz = rs * (u - a - h * b)
    if zero_pad:
        dz = dz * (torch.arange(128) < d).float()
    ds = torch.zeros(128)
    do = torch.zeros(128)
    for r0 in range(0, z.shape[0], LNB_ROWS):
        ds += (g * h)[r0:r0 + LNB_ROWS].sum(0)
        do += g[r0:r0 + LNB_ROWS].sum(0)
    return dz, ds, do


def embed_twin(x, pt, col0, emb, ntypes):
    q = torch.where(pt < 0, pt + ntypes, pt).long()
    return torch.zeros((ntypes, emb), dtype=torch.float32).index_add_(0, q, x[:, col0:col0 + emb].float())


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound over the entries (0 / 0 counts as 0, anything over a zero bound as inf)"""
    err = (got.to(F64) - ref.to(F64)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.to(F64))
    return float(r.max()) if r.numel() else 0.0


def bits(t):
    """the float32 bit patterns of t (+ 0.0: a zero compares without its sign - 0 x -1/4 is -0 in a reference that starts from
    its first product and +0 in an accumulator that starts from +0)"""
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32) + np.float32(0.0)).view(np.uint32)


@lru_cache(maxsize=None)
def dw_case_data(family, rows, K, ldx, seed=0):
    """(X (rows x ldx: the first K columns hold the case, the rest zeros), dY) on the CPU - one copy shared by the tests"""
    X, dY = dw_inputs(family, rows, K, seed=seed)
    Xp = torch.zeros((rows, ldx))
    Xp[:, :K] = X
    return Xp, dY
