// lb_train_painn.h - the PaiNN training step on the device; IMPLEMENTATION INCLUDE of lb_train.hip (one translation unit: it
// uses that file's fp32-MFMA products, ordered reductions, loss bookkeeping and AdamW), as lb_train_egnn.h is.
//
// Reference: PaiNN.__call__ / _embed / _get_filters / PaiNNLayer._message / _update / PaiNNReadout / GatedEquivariantBlock /
// gaussian_rbf / cosine_cutoff of lagrangebench/models/painn.py under value_and_grad of _mse (train/trainer.py:35-89);
// gradients checked against float64 torch autograd of tests/_painn_oracle.py.
//
// Design.  The forward IS the inference forward: the k_pn_* kernels of lb_painn.hip run on a weightless lb_painn view of the
// handle's weight blob, taps on (s^l, v^l for l = 0 .. L), so the prediction is PaiNN.apply's bit for bit.  The backward
// walks the layers in reverse and recomputes one layer's activations from its taps right before that layer's backward runs.
// The network never moves positions: edge norm, direction, cutoff and the radial basis input are constants of the step and
// no gradient flows into geometry.  Device blobs are 128 wide (hidden < 128 is zero-padded as in EGNN training; the
// caller's blob goes through t->cmap): the layout is lb_painn_create's at hidden 128.  A padded unit is 0 everywhere but
// in the two norms sqrt(sum_d v_r^2 + eps) = 1e-4, which meet zero weight rows in the forward; the backward's recomputed
// norm columns are written as 0 there, so those rows get zero gradients and stay zero under AdamW.
// Products.  Every dense contraction runs on the exact-fp32 kernels of the training core (k_lin32 / k_lin32f, k_dw_part +
// the ordered k_part_reduce; f16x2 off), 128 output columns at a time: a 3H = 384 wide Linear is three column blocks of one
// row-major matrix (operand stride 384; the weight gradient's descriptor carries the row stride).  Everything else is
// elementwise / gather kernels (k_pnt_*).  The sums over senders of the forward have adjoints that are sums over each
// node's own receiver row (CSR order) of terms gathered from the senders' upstream gradients: every edge sits in exactly
// one receiver row, so an edge held in one direction only is counted once; the recomputed forward sums go through rev[]
// and the orphans as k_pn_msg's do.  Dead edges (cutoff 0) are skipped and leave zero rows in the per-edge filter
// gradient.  No float atomics; every sum has a fixed order: two calls give the same gradient bits.
// Sharing: layers that share parameters (shared_interactions / shared_filters) add into the same gradient entries, so the
// reductions of one layer are flushed (one k_part_reduce launch) before the next layer's are queued.
// Frozen radial basis: widths / offsets are the last 2 R floats of the blob; with rbf_trainable = 0 they are the handle's
// frozen tail (t->n_frozen), outside the range AdamW walks, and nothing is added to their gradient.
// Limits: 13 reductions per layer + 12 share the LB_RED_MAX descriptors of a step: num_mp_steps <= 32.
#pragma once

#define PNT_W 128          // device width of every hidden layer
#define PNT_WH 64          // ... and of the readout's halves
#define PNT_XS 32          // row stride of the scalar embedding's input (n_vels + 9 <= 18 columns)
#define PNT_XV 16          // row stride of the vector embedding's input (n_vels + 3 <= 12 channels)
#define PNT_MAX_LAYERS 32
#define PNT_TN 4           // nodes per workgroup of the message kernels

struct lb_pnt_layer {   // float offsets into the device blobs
  int64_t wi0, bi0, wi1, bi1, wm0, bm0, wm1, bm1, wvm;
};

struct lb_pnt {
  lb_painn_desc desc;        // the model's (hidden = its real width)
  lb_painn* view = nullptr;  // the inference forward on t->w (hidden 128)
  int n_scal = 0, n_vec = 0, c_frc = -1, c_bnd = -1, ldp = 0, rbf_trainable = 0;
  int64_t w_se = 0, b_se = 0, w_ve = 0, w_f = 0, b_f = 0, r0_vm = 0, r0_w0 = 0, r0_b0 = 0, r0_w1 = 0, r0_b1 = 0, ro_vm = 0,
          ro_w0 = 0, ro_b0 = 0, ro_w1 = 0, ro_b1 = 0, widths = 0, offsets = 0;
  std::vector<lb_pnt_layer> layers;
  float *tap_s = nullptr, *tap_v = nullptr;
  // node scratch
  float *xs = nullptr, *xv = nullptr, *ds = nullptr, *dv = nullptr, *dv2 = nullptr, *zi0 = nullptr, *hi = nullptr, *x3 = nullptr,
        *pre_s = nullptr, *pre_v = nullptr, *v_m = nullptr, *vm = nullptr, *ts = nullptr, *zm0 = nullptr, *hm = nullptr,
        *m3 = nullptr, *dm3 = nullptr, *dvm = nullptr, *dhm = nullptr, *dts = nullptr, *dx3 = nullptr;
  float *g1x = nullptr, *dz1 = nullptr, *u1 = nullptr, *dyg = nullptr, *vp = nullptr, *dalr = nullptr;
  // edge scratch
  float *phi = nullptr, *dphi = nullptr, *dpre = nullptr;
  lb_painn_state st{};
  int red_used = 0;   // descriptors of the step already handed to k_part_reduce (pnt_flush)
};

// ---------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ float pnt_silu(float x) { return x / (1.f + expf(-x)); }   // = pn_silu of lb_painn.hip
__device__ __forceinline__ float pnt_dsilu(float x) {
  const float s = 1.f / (1.f + expf(-x));
  return s + x * s * (1.f - s);
}
__device__ __forceinline__ float pnt_clip(float x) { return fminf(fmaxf(x, -100.f), 100.f); }
__device__ __forceinline__ float pnt_pass(float pre, float g) { return fabsf(pre) < 100.f ? g : 0.f; }   // d clip

// the embeddings' input rows (k_pn_embed's values): xs = [vel_mag (| one-hot)], xv[(i, d)] = [v_0 .. v_{K-1} | force | bound_lo | bound_hi][d]
__global__ void k_pnt_xin(int64_t BN, int dim, int isl, int n_vels, int homogeneous, int c_frc, int c_bnd,
                          const float* __restrict__ xnode, const int32_t* __restrict__ ptype, float* __restrict__ xs,
                          float* __restrict__ xv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN) return;
  const float* x = xnode + i * 64;
  const int K = isl - 1;
  float* o = xs + i * PNT_XS;
  int c = 0;
  for (int k = 0; k < n_vels; ++k) o[c++] = x[K * dim + k];
  if (!homogeneous) {
    const int pt = ptype[i];
    for (int j = 0; j < 9; ++j) o[c++] = j == pt ? 1.f : 0.f;
  }
  for (; c < PNT_XS; ++c) o[c] = 0.f;
  for (int d = 0; d < dim; ++d) {
    float* v = xv + (i * dim + d) * PNT_XV;
    int q = 0;
    for (; q < n_vels; ++q) v[q] = x[q * dim + d];
    if (c_frc >= 0) v[q++] = x[c_frc + d];
    if (c_bnd >= 0) {
      v[q++] = x[c_bnd + d];
      v[q++] = x[c_bnd + dim + d];
    }
    for (; q < PNT_XV; ++q) v[q] = 0.f;
  }
}

// e->acc (rows of 4) -> pred (rows of dim)
__global__ void k_pnt_pred(int64_t BN, int dim, const float* __restrict__ acc, float* __restrict__ pred) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN) return;
  for (int d = 0; d < dim; ++d) pred[i * dim + d] = acc[i * 4 + d];
}

// radial basis of every edge: phi[e][q] = exp(-0.5 / w_q^2 (norm_e - o_q)^2), a zero row on a dead edge
__global__ void k_pnt_phi(int64_t E, int R, int ldp, const float* __restrict__ nrm, const float* __restrict__ widths,
                          const float* __restrict__ offsets, float* __restrict__ phi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * ldp) return;
  const int64_t e = i / ldp;
  const int q = (int)(i % ldp);
  const float norm = nrm[e];
  float v = 0.f;
  if (q < R && norm >= 0.f) {
    const float w = widths[q], df = norm - offsets[q];
    v = expf((-0.5f / (w * w)) * (df * df));
  }
  phi[i] = v;
}

// d widths / d offsets terms of every edge, in place: dphi <- dphi phi (x - o)^2 / w^3, phi <- dphi phi (x - o) / w^2
__global__ void k_pnt_rbf_bwd(int64_t E, int R, int ldp, const float* __restrict__ nrm, const float* __restrict__ widths,
                              const float* __restrict__ offsets, float* __restrict__ phi, float* __restrict__ dphi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * ldp) return;
  const int64_t e = i / ldp;
  const int q = (int)(i % ldp);
  const float norm = nrm[e];
  float tw = 0.f, to = 0.f;
  if (q < R && norm >= 0.f) {
    const float w = widths[q], df = norm - offsets[q];
    const float g = dphi[i] * phi[i];
    tw = g * (df * df) / (w * w * w);
    to = g * df / (w * w);
  }
  dphi[i] = tw;
  phi[i] = to;
}

// y = silu(z), dz = dy silu'(z) over n floats
__global__ void k_pnt_silu(int64_t n, const float* __restrict__ z, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = pnt_silu(z[i]);
}
__global__ void k_pnt_dsilu(int64_t n, const float* dy, const float* __restrict__ z, float* dz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dz[i] = dy[i] * pnt_dsilu(z[i]);
}

// the three filter values of edge e at column j: (rbf(norm_e) Wf + bf) * scale_e, as k_pn_msg forms them
struct pnt_filt {
  float f0, f1, f2;
};
__device__ __forceinline__ pnt_filt pnt_filter(float norm, float scale, int n_rbf, const float* s_coef, const float* s_off,
                                               const float* __restrict__ wf, const float* __restrict__ bf, int ldf) {
  float f0 = 0.f, f1 = 0.f, f2 = 0.f;
  for (int q = 0; q < n_rbf; ++q) {
    const float df = norm - s_off[q];
    const float ph = expf(s_coef[q] * (df * df));
    f0 += ph * wf[q * ldf];
    f1 += ph * wf[q * ldf + PNT_W];
    f2 += ph * wf[q * ldf + 2 * PNT_W];
  }
  return pnt_filt{(f0 + bf[0]) * scale, (f1 + bf[PNT_W]) * scale, (f2 + bf[2 * PNT_W]) * scale};
}

struct pnt_msg_args {
  int64_t BN;
  int E, dim, n_rbf, ldf, fcol;
  const int32_t *row_ptr, *rev, *orph, *senders, *receivers;
  const f32x4* geo;
  const float* nrm;
  const float *w_rbf, *o_rbf, *wf, *bf;
  const float* x3;    // [BN][3 W]
  const float* s;     // s^l, v^l (the taps)
  const float* v;
  // forward: pre-clip sums, the message block's outputs (s_m into rows of lds floats)
  float *pre_s, *pre_v, *s_m, *v_m;
  int lds;
  // backward: upstream d s_m, d v_m; d x3 (three planes of BN x W), d v^l, the per-edge d filters * scale (three planes of E x W)
  const float *ds, *dv;
  float *dx3, *dv_out, *dpre;
};

// recomputed message block (k_pn_msg's sums in k_pn_msg's order) with the pre-clip values kept
__global__ void __launch_bounds__(128) k_pnt_msg_fwd(pnt_msg_args a) {
  __shared__ float s_coef[64], s_off[64];
  if (threadIdx.x < a.n_rbf) {
    const float w = a.w_rbf[threadIdx.x];
    s_coef[threadIdx.x] = -0.5f / (w * w);
    s_off[threadIdx.x] = a.o_rbf[threadIdx.x];
  }
  __syncthreads();
  const int dim = a.dim, j = threadIdx.x, E = a.E;
  const int64_t base = (int64_t)blockIdx.x * PNT_TN;
  for (int t = 0; t < PNT_TN; ++t) {
    const int64_t i = base + t;
    if (i >= a.BN) break;
    int k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
    k0 = k0 < E ? k0 : E;
    k1 = k1 < E ? k1 : E;
    float ds = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;
    auto add = [&](int e) {
      const float norm = a.nrm[e];
      if (norm < 0.f) return;
      const f32x4 gm = a.geo[e];
      const int r = a.receivers[e];
      const pnt_filt f = pnt_filter(norm, gm[3], a.n_rbf, s_coef, s_off, a.wf + a.fcol + j, a.bf + a.fcol + j, a.ldf);
      const float* xr = a.x3 + (int64_t)r * 3 * PNT_W + j;
      const float ws = f.f0 * xr[0], wv1 = f.f1 * xr[PNT_W], wv2 = f.f2 * xr[2 * PNT_W];
      const float* vr = a.v + (int64_t)r * dim * PNT_W + j;
      ds += ws;
      dv0 += wv1 * gm[0] + wv2 * vr[0];
      dv1 += wv1 * gm[1] + wv2 * vr[PNT_W];
      if (dim == 3) dv2 += wv1 * gm[2] + wv2 * vr[2 * PNT_W];
    };
    for (int k = k0; k < k1; ++k) {
      const int e = a.rev[k];
      if (e >= 0) add(e);
    }
    lb_for_orphans(a.orph, a.senders, i, add);
    a.pre_s[i * PNT_W + j] = ds;
    a.s_m[i * a.lds + j] = a.s[i * PNT_W + j] + pnt_clip(ds);
    const int64_t o = i * dim * PNT_W + j;
    a.pre_v[o] = dv0;
    a.v_m[o] = a.v[o] + pnt_clip(dv0);
    a.pre_v[o + PNT_W] = dv1;
    a.v_m[o + PNT_W] = a.v[o + PNT_W] + pnt_clip(dv1);
    if (dim == 3) {
      a.pre_v[o + 2 * PNT_W] = dv2;
      a.v_m[o + 2 * PNT_W] = a.v[o + 2 * PNT_W] + pnt_clip(dv2);
    }
  }
}

// message block backward: node r walks its own receiver row (every edge is in exactly one row).  With gS, gV the clipped
// upstream gradients of the edge's sender: d x3[r], d v^l[r] = d v_m[r] + x2[r] sum f2 gV, d filters * scale per edge
__global__ void __launch_bounds__(128) k_pnt_msg_bwd(pnt_msg_args a) {
  __shared__ float s_coef[64], s_off[64];
  if (threadIdx.x < a.n_rbf) {
    const float w = a.w_rbf[threadIdx.x];
    s_coef[threadIdx.x] = -0.5f / (w * w);
    s_off[threadIdx.x] = a.o_rbf[threadIdx.x];
  }
  __syncthreads();
  const int dim = a.dim, j = threadIdx.x, E = a.E;
  const int64_t base = (int64_t)blockIdx.x * PNT_TN;
  const int64_t plane_e = (int64_t)E * PNT_W, plane_n = a.BN * PNT_W;
  for (int t = 0; t < PNT_TN; ++t) {
    const int64_t r = base + t;
    if (r >= a.BN) break;
    int k0 = a.row_ptr[r], k1 = a.row_ptr[r + 1];
    k0 = k0 < E ? k0 : E;
    k1 = k1 < E ? k1 : E;
    const float* xr = a.x3 + r * 3 * PNT_W + j;
    const float x0 = xr[0], x1 = xr[PNT_W], x2 = xr[2 * PNT_W];
    const int64_t ro = r * dim * PNT_W + j;
    const float vr0 = a.v[ro], vr1 = a.v[ro + PNT_W], vr2 = dim == 3 ? a.v[ro + 2 * PNT_W] : 0.f;
    float dx0 = 0.f, dx1 = 0.f, dx2 = 0.f, dva0 = 0.f, dva1 = 0.f, dva2 = 0.f;
    for (int e = k0; e < k1; ++e) {
      const float norm = a.nrm[e];
      float* dp = a.dpre + (int64_t)e * PNT_W + j;
      if (norm < 0.f) {
        dp[0] = 0.f;
        dp[plane_e] = 0.f;
        dp[2 * plane_e] = 0.f;
        continue;
      }
      const f32x4 gm = a.geo[e];
      const int s = a.senders[e];
      const pnt_filt f = pnt_filter(norm, gm[3], a.n_rbf, s_coef, s_off, a.wf + a.fcol + j, a.bf + a.fcol + j, a.ldf);
      const int64_t so = (int64_t)s * dim * PNT_W + j;
      const float gS = pnt_pass(a.pre_s[(int64_t)s * PNT_W + j], a.ds[(int64_t)s * PNT_W + j]);
      const float g0 = pnt_pass(a.pre_v[so], a.dv[so]);
      const float g1 = pnt_pass(a.pre_v[so + PNT_W], a.dv[so + PNT_W]);
      const float g2 = dim == 3 ? pnt_pass(a.pre_v[so + 2 * PNT_W], a.dv[so + 2 * PNT_W]) : 0.f;
      const float t1 = (gm[0] * g0 + gm[1] * g1) + gm[2] * g2;
      const float t2 = (vr0 * g0 + vr1 * g1) + vr2 * g2;
      dx0 += f.f0 * gS;
      dx1 += f.f1 * t1;
      dx2 += f.f2 * t2;
      dva0 += f.f2 * g0;
      dva1 += f.f2 * g1;
      dva2 += f.f2 * g2;
      dp[0] = (x0 * gS) * gm[3];
      dp[plane_e] = (x1 * t1) * gm[3];
      dp[2 * plane_e] = (x2 * t2) * gm[3];
    }
    float* dx = a.dx3 + r * PNT_W + j;
    dx[0] = dx0;
    dx[plane_n] = dx1;
    dx[2 * plane_n] = dx2;
    a.dv_out[ro] = a.dv[ro] + x2 * dva0;
    a.dv_out[ro + PNT_W] = a.dv[ro + PNT_W] + x2 * dva1;
    if (dim == 3) a.dv_out[ro + 2 * PNT_W] = a.dv[ro + 2 * PNT_W] + x2 * dva2;
  }
}

// out[i][ooff + c] = sqrt(sum_d vm[(i, d)][off + c]^2 + eps) for c < nreal, 0 for the padded columns nreal <= c < ncol
__global__ void k_pnt_vnorm(int64_t BN, int dim, const float* __restrict__ vm, int ldvm, int off, int ncol, int nreal,
                            float* __restrict__ out, int ldo, int ooff) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= BN * ncol) return;
  const int64_t i = q / ncol;
  const int c = (int)(q % ncol);
  float y = 0.f;
  if (c < nreal) {
    const float* p = vm + i * dim * ldvm + off + c;
    float acc = p[0] * p[0];
    for (int d = 1; d < dim; ++d) acc = acc + p[d * ldvm] * p[d * ldvm];
    y = sqrtf(acc + 1e-8f);
  }
  out[i * ldo + ooff + c] = y;
}

// update block backward, elementwise part: s' = s + clip(a + c <v_r, v_l>), v' = v + clip(v_l b) with [a | b | c] = m3.
// dm3: three planes (BN x W); dvm: two planes (BN dim x W) = d v_l, d v_r (without the norm's part)
__global__ void k_pnt_upd_bwd(int64_t BN, int dim, const float* __restrict__ m3, const float* __restrict__ vm,
                              const float* __restrict__ ds, const float* __restrict__ dv, float* __restrict__ dm3,
                              float* __restrict__ dvm) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= BN * PNT_W) return;
  const int64_t i = q / PNT_W;
  const int j = (int)(q % PNT_W);
  const float* mm = m3 + i * 3 * PNT_W + j;
  const float b = mm[PNT_W], c = mm[2 * PNT_W];
  const float* pv = vm + i * dim * 2 * PNT_W + j;
  float dot = pv[0] * pv[PNT_W];
  for (int d = 1; d < dim; ++d) dot = dot + pv[d * 2 * PNT_W] * pv[d * 2 * PNT_W + PNT_W];
  const float gs = pnt_pass(mm[0] + c * dot, ds[q]);
  const float gdot = gs * c;
  const int64_t plane = BN * dim * PNT_W;
  float db = 0.f;
  for (int d = 0; d < dim; ++d) {
    const float vl = pv[d * 2 * PNT_W], vr = pv[d * 2 * PNT_W + PNT_W];
    const int64_t o = (i * dim + d) * PNT_W + j;
    const float gv = pnt_pass(vl * b, dv[o]);
    db += gv * vl;
    dvm[o] = gv * b + gdot * vr;
    dvm[plane + o] = gdot * vl;
  }
  dm3[q] = gs;
  dm3[BN * PNT_W + q] = db;
  dm3[2 * BN * PNT_W + q] = gs * dot;
}

// the norm's part: with dts = d [s | |v_r|] (rows of ldt, the norms from column noff), ts its forward value:
// ds (+)= dts[:, :W] (first ncs columns), d v_r (+)= d norm v_r / norm.  set = 1: both are stored, not added
__global__ void k_pnt_norm_bwd(int64_t BN, int dim, int ncol, const float* __restrict__ dts, const float* __restrict__ ts, int ldt,
                               int noff, const float* __restrict__ vr, int ldv, float* __restrict__ dvr, int ldd, float* __restrict__ ds,
                               int set) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= BN * PNT_W) return;
  const int64_t i = q / PNT_W;
  const int j = (int)(q % PNT_W);
  const float g = dts[i * ldt + j];
  ds[q] = set ? g : ds[q] + g;
  if (j >= ncol) return;
  const float dn = dts[i * ldt + noff + j], n = ts[i * ldt + noff + j];
  for (int d = 0; d < dim; ++d) {
    const float t = n > 0.f ? dn * vr[(i * dim + d) * ldv + j] / n : 0.f;
    float* o = dvr + (i * dim + d) * ldd + j;
    *o = set ? t : *o + t;
  }
}

// The last gated block (H/2 -> 1) forward and backward, one thread per node (k_pn_readout's arithmetic).  In: y = the first
// block's gate net output (s' | gate), vm0 = its vector mix (v_l = the first 64 columns), dacc (BN x dim).  Out: dy = d y,
// d v_l into the first 64 columns of dvm0, and the operands of the block's weight gradients: g1x = [s' | |a_r| | 1],
// dz1 = d (gate_0 pre-activation), u1 = [silu | 1], dyg = (0, d gate'), vp = v_l gate per row, dalr = (d a_l, d a_r) per row
__global__ void __launch_bounds__(64) k_pnt_ro_bwd(int64_t BN, int dim, const float* __restrict__ y, const float* __restrict__ vm0,
                                                   const float* __restrict__ wvm, const float* __restrict__ w0,
                                                   const float* __restrict__ b0, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, const float* __restrict__ dacc,
                                                   float* __restrict__ dy, float* __restrict__ dvm0, float* __restrict__ g1x,
                                                   float* __restrict__ dz1, float* __restrict__ u1, float* __restrict__ dyg,
                                                   float* __restrict__ vp, float* __restrict__ dalr) {
  __shared__ float gin[64][65];
  __shared__ float zz[64][65];
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= BN) return;
  const int Hh = PNT_WH;
  const float* yi = y + i * PNT_W;
  float al0 = 0.f, al1 = 0.f, al2 = 0.f, ar0 = 0.f, ar1 = 0.f, ar2 = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d >= dim) continue;
    const float* vl = vm0 + (i * dim + d) * PNT_W;
    float l = 0.f, r = 0.f;
    for (int c = 0; c < Hh; ++c) {
      const float v = vl[c] * yi[Hh + c];
      l += v * wvm[2 * c];
      r += v * wvm[2 * c + 1];
    }
    if (d == 0) { al0 = l; ar0 = r; }
    if (d == 1) { al1 = l; ar1 = r; }
    if (d == 2) { al2 = l; ar2 = r; }
  }
  float q = ar0 * ar0;
  q = q + ar1 * ar1;
  if (dim == 3) q = q + ar2 * ar2;
  const float nn = sqrtf(q + 1e-8f);
  float* g = gin[threadIdx.x];
  float* z = zz[threadIdx.x];
  for (int c = 0; c < Hh; ++c) g[c] = yi[c];
  g[Hh] = nn;
  float gate = 0.f;
  for (int c = 0; c < Hh; ++c) {
    float zc = 0.f;
    for (int k = 0; k <= Hh; ++k) zc += g[k] * w0[k * Hh + c];
    zc = zc + b0[c];
    z[c] = zc;
    gate += pnt_silu(zc) * w1[2 * c + 1];
  }
  gate = gate + b1[1];
  const float* da = dacc + i * dim;
  const float d0 = da[0], d1 = da[1], d2 = dim == 3 ? da[2] : 0.f;
  const float dgp = (d0 * al0 + d1 * al1) + d2 * al2;
  const float dal0 = d0 * gate, dal1 = d1 * gate, dal2 = d2 * gate;
  for (int c = 0; c < Hh; ++c) {
    const float zc = z[c];
    const float dz = dgp * w1[2 * c + 1] * pnt_dsilu(zc);
    z[c] = dz;
    dz1[i * Hh + c] = dz;
    u1[i * 68 + c] = pnt_silu(zc);
  }
  u1[i * 68 + Hh] = 1.f;
  dyg[i * 2] = 0.f;
  dyg[i * 2 + 1] = dgp;
  for (int k = 0; k <= Hh; ++k) g1x[i * 68 + k] = g[k];
  g1x[i * 68 + Hh + 1] = 1.f;
  float dn = 0.f;
  for (int k = 0; k <= Hh; ++k) {
    float acc = 0.f;
    for (int c = 0; c < Hh; ++c) acc += w0[k * Hh + c] * z[c];
    if (k < Hh) dy[i * PNT_W + k] = acc;
    else dn = acc;
  }
  const float k_n = dn / nn;
  const float dar0 = k_n * ar0, dar1 = k_n * ar1, dar2 = k_n * ar2;
  for (int c = 0; c < Hh; ++c) {
    const float gt = yi[Hh + c], wl = wvm[2 * c], wr = wvm[2 * c + 1];
    float dg = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= dim) continue;
      const float dl = d == 0 ? dal0 : (d == 1 ? dal1 : dal2), dr = d == 0 ? dar0 : (d == 1 ? dar1 : dar2);
      const int64_t row = i * dim + d;
      const float vl = vm0[row * PNT_W + c];
      vp[row * Hh + c] = vl * gt;
      const float dvp = wl * dl + wr * dr;
      dg += dvp * vl;
      dvm0[row * PNT_W + c] = dvp * gt;
    }
    dy[i * PNT_W + Hh + c] = dg;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d >= dim) continue;
    dalr[(i * dim + d) * 2] = d == 0 ? dal0 : (d == 1 ? dal1 : dal2);
    dalr[(i * dim + d) * 2 + 1] = d == 0 ? dar0 : (d == 1 ? dar1 : dar2);
  }
}

// dW[K x 64] += X^T dY for K <= 68 (the last block's gate_0 with its bias row): wave kg of a 256-thread workgroup owns the
// rows k = kg, kg + 4, ... of dW, thread c its column c, over a contiguous chunk of rows; part[g][K][64] summed over g in
// ascending order by k_part_reduce
__global__ void __launch_bounds__(256) k_pnt_dw_small(const float* __restrict__ X, int ldx, int K, const float* __restrict__ dY,
                                                      int64_t rows, int64_t chunk, float* __restrict__ part) {
  const int c = threadIdx.x & 63, kg = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float acc[17];
#pragma unroll
  for (int a = 0; a < 17; ++a) acc[a] = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float dyv = dY[r * 64 + c];
    const float* xr = X + r * ldx;
#pragma unroll
    for (int a = 0; a < 17; ++a) {
      const int k = kg + 4 * a;
      acc[a] += (k < K ? xr[k] : 0.f) * dyv;
    }
  }
#pragma unroll
  for (int a = 0; a < 17; ++a) {
    const int k = kg + 4 * a;
    if (k < K) part[((int64_t)blockIdx.x * K + k) * 64 + c] = acc[a];
  }
}

// ------------------------------------------------------------------------------------------------------------- host
static void pnt_free(lb_gns_train* t) {
  lb_pnt* g = t->pa;
  if (!g) return;
  if (g->view) lb_painn_destroy(g->view);
  delete g;  // (its buffers are the handle arena's)
  t->pa = nullptr;
}

static int pnt_ensure(lb_gns_train* t, int64_t BN, int64_t E) {
  return train_ensure(t, BN, E, [t](int64_t cn, int64_t ce, int64_t) -> int {
    lb_pnt* g = t->pa;
    const size_t L = (size_t)g->desc.num_mp_steps, W = PNT_W, n = (size_t)cn, nd = (size_t)cn * t->eng->g.dim;
    LB_TRY(t->mem.get(&g->tap_s, (L + 1) * n * W));
    LB_TRY(t->mem.get(&g->tap_v, (L + 1) * nd * W));
    LB_TRY(t->mem.get(&t->pred, n * 4));
    LB_TRY(t->mem.get(&t->dy, n * 4));
    LB_TRY(t->mem.get(&g->xs, n * PNT_XS));
    LB_TRY(t->mem.get(&g->xv, nd * PNT_XV));
    for (float** p : {&g->ds, &g->zi0, &g->hi, &g->pre_s, &g->zm0, &g->hm, &g->dhm}) LB_TRY(t->mem.get(p, n * W));
    for (float** p : {&g->dv, &g->dv2, &g->pre_v, &g->v_m}) LB_TRY(t->mem.get(p, nd * W));
    for (float** p : {&g->x3, &g->m3, &g->dm3, &g->dx3}) LB_TRY(t->mem.get(p, n * 3 * W));
    LB_TRY(t->mem.get(&g->vm, nd * 2 * W));
    LB_TRY(t->mem.get(&g->dvm, nd * 2 * W));
    LB_TRY(t->mem.get(&g->ts, n * 2 * W));
    LB_TRY(t->mem.get(&g->dts, n * 2 * W));
    LB_TRY(t->mem.get(&g->g1x, n * 68));
    LB_TRY(t->mem.get(&g->u1, n * 68));
    LB_TRY(t->mem.get(&g->dz1, n * PNT_WH));
    LB_TRY(t->mem.get(&g->dyg, n * 2));
    LB_TRY(t->mem.get(&g->vp, nd * PNT_WH));
    LB_TRY(t->mem.get(&g->dalr, nd * 2));
    LB_TRY(t->mem.get(&g->phi, (size_t)ce * g->ldp));
    LB_TRY(t->mem.get(&g->dphi, (size_t)ce * g->ldp));
    LB_TRY(t->mem.get(&g->dpre, (size_t)ce * 3 * W));
    // partial-sum slots of the largest flush segment (one layer; the readout and the embeddings need less)
    const int64_t cnd = (int64_t)nd;
    t->red_cap = 8 * dw_acc_floats(cnd, 128) + 2 * dw_acc_floats(cn, 256) + 3 * dw_acc_floats(ce, 64) + 2 * colsum_floats(ce) +
                 2 * (DW_MAX_G * 128 * 4) + 64 * 68 * 64 + 4096;   // (... the readout's two dw_narrow, k_pnt_dw_small)
    return LB_OK;
  });
}

// one product on the training core's kernels: Y[rows x NO] (ldy) (+)= X[rows x NR] (ldx) Wop (+ bias), Wop = W (trans 0) or
// W^T (trans 1) of a row-major matrix with row stride ldw inside the weight blob
static int pnt_mm(lb_gns_train* t, int64_t rows, int NR, int NO, const float* X, int ldx, const float* W, int ldw, int trans,
                  float* Y, int ldy, int accum = 0, const float* bias = nullptr) {
  lb_lin_args a{};
  a.X = X; a.ldx = ldx; a.NR = NR; a.Y = Y; a.ldy = ldy; a.NO = NO; a.rows = rows; a.bias = bias; a.accum = accum;
  return lin32(t, a, W, ldw, trans);
}
// dW[K x 128] (row stride ldw) += X^T dY, db[128] += column sums of dY
static int pnt_dw(lb_gns_train* t, int64_t rows, int K, const float* X, int ldx, const float* dY, float* dW, int ldw, float* db) {
  if (rows <= 0) return LB_OK;
  if (!dw_acc(t, rows, K, X, ldx, dY, dW, db)) return LB_ERR_STATE;
  if (ldw != 128) t->red_tab.back().ld0 = ldw;
  return LB_OK;
}
// the reductions queued so far -> the gradient blob (one k_part_reduce launch); the descriptors of a step share red_host / red_dev
static int pnt_flush(lb_gns_train* t) {
  lb_pnt* g = t->pa;
  const size_t n = t->red_tab.size();
  if (n) {
    if (g->red_used + n > LB_RED_MAX) return lb_fail(LB_ERR_STATE, "painn training: more than %d reductions in a step", LB_RED_MAX);
    hipStream_t s = t->eng->stream;
    memcpy(t->red_host + g->red_used, t->red_tab.data(), n * sizeof(lb_red_ent));
    LB_HIP(hipMemcpyAsync(t->red_dev + g->red_used, t->red_host + g->red_used, n * sizeof(lb_red_ent), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_part_reduce, dim3((unsigned)t->red_blocks), dim3(1024), 0, s, t->dwpart, t->red_dev + g->red_used, (int)n,
                       t->g, t->dw_flag);
    g->red_used += (int)n;
  }
  red_reset(t);
  return LB_OK;
}

static int painn_forward(lb_gns_train* t, const float** pred);
static int painn_backward(lb_gns_train* t, double* dpos_out_dev);
// (lb_gns_train_loss_grad is its loss entry; the guard never fires - f16x2 off, no sender view: one attempt)
static const lb_train_model painn_model = {"PaiNN", "lb_gns_train_loss_grad", false, false, true, pnt_free, pnt_ensure,
                                           painn_forward, painn_backward, nullptr};

extern "C" int lb_painn_train_create(lb_engine* e, const lb_painn_desc* d, const float* w, int64_t n_floats, int32_t rbf_trainable,
                                     lb_gns_train** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->hidden < 64 || d->hidden > 128 || d->hidden % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "painn training: hidden size %d (a multiple of 16 from 64 to 128 is built)", d->hidden);
  if (d->num_mp_steps < 1 || d->num_mp_steps > PNT_MAX_LAYERS)
    return lb_fail(LB_ERR_UNSUPPORTED, "painn training: num_mp_steps %d (1 .. %d)", d->num_mp_steps, PNT_MAX_LAYERS);
  if (d->n_vels < 1 || d->n_vels > 9) return lb_fail(LB_ERR_ARG, "bad n_vels %d (1 .. 9)", d->n_vels);
  if (d->n_vels != e->g.isl - 1) return lb_fail(LB_ERR_ARG, "n_vels %d != input_seq_length-1", d->n_vels);
  if (d->n_rbf < 1 || d->n_rbf > 64) return lb_fail(LB_ERR_ARG, "bad n_rbf %d (1 .. 64)", d->n_rbf);
  const int L = d->num_mp_steps, H = d->hidden, Hh = H / 2, W = PNT_W, Wh = PNT_WH, R = d->n_rbf;
  lb_gns_train* t = new lb_gns_train();
  lb_pnt* g = new lb_pnt();
  t->model = &painn_model;
  t->pa = g;
  t->eng = e;
  t->f16x2 = false;   // exact fp32 products throughout (the reference's fp32 policy)
  g->desc = *d;
  g->rbf_trainable = rbf_trainable ? 1 : 0;
  const int dim = e->g.dim, K = e->g.isl - 1;
  g->n_scal = d->n_vels + (d->homogeneous ? 0 : 9);
  const int c_bnd = K * dim + K;   // raw row [vel_hist | vel_mag | bound | force] (lb_painn_create)
  g->c_bnd = e->g.has_bound ? c_bnd : -1;
  g->c_frc = e->g.force_kind != LB_FORCE_NONE ? c_bnd + (e->g.has_bound ? 2 * dim : 0) : -1;
  g->n_vec = d->n_vels + (g->c_frc >= 0 ? 1 : 0) + (g->c_bnd >= 0 ? 2 : 0);
  g->ldp = (R + 4) & ~3;   // (> R: k_dw_part's pair load of an odd R reads a padding column)
  const int n_sets = d->shared_interactions ? 1 : L, n_filt = d->shared_filters ? 1 : L;
  // device layout: lb_painn_create's with hidden 128; the caller's (PaiNN.flatten, hidden H) maps into it entry by entry
  int64_t o = 0, oc = 0;
  auto mat = [&](int rows_c, int cols_c, int rows_d, int cols_d, auto row_dev, auto col_dev) {
    const int64_t base = o;
    if (H != W)
      for (int r = 0; r < rows_c; ++r)
        for (int c = 0; c < cols_c; ++c) t->cmap.push_back(base + (int64_t)row_dev(r) * cols_d + col_dev(c));
    oc += (int64_t)rows_c * cols_c;
    o += (int64_t)rows_d * cols_d;
    return base;
  };
  auto same = [](int r) { return r; };
  auto blk = [H](int r) { return (r / H) * W + r % H; };              // blocks of H -> blocks of 128
  auto half = [Hh](int r) { return r < Hh ? r : Wh + (r - Hh); };    // the readout's two halves
  auto g0row = [H](int r) { return r < H ? r : W + (r - H); };        // [s (H) | norms (H / 2)]
  auto g1row = [Hh](int r) { return r < Hh ? r : Wh; };              // [s' (H / 2) | norm]
  g->w_se = mat(g->n_scal, H, g->n_scal, W, same, same);
  g->b_se = mat(1, H, 1, W, same, same);
  g->w_ve = mat(g->n_vec, H, g->n_vec, W, same, same);
  g->w_f = mat(R, n_filt * 3 * H, R, n_filt * 3 * W, same, blk);
  g->b_f = mat(1, n_filt * 3 * H, 1, n_filt * 3 * W, same, blk);
  for (int k = 0; k < n_sets; ++k) {
    lb_pnt_layer l{};
    l.wi0 = mat(H, H, W, W, same, same);
    l.bi0 = mat(1, H, 1, W, same, same);
    l.wi1 = mat(H, 3 * H, W, 3 * W, same, blk);
    l.bi1 = mat(1, 3 * H, 1, 3 * W, same, blk);
    l.wm0 = mat(2 * H, H, 2 * W, W, blk, same);
    l.bm0 = mat(1, H, 1, W, same, same);
    l.wm1 = mat(H, 3 * H, W, 3 * W, same, blk);
    l.bm1 = mat(1, 3 * H, 1, 3 * W, same, blk);
    l.wvm = mat(H, 2 * H, W, 2 * W, same, blk);
    g->layers.push_back(l);
  }
  g->r0_vm = mat(H, H, W, W, same, half);
  g->r0_w0 = mat(H + Hh, H, W + Wh, W, g0row, same);
  g->r0_b0 = mat(1, H, 1, W, same, same);
  g->r0_w1 = mat(H, H, W, W, same, half);
  g->r0_b1 = mat(1, H, 1, W, same, half);
  g->ro_vm = mat(Hh, 2, Wh, 2, same, same);
  g->ro_w0 = mat(Hh + 1, Hh, Wh + 1, Wh, g1row, same);
  g->ro_b0 = mat(1, Hh, 1, Wh, same, same);
  g->ro_w1 = mat(Hh, 2, Wh, 2, same, same);
  g->ro_b1 = mat(1, 2, 1, 2, same, same);
  g->widths = mat(1, R, 1, R, same, same);
  g->offsets = mat(1, R, 1, R, same, same);
  t->n_floats = o;
  t->n_compact = oc;
  t->n_frozen = g->rbf_trainable ? 0 : 2 * R;
  int rc = train_handle_init(t, "painn weight blob", w, n_floats);
  if (!rc) {
    lb_painn_desc vd = *d;
    vd.hidden = W;
    rc = lbk_painn_view_create(e, &vd, t->w, t->n_floats, &g->view);
  }
  return train_create_finish(t, rc, out);
}

// The inference view of the handle (lbk_painn_view_create on t->w): lb_painn_forward / lb_painn_rollout on it run on the
// CURRENT weights.  Borrowed: it lives and dies with t.
extern "C" int lb_painn_train_model(lb_gns_train* t, lb_painn** out) {
  if (!t || !out) return lb_fail(LB_ERR_ARG, "null argument");
  if (t->model != &painn_model) return lb_fail(LB_ERR_ARG, "not a PaiNN training handle");
  *out = t->pa->view;
  return LB_OK;
}

// The step in two parts, split at d loss / d pred (t->dy, BN x dim).  Forward part: the inference kernels on the current
// weights, taps on -> t->pred
static int painn_forward(lb_gns_train* t, const float**) {
  lb_engine* e = t->eng;
  lb_pnt* g = t->pa;
  const int64_t BN = t->fwd_BN;
  g->red_used = 0;
  LB_TRY(lb_painn_set_tap(g->view, g->tap_s, g->tap_v));
  g->st = lb_painn_state{};
  LB_TRY(lbk_painn_train_forward(e, g->view, &g->st));
  hipLaunchKernelGGL(k_pnt_pred, GRID1(BN), 0, e->stream, BN, e->g.dim, e->acc, t->pred);
  return LB_OK;
}

// from d loss / d pred in t->dy
static int painn_backward(lb_gns_train* t, double*) {
  lb_engine* e = t->eng;
  lb_pnt* g = t->pa;
  hipStream_t s = e->stream;
  const int64_t E = t->fwd_E, BN = t->fwd_BN;
  const int L = g->desc.num_mp_steps, dim = e->g.dim, W = PNT_W, Wh = PNT_WH, H = g->desc.hidden, R = g->desc.n_rbf;
  const int64_t BNd = BN * dim, nW = BN * W;
  const lb_painn_state& st = g->st;
  float* G = t->g;
  const float* Wt = t->w;
  const int n_filt = g->desc.shared_filters ? 1 : L, ldf = n_filt * 3 * W;
  hipLaunchKernelGGL(k_pnt_xin, GRID1(BN), 0, s, BN, dim, e->g.isl, g->desc.n_vels, g->desc.homogeneous, g->c_frc, g->c_bnd,
                     st.xnode, e->ptype, g->xs, g->xv);
  if (E)
    hipLaunchKernelGGL(k_pnt_phi, GRID1(E * g->ldp), 0, s, E, R, g->ldp, st.nrm, Wt + g->widths, Wt + g->offsets, g->phi);
  const float* sL = g->tap_s + (size_t)L * nW;
  const float* vL = g->tap_v + (size_t)L * BNd * W;
  // ---- readout.  Block 0 recomputed: vm0 = v^L Wvm (v_l | v_r), g0 = [s^L | |v_r|], y = silu(g0 W0 + b0) W1 + b1
  float *vm0 = g->vm, *g0 = g->ts, *zr0 = g->zm0, *hr = g->hm, *y = g->zi0, *dy = g->hi, *dvm0 = g->dvm, *dg0 = g->dts;
  const int K0 = W + Wh;
  LB_TRY(pnt_mm(t, BNd, W, W, vL, W, Wt + g->r0_vm, W, 0, vm0, W));
  LB_HIP(hipMemcpy2DAsync(g0, sizeof(float) * K0, sL, sizeof(float) * W, sizeof(float) * W, (size_t)BN, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_pnt_vnorm, GRID1(BN * Wh), 0, s, BN, dim, vm0, W, Wh, Wh, H / 2, g0, K0, W);
  LB_TRY(pnt_mm(t, BN, K0, W, g0, K0, Wt + g->r0_w0, W, 0, zr0, W, 0, Wt + g->r0_b0));
  hipLaunchKernelGGL(k_pnt_silu, GRID1(nW), 0, s, nW, zr0, hr);
  LB_TRY(pnt_mm(t, BN, W, W, hr, W, Wt + g->r0_w1, W, 0, y, W, 0, Wt + g->r0_b1));
  // the last block and its weight gradients
  hipLaunchKernelGGL(k_pnt_ro_bwd, dim3((unsigned)((BN + 63) / 64)), dim3(64), 0, s, BN, dim, y, vm0, Wt + g->ro_vm, Wt + g->ro_w0,
                     Wt + g->ro_b0, Wt + g->ro_w1, Wt + g->ro_b1, t->dy, dy, dvm0, g->g1x, g->dz1, g->u1, g->dyg, g->vp, g->dalr);
  LB_TRY(dw_narrow(t, BNd, 2, Wh, g->vp, Wh, g->dalr, 2, G + g->ro_vm));
  LB_TRY(dw_narrow(t, BN, 2, Wh + 1, g->u1, 68, g->dyg, 2, G + g->ro_w1));   // (row 64: gate_1's bias, next in the blob)
  {
    const int Ks = Wh + 2;   // [s' | norm | 1]: gate_0's weight and, as the last row, its bias (next in the blob)
    int64_t chunk = (BN + 63) / 64, off = 0;
    if (chunk < 64) chunk = 64;
    const int Gs = (int)((BN + chunk - 1) / chunk);
    float* part = red_slot(t, (int64_t)Gs * Ks * Wh, &off);
    if (!part) return LB_ERR_STATE;
    hipLaunchKernelGGL(k_pnt_dw_small, dim3(Gs), dim3(256), 0, s, g->g1x, 68, Ks, g->dz1, BN, chunk, part);
    red_push(t, off, Gs, (int64_t)Ks * Wh, Ks * Wh, 0, 0, G + g->ro_w0, nullptr);
  }
  // block 0 backward
  LB_TRY(pnt_dw(t, BN, W, hr, W, dy, G + g->r0_w1, W, G + g->r0_b1));
  LB_TRY(pnt_mm(t, BN, W, W, dy, W, Wt + g->r0_w1, W, 1, g->dhm, W));
  hipLaunchKernelGGL(k_pnt_dsilu, GRID1(nW), 0, s, nW, g->dhm, zr0, g->dhm);   // dhm = d zr0
  LB_TRY(pnt_dw(t, BN, K0, g0, K0, g->dhm, G + g->r0_w0, W, G + g->r0_b0));
  LB_TRY(pnt_mm(t, BN, W, W, g->dhm, W, Wt + g->r0_w0, W, 1, dg0, K0));
  LB_TRY(pnt_mm(t, BN, W, Wh, g->dhm, W, Wt + g->r0_w0 + (size_t)W * W, W, 1, dg0 + W, K0));
  // ds = d s^L, d v_r into the second half of dvm0
  hipLaunchKernelGGL(k_pnt_norm_bwd, GRID1(nW), 0, s, BN, dim, Wh, dg0, g0, K0, W, vm0 + Wh, W, dvm0 + Wh, W, g->ds, 1);
  LB_TRY(pnt_dw(t, BNd, W, vL, W, dvm0, G + g->r0_vm, W, nullptr));
  LB_TRY(pnt_mm(t, BNd, W, W, dvm0, W, Wt + g->r0_vm, W, 1, g->dv, W));
  LB_TRY(pnt_flush(t));
  // ---- layers in reverse; each layer's activations are recomputed from its taps first
  bool dphi_live = false;
  for (int k = L - 1; k >= 0; --k) {
    const lb_pnt_layer& l = g->layers[g->desc.shared_interactions ? 0 : k];
    const int fcol = g->desc.shared_filters ? 0 : k * 3 * W;
    const float* sk = g->tap_s + (size_t)k * nW;
    const float* vk = g->tap_v + (size_t)k * BNd * W;
    // recompute: interaction MLP, message sums (pre-clip values kept), vector mixing, norms, mixing MLP
    LB_TRY(pnt_mm(t, BN, W, W, sk, W, Wt + l.wi0, W, 0, g->zi0, W, 0, Wt + l.bi0));
    hipLaunchKernelGGL(k_pnt_silu, GRID1(nW), 0, s, nW, g->zi0, g->hi);
    for (int c = 0; c < 3; ++c)
      LB_TRY(pnt_mm(t, BN, W, W, g->hi, W, Wt + l.wi1 + c * W, 3 * W, 0, g->x3 + c * W, 3 * W, 0, Wt + l.bi1 + c * W));
    pnt_msg_args ma{};
    ma.BN = BN; ma.E = (int)E; ma.dim = dim; ma.n_rbf = R; ma.ldf = ldf; ma.fcol = fcol;
    ma.row_ptr = e->row_ptr; ma.rev = st.rev; ma.orph = st.orph; ma.senders = e->senders; ma.receivers = e->receivers;
    ma.geo = st.geo; ma.nrm = st.nrm; ma.w_rbf = Wt + g->widths; ma.o_rbf = Wt + g->offsets; ma.wf = Wt + g->w_f; ma.bf = Wt + g->b_f;
    ma.x3 = g->x3; ma.s = sk; ma.v = vk;
    ma.pre_s = g->pre_s; ma.pre_v = g->pre_v; ma.s_m = g->ts; ma.lds = 2 * W; ma.v_m = g->v_m;
    const unsigned nb_t = (unsigned)((BN + PNT_TN - 1) / PNT_TN);
    hipLaunchKernelGGL(k_pnt_msg_fwd, dim3(nb_t), dim3(128), 0, s, ma);
    for (int c = 0; c < 2; ++c) LB_TRY(pnt_mm(t, BNd, W, W, g->v_m, W, Wt + l.wvm + c * W, 2 * W, 0, g->vm + c * W, 2 * W));
    hipLaunchKernelGGL(k_pnt_vnorm, GRID1(nW), 0, s, BN, dim, g->vm, 2 * W, W, W, H, g->ts, 2 * W, W);
    LB_TRY(pnt_mm(t, BN, 2 * W, W, g->ts, 2 * W, Wt + l.wm0, W, 0, g->zm0, W, 0, Wt + l.bm0));
    hipLaunchKernelGGL(k_pnt_silu, GRID1(nW), 0, s, nW, g->zm0, g->hm);
    for (int c = 0; c < 3; ++c)
      LB_TRY(pnt_mm(t, BN, W, W, g->hm, W, Wt + l.wm1 + c * W, 3 * W, 0, g->m3 + c * W, 3 * W, 0, Wt + l.bm1 + c * W));
    // update block backward (ds, dv = d s^{k+1}, d v^{k+1}; the residual passes them through)
    hipLaunchKernelGGL(k_pnt_upd_bwd, GRID1(nW), 0, s, BN, dim, g->m3, g->vm, g->ds, g->dv, g->dm3, g->dvm);
    for (int c = 0; c < 3; ++c) {
      LB_TRY(pnt_dw(t, BN, W, g->hm, W, g->dm3 + c * nW, G + l.wm1 + c * W, 3 * W, G + l.bm1 + c * W));
      LB_TRY(pnt_mm(t, BN, W, W, g->dm3 + c * nW, W, Wt + l.wm1 + c * W, 3 * W, 1, g->dhm, W, c > 0));
    }
    hipLaunchKernelGGL(k_pnt_dsilu, GRID1(nW), 0, s, nW, g->dhm, g->zm0, g->dhm);   // dhm = d zm0
    LB_TRY(pnt_dw(t, BN, 2 * W, g->ts, 2 * W, g->dhm, G + l.wm0, W, G + l.bm0));
    for (int c = 0; c < 2; ++c) LB_TRY(pnt_mm(t, BN, W, W, g->dhm, W, Wt + l.wm0 + (size_t)c * W * W, W, 1, g->dts + c * W, 2 * W));
    hipLaunchKernelGGL(k_pnt_norm_bwd, GRID1(nW), 0, s, BN, dim, W, g->dts, g->ts, 2 * W, W, g->vm + W, 2 * W, g->dvm + BNd * W, W,
                       g->ds, 0);
    for (int c = 0; c < 2; ++c) {
      LB_TRY(pnt_dw(t, BNd, W, g->v_m, W, g->dvm + c * BNd * W, G + l.wvm + c * W, 2 * W, nullptr));
      LB_TRY(pnt_mm(t, BNd, W, W, g->dvm + c * BNd * W, W, Wt + l.wvm + c * W, 2 * W, 1, g->dv, W, 1));
    }
    // message block backward (ds, dv = d s_m, d v_m)
    ma.ds = g->ds; ma.dv = g->dv; ma.dx3 = g->dx3; ma.dv_out = g->dv2; ma.dpre = g->dpre;
    hipLaunchKernelGGL(k_pnt_msg_bwd, dim3(nb_t), dim3(128), 0, s, ma);
    std::swap(g->dv, g->dv2);
    for (int c = 0; c < 3 && E; ++c) {
      const float* dp = g->dpre + (size_t)c * E * W;
      LB_TRY(pnt_dw(t, E, R, g->phi, g->ldp, dp, G + g->w_f + fcol + c * W, ldf, G + g->b_f + fcol + c * W));
      if (g->rbf_trainable) {
        LB_TRY(pnt_mm(t, E, W, R, dp, W, Wt + g->w_f + fcol + c * W, ldf, 1, g->dphi, g->ldp, dphi_live));
        dphi_live = true;
      }
    }
    // interaction MLP
    for (int c = 0; c < 3; ++c) {
      LB_TRY(pnt_dw(t, BN, W, g->hi, W, g->dx3 + c * nW, G + l.wi1 + c * W, 3 * W, G + l.bi1 + c * W));
      LB_TRY(pnt_mm(t, BN, W, W, g->dx3 + c * nW, W, Wt + l.wi1 + c * W, 3 * W, 1, g->dhm, W, c > 0));
    }
    hipLaunchKernelGGL(k_pnt_dsilu, GRID1(nW), 0, s, nW, g->dhm, g->zi0, g->dhm);   // dhm = d zi0
    LB_TRY(pnt_dw(t, BN, W, sk, W, g->dhm, G + l.wi0, W, G + l.bi0));
    LB_TRY(pnt_mm(t, BN, W, W, g->dhm, W, Wt + l.wi0, W, 1, g->ds, W, 1));
    LB_TRY(pnt_flush(t));   // (layers may share their parameters: this layer's sums land before the next one's are queued)
  }
  // ---- embeddings and the radial basis
  LB_TRY(pnt_dw(t, BN, g->n_scal, g->xs, PNT_XS, g->ds, G + g->w_se, W, G + g->b_se));
  LB_TRY(pnt_dw(t, BNd, g->n_vec, g->xv, PNT_XV, g->dv, G + g->w_ve, W, nullptr));
  if (g->rbf_trainable && dphi_live) {
    hipLaunchKernelGGL(k_pnt_rbf_bwd, GRID1(E * g->ldp), 0, s, E, R, g->ldp, st.nrm, Wt + g->widths, Wt + g->offsets, g->phi, g->dphi);
    LB_TRY(colsum_add(t, g->dphi, E, R, g->ldp, G + g->widths));
    LB_TRY(colsum_add(t, g->phi, E, R, g->ldp, G + g->offsets));
  }
  return pnt_flush(t);
}
