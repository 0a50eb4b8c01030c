// lb_train_egnn.h - the EGNN training step on the device; IMPLEMENTATION INCLUDE of lb_train.hip (one translation unit: it
// uses that file's fp32-MFMA products, ordered reductions, loss bookkeeping and AdamW), as lb_train_segnn.h is.
//
// Reference: EGNN.__call__ / EGNNLayer / _postprocess of lagrangebench/models/egnn.py:119-206,361-400 under value_and_grad
// of _mse (train/trainer.py:35-89); gradients checked against float64 torch autograd of tests/_egnn_oracle.py.
//
// Design.  The forward IS the inference forward: the k_eg_* kernels of lb_egnn.hip run on the handle's weight blob (a
// weightless lb_egnn "view" of it), with the taps on, so the returned prediction is EGNN.apply's bit for bit.  The taps keep
// what the backward needs - h^l and x^l of every layer - and each layer's edge and node activations are recomputed in the
// backward, right before that layer's backward runs (one layer's activations live at a time).  Device blobs are 128 wide
// (hidden < 128 is zero-padded, as GNS training pads its latents; the caller's blob goes through t->cmap): a padded unit is
// silu(0) = 0 in every layer, its weights get zero gradients and stay zero under AdamW, and the forward kernels add +0.0
// terms only, so the padded model's positions carry the same bits as the compact one's.
// Products.  Every dense contraction - recomputed Linears (X W, nodes and edges), dX = dY W^T, dW = X^T dY - is a 128-wide
// tall-skinny product on the exact-fp32 kernels of the training core (k_lin32f, k_dw_part + the ordered k_part_reduce; the
// handle has f16x2 off: the reference trains EGNN in fp32).  The first edge Linear is split by rows as in the forward:
// [h_s | h_r] W0 = P_s[s] + P_r[r] with P = h W0 per NODE; its backward sums dz0 per node first (the sender sum through the
// transposed edge rev[] and then the orphans - edges without a transpose, lb_internal.h: lbk_edge_rev -, the receiver sum
// over the CSR row) and takes node-sized products.  What is left is elementwise
// (silu and its derivative, gathers, the 128-long dots of the two scalar heads with a fixed-order lane reduction) and the
// per-node sums of the position gradients through rev[] and the orphans - every sum in a fixed order, no float atomics: two calls give the
// same gradient bits.
// Limits: normalize = 1 is refused (coord_diff / (sqrt(radial) + 1e-8) has a 0 * inf derivative on the self-edges every radius
// graph here holds: the reference's own gradient is NaN for num_mp_steps >= 2); num_mp_steps <= 40 (the step's reductions
// share one descriptor table of LB_RED_MAX entries).
#pragma once

#define EGT_W 128         // device width of every hidden layer
#define EGT_XIN 32        // row stride of the embedding input (n_vels + 9 <= 18 columns)
#define EGT_MAX_LAYERS 40

struct lb_egt_layer {   // float offsets into the device blobs (lb_egnn_create's layout with hidden 128)
  int64_t w0, b0, w1, b1, wn0, bn0, wn1, bn1, wx0, bx0, wx1, wv0, bv0, wv1;
};

struct lb_egt {
  lb_egnn_desc desc;       // the model's (hidden = its real width)
  lb_egnn* view = nullptr;  // the inference forward on t->w (hidden 128)
  int node_in = 0, n_attr = 0;
  int64_t w_emb = 0, b_emb = 0;
  std::vector<lb_egt_layer> layers;
  // taps: h^l (L+1 x BN x 128), x^l (L+1 x BN x dim)
  float *tap_h = nullptr, *tap_x = nullptr;
  // node scratch
  float *xin = nullptr, *attr2 = nullptr, *ps = nullptr, *pr = nullptr, *xn = nullptr, *zn0 = nullptr, *u = nullptr,
        *zv0 = nullptr, *vv = nullptr, *dpsi = nullptr, *dh = nullptr, *dx = nullptr, *dzn = nullptr, *du = nullptr,
        *dagg = nullptr;
  // edge scratch
  float *cdr = nullptr, *ea2 = nullptr, *z0 = nullptr, *a = nullptr, *z1 = nullptr, *m = nullptr, *zx0 = nullptr, *q = nullptr,
        *phi = nullptr, *dphi = nullptr, *dcd = nullptr, *de1 = nullptr, *de2 = nullptr;
  lb_egnn_state st{};      // what the step's forward part hands to its loss and backward part
};

// ---------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ float egt_sig(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float egt_silu(float x) { return x / (1.f + expf(-x)); }  // = eg_silu of lb_egnn.hip
__device__ __forceinline__ float egt_dsilu(float x) {
  const float s = egt_sig(x);
  return s + x * s * (1.f - s);
}
// jax_md.space.periodic displacement in fp32 (= eg_disp of lb_egnn.hip)
__device__ __forceinline__ float egt_disp(float a, float b, float L, int periodic) {
  const float d = a - b;
  if (!periodic) return d;
  float r = fmodf(d + 0.5f * L, L);
  if (r != 0.f && r < 0.f) r = r + L;
  return r - 0.5f * L;
}
// fixed-order sum over the 32 lanes of a half wave (lanes 32 h .. 32 h + 31): every lane gets the same value
__device__ __forceinline__ float egt_sum32(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct lb_egt_geo {
  int dim, periodic;
  float box[3];
};

// the embedding's input rows [|v_1| .. |v_K| | one-hot(type) | 0] (k_eg_prologue's values) and [|force|, 0]
__global__ void k_egt_xin(int64_t BN, int dim, int n_vels, int homogeneous, const float* __restrict__ xnode,
                          const int32_t* __restrict__ ptype, const float* __restrict__ nattr, int n_attr,
                          float* __restrict__ xin, float* __restrict__ attr2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN) return;
  const float* x = xnode + i * 64;
  float* o = xin + i * EGT_XIN;
  int c = 0;
  for (int k = 0; k < n_vels; ++k) {
    const float v0 = x[k * dim], v1 = x[k * dim + 1], v2 = dim == 3 ? x[k * dim + 2] : 0.f;
    float s = v0 * v0 + v1 * v1;
    if (dim == 3) s = s + v2 * v2;
    o[c++] = sqrtf(s);
  }
  if (!homogeneous) {
    const int pt = ptype[i];
    for (int j = 0; j < 9; ++j) o[c++] = j == pt ? 1.f : 0.f;
  }
  for (; c < EGT_XIN; ++c) o[c] = 0.f;
  attr2[2 * i] = n_attr ? nattr[i] : 0.f;
  attr2[2 * i + 1] = 0.f;
}

// recomputed first edge Linear of a layer: coord_diff, radial; z0 = P_s[s] + P_r[r] + radial w_rad + rel_dist w_ea + b0,
// a = silu(z0).  32 lanes per edge, four columns each.  cdr[e] = (coord_diff, radial), ea2[e] = (radial, rel_dist).
__global__ void k_egt_edge_pre(int64_t E, lb_egt_geo g, const float* __restrict__ x, const int32_t* __restrict__ snd,
                               const int32_t* __restrict__ rcv, const float* __restrict__ efeat, const float* __restrict__ ps,
                               const float* __restrict__ pr, const float* __restrict__ w0, const float* __restrict__ b0,
                               float* __restrict__ z0, float* __restrict__ a, f32x4* __restrict__ cdr, float* __restrict__ ea2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * 32) return;
  const int64_t e = i >> 5;
  const int qd = (int)(i & 31);
  const int s = snd[e], r = rcv[e], dim = g.dim;
  const float c0 = egt_disp(x[(int64_t)s * dim], x[(int64_t)r * dim], g.box[0], g.periodic);
  const float c1 = egt_disp(x[(int64_t)s * dim + 1], x[(int64_t)r * dim + 1], g.box[1], g.periodic);
  const float c2 = dim == 3 ? egt_disp(x[(int64_t)s * dim + 2], x[(int64_t)r * dim + 2], g.box[2], g.periodic) : 0.f;
  float rad = c0 * c0 + c1 * c1;
  if (dim == 3) rad = rad + c2 * c2;
  const float ea = efeat[e * 8 + dim];
  if (qd == 0) {
    cdr[e] = f32x4{c0, c1, c2, rad};
    ea2[2 * e] = rad;
    ea2[2 * e + 1] = ea;
  }
  const f32x4 vs = reinterpret_cast<const f32x4*>(ps)[(int64_t)s * 32 + qd];
  const f32x4 vr = reinterpret_cast<const f32x4*>(pr)[(int64_t)r * 32 + qd];
  const f32x4 wr = reinterpret_cast<const f32x4*>(w0 + 2 * EGT_W * EGT_W)[qd];
  const f32x4 we = reinterpret_cast<const f32x4*>(w0 + (2 * EGT_W + 1) * EGT_W)[qd];
  const f32x4 bb = reinterpret_cast<const f32x4*>(b0)[qd];
  f32x4 z, av;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    z[j] = vs[j] + vr[j] + rad * wr[j] + ea * we[j] + bb[j];
    av[j] = egt_silu(z[j]);
  }
  reinterpret_cast<f32x4*>(z0)[i] = z;
  reinterpret_cast<f32x4*>(a)[i] = av;
}

// y = silu(z) (n4 float quads)
__global__ void k_egt_silu(int64_t n4, const float* __restrict__ z, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const f32x4 v = reinterpret_cast<const f32x4*>(z)[i];
  reinterpret_cast<f32x4*>(y)[i] = f32x4{egt_silu(v[0]), egt_silu(v[1]), egt_silu(v[2]), egt_silu(v[3])};
}
// dz = dy * silu'(z) (in place allowed)
__global__ void k_egt_dsilu(int64_t n4, const float* dy, const float* __restrict__ z, float* dz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const f32x4 v = reinterpret_cast<const f32x4*>(z)[i];
  const f32x4 d = reinterpret_cast<const f32x4*>(dy)[i];
  reinterpret_cast<f32x4*>(dz)[i] =
      f32x4{d[0] * egt_dsilu(v[0]), d[1] * egt_dsilu(v[1]), d[2] * egt_dsilu(v[2]), d[3] * egt_dsilu(v[3])};
}

// position net head: q = silu(zx0), phi = q . wx1 [tanh] (32 lanes per edge, fixed-order lane sum)
__global__ void k_egt_phi(int64_t E, const float* __restrict__ zx0, const float* __restrict__ wx1, int tanh_pos,
                          float* __restrict__ q, float* __restrict__ phi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < E * 32;
  const int qd = (int)(i & 31);
  float s = 0.f;
  if (ok) {
    const f32x4 z = reinterpret_cast<const f32x4*>(zx0)[i];
    const f32x4 w = reinterpret_cast<const f32x4*>(wx1)[qd];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = egt_silu(z[j]);
    reinterpret_cast<f32x4*>(q)[i] = v;
    s = ((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3];
  }
  s = egt_sum32(s);   // (E * 32 is a multiple of 32: a half wave is all in or all out)
  if (ok && qd == 0) phi[i >> 5] = tanh_pos ? tanhf(s) : s;
}

// node MLP input's |force| row and activation: zn0 += |force| w_attr; u = silu(zn0)
__global__ void k_egt_node_pre(int64_t BN, float* __restrict__ zn0, const float* __restrict__ attr2,
                               const float* __restrict__ w_attr, float* __restrict__ u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN * 32) return;
  const int qd = (int)(i & 31);
  f32x4 z = reinterpret_cast<const f32x4*>(zn0)[i];
  if (w_attr) {
    const float at = attr2[2 * (i >> 5)];
    const f32x4 w = reinterpret_cast<const f32x4*>(w_attr)[qd];
    z = z + at * w;
    reinterpret_cast<f32x4*>(zn0)[i] = z;
  }
  reinterpret_cast<f32x4*>(u)[i] = f32x4{egt_silu(z[0]), egt_silu(z[1]), egt_silu(z[2]), egt_silu(z[3])};
}

// velocity net backward: x' = shift(y, psi vel): dpsi = dx' . vel; vv = silu(zv0); dzv0 = dpsi wv1 silu'(zv0)
__global__ void k_egt_vel_bwd(int64_t BN, int dim, const float* __restrict__ zv0, const float* __restrict__ dx,
                              const float* __restrict__ vel, const float* __restrict__ wv1, float* __restrict__ vv,
                              float* __restrict__ dzv0, float* __restrict__ dpsi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN * 32) return;
  const int64_t n = i >> 5;
  const int qd = (int)(i & 31);
  float p = dx[n * 4] * vel[n * 4] + dx[n * 4 + 1] * vel[n * 4 + 1];
  if (dim == 3) p = p + dx[n * 4 + 2] * vel[n * 4 + 2];
  const f32x4 z = reinterpret_cast<const f32x4*>(zv0)[i];
  const f32x4 w = reinterpret_cast<const f32x4*>(wv1)[qd];
  f32x4 v, d;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = egt_silu(z[j]);
    d[j] = p * w[j] * egt_dsilu(z[j]);
  }
  reinterpret_cast<f32x4*>(vv)[i] = v;
  reinterpret_cast<f32x4*>(dzv0)[i] = d;
  if (qd == 0) dpsi[n] = p;
}

// position update backward: y = shift(x, sum_{sender = i} coord_diff phi): d trans[e] = dx'[s(e)];
// d phi = d trans . coord_diff (tanh: * (1 - phi^2)); d coord_diff = d trans phi; dzx0 = d phi wx1 silu'(zx0)
__global__ void k_egt_pos_bwd(int64_t E, int dim, int tanh_pos, const int32_t* __restrict__ snd, const float* __restrict__ dx,
                              const f32x4* __restrict__ cdr, const float* __restrict__ phi, const float* __restrict__ zx0,
                              const float* __restrict__ wx1, float* __restrict__ dzx0, float* __restrict__ dphi,
                              f32x4* __restrict__ dcd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * 32) return;
  const int64_t e = i >> 5;
  const int qd = (int)(i & 31);
  const int s = snd[e];
  const f32x4 c = cdr[e];
  const float t0 = dx[(int64_t)s * 4], t1 = dx[(int64_t)s * 4 + 1], t2 = dim == 3 ? dx[(int64_t)s * 4 + 2] : 0.f;
  float dp = t0 * c[0] + t1 * c[1];
  if (dim == 3) dp = dp + t2 * c[2];
  const float ph = phi[e];
  if (tanh_pos) dp = dp * (1.f - ph * ph);
  const f32x4 z = reinterpret_cast<const f32x4*>(zx0)[i];
  const f32x4 w = reinterpret_cast<const f32x4*>(wx1)[qd];
  f32x4 d;
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = dp * w[j] * egt_dsilu(z[j]);
  reinterpret_cast<f32x4*>(dzx0)[i] = d;
  if (qd == 0) {
    dphi[e] = dp;
    dcd[e] = f32x4{t0 * ph, t1 * ph, t2 * ph, 0.f};
  }
}

// messages: d m[e] += d agg[r(e)] (segment_sum over receivers), dz1 = d m silu'(z1)
__global__ void k_egt_msg_bwd(int64_t E, const int32_t* __restrict__ rcv, const float* __restrict__ dagg,
                              const float* __restrict__ dm, const float* __restrict__ z1, float* __restrict__ dz1) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * 32) return;
  const int64_t e = i >> 5;
  const int qd = (int)(i & 31);
  const f32x4 g = reinterpret_cast<const f32x4*>(dagg)[(int64_t)rcv[e] * 32 + qd];
  const f32x4 d = reinterpret_cast<const f32x4*>(dm)[i] + g;
  const f32x4 z = reinterpret_cast<const f32x4*>(z1)[i];
  reinterpret_cast<f32x4*>(dz1)[i] =
      f32x4{d[0] * egt_dsilu(z[0]), d[1] * egt_dsilu(z[1]), d[2] * egt_dsilu(z[2]), d[3] * egt_dsilu(z[3])};
}

// radial: d radial = dz0 . w_rad (fixed-order lane sum); d coord_diff += 2 coord_diff d radial
__global__ void k_egt_drad(int64_t E, const float* __restrict__ dz0, const float* __restrict__ w_rad, const f32x4* __restrict__ cdr,
                           f32x4* __restrict__ dcd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < E * 32;
  const int qd = (int)(i & 31);
  float s = 0.f;
  if (ok) {
    const f32x4 d = reinterpret_cast<const f32x4*>(dz0)[i];
    const f32x4 w = reinterpret_cast<const f32x4*>(w_rad)[qd];
    s = ((d[0] * w[0] + d[1] * w[1]) + d[2] * w[2]) + d[3] * w[3];
  }
  s = egt_sum32(s);
  if (ok && qd == 0) {
    const int64_t e = i >> 5;
    const f32x4 c = cdr[e];
    const float k = 2.f * s;
    dcd[e] = dcd[e] + f32x4{k * c[0], k * c[1], k * c[2], 0.f};
  }
}

// transpose of the first edge Linear's gathers: dPs[i] = sum of dz0 over the edges i SENDS (rev[] of row i, row order, then
// i's orphans in slot order: the forward's sender sum), dPr[i] = sum over the edges i RECEIVES (its CSR row)
__global__ void k_egt_dP(int64_t BN, int64_t E, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ rev,
                         const int32_t* __restrict__ orph, const int32_t* __restrict__ senders,
                         const float* __restrict__ dz0, float* __restrict__ dps, float* __restrict__ dpr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BN * 32) return;
  const int64_t n = i >> 5;
  const int qd = (int)(i & 31);
  int k0 = row_ptr[n], k1 = row_ptr[n + 1];
  k0 = k0 < E ? k0 : (int)E;
  k1 = k1 < E ? k1 : (int)E;
  f32x4 as = {0.f, 0.f, 0.f, 0.f}, ar = {0.f, 0.f, 0.f, 0.f};
  for (int k = k0; k < k1; ++k) {
    const int e = rev[k];
    if (e >= 0) as = as + reinterpret_cast<const f32x4*>(dz0)[(int64_t)e * 32 + qd];
    ar = ar + reinterpret_cast<const f32x4*>(dz0)[(int64_t)k * 32 + qd];
  }
  lb_for_orphans(orph, senders, n, [&](int e) { as = as + reinterpret_cast<const f32x4*>(dz0)[(int64_t)e * 32 + qd]; });
  reinterpret_cast<f32x4*>(dps)[i] = as;
  reinterpret_cast<f32x4*>(dpr)[i] = ar;
}

// positions: coord_diff = disp(x_s, x_r) -> dx[i] += sum over the edges i sends of d coord_diff - sum over those it receives
__global__ void k_egt_dx(int64_t BN, int64_t E, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ rev,
                         const int32_t* __restrict__ orph, const int32_t* __restrict__ senders,
                         const f32x4* __restrict__ dcd, float* __restrict__ dx) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= BN) return;
  int k0 = row_ptr[n], k1 = row_ptr[n + 1];
  k0 = k0 < E ? k0 : (int)E;
  k1 = k1 < E ? k1 : (int)E;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, r = {0.f, 0.f, 0.f, 0.f};
  for (int k = k0; k < k1; ++k) {
    const int e = rev[k];
    if (e >= 0) s = s + dcd[e];
    r = r + dcd[k];
  }
  lb_for_orphans(orph, senders, n, [&](int e) { s = s + dcd[e]; });
  f32x4 d = reinterpret_cast<f32x4*>(dx)[n];
  d = d + (s - r);
  reinterpret_cast<f32x4*>(dx)[n] = d;
}

// _mse over EGNN's three outputs (egnn.py:361-369, trainer.py:35-60): pos = x^L, vel = disp(x^L, x^0), acc = vel - the
// NORMALISED last velocity feature, each in fp32; residuals against the fp64 targets in fp64, masked, / n_nonkinematic(b);
// loss averaged over the batch (partials per wave), d loss / d x^L (summed over the batch) into dx [BN][4]
struct lb_egt_loss_args {
  int64_t BN;
  int N, dim, periodic, K;
  float box[3];
  double wp, wv, wa, inv_b;
  const float *xl, *x0, *xnode;
  const double *tp, *tv, *ta;
  const int32_t *ptype, *cnt;
  float* dx;
  double* loss_part;
};
__global__ void k_egt_loss(lb_egt_loss_args a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double l = 0.0;
  if (i < a.BN) {
    const int pt = a.ptype[i];
    const bool kin = pt == 1 || pt == 2 || pt == -1;   // utils.py:28-35
    const int c = a.cnt[i / a.N];
    const double w = (kin || c <= 0) ? 0.0 : 1.0 / (double)c;
    for (int d = 0; d < 4; ++d) {
      double g = 0.0;
      if (d < a.dim) {
        const float xp = a.xl[i * a.dim + d];
        const float v = egt_disp(xp, a.x0[i * a.dim + d], a.box[d], a.periodic);
        const float ac = v - a.xnode[i * 64 + (a.K - 1) * a.dim + d];
        double gv = 0.0;
        if (a.wa != 0.0) {
          const double r = (double)ac - a.ta[i * a.dim + d];
          l += w * a.wa * r * r;
          gv += 2.0 * a.wa * w * r;
        }
        if (a.wv != 0.0) {
          const double r = (double)v - a.tv[i * a.dim + d];
          l += w * a.wv * r * r;
          gv += 2.0 * a.wv * w * r;
        }
        g = gv;
        if (a.wp != 0.0) {
          const double r = (double)xp - a.tp[i * a.dim + d];
          l += w * a.wp * r * r;
          g += 2.0 * a.wp * w * r;
        }
      }
      a.dx[i * 4 + d] = (float)g;
    }
  }
  for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
  if ((threadIdx.x & 63) == 0) a.loss_part[i >> 6] = l * a.inv_b;
}

// ------------------------------------------------------------------------------------------------------------- host
static void egt_free(lb_gns_train* t) {
  lb_egt* g = t->eg;
  if (!g) return;
  if (g->view) lb_egnn_destroy(g->view);
  delete g;  // (its buffers are the handle arena's)
  t->eg = nullptr;
}

static int egt_ensure(lb_gns_train* t, int64_t BN, int64_t E) {
  return train_ensure(t, BN, E, [t](int64_t cn, int64_t ce, int64_t) -> int {
    lb_egt* g = t->eg;
    const int L = g->desc.num_mp_steps, dim = t->eng->g.dim;
    const size_t W = EGT_W;
    LB_TRY(t->mem.get(&g->tap_h, (size_t)(L + 1) * cn * W));
    LB_TRY(t->mem.get(&g->tap_x, (size_t)(L + 1) * cn * dim));
    LB_TRY(t->mem.get(&g->xin, (size_t)cn * EGT_XIN));
    LB_TRY(t->mem.get(&g->attr2, (size_t)cn * 2));
    LB_TRY(t->mem.get(&g->xn, (size_t)cn * 2 * W));
    LB_TRY(t->mem.get(&g->dpsi, (size_t)cn));
    LB_TRY(t->mem.get(&g->dx, (size_t)cn * 4));
    for (float** p : {&g->ps, &g->pr, &g->zn0, &g->u, &g->zv0, &g->vv, &g->dh, &g->dzn, &g->du, &g->dagg})
      LB_TRY(t->mem.get(p, (size_t)cn * W));
    LB_TRY(t->mem.get(&g->cdr, (size_t)ce * 4));
    LB_TRY(t->mem.get(&g->dcd, (size_t)ce * 4));
    LB_TRY(t->mem.get(&g->ea2, (size_t)ce * 2));
    LB_TRY(t->mem.get(&g->phi, (size_t)ce));
    LB_TRY(t->mem.get(&g->dphi, (size_t)ce));
    for (float** p : {&g->z0, &g->a, &g->z1, &g->m, &g->zx0, &g->q, &g->de1, &g->de2}) LB_TRY(t->mem.get(p, (size_t)ce * W));
    // partial-sum slots of the step's reductions: the producers of egnn_backward, per layer and for the embedding
    t->red_cap = (int64_t)L * (4 * dw_acc_floats(cn, W) + dw_acc_floats(cn, 2 * W) + dw_acc_floats(cn, 1) +
                               2 * dw_acc_floats(ce, W) + dw_acc_floats(ce, 2) + dw_narrow_floats(cn, W, 1) +
                               dw_narrow_floats(ce, W, 1)) + dw_acc_floats(cn, EGT_XIN) + 4096;
    return LB_OK;
  });
}

// dW += X^T dY (+ db), refusals reported as LB_ERR_STATE (red_slot / dw_acc said why); nothing to add for zero rows
static int egt_dw(lb_gns_train* t, int64_t rows, int K, const float* X, int ldx, const float* dY, float* dW, float* db) {
  if (rows <= 0) return LB_OK;
  return dw_acc(t, rows, K, X, ldx, dY, dW, db) ? LB_OK : LB_ERR_STATE;
}

static int egnn_forward(lb_gns_train* t, const float** pred);
static int egnn_backward(lb_gns_train* t, double* dpos_out_dev);
// the backward starts from d loss / d x^L in g->dx, rows of 4 floats: k_egt_loss writes it, lb_train_backward spreads into it
static int egnn_dpred_load(lb_gns_train* t) {
  const int64_t BN = t->fwd_BN;
  hipLaunchKernelGGL(k_dpred_spread, GRID1(BN), 0, t->eng->stream, t->dsave, BN, t->eng->g.dim, 4, t->eg->dx);
  return LB_OK;
}
static const lb_train_model egnn_model = {"EGNN", "lb_egnn_train_loss_grad", false, false, false, egt_free, egt_ensure,
                                          egnn_forward, egnn_backward, egnn_dpred_load};

extern "C" int lb_egnn_train_create(lb_engine* e, const lb_egnn_desc* d, const float* w, int64_t n_floats, lb_gns_train** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->normalize)
    return lb_fail(LB_ERR_ARG, "egnn training: normalize = 1 is refused (coord_diff / (sqrt(radial) + 1e-8) has a 0 * inf "
                   "derivative on the radius graph's self-edges: the reference's gradient is NaN)");
  if (d->hidden < 16 || d->hidden > 128 || d->hidden % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "EGNN hidden size %d: a multiple of 16 up to 128 is built", d->hidden);
  if (d->num_mp_steps < 1 || d->num_mp_steps > EGT_MAX_LAYERS)
    return lb_fail(LB_ERR_UNSUPPORTED, "egnn training: num_mp_steps %d (1 .. %d)", d->num_mp_steps, EGT_MAX_LAYERS);
  if (d->n_vels < 1 || d->n_vels > 9) return lb_fail(LB_ERR_ARG, "bad n_vels %d (1 .. 9)", d->n_vels);
  if (d->n_vels != e->g.isl - 1) return lb_fail(LB_ERR_ARG, "n_vels %d != input_seq_length-1", d->n_vels);
  const int L = d->num_mp_steps, H = d->hidden, W = EGT_W;
  lb_gns_train* t = new lb_gns_train();
  lb_egt* g = new lb_egt();
  t->model = &egnn_model;
  t->eg = g;
  t->eng = e;
  t->f16x2 = false;   // exact fp32 products throughout (the reference's fp32 policy)
  g->desc = *d;
  g->node_in = d->n_vels + (d->homogeneous ? 0 : 9);
  g->n_attr = e->g.force_kind != LB_FORCE_NONE ? 1 : 0;
  // device layout: lb_egnn_create's with hidden 128; caller's (EGNN.flatten, hidden H) maps into it row by row
  int64_t o = 0, oc = 0;
  auto mat = [&](int rows_c, int cols_c, auto row_dev) {   // caller (rows_c x cols_c) -> rows row_dev(r) of a 128-wide block
    const int64_t base = o;
    if (H != W)
      for (int r = 0; r < rows_c; ++r)
        for (int c = 0; c < cols_c; ++c) t->cmap.push_back(base + (int64_t)row_dev(r) * (cols_c == 1 ? 1 : W) + c);
    oc += (int64_t)rows_c * cols_c;
    return base;
  };
  auto same = [](int r) { return r; };
  auto blocks = [H](int r) { return r < 2 * H ? (r / H) * W + r % H : 2 * W + (r - 2 * H); };
  g->w_emb = mat(g->node_in, H, same); o += (int64_t)g->node_in * W;
  g->b_emb = mat(1, H, same); o += W;
  for (int k = 0; k < L; ++k) {
    lb_egt_layer l{};
    l.w0 = mat(2 * H + 2, H, blocks); o += (int64_t)(2 * W + 2) * W;
    l.b0 = mat(1, H, same); o += W;
    l.w1 = mat(H, H, same); o += (int64_t)W * W;
    l.b1 = mat(1, H, same); o += W;
    l.wn0 = mat(2 * H + g->n_attr, H, blocks); o += (int64_t)(2 * W + g->n_attr) * W;
    l.bn0 = mat(1, H, same); o += W;
    l.wn1 = mat(H, H, same); o += (int64_t)W * W;
    l.bn1 = mat(1, H, same); o += W;
    l.wx0 = mat(H, H, same); o += (int64_t)W * W;
    l.bx0 = mat(1, H, same); o += W;
    l.wx1 = mat(H, 1, same); o += W;
    l.wv0 = mat(H, H, same); o += (int64_t)W * W;
    l.bv0 = mat(1, H, same); o += W;
    l.wv1 = mat(H, 1, same); o += W;
    g->layers.push_back(l);
  }
  t->n_floats = o;
  t->n_compact = oc;
  int rc = train_handle_init(t, "egnn weight blob", w, n_floats);
  if (!rc) {
    lb_egnn_desc vd = *d;
    vd.hidden = W;
    rc = lbk_egnn_view_create(e, &vd, t->w, &g->view);
  }
  return train_create_finish(t, rc, out);
}

// The inference view of the handle (lbk_egnn_view_create on t->w): lb_egnn_forward / lb_egnn_rollout on it run on the CURRENT
// weights.  Borrowed: it lives and dies with t.
extern "C" int lb_egnn_train_model(lb_gns_train* t, lb_egnn** out) {
  if (!t || !out) return lb_fail(LB_ERR_ARG, "null argument");
  if (t->model != &egnn_model) return lb_fail(LB_ERR_ARG, "not an EGNN training handle");
  *out = t->eg->view;
  return LB_OK;
}

// The step in three parts, split at d loss / d x^L (g->dx, rows of 4 floats).  Forward part: the inference kernels on the
// current weights, taps on (returns after checking every edge's transpose: nothing has been accumulated yet when it refuses)
// The prediction is the last tap, x^L
static int egnn_forward(lb_gns_train* t, const float** pred) {
  lb_engine* e = t->eng;
  lb_egt* g = t->eg;
  LB_TRY(lb_egnn_set_tap(g->view, g->tap_h, g->tap_x));
  g->st = lb_egnn_state{};
  LB_TRY(lbk_egnn_train_forward(e, g->view, &g->st));
  *pred = g->tap_x + (size_t)g->desc.num_mp_steps * t->fwd_BN * e->g.dim;
  return LB_OK;
}
// ---- loss and d loss / d x^L
static int egnn_loss_part(lb_gns_train* t, const double* tgt_pos, const double* tgt_vel, const double* tgt_acc, float w_pos,
                          float w_vel, float w_acc) {
  lb_engine* e = t->eng;
  lb_egt* g = t->eg;
  hipStream_t s = e->stream;
  const int64_t BN = t->fwd_BN;
  const int L = g->desc.num_mp_steps, dim = e->g.dim;
  const lb_egnn_state& st = g->st;
  const float* xl = g->tap_x + (size_t)L * BN * dim;
  LB_HIP(hipMemsetAsync(t->cnt_dev, 0, sizeof(int32_t) * e->g.B, s));
  LB_HIP(hipMemsetAsync(t->loss_dev, 0, sizeof(double), s));
  hipLaunchKernelGGL(k_count_nonkin, GRID1(BN), 0, s, e->ptype, BN, e->g.N, t->cnt_dev);
  lb_egt_loss_args la{};
  la.BN = BN; la.N = e->g.N; la.dim = dim; la.periodic = e->g.periodic; la.K = e->g.isl - 1;
  for (int d = 0; d < 3; ++d) la.box[d] = (float)e->g.box[d];
  la.wp = w_pos; la.wv = w_vel; la.wa = w_acc; la.inv_b = 1.0 / (double)e->g.B;
  la.xl = xl; la.x0 = g->tap_x; la.xnode = st.xnode;
  la.tp = tgt_pos; la.tv = tgt_vel; la.ta = tgt_acc;
  la.ptype = e->ptype; la.cnt = t->cnt_dev; la.dx = g->dx; la.loss_part = t->loss_part;
  hipLaunchKernelGGL(k_egt_loss, GRID1(BN), 0, s, la);
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(64), 0, s, t->loss_part, (int64_t)((BN + 255) / 256) * 4, t->loss_dev);
  return LB_OK;
}
static int egnn_backward(lb_gns_train* t, double*) {
  lb_engine* e = t->eng;
  lb_egt* g = t->eg;
  hipStream_t s = e->stream;
  const int64_t E = t->fwd_E, BN = t->fwd_BN;
  const int L = g->desc.num_mp_steps, dim = e->g.dim, W = EGT_W;
  const lb_egnn_state& st = g->st;
  hipLaunchKernelGGL(k_egt_xin, GRID1(BN), 0, s, BN, dim, g->desc.n_vels, g->desc.homogeneous, st.xnode, e->ptype, st.nattr,
                     g->n_attr, g->xin, g->attr2);
  LB_HIP(hipMemsetAsync(g->dh, 0, sizeof(float) * BN * W, s));   // h^L has no reader
  lb_egt_geo geo{};
  geo.dim = dim;
  geo.periodic = e->g.periodic;
  for (int d = 0; d < 3; ++d) geo.box[d] = (float)e->g.box[d];
  const int64_t nq = BN * 32, eq = E * 32;   // float quads of a node- / edge-sized 128-wide array
  float* G = t->g;
  const float* Wt = t->w;
  // ---- backward, layer by layer in reverse; each layer's activations are recomputed first
  for (int k = L - 1; k >= 0; --k) {
    const lb_egt_layer& l = g->layers[k];
    const float* h = g->tap_h + (size_t)k * BN * W;
    const float* h1 = g->tap_h + (size_t)(k + 1) * BN * W;
    const float* x = g->tap_x + (size_t)k * BN * dim;
    // recompute: P = h [W0_s | W0_r]; z0, a; z1, m; zx0, q, phi; [h | agg], zn0, u; zv0 (vv in k_egt_vel_bwd)
    LB_TRY(gemm_nn(t, BN, W, W, h, W, Wt + l.w0, g->ps, W));
    LB_TRY(gemm_nn(t, BN, W, W, h, W, Wt + l.w0 + (size_t)W * W, g->pr, W));
    if (E) {
      hipLaunchKernelGGL(k_egt_edge_pre, GRID1(eq), 0, s, E, geo, x, e->senders, e->receivers, e->efeat, g->ps, g->pr, Wt + l.w0,
                         Wt + l.b0, g->z0, g->a, reinterpret_cast<f32x4*>(g->cdr), g->ea2);
      LB_TRY(gemm_nn(t, E, W, W, g->a, W, Wt + l.w1, g->z1, W, 0.f, Wt + l.b1));
      hipLaunchKernelGGL(k_egt_silu, GRID1(eq), 0, s, eq, g->z1, g->m);
      LB_TRY(gemm_nn(t, E, W, W, g->m, W, Wt + l.wx0, g->zx0, W, 0.f, Wt + l.bx0));
      hipLaunchKernelGGL(k_egt_phi, GRID1(eq), 0, s, E, g->zx0, Wt + l.wx1, g->desc.tanh_pos, g->q, g->phi);
    }
    hipLaunchKernelGGL(k_seg_sum, GRID1(nq), 0, s, e->row_ptr, g->m, (float*)nullptr, BN, E, h, g->xn);
    LB_TRY(gemm_nn(t, BN, W, 2 * W, g->xn, 2 * W, Wt + l.wn0, g->zn0, W, 0.f, Wt + l.bn0));
    hipLaunchKernelGGL(k_egt_node_pre, GRID1(nq), 0, s, BN, g->zn0, g->attr2,
                       g->n_attr ? Wt + l.wn0 + (size_t)2 * W * W : (const float*)nullptr, g->u);
    LB_TRY(gemm_nn(t, BN, W, W, h1, W, Wt + l.wv0, g->zv0, W, 0.f, Wt + l.bv0));
    // velocity net (dx = d x^{k+1}; the shifts have derivative 1)
    hipLaunchKernelGGL(k_egt_vel_bwd, GRID1(nq), 0, s, BN, dim, g->zv0, g->dx, st.vel, Wt + l.wv1, g->vv, g->dzn, g->dpsi);
    LB_TRY(egt_dw(t, BN, W, h1, W, g->dzn, G + l.wv0, G + l.bv0));
    LB_TRY(dw_narrow(t, BN, 1, W, g->vv, W, g->dpsi, 1, G + l.wv1));
    LB_TRY(gemm_nt(t, BN, W, W, g->dzn, Wt + l.wv0, g->dh, W, 1.f));   // dh = d h^{k+1} in full
    // position net and the sender sum of coord_diff phi
    if (E) {
      hipLaunchKernelGGL(k_egt_pos_bwd, GRID1(eq), 0, s, E, dim, g->desc.tanh_pos, e->senders, g->dx,
                         reinterpret_cast<const f32x4*>(g->cdr), g->phi, g->zx0, Wt + l.wx1, g->de1, g->dphi,
                         reinterpret_cast<f32x4*>(g->dcd));
      LB_TRY(egt_dw(t, E, W, g->m, W, g->de1, G + l.wx0, G + l.bx0));
      LB_TRY(dw_narrow(t, E, 1, W, g->q, W, g->dphi, 1, G + l.wx1));
      LB_TRY(gemm_nt(t, E, W, W, g->de1, Wt + l.wx0, g->de2, W));   // de2 = d m (position net part)
    }
    // node MLP: h^{k+1} = [h^k +] (silu([h | agg | |force|] Wn0 + bn0) Wn1 + bn1)
    LB_TRY(egt_dw(t, BN, W, g->u, W, g->dh, G + l.wn1, G + l.bn1));
    LB_TRY(gemm_nt(t, BN, W, W, g->dh, Wt + l.wn1, g->du, W));
    hipLaunchKernelGGL(k_egt_dsilu, GRID1(nq), 0, s, nq, g->du, g->zn0, g->dzn);
    LB_TRY(egt_dw(t, BN, 2 * W, g->xn, 2 * W, g->dzn, G + l.wn0, G + l.bn0));
    if (g->n_attr) LB_TRY(egt_dw(t, BN, 1, g->attr2, 2, g->dzn, G + l.wn0 + (size_t)2 * W * W, nullptr));
    LB_TRY(gemm_nt(t, BN, W, W, g->dzn, Wt + l.wn0 + (size_t)W * W, g->dagg, W));
    // (dh has been read by the products above: stream order) d h^k = [dh +] dzn0 Wn0[h rows]^T
    LB_TRY(gemm_nt(t, BN, W, W, g->dzn, Wt + l.wn0, g->dh, W, g->desc.residual ? 1.f : 0.f));
    if (E) {
      // edge MLP: m = silu(silu(z0) W1 + b1)
      hipLaunchKernelGGL(k_egt_msg_bwd, GRID1(eq), 0, s, E, e->receivers, g->dagg, g->de2, g->z1, g->de1);   // de1 = dz1
      LB_TRY(egt_dw(t, E, W, g->a, W, g->de1, G + l.w1, G + l.b1));
      LB_TRY(gemm_nt(t, E, W, W, g->de1, Wt + l.w1, g->de2, W));
      hipLaunchKernelGGL(k_egt_dsilu, GRID1(eq), 0, s, eq, g->de2, g->z0, g->de2);   // de2 = dz0
      // first edge Linear: radial / rel_dist rows + bias (edge-sized), node blocks through the per-node sums of dz0
      LB_TRY(egt_dw(t, E, 2, g->ea2, 2, g->de2, G + l.w0 + (size_t)2 * W * W, G + l.b0));
      hipLaunchKernelGGL(k_egt_drad, GRID1(eq), 0, s, E, g->de2, Wt + l.w0 + (size_t)2 * W * W,
                         reinterpret_cast<const f32x4*>(g->cdr), reinterpret_cast<f32x4*>(g->dcd));
      hipLaunchKernelGGL(k_egt_dP, GRID1(nq), 0, s, BN, E, e->row_ptr, st.rev, st.orph, e->senders, g->de2, g->ps,
                         g->pr);   // ps / pr = dPs / dPr
      LB_TRY(egt_dw(t, BN, W, h, W, g->ps, G + l.w0, nullptr));
      LB_TRY(egt_dw(t, BN, W, h, W, g->pr, G + l.w0 + (size_t)W * W, nullptr));
      LB_TRY(gemm_nt(t, BN, W, W, g->ps, Wt + l.w0, g->dh, W, 1.f));
      LB_TRY(gemm_nt(t, BN, W, W, g->pr, Wt + l.w0 + (size_t)W * W, g->dh, W, 1.f));
      // positions: d x^k = d x^{k+1} + the coord_diff terms of both endpoints
      hipLaunchKernelGGL(k_egt_dx, GRID1(BN), 0, s, BN, E, e->row_ptr, st.rev, st.orph, e->senders,
                         reinterpret_cast<const f32x4*>(g->dcd), g->dx);
    }
  }
  // embedding: h^0 = xin W_emb + b_emb
  return egt_dw(t, BN, g->node_in, g->xin, EGT_XIN, g->dh, G + g->w_emb, G + g->b_emb);
}
// value_and_grad of _mse for EGNN on the engine's CURRENT window / neighbor list (include/lbhip.h): the frame's two halves
// around the three-target loss
extern "C" int lb_egnn_train_loss_grad(lb_gns_train* t, const double* tgt_pos, const double* tgt_vel, const double* tgt_acc,
                                       float w_pos, float w_vel, float w_acc, double* loss_out, float* pred_pos_out_dev) {
  if (t && !t->model) return blob_refuse("lb_egnn_train_loss_grad");
  if (!t || t->model != &egnn_model) return lb_fail(LB_ERR_ARG, "null argument / not an EGNN training handle");
  if ((w_pos != 0.f && !tgt_pos) || (w_vel != 0.f && !tgt_vel) || (w_acc != 0.f && !tgt_acc))
    return lb_fail(LB_ERR_ARG, "egnn training: a target with a non-zero loss weight is null");
  t->fwd_live = false;
  // The guard never fires here: the handle has f16x2 off, so no k_dw_part_h launch can raise bits 1 | 2, and the step does
  // not build a sender view (its sender sums go through rev[] and the orphans), so k_sender_transpose never raises bit 4.
  // The loop is then one attempt and its synchronisation the step's last.
  return train_loss_grad_guarded(t, loss_out, [&] {
    LB_TRY(train_forward_part(t, egnn_model.loss_entry, pred_pos_out_dev));
    LB_TRY(egnn_loss_part(t, tgt_pos, tgt_vel, tgt_acc, w_pos, w_vel, w_acc));
    return train_backward_part(t, nullptr);
  });
}
