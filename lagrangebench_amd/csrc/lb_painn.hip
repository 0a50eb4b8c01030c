// lb_painn.hip - PaiNN (polarizable interaction network) forward pass and rollout step on gfx950.
//
// Reference functions replaced (paths relative to the reference repo):
//   PaiNN._transform                        lagrangebench/models/painn.py:452-486
//   PaiNN.__call__ (norm, dir, filters,     lagrangebench/models/painn.py:488-510
//                   embedding, layers)
//   gaussian_rbf / cosine_cutoff            lagrangebench/models/painn.py:108-170
//   PaiNNLayer._message / _update           lagrangebench/models/painn.py:278-348
//   PaiNNReadout / GatedEquivariantBlock    lagrangebench/models/painn.py:34-105,173-215
//   case.integrate for an "acc" output      lagrangebench/case_setup/case.py (the GNS integrator, lb_state.hip)
//
// Arithmetic: fp32 throughout (runner.py:71-72); every sum runs in a fixed order (no float atomics), so two runs give
// identical bits.  Hidden width H: a multiple of 16, <= 128.  Shapes: s [BN][H], v [BN][dim][H] (row = node * dim + d).
//
// Kernels of one forward (L = num_mp_steps):
//   k_pn_embed    s0 = [vel_mag (| one-hot)] W_se + b, v0[d] = [v_0 .. v_{K-1} | force | bound_lo | bound_hi][d] W_ve
//   k_pn_edge     per edge: norm = sqrt(|rel_disp|^2 + eps), dir = rel_disp / (norm + eps), the filter scale (cosine
//                 cutoff or norm itself) and whether the edge is live (norm < cutoff; every edge without a cutoff)
//   lbk_edge_rev  (lb_egnn.hip) the transposed edge of every edge: the sum over senders runs through the receiver CSR,
//                 then over the few edges that have no transpose (orphans, lb_internal.h)
//   per layer:
//   k_pn_lin x2   x = silu(s Wi0 + bi0) Wi1 + bi1                              interaction block  (N x H -> N x 3H)
//   k_pn_msg      per node i, the row of i in order, e = rev[e'], then i's orphans: live edges only, W = (rbf(norm_e) Wf + bf) * scale_e
//                 (the layer's 3H filter columns, computed here), ds += W_s x_r, dv += W_v1 x_r dir_e + W_v2 x_r v_r
//                 with r = receivers[e]; s += clip(ds), v += clip(dv)  (v to the other buffer: the old v is gathered)
//   k_pn_lin      [v_l | v_r] = v W_vm                                          (N*dim x H -> N*dim x 2H)
//   k_pn_norm     [s | sqrt(sum_d v_r^2 + eps)]
//   k_pn_lin x2   [ds | dv | dsv] = silu([s | |v_r|] Wm0 + bm0) Wm1 + bm1       mixing block
//   k_pn_update   s += clip(ds + dsv sum_d v_r v_l), v += clip(v_l dv)
//   readout: k_pn_lin (vector_mix_net), k_pn_norm, k_pn_lin x2 (gate net), k_pn_readout (gate, last block) -> e->acc
//
// k_pn_lin: Y = act(X W + b) on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate), the workgroup's 64-column
// slice of W staged in LDS in MFMA fragment order (packed once on the host by lb_painn_create; the scheme of lb_lin32.h).
// The dead-edge skip is exact: a dead edge's filter is multiplied by a cutoff of exactly 0, so with finite features its
// message adds (+-)0 to the sums.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lb_device.h"

#define PN_TN 4         // nodes per workgroup of k_pn_msg / k_pn_embed
#define PN_KPAD 64      // node feature row stride (vel_hist | vel_mag | bound | force <= 45 columns)
#define PN_MAX_RBF 64
#define PN_WG 256       // k_pn_lin: 4 waves
#define PN_TPW 2        // 16-row tiles per wave
#define PN_CB 4         // 16-column output blocks per workgroup (64 columns)
#define PN_KMAX 256     // largest K on the MFMA path (2H): 16 k-fragments x 4 blocks x 64 lanes x 16 B = 64 KiB of LDS

struct pn_lin {   // one Linear on the MFMA path
  const f32x4* wp;  // fragments [NJ][NOB][64]: entry ((j NOB + mb) 64 + lane)[i] = W[16 j + 4 (lane >> 4) + i][16 mb + (lane & 15)]
  const float* b;   // [NO] or null
  int K, NO, NJ, NOB;  // NJ = ceil(K / 16), NOB = ceil(NO / 64) * 4 (zero padded)
};

struct pn_layer {
  const float *wi0, *bi0, *wi1, *bi1, *wm0, *bm0, *wm1, *bm1, *wvm;  // row-major (fan_in, fan_out)
  pn_lin li0, li1, lm0, lm1, lvm;
};

struct lb_painn {
  lb_arena mem;  // owns every buffer below
  lb_painn_desc desc;
  lb_engine* eng;
  int n_scal, n_vec, c_frc, c_bnd;  // scalar inputs, vector channels, raw-row columns of force / bound (-1: absent)
  int n_sets, n_filt;               // parameter sets of the layers, filter blocks
  float* blob = nullptr;            // the weights as given (a view: the caller's device blob)
  f32x4* packed = nullptr;          // MFMA fragment images
  const float *w_se = nullptr, *b_se = nullptr, *w_ve = nullptr, *w_f = nullptr, *b_f = nullptr;
  const float *w_rbf = nullptr, *o_rbf = nullptr;
  std::vector<pn_layer> layers;
  const float *r0_vm, *r0_b0, *r0_b1;  // readout_block_0: vector_mix_net (H, H); gate biases
  pn_lin r0_lvm, r0_l0, r0_l1;
  const float *ro_vm, *ro_w0, *ro_b0, *ro_w1, *ro_b1;  // readout_block_out
  float* xnode = nullptr;  // [BN][PN_KPAD]
  float* s = nullptr;      // [BN][H]
  float* va = nullptr;     // [BN][dim][H] (two buffers)
  float* vb = nullptr;
  float* x3 = nullptr;     // [BN][3H]: interaction output, then the mixing block's output
  float* h1 = nullptr;     // [BN][H]
  float* ts = nullptr;     // [BN][2H]
  float* vm = nullptr;     // [BN][dim][2H]
  int64_t e_alloc = 0;
  int32_t* rev = nullptr;  // [e_alloc]
  int32_t* orph = nullptr; // [e_alloc + 1] edges without a transpose (count first)
  f32x4* geo = nullptr;    // [e_alloc]: dir (3), filter scale (0 on a dead edge)
  float* nrm = nullptr;    // [e_alloc]: norm, or -1 on a dead edge
  float* tap_s = nullptr;
  float* tap_v = nullptr;
  // a view (lbk_painn_view_create): blob belongs to the caller, the fragment images are re-made from it by every forward
  struct pack_job { int64_t src, dst; int K, NO; };  // float offsets into blob / packed
  pack_job* jobs_dev = nullptr;
  int n_jobs = 0;   // > 0: a view
};

__device__ __forceinline__ float pn_silu(float x) { return x / (1.f + expf(-x)); }
__device__ __forceinline__ float pn_clip(float x) { return fminf(fmaxf(x, -100.f), 100.f); }

// ------------------------------------------------------------------------------- embedding
struct pn_embed_args {
  const lb_ctrl* ctrl;
  lb_geom g;
  int64_t BN;
  int H, n_vels, homogeneous, n_vec, c_frc, c_bnd;
  const float* xnode;
  const int32_t* ptype;
  const float *w_se, *b_se, *w_ve;
  float* s;
  float* v;
};

__global__ void __launch_bounds__(128) k_pn_embed(pn_embed_args a) {
  if (a.ctrl->overflow_step >= 0) return;
  __shared__ float sc[PN_TN][20];
  __shared__ float vc[PN_TN][3][12];
  const int64_t base = (int64_t)blockIdx.x * PN_TN;
  const int dim = a.g.dim, K = a.g.isl - 1;
  const int n_scal = a.n_vels + (a.homogeneous ? 0 : 9);
  if (threadIdx.x < PN_TN) {
    const int t = threadIdx.x;
    const int64_t i = base + t;
    if (i < a.BN) {
      const float* x = a.xnode + i * PN_KPAD;
      for (int k = 0; k < a.n_vels; ++k) sc[t][k] = x[K * dim + k];  // vel_mag (painn.py:481)
      if (!a.homogeneous) {
        const int pt = a.ptype[i];  // jax.nn.one_hot: an index outside [0, 9) gives a zero row
        for (int j = 0; j < 9; ++j) sc[t][a.n_vels + j] = j == pt ? 1.f : 0.f;
      }
      // vector channels [v_0 .. v_{K-1} | force | bound_lo | bound_hi] (painn.py:470-478)
      for (int d = 0; d < dim; ++d) {
        int c = 0;
        for (; c < a.n_vels; ++c) vc[t][d][c] = x[c * dim + d];
        if (a.c_frc >= 0) vc[t][d][c++] = x[a.c_frc + d];
        if (a.c_bnd >= 0) {
          vc[t][d][c++] = x[a.c_bnd + d];
          vc[t][d][c++] = x[a.c_bnd + dim + d];
        }
      }
    }
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= a.H) return;
  const int H = a.H;
  for (int t = 0; t < PN_TN; ++t) {
    const int64_t i = base + t;
    if (i >= a.BN) break;
    float acc = 0.f;
    for (int k = 0; k < n_scal; ++k) acc += sc[t][k] * a.w_se[k * H + j];
    a.s[i * H + j] = acc + a.b_se[j];
    for (int d = 0; d < dim; ++d) {
      float av = 0.f;
      for (int c = 0; c < a.n_vec; ++c) av += vc[t][d][c] * a.w_ve[c * H + j];
      a.v[(i * dim + d) * H + j] = av;
    }
  }
}

// ------------------------------------------------------------------------------- edge geometry
__global__ void k_pn_edge(const lb_ctrl* __restrict__ ctrl, int64_t cap, int dim, int has_cutoff, float cutoff,
                          const float* __restrict__ efeat, f32x4* __restrict__ geo, float* __restrict__ nrm) {
  if (ctrl->overflow_step >= 0) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int E = ctrl->n_edges_total;
  if (e >= E || e >= cap) return;
  const float r0 = efeat[e * 8], r1 = efeat[e * 8 + 1], r2 = dim == 3 ? efeat[e * 8 + 2] : 0.f;
  float q = r0 * r0 + r1 * r1;
  if (dim == 3) q = q + r2 * r2;
  const float norm = sqrtf(q + 1e-8f);
  const float den = norm + 1e-8f;
  float scale;
  bool live = true;
  if (has_cutoff) {  // cosine_cutoff (painn.py:162-168): 0.5 (cos(x pi / rc) + 1) (x < rc)
    live = norm < cutoff;
    scale = live ? 0.5f * (cosf(norm * 3.14159265358979323846f / cutoff) + 1.f) : 0.f;
  } else {
    scale = norm;  // painn.py:433-436: the filters are multiplied by the norm itself
  }
  geo[e] = f32x4{r0 / den, r1 / den, r2 / den, scale};
  nrm[e] = live ? norm : -1.f;
}

// ------------------------------------------------------------------------------- Linear on the MFMA
template <int ACT>
__global__ void __launch_bounds__(PN_WG) k_pn_lin(const lb_ctrl* __restrict__ ctrl, int64_t rows,
                                                  const float* __restrict__ X, int ldx, pn_lin w, float* __restrict__ Y,
                                                  int ldy) {
  if (ctrl->overflow_step >= 0) return;
  __shared__ f32x4 s_w[PN_KMAX / 16 * PN_CB * 64];
  const int cb = blockIdx.y;
  for (int q = threadIdx.x; q < w.NJ * PN_CB * 64; q += PN_WG) {
    const int j = q / (PN_CB * 64), r = q % (PN_CB * 64);
    s_w[q] = w.wp[((int64_t)j * w.NOB + cb * PN_CB) * 64 + r];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kq = lane >> 4;
  for (int tt = 0; tt < PN_TPW; ++tt) {
    const int64_t row0 = (((int64_t)blockIdx.x * (PN_WG / 64) + wave) * PN_TPW + tt) * 16;
    if (row0 >= rows) break;
    const int64_t row = row0 + n;
    const bool rok = row < rows;
    const float* xr = X + (rok ? row : 0) * ldx;
    f32x4 acc[PN_CB];
#pragma unroll
    for (int mb = 0; mb < PN_CB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < w.NJ; ++j) {
      float x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * j + 4 * kq + i;
        x[i] = (rok && k < w.K) ? xr[k] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int mb = 0; mb < PN_CB; ++mb)
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(j * PN_CB + mb) * 64 + lane][i], x[i], acc[mb], 0, 0, 0);
      }
    }
    // D: lane (n, kq) holds Y[row n][16 mb + 4 kq + t]
    if (rok) {
#pragma unroll
      for (int mb = 0; mb < PN_CB; ++mb) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int col = cb * 64 + 16 * mb + 4 * kq + t;
          if (col < w.NO) {
            float y = acc[mb][t];
            if (w.b) y = y + w.b[col];
            if (ACT) y = pn_silu(y);
            Y[row * ldy + col] = y;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------- message
struct pn_msg_args {
  const lb_ctrl* ctrl;
  int64_t BN;
  int H, dim, n_rbf, ldf, fcol;  // ldf = filter_net's output width, fcol = this layer's first filter column
  const int32_t* row_ptr;
  const int32_t* rev;
  const int32_t* orph;
  const int32_t* senders;
  const int32_t* receivers;
  const f32x4* geo;
  const float* nrm;
  const float *w_rbf, *o_rbf;  // widths, offsets
  const float *wf, *bf;        // filter_net (n_rbf, ldf), (ldf)
  const float* x3;             // [BN][3H]
  const float* vin;            // [BN][dim][H]
  float* s;                    // in / out
  float* vout;
};

__global__ void __launch_bounds__(128) k_pn_msg(pn_msg_args a) {
  if (a.ctrl->overflow_step >= 0) return;
  __shared__ float s_coef[PN_MAX_RBF], s_off[PN_MAX_RBF];
  if (threadIdx.x < a.n_rbf) {
    const float w = a.w_rbf[threadIdx.x];
    s_coef[threadIdx.x] = -0.5f / (w * w);  // painn.py:137: -0.5 / widths^2
    s_off[threadIdx.x] = a.o_rbf[threadIdx.x];
  }
  __syncthreads();
  const int H = a.H, dim = a.dim, j = threadIdx.x;
  if (j >= H) return;
  const int E = a.ctrl->n_edges_total;
  const int64_t base = (int64_t)blockIdx.x * PN_TN;
  for (int t = 0; t < PN_TN; ++t) {
    const int64_t i = base + t;
    if (i >= a.BN) break;
    int k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
    k0 = k0 < E ? k0 : E;
    k1 = k1 < E ? k1 : E;
    float ds = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;
    // the edges whose SENDER is i (painn.py:301-303 aggregates at senders): the transposes of row i, in row order, then
    // the orphans sent by i (edges without a transpose: lb_internal.h, lbk_edge_rev) in slot order
    auto add = [&](int e) {
      const float norm = a.nrm[e];
      if (norm < 0.f) return;  // dead: the filter is exactly 0
      const f32x4 gm = a.geo[e];
      const int r = a.receivers[e];
      float f0 = 0.f, f1 = 0.f, f2 = 0.f;
      const float* wf = a.wf + a.fcol + j;
      for (int q = 0; q < a.n_rbf; ++q) {
        const float df = norm - s_off[q];
        const float phi = expf(s_coef[q] * (df * df));
        f0 += phi * wf[q * a.ldf];
        f1 += phi * wf[q * a.ldf + H];
        f2 += phi * wf[q * a.ldf + 2 * H];
      }
      const float* bf = a.bf + a.fcol + j;
      f0 = (f0 + bf[0]) * gm[3];
      f1 = (f1 + bf[H]) * gm[3];
      f2 = (f2 + bf[2 * H]) * gm[3];
      const float* xr = a.x3 + (int64_t)r * 3 * H + j;
      const float ws = f0 * xr[0], wv1 = f1 * xr[H], wv2 = f2 * xr[2 * H];
      const float* vr = a.vin + (int64_t)r * dim * H + j;
      ds += ws;
      dv0 += wv1 * gm[0] + wv2 * vr[0];
      dv1 += wv1 * gm[1] + wv2 * vr[H];
      if (dim == 3) dv2 += wv1 * gm[2] + wv2 * vr[2 * H];
    };
    for (int k = k0; k < k1; ++k) {
      const int e = a.rev[k];
      if (e >= 0) add(e);   // (rev = -1: i does not send to the sender of slot k)
    }
    lb_for_orphans(a.orph, a.senders, i, add);
    a.s[i * H + j] = a.s[i * H + j] + pn_clip(ds);
    const float* vi = a.vin + i * dim * H + j;
    float* vo = a.vout + i * dim * H + j;
    vo[0] = vi[0] + pn_clip(dv0);
    vo[H] = vi[H] + pn_clip(dv1);
    if (dim == 3) vo[2 * H] = vi[2 * H] + pn_clip(dv2);
  }
}

// ------------------------------------------------------------------------------- update
// out[i] = [s[i][0 .. ns) | sqrt(sum_d vm[i][d][off + c]^2 + eps) for c < nv]
__global__ void k_pn_norm(const lb_ctrl* __restrict__ ctrl, int64_t BN, int dim, const float* __restrict__ s, int ns,
                          const float* __restrict__ vm, int ldvm, int off, int nv, float* __restrict__ out) {
  if (ctrl->overflow_step >= 0) return;
  const int w = ns + nv;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= BN * w) return;
  const int64_t i = q / w;
  const int c = (int)(q % w);
  float y;
  if (c < ns) {
    y = s[i * ns + c];
  } else {
    const float* p = vm + i * dim * ldvm + off + (c - ns);
    float acc = p[0] * p[0];
    for (int d = 1; d < dim; ++d) acc = acc + p[d * ldvm] * p[d * ldvm];
    y = sqrtf(acc + 1e-8f);
  }
  out[i * w + c] = y;
}

// s += clip(ds + dsv sum_d v_r v_l), v += clip(v_l dv)  (painn.py:320-337)
__global__ void k_pn_update(const lb_ctrl* __restrict__ ctrl, int64_t BN, int dim, int H, const float* __restrict__ m3,
                            const float* __restrict__ vm, float* __restrict__ s, float* __restrict__ v) {
  if (ctrl->overflow_step >= 0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= BN * H) return;
  const int64_t i = q / H;
  const int j = (int)(q % H);
  const float* mm = m3 + i * 3 * H + j;
  const float* pv = vm + i * dim * 2 * H + j;
  float dot = pv[0] * pv[H];
  for (int d = 1; d < dim; ++d) dot = dot + pv[d * 2 * H] * pv[d * 2 * H + H];
  s[q] = s[q] + pn_clip(mm[0] + mm[2 * H] * dot);
  float* vv = v + i * dim * H + j;
  for (int d = 0; d < dim; ++d) vv[d * H] = vv[d * H] + pn_clip(pv[d * 2 * H] * mm[H]);
}

// ------------------------------------------------------------------------------- readout
// The second gated block, one thread per node.  y: gate net output of the first block [BN][H]: s' = y[:, :H/2],
// gate = y[:, H/2:]; vm: the first block's vector_mix_net output [BN][dim][H] (v_l = its first H/2 columns).
// v' = v_l gate; [a_l | a_r] = v' W_vm (H/2, 2); acc = a_l * (silu([s' | |a_r|] W0 + b0) W1 + b1)[:, 1].
__global__ void __launch_bounds__(64) k_pn_readout(const lb_ctrl* __restrict__ ctrl, int64_t BN, int dim, int H,
                                                   const float* __restrict__ y, const float* __restrict__ vm,
                                                   const float* __restrict__ wvm, const float* __restrict__ w0,
                                                   const float* __restrict__ b0, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, float* __restrict__ acc) {
  if (ctrl->overflow_step >= 0) return;
  __shared__ float gin[64][65];
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= BN) return;
  const int Hh = H / 2;
  const float* yi = y + i * H;
  float al[3] = {0.f, 0.f, 0.f}, ar[3] = {0.f, 0.f, 0.f};
  for (int d = 0; d < dim; ++d) {
    const float* vl = vm + (i * dim + d) * H;
    float l = 0.f, r = 0.f;
    for (int c = 0; c < Hh; ++c) {
      const float vp = vl[c] * yi[Hh + c];
      l += vp * wvm[2 * c];
      r += vp * wvm[2 * c + 1];
    }
    al[d] = l;
    ar[d] = r;
  }
  float q = ar[0] * ar[0];
  for (int d = 1; d < dim; ++d) q = q + ar[d] * ar[d];
  float* g = gin[threadIdx.x];
  for (int c = 0; c < Hh; ++c) g[c] = yi[c];
  g[Hh] = sqrtf(q + 1e-8f);
  float gate = 0.f;
  for (int c = 0; c < Hh; ++c) {
    float z = 0.f;
    for (int k = 0; k <= Hh; ++k) z += g[k] * w0[k * Hh + c];
    gate += pn_silu(z + b0[c]) * w1[2 * c + 1];
  }
  gate = gate + b1[1];
  float* o = acc + i * 4;
  o[0] = al[0] * gate;
  o[1] = al[1] * gate;
  o[2] = dim == 3 ? al[2] * gate : 0.f;
  o[3] = 0.f;
}

// ------------------------------------------------------------------------------- model
static int64_t pn_frag_floats(int K, int NO) {
  const int NJ = (K + 15) / 16, NOB = (NO + 63) / 64 * 4;
  return (int64_t)NJ * NOB * 64 * 4;
}

// row-major W (K, NO) -> fragment order at dst (zero padded)
static void pn_pack(const float* W, int K, int NO, float* dst) {
  const int NJ = (K + 15) / 16, NOB = (NO + 63) / 64 * 4;
  for (int j = 0; j < NJ; ++j)
    for (int mb = 0; mb < NOB; ++mb)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * j + 4 * (lane >> 4) + i, m = 16 * mb + (lane & 15);
          dst[(((int64_t)j * NOB + mb) * 64 + lane) * 4 + i] = (k < K && m < NO) ? W[(int64_t)k * NO + m] : 0.f;
        }
}

// the same on the device, for a view: one job per blockIdx.y
__global__ void __launch_bounds__(256) k_pn_pack(const float* __restrict__ blob, float* __restrict__ packed,
                                                 const lb_painn::pack_job* __restrict__ jobs) {
  const lb_painn::pack_job jb = jobs[blockIdx.y];
  const int NJ = (jb.K + 15) / 16, NOB = (jb.NO + 63) / 64 * 4;
  const int64_t total = (int64_t)NJ * NOB * 256;
  const float* W = blob + jb.src;
  float* dst = packed + jb.dst;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int i = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const int64_t q = idx >> 8;
    const int mb = (int)(q % NOB), j = (int)(q / NOB);
    const int k = 16 * j + 4 * (lane >> 4) + i, m = 16 * mb + (lane & 15);
    dst[idx] = (k < jb.K && m < jb.NO) ? W[(int64_t)k * jb.NO + m] : 0.f;
  }
}

static int pn_ensure_edges(lb_painn* m) {
  lb_engine* e = m->eng;
  if (m->e_alloc >= e->e_alloc) return LB_OK;
  return lb_regrow(e->stream, &m->e_alloc, e->e_alloc, [&](int64_t cap) {
    const size_t n = (size_t)cap;
    LB_TRY(m->mem.get(&m->rev, n));
    LB_TRY(m->mem.get(&m->orph, n + 1));
    LB_TRY(m->mem.get(&m->geo, n));
    return m->mem.get(&m->nrm, n);
  });
}

extern "C" void lb_painn_destroy(lb_painn* m) {
  delete m;
}

static int64_t pn_n_floats(const lb_painn_desc* d, int n_scal, int n_vec) {
  const int64_t H = d->hidden, R = d->n_rbf, Hh = H / 2;
  const int64_t sets = d->shared_interactions ? 1 : d->num_mp_steps;
  const int64_t filt = d->shared_filters ? 1 : d->num_mp_steps;
  const int64_t layer = H * H + H + H * 3 * H + 3 * H + 2 * H * H + H + H * 3 * H + 3 * H + H * 2 * H;
  const int64_t ro0 = H * H + (H + Hh) * H + H + H * H + H;
  const int64_t ro1 = Hh * 2 + (Hh + 1) * Hh + Hh + Hh * 2 + 2;
  return n_scal * H + H + n_vec * H + R * filt * 3 * H + filt * 3 * H + sets * layer + ro0 + ro1 + 2 * R;
}

// w: the caller's host blob (a model), or null with w_dev: a view of a device blob in the same layout that the caller owns
static int pn_create(lb_engine* e, const lb_painn_desc* d, const float* w, const float* w_dev, int64_t n_floats,
                     lb_painn** out) {
  if (!e || !d || (!w && !w_dev) || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->hidden < 16 || d->hidden > 128 || d->hidden % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "PaiNN hidden size %d: a multiple of 16 up to 128 is built", d->hidden);
  if (d->num_mp_steps < 1 || d->num_mp_steps > 64) return lb_fail(LB_ERR_ARG, "bad num_mp_steps %d", d->num_mp_steps);
  if (d->n_vels < 1 || d->n_vels > 9) return lb_fail(LB_ERR_ARG, "bad n_vels %d (1 .. 9)", d->n_vels);
  if (d->n_vels != e->g.isl - 1) return lb_fail(LB_ERR_ARG, "n_vels %d != input_seq_length-1", d->n_vels);
  if (d->n_rbf < 1 || d->n_rbf > PN_MAX_RBF) return lb_fail(LB_ERR_ARG, "bad n_rbf %d (1 .. %d)", d->n_rbf, PN_MAX_RBF);
  if (d->has_cutoff && !(d->cutoff > 0.f)) return lb_fail(LB_ERR_ARG, "cutoff must be > 0");
  if (!e->g.has_vel_mag)
    return lb_fail(LB_ERR_ARG, "PaiNN takes the velocity magnitudes as its scalars: build the case with "
                   "magnitude_features (the reference's runner asserts it)");
  lb_painn* m = new lb_painn();
  m->desc = *d;
  m->eng = e;
  const int dim = e->g.dim, K = e->g.isl - 1;
  m->n_scal = d->n_vels + (d->homogeneous ? 0 : 9);
  const int c_bnd = K * dim + K;  // raw row [vel_hist | vel_mag | bound | force]
  m->c_bnd = e->g.has_bound ? c_bnd : -1;
  m->c_frc = e->g.force_kind != LB_FORCE_NONE ? c_bnd + (e->g.has_bound ? 2 * dim : 0) : -1;
  m->n_vec = d->n_vels + (m->c_frc >= 0 ? 1 : 0) + (m->c_bnd >= 0 ? 2 : 0);
  m->n_sets = d->shared_interactions ? 1 : d->num_mp_steps;
  m->n_filt = d->shared_filters ? 1 : d->num_mp_steps;
  const int64_t need = pn_n_floats(d, m->n_scal, m->n_vec);
  if (n_floats != need) {
    delete m;
    return lb_fail(LB_ERR_ARG, "PaiNN weights: expected %lld floats, got %lld", (long long)need, (long long)n_floats);
  }
  const int64_t BN = e->BN, H = d->hidden, Hh = H / 2;
  int rc = LB_OK;
  auto step = [&](int r) {
    if (!rc) rc = r;
  };
  if (w) {
    step(m->mem.get(&m->blob, (size_t)n_floats));
    if (!rc) {
      const hipError_t he = hipMemcpy(m->blob, w, sizeof(float) * n_floats, hipMemcpyHostToDevice);
      if (he != hipSuccess) rc = lb_fail(LB_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(he));
    }
  } else {
    m->blob = const_cast<float*>(w_dev);   // (not the arena's: never freed here)
  }
  step(m->mem.get(&m->xnode, (size_t)BN * PN_KPAD));
  step(m->mem.get(&m->s, (size_t)BN * H));
  step(m->mem.get(&m->va, (size_t)BN * dim * H));
  step(m->mem.get(&m->vb, (size_t)BN * dim * H));
  step(m->mem.get(&m->x3, (size_t)BN * 3 * H));
  step(m->mem.get(&m->h1, (size_t)BN * H));
  step(m->mem.get(&m->ts, (size_t)BN * 2 * H));
  step(m->mem.get(&m->vm, (size_t)BN * dim * 2 * H));
  if (rc) {
    lb_painn_destroy(m);
    return rc;
  }
  // carve the blob (include/lbhip.h: lb_painn_create); h_* point into the host copy for packing (a view: into the device blob, read for their offsets only)
  int64_t o = 0;
  const float* const hbase = w ? w : m->blob;
  auto take = [&](int64_t n, const float** h) {
    const float* r = m->blob + o;
    *h = hbase + o;
    o += n;
    return r;
  };
  const float* hd;
  m->w_se = take(m->n_scal * H, &hd);
  m->b_se = take(H, &hd);
  m->w_ve = take(m->n_vec * H, &hd);
  const int64_t ldf = m->n_filt * 3 * H;
  m->w_f = take(d->n_rbf * ldf, &hd);
  m->b_f = take(ldf, &hd);
  // fragment images: per set 5 Linears, readout_block_0 3
  struct Job {
    const float* host;
    int K, NO;
    pn_lin* dst;
    const float* bias;
  };
  std::vector<Job> jobs;
  m->layers.resize(m->n_sets);
  for (auto& l : m->layers) {
    const float* h;
    l.wi0 = take(H * H, &h);
    jobs.push_back({h, (int)H, (int)H, &l.li0, nullptr});
    l.bi0 = take(H, &hd);
    l.wi1 = take(H * 3 * H, &h);
    jobs.push_back({h, (int)H, (int)(3 * H), &l.li1, nullptr});
    l.bi1 = take(3 * H, &hd);
    l.wm0 = take(2 * H * H, &h);
    jobs.push_back({h, (int)(2 * H), (int)H, &l.lm0, nullptr});
    l.bm0 = take(H, &hd);
    l.wm1 = take(H * 3 * H, &h);
    jobs.push_back({h, (int)H, (int)(3 * H), &l.lm1, nullptr});
    l.bm1 = take(3 * H, &hd);
    l.wvm = take(H * 2 * H, &h);
    jobs.push_back({h, (int)H, (int)(2 * H), &l.lvm, nullptr});
    l.li0.b = l.bi0;
    l.li1.b = l.bi1;
    l.lm0.b = l.bm0;
    l.lm1.b = l.bm1;
  }
  {
    const float* h;
    m->r0_vm = take(H * H, &h);
    jobs.push_back({h, (int)H, (int)H, &m->r0_lvm, nullptr});
    take((H + Hh) * H, &h);
    jobs.push_back({h, (int)(H + Hh), (int)H, &m->r0_l0, nullptr});
    m->r0_b0 = take(H, &hd);
    take(H * H, &h);
    jobs.push_back({h, (int)H, (int)H, &m->r0_l1, nullptr});
    m->r0_b1 = take(H, &hd);
    m->r0_l0.b = m->r0_b0;
    m->r0_l1.b = m->r0_b1;
  }
  m->ro_vm = take(Hh * 2, &hd);
  m->ro_w0 = take((Hh + 1) * Hh, &hd);
  m->ro_b0 = take(Hh, &hd);
  m->ro_w1 = take(Hh * 2, &hd);
  m->ro_b1 = take(2, &hd);
  m->w_rbf = take(d->n_rbf, &hd);
  m->o_rbf = take(d->n_rbf, &hd);
  int64_t pf = 0;
  for (auto& j : jobs) pf += pn_frag_floats(j.K, j.NO);
  std::vector<float> img(w ? (size_t)pf : 0);
  int64_t po = 0;
  std::vector<int64_t> offs;
  std::vector<lb_painn::pack_job> pj;
  for (auto& j : jobs) {
    if (w) pn_pack(j.host, j.K, j.NO, img.data() + po);
    else pj.push_back({(int64_t)(j.host - hbase), po, j.K, j.NO});
    offs.push_back(po);
    po += pn_frag_floats(j.K, j.NO);
  }
  if (m->mem.get(&m->packed, (size_t)pf / 4) == LB_OK) {
    hipError_t he = hipSuccess;
    if (w) {
      he = hipMemcpy(m->packed, img.data(), sizeof(float) * pf, hipMemcpyHostToDevice);
    } else if (m->mem.get(&m->jobs_dev, pj.size()) == LB_OK) {
      he = hipMemcpy(m->jobs_dev, pj.data(), sizeof(lb_painn::pack_job) * pj.size(), hipMemcpyHostToDevice);
      m->n_jobs = (int)pj.size();
    } else {
      rc = LB_ERR_HIP;
    }
    if (he != hipSuccess) rc = lb_fail(LB_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(he));
  } else {
    rc = LB_ERR_HIP;
  }
  if (rc) {
    lb_painn_destroy(m);
    return rc;
  }
  for (size_t k = 0; k < jobs.size(); ++k) {
    pn_lin& l = *jobs[k].dst;
    l.wp = m->packed + offs[k] / 4;
    l.K = jobs[k].K;
    l.NO = jobs[k].NO;
    l.NJ = (l.K + 15) / 16;
    l.NOB = (l.NO + 63) / 64 * 4;
  }
  *out = m;
  return LB_OK;
}

extern "C" int lb_painn_create(lb_engine* e, const lb_painn_desc* d, const float* w, int64_t n_floats,
                               lb_painn** out) {
  if (!w) return lb_fail(LB_ERR_ARG, "null argument");
  return pn_create(e, d, w, nullptr, n_floats, out);
}

// the training handle's view (lb_train_painn.h): a model on the caller's device blob w_dev (lb_painn_create's layout)
int lbk_painn_view_create(lb_engine* e, const lb_painn_desc* d, const float* w_dev, int64_t n_floats, lb_painn** out) {
  if (!w_dev) return lb_fail(LB_ERR_ARG, "null argument");
  return pn_create(e, d, nullptr, w_dev, n_floats, out);
}

extern "C" int lb_painn_set_tap(lb_painn* m, float* s_out_dev, float* v_out_dev) {
  if (!m) return lb_fail(LB_ERR_ARG, "null model");
  m->tap_s = s_out_dev;
  m->tap_v = v_out_dev;
  return LB_OK;
}

template <int ACT>
static void pn_lin_launch(lb_engine* e, int64_t rows, const float* X, int ldx, const pn_lin& w, float* Y, int ldy) {
  const int64_t rpb = (PN_WG / 64) * PN_TPW * 16;
  const unsigned nb = (unsigned)((rows + rpb - 1) / rpb);
  hipLaunchKernelGGL(k_pn_lin<ACT>, dim3(nb ? nb : 1, (unsigned)(w.NOB / PN_CB)), dim3(PN_WG), 0, e->stream, e->ctrl,
                     rows, X, ldx, w, Y, ldy);
}

static int lbk_painn_forward(lb_engine* e, lb_painn* m) {
  hipStream_t st = e->stream;
  const int64_t BN = e->BN;
  const int H = m->desc.hidden, dim = e->g.dim, Hh = H / 2;
  LB_TRY(pn_ensure_edges(m));
  if (m->n_jobs)   // a view: the weights may have moved since the last forward
    hipLaunchKernelGGL(k_pn_pack, dim3(16, (unsigned)m->n_jobs), dim3(256), 0, st, m->blob, reinterpret_cast<float*>(m->packed),
                       m->jobs_dev);
  const int64_t ecap = (int64_t)e->e_cap * e->g.B;
  const unsigned nb_t = (unsigned)((BN + PN_TN - 1) / PN_TN), nb_e = (unsigned)((ecap + 255) / 256);
  float* v = m->va;
  float* v2 = m->vb;
  auto tap = [&](int slot) -> int {
    if (m->tap_s)
      LB_HIP(hipMemcpyAsync(m->tap_s + (size_t)slot * BN * H, m->s, sizeof(float) * BN * H, hipMemcpyDeviceToDevice, st));
    if (m->tap_v)
      LB_HIP(hipMemcpyAsync(m->tap_v + (size_t)slot * BN * dim * H, v, sizeof(float) * BN * dim * H,
                            hipMemcpyDeviceToDevice, st));
    return LB_OK;
  };
  lb_tic(e, LB_T_NODEFEAT);
  LB_TRY(lbk_node_features_raw(e, m->xnode, PN_KPAD));
  pn_embed_args ea{e->ctrl, e->g, BN, H, m->desc.n_vels, m->desc.homogeneous, m->n_vec, m->c_frc, m->c_bnd,
                   m->xnode, e->ptype, m->w_se, m->b_se, m->w_ve, m->s, v};
  hipLaunchKernelGGL(k_pn_embed, dim3(nb_t), dim3(128), 0, st, ea);
  hipLaunchKernelGGL(k_pn_edge, dim3(nb_e ? nb_e : 1), dim3(256), 0, st, e->ctrl, ecap, dim, m->desc.has_cutoff,
                     m->desc.cutoff, e->efeat, m->geo, m->nrm);
  LB_TRY(lbk_edge_rev(e, m->rev, m->orph));
  lb_toc(e);
  LB_HIP(hipGetLastError());
  LB_TRY(tap(0));
  const unsigned nb_nh = (unsigned)((BN * H + 255) / 256), nb_n2 = (unsigned)((BN * 2 * H + 255) / 256);
  for (int k = 0; k < m->desc.num_mp_steps; ++k) {
    const pn_layer& l = m->layers[m->desc.shared_interactions ? 0 : k];
    lb_tic(e, LB_T_EDGE_MLP);
    pn_lin_launch<1>(e, BN, m->s, H, l.li0, m->h1, H);
    pn_lin_launch<0>(e, BN, m->h1, H, l.li1, m->x3, 3 * H);
    pn_msg_args ma{};
    ma.ctrl = e->ctrl;
    ma.BN = BN;
    ma.H = H;
    ma.dim = dim;
    ma.n_rbf = m->desc.n_rbf;
    ma.ldf = m->n_filt * 3 * H;
    ma.fcol = m->desc.shared_filters ? 0 : k * 3 * H;
    ma.row_ptr = e->row_ptr;
    ma.rev = m->rev;
    ma.orph = m->orph;
    ma.senders = e->senders;
    ma.receivers = e->receivers;
    ma.geo = m->geo;
    ma.nrm = m->nrm;
    ma.w_rbf = m->w_rbf;
    ma.o_rbf = m->o_rbf;
    ma.wf = m->w_f;
    ma.bf = m->b_f;
    ma.x3 = m->x3;
    ma.vin = v;
    ma.s = m->s;
    ma.vout = v2;
    hipLaunchKernelGGL(k_pn_msg, dim3(nb_t), dim3(128), 0, st, ma);
    std::swap(v, v2);
    lb_toc(e);
    lb_tic(e, LB_T_NODE_MLP);
    pn_lin_launch<0>(e, BN * dim, v, H, l.lvm, m->vm, 2 * H);
    hipLaunchKernelGGL(k_pn_norm, dim3(nb_n2), dim3(256), 0, st, e->ctrl, BN, dim, m->s, H, m->vm, 2 * H, H, H, m->ts);
    pn_lin_launch<1>(e, BN, m->ts, 2 * H, l.lm0, m->h1, H);
    pn_lin_launch<0>(e, BN, m->h1, H, l.lm1, m->x3, 3 * H);
    hipLaunchKernelGGL(k_pn_update, dim3(nb_nh), dim3(256), 0, st, e->ctrl, BN, dim, H, m->x3, m->vm, m->s, v);
    lb_toc(e);
    LB_HIP(hipGetLastError());
    LB_TRY(tap(k + 1));
  }
  // readout (painn.py:173-215): block 0 on the MFMA, the last block per node
  lb_tic(e, LB_T_DECODER);
  pn_lin_launch<0>(e, BN * dim, v, H, m->r0_lvm, m->vm, H);
  const unsigned nb_g = (unsigned)((BN * (H + Hh) + 255) / 256);
  hipLaunchKernelGGL(k_pn_norm, dim3(nb_g), dim3(256), 0, st, e->ctrl, BN, dim, m->s, H, m->vm, H, Hh, Hh, m->ts);
  pn_lin_launch<1>(e, BN, m->ts, H + Hh, m->r0_l0, m->h1, H);
  pn_lin_launch<0>(e, BN, m->h1, H, m->r0_l1, m->x3, H);
  hipLaunchKernelGGL(k_pn_readout, dim3((unsigned)((BN + 63) / 64)), dim3(64), 0, st, e->ctrl, BN, dim, H, m->x3,
                     m->vm, m->ro_vm, m->ro_w0, m->ro_b0, m->ro_w1, m->ro_b1, e->acc);
  lb_toc(e);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

extern "C" int lb_painn_forward(lb_engine* e, lb_painn* m, float* acc_out_dev) {
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  LB_TRY(lb_forward_check(e, "lb_painn_forward"));
  LB_TRY(lbk_painn_forward(e, m));
  if (acc_out_dev) LB_TRY(lb_export_rows(e, e->acc, acc_out_dev, true));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// one forward of the view for the training step: the state its backward reads
int lbk_painn_train_forward(lb_engine* e, lb_painn* m, lb_painn_state* st) {
  LB_TRY(lbk_painn_forward(e, m));
  st->xnode = m->xnode;
  st->rev = m->rev;
  st->orph = m->orph;
  st->geo = m->geo;
  st->nrm = m->nrm;
  return LB_OK;
}

// one rollout step's model; lb_rollout_generic integrates e->acc with the GNS integrator
static int pn_forward_thunk(lb_engine* e, void* model) { return lbk_painn_forward(e, (lb_painn*)model); }

extern "C" int lb_painn_rollout(lb_engine* e, lb_painn* m, const double* traj_dev, int32_t T, int32_t n_steps,
                                double* pred_out_dev, int32_t* n_realloc_out) {
  if (!traj_dev || !pred_out_dev) return lb_fail(LB_ERR_ARG, "null argument");
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  return lb_rollout_generic(e, pn_forward_thunk, m, traj_dev, T, n_steps, pred_out_dev, n_realloc_out);
}
