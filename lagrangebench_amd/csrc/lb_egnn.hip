// lb_egnn.hip - EGNN (E(n)-equivariant GNN) forward pass and rollout step on gfx950.
//
// Reference functions replaced (paths relative to the reference repo):
//   EGNN._transform                       lagrangebench/models/egnn.py:318-359
//   EGNN.__call__ (embedding, layers)     lagrangebench/models/egnn.py:372-400
//   EGNNLayer (_coord2radial, _message,   lagrangebench/models/egnn.py:119-206
//              _update, _pos_update, velocity correction)
//   case.integrate for a "pos" output     lagrangebench/case_setup/case.py:235-237
//   _forward_eval (mask + window shift)   lagrangebench/evaluate/rollout.py:61-73
//
// Arithmetic: fp32 throughout (runner.py:71-72 runs the model under an fp32 jmp policy), positions included; every sum
// runs in a fixed order (no float atomics), so two runs give identical bits.  Hidden width H: a multiple of 16, <= 128.
//
// Kernels of one forward (L = num_mp_steps):
//   k_eg_prologue  node inputs |v_k| (+ one-hot), h0 = x W_emb + b, x32 (newest positions), vel (un-normalised last
//                  velocity), node attribute |force|
//   k_eg_rev       rev[e]: the slot of the transposed edge (r=s(e), s=r(e)), binary search in the sender-sorted row;
//                  an edge without one gets rev = -1 and goes on the orphan list (lb_internal.h: lbk_edge_rev)
//   per layer:
//   k_eg_proj      [P_s | P_r] = h [W0[0:H] | W0[H:2H]]  (the first edge Linear split by input block)
//   k_eg_edge      coord_diff = disp(x_s, x_r), radial; a = silu(P_s[s] + P_r[r] + radial w_rad + rel_dist w_ea + b0);
//                  m = silu(a W1 + b1) -> msg; phi = silu(m Wx0 + bx0) . wx1 (+ tanh); trans = coord_diff phi
//   k_eg_node      agg = sum of msg over the receiver row (row order); h' = [h +] silu([h|agg|attr] Wn0 + bn0) Wn1 + bn1;
//                  psi = silu(h' Wv0 + bv0) . wv1; x <- shift(x, sum_{sender = i} trans) (through rev, row order,
//                  then the orphans sent by i in slot order);
//                  x <- shift(x, psi vel)
//   k_eg_integrate (rollout step) kinematic select, window advance, prediction store, step counter
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lb_device.h"

#define EG_THREADS 128  // one thread per hidden column (H <= 128; columns >= H idle)
#define EG_TE 32        // edges per workgroup tile
#define EG_TN 16        // nodes per workgroup tile
#define EG_KPAD 64      // node feature row stride (vel_hist | vel_mag | bound | force <= 45 columns)

struct lb_egnn_layer {
  const float *w0, *b0, *w1, *b1;      // edge MLP: W0 (2H+2, H), W1 (H, H)
  const float *wn0, *bn0, *wn1, *bn1;  // node MLP: Wn0 (2H+A, H), Wn1 (H, H)
  const float *wx0, *bx0, *wx1;        // position net: (H, H), (H), (H, 1)
  const float *wv0, *bv0, *wv1;        // velocity net
};

struct lb_egnn {
  lb_arena mem;  // owns every buffer below (a view's weights belong to its caller)
  lb_egnn_desc desc;
  lb_engine* eng;
  int node_in, n_attr;
  float* blob = nullptr;
  const float *w_emb = nullptr, *b_emb = nullptr;
  std::vector<lb_egnn_layer> layers;
  float* xnode = nullptr;  // [BN][EG_KPAD]
  float* h = nullptr;      // [BN][H]
  float* p = nullptr;      // [BN][2H]
  float* x32 = nullptr;    // [BN][4]
  float* vel = nullptr;    // [BN][4]
  float* nattr = nullptr;  // [BN]
  int64_t e_alloc = 0;
  float* msg = nullptr;    // [e_alloc][H]
  float* trans = nullptr;  // [e_alloc][4]
  int32_t* rev = nullptr;  // [e_alloc]
  int32_t* orph = nullptr; // [e_alloc + 1] edges without a transpose (count first)
  float* tap_h = nullptr;
  float* tap_x = nullptr;
};

__device__ __forceinline__ float eg_silu(float x) { return x / (1.f + expf(-x)); }

// jnp.mod(x, L) in fp32 (jax_md.space.periodic): C fmod, a remainder of the wrong sign moves by L
__device__ __forceinline__ float eg_mod(float x, float L) {
  float r = fmodf(x, L);
  if (r != 0.f && r < 0.f) r = r + L;
  return r;
}
__device__ __forceinline__ float eg_disp(float a, float b, float L, int periodic) {
  const float d = a - b;
  if (!periodic) return d;
  return eg_mod(d + 0.5f * L, L) - 0.5f * L;
}
__device__ __forceinline__ float eg_shift(float r, float dr, float L, int periodic) {
  const float s = r + dr;
  return periodic ? eg_mod(s, L) : s;
}

// Fixed-order sum over the 128 columns of red[t][*] for t < nt: 8 partial sums of 16 consecutive columns, then the 8
// partials in order.  red: [nt][128], part: [nt][8].  Called by all EG_THREADS threads; result in out[t].
template <int NT>
__device__ __forceinline__ void eg_rowsum(float (*red)[EG_THREADS], float (*part)[8], float* out) {
  static_assert(NT * 8 % EG_THREADS == 0 || NT * 8 < EG_THREADS, "tile");
  __syncthreads();
  for (int q = threadIdx.x; q < NT * 8; q += EG_THREADS) {
    const int t = q >> 3, c = (q & 7) * 16;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) s += red[t][c + u];
    part[t][q & 7] = s;
  }
  __syncthreads();
  if (threadIdx.x < NT) {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += part[threadIdx.x][u];
    out[threadIdx.x] = s;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------- prologue
__global__ void __launch_bounds__(EG_THREADS)
    k_eg_prologue(lb_geom g, int64_t BN, const lb_ctrl* __restrict__ ctrl, const double* __restrict__ win,
                  const float* __restrict__ xnode, const int32_t* __restrict__ ptype, int H, int n_vels, int homogeneous,
                  int n_attr, const float* __restrict__ w_emb, const float* __restrict__ b_emb, float* __restrict__ h,
                  float* __restrict__ x32, float* __restrict__ vel, float* __restrict__ nattr) {
  if (ctrl->overflow_step >= 0) return;
  __shared__ float xin[EG_TN][20];
  const int64_t base = (int64_t)blockIdx.x * EG_TN;
  const int node_in = n_vels + (homogeneous ? 0 : 9);
  const int dim = g.dim, K = g.isl - 1;
  if (threadIdx.x < EG_TN) {
    const int t = threadIdx.x;
    const int64_t i = base + t;
    if (i < BN) {
      const float* x = xnode + i * EG_KPAD;
      // |v_k| of the normalised velocities (egnn.py:343-349): sum of squares over dim, then sqrt
      for (int k = 0; k < n_vels; ++k) {
        const float v0 = x[k * dim], v1 = x[k * dim + 1], v2 = dim == 3 ? x[k * dim + 2] : 0.f;
        float s = v0 * v0 + v1 * v1;
        if (dim == 3) s = s + v2 * v2;
        xin[t][k] = sqrtf(s);
      }
      if (!homogeneous) {
        const int pt = ptype[i];  // jax.nn.one_hot: an index outside [0, 9) (PAD_VALUE -1) gives a zero row
        for (int j = 0; j < 9; ++j) xin[t][n_vels + j] = j == pt ? 1.f : 0.f;
      }
      // newest positions in fp32 (features["abs_pos"][:, -1] under the fp32 policy)
      const int step = ctrl->step;
      float* xo = x32 + i * 4;
      xo[3] = 0.f;
      xo[2] = 0.f;
      for (int d = 0; d < dim; ++d) xo[d] = (float)lb_pos(win, g, BN, step, K, d, i);
      // un-normalised last velocity (egnn.py:378-380): vel_hist[:, -1] * std + mean
      float* vo = vel + i * 4;
      vo[3] = 0.f;
      vo[2] = 0.f;
      for (int d = 0; d < dim; ++d) vo[d] = x[(K - 1) * dim + d] * (float)g.vel_std[d] + (float)g.vel_mean[d];
      // node attribute |force| (egnn.py:334-338)
      if (n_attr) {
        const int c = K * dim + (g.has_vel_mag ? K : 0) + (g.has_bound ? 2 * dim : 0);
        const float f0 = x[c], f1 = x[c + 1], f2 = dim == 3 ? x[c + 2] : 0.f;
        float s = f0 * f0 + f1 * f1;
        if (dim == 3) s = s + f2 * f2;
        nattr[i] = sqrtf(s);
      }
    }
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= H) return;
  const float b = b_emb[j];
  for (int t = 0; t < EG_TN; ++t) {
    const int64_t i = base + t;
    if (i >= BN) break;
    float acc = 0.f;
    for (int k = 0; k < node_in; ++k) acc += xin[t][k] * w_emb[k * H + j];
    h[i * H + j] = acc + b;
  }
}

// ------------------------------------------------------------------------ reverse edges
// Edge e = (r, s) almost always has a transpose (s, r), found by binary search in row s (senders ascending inside a row:
// lb_neighbor.hip).  A pair within one rounding of the cutoff can be an edge in one direction only (lb_internal.h:
// lbk_edge_rev): e gets rev = -1 - row r's slot k = (r, s) has no edge sent by r to s - and goes on the orphan list,
// since s does send e.  orph[0] is zero on entry.
__global__ void k_eg_rev(const lb_ctrl* __restrict__ ctrl, int64_t cap, const int32_t* __restrict__ row_ptr,
                         const int32_t* __restrict__ senders, const int32_t* __restrict__ receivers,
                         int32_t* __restrict__ rev, int32_t* __restrict__ orph) {
  if (ctrl->overflow_step >= 0) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int E = ctrl->n_edges_total;
  if (e >= E || e >= cap) return;
  const int r = receivers[e], s = senders[e];
  int lo = row_ptr[s], hi = row_ptr[s + 1];
  lo = lo < E ? lo : E;
  hi = hi < E ? hi : E;
  int found = -1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int v = senders[mid];
    if (v == r) {
      found = mid;
      break;
    }
    if (v < r) lo = mid + 1;
    else hi = mid;
  }
  if (found < 0) orph[1 + atomicAdd(orph, 1)] = (int32_t)e;   // at most E < cap appends
  rev[e] = found;
}

int lbk_edge_rev(lb_engine* e, int32_t* rev, int32_t* orph) {
  const int64_t ecap = (int64_t)e->e_cap * e->g.B;
  const unsigned nb = (unsigned)((ecap + 255) / 256);
  LB_HIP(hipMemsetAsync(orph, 0, sizeof(int32_t), e->stream));
  hipLaunchKernelGGL(k_eg_rev, dim3(nb ? nb : 1), dim3(256), 0, e->stream, e->ctrl, ecap, e->row_ptr, e->senders,
                     e->receivers, rev, orph);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

// -------------------------------------------------------------------- node projection
// P[i] = [h_i W0[0:H] | h_i W0[H:2H]]: the sender and receiver blocks of the first edge Linear, once per node.
__global__ void __launch_bounds__(EG_THREADS)
    k_eg_proj(int64_t BN, const lb_ctrl* __restrict__ ctrl, int H, const float* __restrict__ h,
              const float* __restrict__ w0, float* __restrict__ p) {
  if (ctrl->overflow_step >= 0) return;
  __shared__ float hs[EG_TN][EG_THREADS];
  const int64_t base = (int64_t)blockIdx.x * EG_TN;
  const int j = threadIdx.x;
  for (int t = 0; t < EG_TN; ++t) {
    const int64_t i = base + t;
    hs[t][j] = (i < BN && j < H) ? h[i * H + j] : 0.f;
  }
  __syncthreads();
  if (j >= H) return;
  float as[EG_TN], ar[EG_TN];
#pragma unroll
  for (int t = 0; t < EG_TN; ++t) as[t] = ar[t] = 0.f;
  for (int k = 0; k < H; ++k) {
    const float ws = w0[k * H + j], wr = w0[(H + k) * H + j];
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) {
      as[t] += hs[t][k] * ws;
      ar[t] += hs[t][k] * wr;
    }
  }
#pragma unroll
  for (int t = 0; t < EG_TN; ++t) {
    const int64_t i = base + t;
    if (i < BN) {
      p[i * 2 * H + j] = as[t];
      p[i * 2 * H + H + j] = ar[t];
    }
  }
}

// ----------------------------------------------------------------------------- edges
struct lb_eg_edge_args {
  const lb_ctrl* ctrl;
  int64_t cap;
  int H, dim, periodic, normalize, tanh_pos;
  float box[3];
  const int32_t* senders;
  const int32_t* receivers;
  const float* efeat;  // [E][8], rel_dist at column dim
  const float* x32;
  const float* p;
  const float *w0, *b0, *w1, *b1, *wx0, *bx0, *wx1;
  float* msg;
  float* trans;
};

__global__ void __launch_bounds__(EG_THREADS) k_eg_edge(lb_eg_edge_args a) {
  if (a.ctrl->overflow_step >= 0) return;
  __shared__ float s_cd[EG_TE][4];
  __shared__ float s_rad[EG_TE], s_ea[EG_TE], s_phi[EG_TE];
  __shared__ int s_s[EG_TE], s_r[EG_TE];
  __shared__ float s_a[EG_TE][EG_THREADS];  // first hidden layer, then reused for the position net's reduction
  __shared__ float s_m[EG_TE][EG_THREADS];
  __shared__ float s_part[EG_TE][8];
  const int E = a.ctrl->n_edges_total;
  const int64_t base = (int64_t)blockIdx.x * EG_TE;
  if (base >= E || base >= a.cap) return;
  const int H = a.H, j = threadIdx.x;
  if (j < EG_TE) {
    const int64_t k = base + j;
    const bool ok = k < E && k < a.cap;
    const int s = ok ? a.senders[k] : 0, r = ok ? a.receivers[k] : 0;
    s_s[j] = s;
    s_r[j] = r;
    // _coord2radial (egnn.py:166-173): coord_diff = displacement(x[s], x[r]), radial = sum coord_diff^2
    const float* xs = a.x32 + (int64_t)s * 4;
    const float* xr = a.x32 + (int64_t)r * 4;
    const float c0 = eg_disp(xs[0], xr[0], a.box[0], a.periodic);
    const float c1 = eg_disp(xs[1], xr[1], a.box[1], a.periodic);
    const float c2 = a.dim == 3 ? eg_disp(xs[2], xr[2], a.box[2], a.periodic) : 0.f;
    float rad = c0 * c0 + c1 * c1;
    if (a.dim == 3) rad = rad + c2 * c2;
    float n0 = c0, n1 = c1, n2 = c2;
    if (a.normalize) {
      const float nrm = sqrtf(rad) + 1e-8f;
      n0 = c0 / nrm;
      n1 = c1 / nrm;
      n2 = c2 / nrm;
    }
    s_cd[j][0] = n0;
    s_cd[j][1] = n1;
    s_cd[j][2] = n2;
    s_rad[j] = rad;
    s_ea[j] = ok ? a.efeat[k * 8 + a.dim] : 0.f;
  }
  __syncthreads();
  // first edge Linear: [h_s | h_r | radial | rel_dist] W0 + b0, the node blocks from the projection
  if (j < H) {
    const float wrad = a.w0[(2 * H) * H + j], wea = a.w0[(2 * H + 1) * H + j], b0 = a.b0[j];
    for (int t = 0; t < EG_TE; ++t) {
      const float z = a.p[(int64_t)s_s[t] * 2 * H + j] + a.p[(int64_t)s_r[t] * 2 * H + H + j];
      s_a[t][j] = eg_silu(z + s_rad[t] * wrad + s_ea[t] * wea + b0);
    }
  }
  __syncthreads();
  // second edge Linear (activate_final=True): m = silu(a W1 + b1)
  float acc[EG_TE];
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TE; ++t) acc[t] = 0.f;
    for (int k = 0; k < H; ++k) {
      const float w = a.w1[k * H + j];
#pragma unroll
      for (int t = 0; t < EG_TE; ++t) acc[t] += s_a[t][k] * w;
    }
    const float b1 = a.b1[j];
#pragma unroll
    for (int t = 0; t < EG_TE; ++t) {
      const float m = eg_silu(acc[t] + b1);
      s_m[t][j] = m;
      const int64_t k = base + t;
      if (k < E && k < a.cap) a.msg[k * H + j] = m;
    }
  }
  __syncthreads();
  // position net (egnn.py:95-104): phi = silu(m Wx0 + bx0) . wx1 [tanh]
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TE; ++t) acc[t] = 0.f;
    for (int k = 0; k < H; ++k) {
      const float w = a.wx0[k * H + j];
#pragma unroll
      for (int t = 0; t < EG_TE; ++t) acc[t] += s_m[t][k] * w;
    }
    const float bx = a.bx0[j], w1 = a.wx1[j];
#pragma unroll
    for (int t = 0; t < EG_TE; ++t) s_a[t][j] = eg_silu(acc[t] + bx) * w1;
  } else {
#pragma unroll
    for (int t = 0; t < EG_TE; ++t) s_a[t][j] = 0.f;
  }
  eg_rowsum<EG_TE>(s_a, s_part, s_phi);
  // trans = coord_diff * phi (egnn.py:119-126)
  if (j < EG_TE) {
    const int64_t k = base + j;
    if (k < E && k < a.cap) {
      float phi = s_phi[j];
      if (a.tanh_pos) phi = tanhf(phi);
      reinterpret_cast<f32x4*>(a.trans)[k] = f32x4{s_cd[j][0] * phi, s_cd[j][1] * phi, s_cd[j][2] * phi, 0.f};
    }
  }
}

// ----------------------------------------------------------------------------- nodes
struct lb_eg_node_args {
  const lb_ctrl* ctrl;
  int64_t BN;
  int H, dim, periodic, residual, n_attr;
  float box[3];
  const int32_t* row_ptr;
  const int32_t* rev;
  const int32_t* orph;
  const int32_t* senders;
  const float* msg;
  const float* trans;
  const float* nattr;
  const float* vel;
  float* h;    // in / out
  float* x32;  // in / out
  const float *wn0, *bn0, *wn1, *bn1, *wv0, *bv0, *wv1;
};

__global__ void __launch_bounds__(EG_THREADS) k_eg_node(lb_eg_node_args a) {
  if (a.ctrl->overflow_step >= 0) return;
  __shared__ float s_h[EG_TN][EG_THREADS];
  __shared__ float s_g[EG_TN][EG_THREADS];  // aggregated messages, then the node MLP's hidden layer
  __shared__ float s_u[EG_TN][EG_THREADS];  // updated h, then the velocity net's reduction
  __shared__ float s_part[EG_TN][8];
  __shared__ float s_psi[EG_TN];
  const int64_t base = (int64_t)blockIdx.x * EG_TN;
  const int H = a.H, j = threadIdx.x;
  const int E = a.ctrl->n_edges_total;
  // h and agg = segment_sum of the messages over receivers (CSR row order)
  for (int t = 0; t < EG_TN; ++t) {
    const int64_t i = base + t;
    float hv = 0.f, g = 0.f;
    if (i < a.BN && j < H) {
      hv = a.h[i * H + j];
      int k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
      k0 = k0 < E ? k0 : E;
      k1 = k1 < E ? k1 : E;
      for (int k = k0; k < k1; ++k) g += a.msg[(int64_t)k * H + j];
    }
    s_h[t][j] = hv;
    s_g[t][j] = g;
  }
  __syncthreads();
  float acc[EG_TN];
  float u[EG_TN];
  // node MLP first Linear: [h | agg | |force|] Wn0 + bn0, silu
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) acc[t] = 0.f;
    for (int k = 0; k < H; ++k) {
      const float w = a.wn0[k * H + j];
#pragma unroll
      for (int t = 0; t < EG_TN; ++t) acc[t] += s_h[t][k] * w;
    }
    for (int k = 0; k < H; ++k) {
      const float w = a.wn0[(H + k) * H + j];
#pragma unroll
      for (int t = 0; t < EG_TN; ++t) acc[t] += s_g[t][k] * w;
    }
    if (a.n_attr) {
      const float w = a.wn0[(2 * H) * H + j];
#pragma unroll
      for (int t = 0; t < EG_TN; ++t) {
        const int64_t i = base + t;
        acc[t] += (i < a.BN ? a.nattr[i] : 0.f) * w;
      }
    }
    const float b = a.bn0[j];
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) u[t] = eg_silu(acc[t] + b);
  }
  __syncthreads();  // every thread has read s_g
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) s_g[t][j] = u[t];
  }
  __syncthreads();
  // second Linear (no final activation) + residual (egnn.py:160-164)
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) acc[t] = 0.f;
    for (int k = 0; k < H; ++k) {
      const float w = a.wn1[k * H + j];
#pragma unroll
      for (int t = 0; t < EG_TN; ++t) acc[t] += s_g[t][k] * w;
    }
    const float b = a.bn1[j];
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) {
      float hn = acc[t] + b;
      if (a.residual) hn = s_h[t][j] + hn;
      s_u[t][j] = hn;
      const int64_t i = base + t;
      if (i < a.BN) a.h[i * H + j] = hn;
    }
  }
  __syncthreads();
  // velocity net on the UPDATED h: psi = silu(h' Wv0 + bv0) . wv1
  if (j < H) {
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) acc[t] = 0.f;
    for (int k = 0; k < H; ++k) {
      const float w = a.wv0[k * H + j];
#pragma unroll
      for (int t = 0; t < EG_TN; ++t) acc[t] += s_u[t][k] * w;
    }
  }
  __syncthreads();  // every thread has read s_u
  {
    const float b = j < H ? a.bv0[j] : 0.f, w1 = j < H ? a.wv1[j] : 0.f;
#pragma unroll
    for (int t = 0; t < EG_TN; ++t) s_u[t][j] = j < H ? eg_silu(acc[t] + b) * w1 : 0.f;
  }
  eg_rowsum<EG_TN>(s_u, s_part, s_psi);
  // positions: shift by the sender sum of trans (rev[k] over row i, then the orphans sent by i = the edges whose sender
  // is i), then by psi * vel
  if (j < EG_TN) {
    const int64_t i = base + j;
    if (i < a.BN) {
      int k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
      k0 = k0 < E ? k0 : E;
      k1 = k1 < E ? k1 : E;
      float d0 = 0.f, d1 = 0.f, d2 = 0.f;
      for (int k = k0; k < k1; ++k) {
        const int e = a.rev[k];
        if (e < 0) continue;   // i does not send to the sender of slot k
        const f32x4 tr = reinterpret_cast<const f32x4*>(a.trans)[e];
        d0 += tr[0];
        d1 += tr[1];
        d2 += tr[2];
      }
      lb_for_orphans(a.orph, a.senders, i, [&](int e) {
        const f32x4 tr = reinterpret_cast<const f32x4*>(a.trans)[e];
        d0 += tr[0];
        d1 += tr[1];
        d2 += tr[2];
      });
      const float psi = s_psi[j];
      float* x = a.x32 + i * 4;
      const float* v = a.vel + i * 4;
      x[0] = eg_shift(eg_shift(x[0], d0, a.box[0], a.periodic), psi * v[0], a.box[0], a.periodic);
      x[1] = eg_shift(eg_shift(x[1], d1, a.box[1], a.periodic), psi * v[1], a.box[1], a.periodic);
      if (a.dim == 3) x[2] = eg_shift(eg_shift(x[2], d2, a.box[2], a.periodic), psi * v[2], a.box[2], a.periodic);
    }
  }
}

// -------------------------------------------------------------------------- integrator
// case.integrate returns pred["pos"] (case.py:235-237); kinematic particles take their targets, the window advances by
// one frame, the prediction is stored (rollout.py:61-73,165-167).  The last workgroup advances the step counter.
__global__ void k_eg_integrate(lb_geom g, int64_t BN, double* __restrict__ win, lb_ctrl* __restrict__ ctrl,
                               int32_t* __restrict__ blocks_done, const int32_t* __restrict__ ptype,
                               const float* __restrict__ x32, const double* __restrict__ traj, int T,
                               double* __restrict__ pred, int pred_T) {
  if (ctrl->overflow_step >= 0) return;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int step = ctrl->step;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(blocks_done, 1) == (int)gridDim.x - 1) {
      *blocks_done = 0;
      ctrl->step = step + 1;
    }
  }
  if (gi >= BN) return;
  const int b = (int)(gi / g.N), i = (int)(gi % g.N);
  const int pt = ptype[gi];
  const bool kinematic = (pt == 1) || (pt == 2) || (pt == -1);  // utils.py:28-35
  const int slot_new = (step + g.isl) % g.isl;
  int tf = g.isl + step;
  if (tf > T - 1) tf = T - 1;  // JAX clamps the out-of-range gather (rollout.py:159)
  for (int d = 0; d < g.dim; ++d) {
    const double out = kinematic ? traj[(gi * T + tf) * g.dim + d] : (double)x32[gi * 4 + d];
    win[((int64_t)slot_new * g.dim + d) * BN + gi] = out;
    if (pred && step < pred_T) pred[(((int64_t)b * pred_T + step) * g.N + i) * g.dim + d] = out;
  }
}

// ------------------------------------------------------------------------------- model
static int eg_ensure_edges(lb_egnn* m) {
  lb_engine* e = m->eng;
  if (m->e_alloc >= e->e_alloc) return LB_OK;
  return lb_regrow(e->stream, &m->e_alloc, e->e_alloc, [&](int64_t cap) {
    const size_t n = (size_t)cap;
    LB_TRY(m->mem.get(&m->msg, n * m->desc.hidden));
    LB_TRY(m->mem.get(&m->trans, n * 4));
    LB_TRY(m->mem.get(&m->rev, n));
    return m->mem.get(&m->orph, n + 1);
  });
}

extern "C" void lb_egnn_destroy(lb_egnn* m) {
  delete m;
}

// the node-sized buffers of a model or a view
static int eg_alloc_nodes(lb_egnn* m) {
  const int64_t BN = m->eng->BN, H = m->desc.hidden;
  LB_TRY(m->mem.get(&m->xnode, (size_t)BN * EG_KPAD));
  LB_TRY(m->mem.get(&m->h, (size_t)BN * H));
  LB_TRY(m->mem.get(&m->p, (size_t)BN * 2 * H));
  LB_TRY(m->mem.get(&m->x32, (size_t)BN * 4));
  LB_TRY(m->mem.get(&m->vel, (size_t)BN * 4));
  return m->mem.get(&m->nattr, (size_t)BN);
}

static int64_t eg_n_floats(const lb_egnn_desc* d, int node_in, int n_attr) {
  const int64_t H = d->hidden;
  const int64_t layer = (2 * H + 2) * H + H + H * H + H      // edge MLP
                        + (2 * H + n_attr) * H + H + H * H + H  // node MLP
                        + 2 * (H * H + H + H);                  // position and velocity nets
  return (int64_t)node_in * H + H + d->num_mp_steps * layer;
}

// the layer pointers into a weight blob in lb_egnn_create's layout (include/lbhip.h)
static void eg_carve(lb_egnn* m, const float* q) {
  const int64_t H = m->desc.hidden, node_in = m->node_in, n_attr = m->n_attr;
  auto take = [&](int64_t n) {
    const float* r = q;
    q += n;
    return r;
  };
  m->w_emb = take(node_in * H);
  m->b_emb = take(H);
  m->layers.resize(m->desc.num_mp_steps);
  for (auto& l : m->layers) {
    l.w0 = take((2 * H + 2) * H);
    l.b0 = take(H);
    l.w1 = take(H * H);
    l.b1 = take(H);
    l.wn0 = take((2 * H + n_attr) * H);
    l.bn0 = take(H);
    l.wn1 = take(H * H);
    l.bn1 = take(H);
    l.wx0 = take(H * H);
    l.bx0 = take(H);
    l.wx1 = take(H);
    l.wv0 = take(H * H);
    l.bv0 = take(H);
    l.wv1 = take(H);
  }
}

extern "C" int lb_egnn_create(lb_engine* e, const lb_egnn_desc* d, const float* w, int64_t n_floats, lb_egnn** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->hidden < 16 || d->hidden > 128 || d->hidden % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "EGNN hidden size %d: a multiple of 16 up to 128 is built", d->hidden);
  if (d->num_mp_steps < 1 || d->num_mp_steps > 64) return lb_fail(LB_ERR_ARG, "bad num_mp_steps %d", d->num_mp_steps);
  if (d->n_vels < 1 || d->n_vels > 9) return lb_fail(LB_ERR_ARG, "bad n_vels %d (1 .. 9)", d->n_vels);
  if (d->n_vels != e->g.isl - 1) return lb_fail(LB_ERR_ARG, "n_vels %d != input_seq_length-1", d->n_vels);
  const int node_in = d->n_vels + (d->homogeneous ? 0 : 9);
  const int n_attr = e->g.force_kind != LB_FORCE_NONE ? 1 : 0;
  const int64_t need = eg_n_floats(d, node_in, n_attr);
  if (n_floats != need) return lb_fail(LB_ERR_ARG, "EGNN weights: expected %lld floats, got %lld", (long long)need,
                                       (long long)n_floats);
  lb_egnn* m = new lb_egnn();
  m->desc = *d;
  m->eng = e;
  m->node_in = node_in;
  m->n_attr = n_attr;
  int rc = m->mem.get(&m->blob, (size_t)n_floats);
  if (!rc) {
    const hipError_t he = hipMemcpy(m->blob, w, sizeof(float) * n_floats, hipMemcpyHostToDevice);
    if (he != hipSuccess) rc = lb_fail(LB_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(he));
  }
  if (!rc) rc = eg_alloc_nodes(m);
  if (rc) {
    lb_egnn_destroy(m);
    return rc;
  }
  eg_carve(m, m->blob);
  *out = m;
  return LB_OK;
}

// Training (lb_train_egnn.h): a model that runs on a weight blob the caller owns and keeps in lb_egnn_create's layout (the
// training handle's device weights, which AdamW updates in place).  Nothing is copied; lb_egnn_destroy leaves the blob alone.
int lbk_egnn_view_create(lb_engine* e, const lb_egnn_desc* d, const float* w_dev, lb_egnn** out) {
  *out = nullptr;
  const int node_in = d->n_vels + (d->homogeneous ? 0 : 9);
  lb_egnn* m = new lb_egnn();
  m->desc = *d;
  m->eng = e;
  m->node_in = node_in;
  m->n_attr = e->g.force_kind != LB_FORCE_NONE ? 1 : 0;
  if (const int rc = eg_alloc_nodes(m)) {
    lb_egnn_destroy(m);
    return rc;
  }
  eg_carve(m, w_dev);
  *out = m;
  return LB_OK;
}

extern "C" int lb_egnn_set_tap(lb_egnn* m, float* h_out_dev, float* pos_out_dev) {
  if (!m) return lb_fail(LB_ERR_ARG, "null model");
  m->tap_h = h_out_dev;
  m->tap_x = pos_out_dev;
  return LB_OK;
}

static int lbk_egnn_forward(lb_engine* e, lb_egnn* m) {
  hipStream_t s = e->stream;
  const int64_t BN = e->BN;
  const int H = m->desc.hidden, dim = e->g.dim;
  LB_TRY(eg_ensure_edges(m));
  const int64_t ecap = (int64_t)e->e_cap * e->g.B;
  const unsigned nb_t = (unsigned)((BN + EG_TN - 1) / EG_TN);
  const unsigned nb_te = (unsigned)((ecap + EG_TE - 1) / EG_TE);
  auto tap = [&](int slot) -> int {
    if (m->tap_h)
      LB_HIP(hipMemcpyAsync(m->tap_h + (size_t)slot * BN * H, m->h, sizeof(float) * BN * H, hipMemcpyDeviceToDevice, s));
    if (m->tap_x) LB_TRY(lb_export_rows(e, m->x32, m->tap_x + (size_t)slot * BN * dim, false));
    return LB_OK;
  };
  lb_tic(e, LB_T_NODEFEAT);
  LB_TRY(lbk_node_features_raw(e, m->xnode, EG_KPAD));
  hipLaunchKernelGGL(k_eg_prologue, dim3(nb_t), dim3(EG_THREADS), 0, s, e->g, BN, e->ctrl, e->win, m->xnode, e->ptype, H,
                     m->desc.n_vels, m->desc.homogeneous, m->n_attr, m->w_emb, m->b_emb, m->h, m->x32, m->vel, m->nattr);
  LB_TRY(lbk_edge_rev(e, m->rev, m->orph));
  lb_toc(e);
  LB_HIP(hipGetLastError());
  LB_TRY(tap(0));
  float box[3] = {(float)e->g.box[0], (float)e->g.box[1], (float)e->g.box[2]};
  for (int k = 0; k < m->desc.num_mp_steps; ++k) {
    const lb_egnn_layer& l = m->layers[k];
    lb_tic(e, LB_T_EDGE_MLP);
    hipLaunchKernelGGL(k_eg_proj, dim3(nb_t), dim3(EG_THREADS), 0, s, BN, e->ctrl, H, m->h, l.w0, m->p);
    lb_eg_edge_args ea{};
    ea.ctrl = e->ctrl;
    ea.cap = ecap;
    ea.H = H;
    ea.dim = dim;
    ea.periodic = e->g.periodic;
    ea.normalize = m->desc.normalize;
    ea.tanh_pos = m->desc.tanh_pos;
    for (int d = 0; d < 3; ++d) ea.box[d] = box[d];
    ea.senders = e->senders;
    ea.receivers = e->receivers;
    ea.efeat = e->efeat;
    ea.x32 = m->x32;
    ea.p = m->p;
    ea.w0 = l.w0;
    ea.b0 = l.b0;
    ea.w1 = l.w1;
    ea.b1 = l.b1;
    ea.wx0 = l.wx0;
    ea.bx0 = l.bx0;
    ea.wx1 = l.wx1;
    ea.msg = m->msg;
    ea.trans = m->trans;
    hipLaunchKernelGGL(k_eg_edge, dim3(nb_te ? nb_te : 1), dim3(EG_THREADS), 0, s, ea);
    lb_toc(e);
    lb_tic(e, LB_T_NODE_MLP);
    lb_eg_node_args na{};
    na.ctrl = e->ctrl;
    na.BN = BN;
    na.H = H;
    na.dim = dim;
    na.periodic = e->g.periodic;
    na.residual = m->desc.residual;
    na.n_attr = m->n_attr;
    for (int d = 0; d < 3; ++d) na.box[d] = box[d];
    na.row_ptr = e->row_ptr;
    na.rev = m->rev;
    na.orph = m->orph;
    na.senders = e->senders;
    na.msg = m->msg;
    na.trans = m->trans;
    na.nattr = m->nattr;
    na.vel = m->vel;
    na.h = m->h;
    na.x32 = m->x32;
    na.wn0 = l.wn0;
    na.bn0 = l.bn0;
    na.wn1 = l.wn1;
    na.bn1 = l.bn1;
    na.wv0 = l.wv0;
    na.bv0 = l.bv0;
    na.wv1 = l.wv1;
    hipLaunchKernelGGL(k_eg_node, dim3(nb_t), dim3(EG_THREADS), 0, s, na);
    lb_toc(e);
    LB_HIP(hipGetLastError());
    LB_TRY(tap(k + 1));
  }
  return LB_OK;
}

extern "C" int lb_egnn_forward(lb_engine* e, lb_egnn* m, double* pos_out_dev) {
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  LB_TRY(lb_forward_check(e, "lb_egnn_forward"));
  LB_TRY(lbk_egnn_forward(e, m));
  if (pos_out_dev) LB_TRY(lb_export_rows(e, m->x32, pos_out_dev, true));
  LB_HIP(hipStreamSynchronize(e->stream));
  return LB_OK;
}

// one rollout step's model + integrator (lb_enqueue_step has set e->integ_job)
static int eg_forward_thunk(lb_engine* e, void* model) {
  lb_egnn* m = (lb_egnn*)model;
  LB_TRY(lbk_egnn_forward(e, m));
  const lb_integ_job& j = e->integ_job;
  lb_tic(e, LB_T_INTEGRATE);
  hipLaunchKernelGGL(k_eg_integrate, dim3((unsigned)((e->BN + 255) / 256)), dim3(256), 0, e->stream, e->g, e->BN, e->win,
                     e->ctrl, e->blocks_done, e->ptype, m->x32, j.traj, j.T, j.pred, j.pred_T);
  lb_toc(e);
  LB_HIP(hipGetLastError());
  e->integ_done = true;
  return LB_OK;
}

extern "C" int lb_egnn_rollout(lb_engine* e, lb_egnn* m, const double* traj_dev, int32_t T, int32_t n_steps,
                               double* pred_out_dev, int32_t* n_realloc_out) {
  if (!traj_dev || !pred_out_dev) return lb_fail(LB_ERR_ARG, "null argument");
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  return lb_rollout_generic(e, eg_forward_thunk, m, traj_dev, T, n_steps, pred_out_dev, n_realloc_out);
}

// one forward as lb_egnn_forward runs it (no export).  Host-synchronous.
int lbk_egnn_train_forward(lb_engine* e, lb_egnn* m, lb_egnn_state* st) {
  if (e->g.force_kind == LB_FORCE_BUFFER && !e->force)
    return lb_fail(LB_ERR_STATE, "LB_FORCE_BUFFER engine: call lb_set_force first");
  LB_TRY(lbk_egnn_forward(e, m));
  LB_HIP(hipStreamSynchronize(e->stream));
  st->xnode = m->xnode;
  st->vel = m->vel;
  st->nattr = m->nattr;
  st->rev = m->rev;
  st->orph = m->orph;
  return LB_OK;
}
