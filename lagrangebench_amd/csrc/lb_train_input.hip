// lb_train_input.hip - the input of one training step made on the device, in one launch: window gather from the
// device-resident dataset, random-walk noise, shift, the (B, N, T, dim) trajectory and the three training targets.
//
// Reference functions replaced (paths relative to the reference repo):
//   H5Dataset.get_window (+ numpy_collate)       lagrangebench/data/data.py:227-257
//   add_gns_noise                                lagrangebench/train/strats.py:12-58
//   _get_random_walk_noise_for_pos_sequence      lagrangebench/train/strats.py:61-83
//   _compute_target                              lagrangebench/case_setup/case.py:142-160
//   _preprocess, noise + target part             lagrangebench/case_setup/case.py:162-178
//
// Dataset layout in HBM: pos[traj][t][i][d] in the file's dtype (the order of the H5 `position` arrays, padded to N
// particles per trajectory), ptype[traj][i].  One thread per particle of the batch; a workgroup is one wave.  The lanes of a
// wave read one frame with unit stride (dim values per lane, neighbours adjacent).  The output rows (T * dim doubles per
// particle) of a wave's 64 particles are ONE contiguous span of the (B, N, T, dim) tensor: the rows are staged in LDS and
// the span is stored with unit stride across the lanes.  Targets are (B, N, dim): dim doubles per lane, neighbours adjacent.
//
// Random numbers: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), key = (seed lo, seed hi), counter =
// (step, global slot, particle, c).  Counter c yields four N(0, 1) values: with u_j = (x_j + 0.5) * 2^-32,
// n_0 = r_01 cos(t_01), n_1 = r_01 sin(t_01), n_2 = r_23 cos(t_23), n_3 = r_23 sin(t_23), r_ab = sqrt(-2 log u_a),
// t_ab = 2 pi u_b, all fp64.  Draw q = k * dim + d (velocity slot k, component d) is value q % 4 of counter q / 4: the noise
// of a slot depends on (seed, step, global slot, particle, frame, component) and on nothing else.
#include "lb_device.h"

#define LB_TB_WAVE 64

struct lb_tb_sel {  // the B samples of the batch, by value: no host-to-device copy per step
  int32_t traj[LB_TRAIN_BATCH_MAX], t0[LB_TRAIN_BATCH_MAX];
  uint32_t slot[LB_TRAIN_BATCH_MAX];
};

struct lb_tb_args {
  const void* pos;         // [n_traj][seq_len][N][dim] float or double
  const int32_t* ptype;    // [n_traj][N]
  int32_t pos_f64, seq_len, T, b0, noisy, periodic;
  uint32_t k0, k1, step;
  double scale;            // noise_std / sqrt(isl - 1)
  double nbox[3];          // the case's box as given (the noise is shifted in fp64, before any rounding to float)
  double* traj_out;        // [B][N][T][dim]
  int32_t* ptype_out;      // [B][N]
  double* t_acc;           // [B][N][dim] each
  double* t_vel;
  double* t_pos;
  double* normals;         // [B][N][isl-1][dim] or null
};

__device__ __forceinline__ void lb_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

__device__ __forceinline__ void lb_box_muller(uint32_t xa, uint32_t xb, double& zc, double& zs) {
  const double ua = ((double)xa + 0.5) * 2.3283064365386963e-10;  // 2^-32
  const double ub = ((double)xb + 0.5) * 2.3283064365386963e-10;
  const double r = sqrt(-2.0 * log(ua));
  const double t = 6.283185307179586 * ub;
  zc = r * cos(t);
  zs = r * sin(t);
}

__global__ void __launch_bounds__(LB_TB_WAVE) k_train_batch(lb_geom g, int64_t BN, lb_tb_sel sel, lb_tb_args a) {
  extern __shared__ double s_rows[];  // [64][T * dim]
  const int tid = threadIdx.x;
  const int64_t gi0 = (int64_t)blockIdx.x * LB_TB_WAVE, gi = gi0 + tid;
  const int TD = a.T * g.dim, K = g.isl - 1;
  if (gi < BN) {
    const int b = (int)(gi / g.N), i = (int)(gi % g.N);
    const int tr = sel.traj[b], t0 = sel.t0[b];
    const int32_t pt = a.ptype[(int64_t)tr * g.N + i];
    a.ptype_out[gi] = pt;
    const bool kin = pt == 1 || pt == 2 || pt == LB_PAD_TYPE;  // utils.get_kinematic_mask
    double vel[3] = {0.0, 0.0, 0.0}, nz[3] = {0.0, 0.0, 0.0}, p3[3][3], z4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int f = 0; f < a.T; ++f) {
      const int64_t src = (((int64_t)tr * a.seq_len + (t0 + f)) * g.N + i) * g.dim;
      for (int d = 0; d < g.dim; ++d) {
        double x = a.pos_f64 ? ((const double*)a.pos)[src + d] : (double)((const float*)a.pos)[src + d];
        x = lb_r(x, g.f32);  // case.py:169
        if (a.noisy) {
          if (f >= 1 && f <= K) {  // frame f carries the running sums up to velocity slot f - 1
            const int q = (f - 1) * g.dim + d;
            if ((q & 3) == 0) {  // q runs 0, 1, 2, ...: a new counter every fourth draw
              uint32_t r[4];
              lb_philox4x32_10(a.step, sel.slot[b], (uint32_t)i, (uint32_t)(q >> 2), a.k0, a.k1, r);
              lb_box_muller(r[0], r[1], z4[0], z4[1]);
              lb_box_muller(r[2], r[3], z4[2], z4[3]);
            }
            const int l = q & 3;
            const double z = l == 0 ? z4[0] : l == 1 ? z4[1] : l == 2 ? z4[2] : z4[3];
            if (a.normals) a.normals[(gi * K + (f - 1)) * g.dim + d] = z;
            vel[d] += z * a.scale;
            nz[d] += vel[d];
          }
          x = lb_r(lb_shift1(x, kin ? 0.0 : nz[d], a.nbox[d], a.periodic, 0), g.f32);
        }
        s_rows[tid * TD + f * g.dim + d] = x;
        if (f == a.b0) p3[0][d] = x;
        if (f == a.b0 + 1) p3[1][d] = x;
        if (f == a.b0 + 2) p3[2][d] = x;
      }
    }
    for (int d = 0; d < g.dim; ++d) {  // case.py:142-160
      const double cur_v = lb_disp1(p3[1][d], p3[0][d], g.box[d], g.half_box[d], g.periodic, g.f32);
      const double nxt_v = lb_disp1(p3[2][d], p3[1][d], g.box[d], g.half_box[d], g.periodic, g.f32);
      const double acc = lb_r(nxt_v - cur_v, g.f32);
      a.t_acc[gi * g.dim + d] = lb_r(lb_r(acc - g.acc_mean[d], g.f32) / g.acc_std[d], g.f32);
      a.t_vel[gi * g.dim + d] = lb_r(lb_r(nxt_v - g.vel_mean[d], g.f32) / g.vel_std[d], g.f32);
      a.t_pos[gi * g.dim + d] = p3[2][d];
    }
  }
  __syncthreads();
  const int64_t rows = BN - gi0 < LB_TB_WAVE ? BN - gi0 : LB_TB_WAVE;
  const int n = (int)rows * TD;
  double* __restrict__ out = a.traj_out + gi0 * TD;
  for (int k = tid; k < n; k += LB_TB_WAVE) out[k] = s_rows[k];
}

extern "C" int lb_train_batch(lb_engine* e, const void* pos_dev, int32_t pos_is_f64, const int32_t* ptype_dev, int32_t n_traj,
                              int32_t seq_len, const int32_t* traj_host, const int32_t* t0_host, const int32_t* slot_host,
                              uint64_t seed, int64_t step, double noise_std, int32_t T, int32_t unroll_steps,
                              double* traj_out_dev, int32_t* ptype_out_dev, double* target_acc_dev, double* target_vel_dev,
                              double* target_pos_dev, double* want_normals_dev) {
  if (!e || !pos_dev || !ptype_dev || !traj_host || !t0_host || !slot_host || !traj_out_dev || !ptype_out_dev ||
      !target_acc_dev || !target_vel_dev || !target_pos_dev)
    return lb_fail(LB_ERR_ARG, "null argument");
  const lb_geom& g = e->g;
  if (g.B > LB_TRAIN_BATCH_MAX)
    return lb_fail(LB_ERR_ARG, "lb_train_batch: batch %d (at most %d samples per call)", g.B, LB_TRAIN_BATCH_MAX);
  if (unroll_steps < 0 || T < g.isl + 1 + unroll_steps)
    return lb_fail(LB_ERR_ARG, "lb_train_batch: T=%d frames, the targets of unroll_steps=%d need %d", T, unroll_steps,
                   g.isl + 1 + unroll_steps);
  if ((size_t)T * g.dim * LB_TB_WAVE * sizeof(double) > 64 * 1024)
    return lb_fail(LB_ERR_ARG, "lb_train_batch: T=%d frames do not fit the staging buffer", T);
  if (!(noise_std >= 0.0) || step < 0 || n_traj <= 0 || seq_len < T)
    return lb_fail(LB_ERR_ARG, "lb_train_batch: noise_std=%g step=%lld n_traj=%d seq_len=%d T=%d", noise_std, (long long)step,
                   n_traj, seq_len, T);
  lb_tb_sel sel{};
  for (int b = 0; b < g.B; ++b) {
    if (traj_host[b] < 0 || traj_host[b] >= n_traj || t0_host[b] < 0 || t0_host[b] + T > seq_len || slot_host[b] < 0)
      return lb_fail(LB_ERR_ARG, "lb_train_batch: sample %d = (trajectory %d, t0 %d, slot %d) outside %d trajectories of %d frames",
                     b, traj_host[b], t0_host[b], slot_host[b], n_traj, seq_len);
    sel.traj[b] = traj_host[b];
    sel.t0[b] = t0_host[b];
    sel.slot[b] = (uint32_t)slot_host[b];
  }
  lb_tb_args a{};
  a.pos = pos_dev;
  a.ptype = ptype_dev;
  a.pos_f64 = pos_is_f64 != 0;
  a.seq_len = seq_len;
  a.T = T;
  a.b0 = g.isl - 2 + unroll_steps;
  a.noisy = noise_std != 0.0;  // case.py:172: without noise the window is the data, unshifted
  a.periodic = g.periodic;
  a.k0 = (uint32_t)(seed & 0xffffffffu);
  a.k1 = (uint32_t)(seed >> 32);
  a.step = (uint32_t)step;
  a.scale = noise_std / sqrt((double)(g.isl - 1));
  for (int d = 0; d < 3; ++d) a.nbox[d] = d < g.dim ? e->desc.box[d] : 1.0;
  a.traj_out = traj_out_dev;
  a.ptype_out = ptype_out_dev;
  a.t_acc = target_acc_dev;
  a.t_vel = target_vel_dev;
  a.t_pos = target_pos_dev;
  a.normals = a.noisy ? want_normals_dev : nullptr;
  const int nb = (int)((e->BN + LB_TB_WAVE - 1) / LB_TB_WAVE);
  const size_t lds = (size_t)T * g.dim * LB_TB_WAVE * sizeof(double);
  hipLaunchKernelGGL(k_train_batch, dim3(nb), dim3(LB_TB_WAVE), lds, e->stream, g, e->BN, sel, a);
  LB_HIP(hipGetLastError());
  return LB_OK;
}
