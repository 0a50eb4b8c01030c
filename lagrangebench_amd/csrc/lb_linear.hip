// lb_linear.hip - the Linear baseline (forward pass and rollout) on gfx950.
//
// Reference functions replaced (paths relative to the reference repo):
//   Linear.__call__ (concat + hk.Linear)    lagrangebench/models/linear.py:30-42
//   case.integrate for an "acc" output      lagrangebench/case_setup/case.py (the GNS integrator, lb_state.hip)
//   the eval step loop                      lagrangebench/evaluate/rollout.py:125-169
//
// acc_i = [vel_hist | vel_mag | bound | force | float(particle_type_i)] W + b, W (F + 1, dim), b (dim), F = the engine's
// node-feature width.  The engine's node row [BN][64] (lb_features.h) has the reference's concat order, so the rows of W
// are used as given; the type column is not part of the row: it is read from ptype and multiplies row F of W.
//
// Arithmetic: fp32 (runner.py:71-72), no fused multiply-add, every sum in a fixed order: two runs give identical bits, and a
// particle's result does not depend on the batch or on the launch grid.
//
// k_ln_forward: 16 lanes x float4 read one particle's 256-byte row (a wave reads four consecutive rows, 1 KiB, per pass).
// Lane l of a 16-lane group keeps rows 4 l .. 4 l + 3 of W in 12 registers (0 past F), the whole group row F and b; the
// lane's partial dot products are summed over the group by an xor butterfly (8, 4, 2, 1: every lane ends with the same
// bits), lane 0 adds the type term and the bias and stores.  No LDS, no atomics, no scratch.
#include <algorithm>

#include "lb_device.h"

#define LN_KPAD 64   // node feature row stride (vel_hist | vel_mag | bound | force <= 63 columns, + the type column <= 64)
#define LN_WG 256    // 4 waves: 16 rows per workgroup pass

struct lb_linear {
  lb_arena mem;  // owns blob (null in a view) and xnode
  lb_linear_desc desc;
  lb_engine* eng;
  float* blob = nullptr;     // the weights as given: w (n_in, out_dim) row-major, then b (out_dim)
  const float* w = nullptr;  // blob, or the weight blob of the training handle this model is a view of
  float* xnode = nullptr;    // [BN][LN_KPAD]
};

// out[i * ldo + d] = acc_i[d] for the rows i < BN; F feature columns, dim <= 3 outputs
__global__ void __launch_bounds__(LN_WG) k_ln_forward(const lb_ctrl* __restrict__ ctrl, int64_t BN, int F, int dim,
                                                      const float* __restrict__ xnode, const int32_t* __restrict__ ptype,
                                                      const float* __restrict__ w, float* __restrict__ out, int ldo) {
  if (ctrl->overflow_step >= 0) return;
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  // this lane's four rows of W, row F (the type column) and the bias
  float wr[4][3], wt[3], wb[3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int k = 4 * sub + j;
      wr[j][d] = (k < F && d < dim) ? w[k * dim + d] : 0.f;
    }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    wt[d] = d < dim ? w[F * dim + d] : 0.f;
    wb[d] = d < dim ? w[(F + 1) * dim + d] : 0.f;
  }
  const int64_t wave = ((int64_t)blockIdx.x * LN_WG + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * LN_WG) >> 6;
  for (int64_t r0 = wave * 4; r0 < BN; r0 += n_waves * 4) {
    const int64_t i = r0 + grp;
    const bool live = i < BN;   // (the tail: whole 16-lane groups are masked, so the butterfly stays inside live groups)
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (live) x = *reinterpret_cast<const f32x4*>(xnode + i * LN_KPAD + 4 * sub);
    float p[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = ((x[0] * wr[0][d] + x[1] * wr[1][d]) + x[2] * wr[2][d]) + x[3] * wr[3][d];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1)
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] += __shfl_xor(p[d], o);
    if (live && sub == 0) {
      const float ty = (float)ptype[i];
#pragma unroll
      for (int d = 0; d < 3; ++d)
        if (d < dim) out[i * ldo + d] = (p[d] + ty * wt[d]) + wb[d];
    }
  }
}

static int ln_check_desc(const lb_engine* e, const lb_linear_desc* d) {
  if (d->n_in != e->g.node_in + 1 || d->out_dim != e->g.dim)
    return lb_fail(LB_ERR_ARG, "Linear (%d, %d) does not match the case: %d node features + the particle type, dim %d", d->n_in,
                   d->out_dim, e->g.node_in, e->g.dim);
  if (d->n_in > LN_KPAD)
    return lb_fail(LB_ERR_UNSUPPORTED, "Linear with %d inputs: up to %d (one node row) are built", d->n_in, LN_KPAD);
  return LB_OK;
}

extern "C" void lb_linear_destroy(lb_linear* m) {
  delete m;  // (m->mem frees the buffers)
}

// a model on the device weights w_dev (lb_linear_create's layout) that the caller owns: the training handle's view
int lbk_linear_view_create(lb_engine* e, const lb_linear_desc* d, const float* w_dev, lb_linear** out) {
  LB_TRY(ln_check_desc(e, d));
  lb_linear* m = new lb_linear();
  m->desc = *d;
  m->eng = e;
  m->w = w_dev;
  const int rc = m->mem.get(&m->xnode, (size_t)e->BN * LN_KPAD);
  if (rc) {
    lb_linear_destroy(m);
    return rc;
  }
  *out = m;
  return LB_OK;
}

extern "C" int lb_linear_create(lb_engine* e, const lb_linear_desc* d, const float* w, int64_t n_floats, lb_linear** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  LB_TRY(ln_check_desc(e, d));
  const int64_t need = (int64_t)(d->n_in + 1) * d->out_dim;
  if (n_floats != need)
    return lb_fail(LB_ERR_ARG, "Linear weights: expected %lld floats, got %lld", (long long)need, (long long)n_floats);
  lb_linear* m = nullptr;
  LB_TRY(lbk_linear_view_create(e, d, nullptr, &m));
  int rc = m->mem.get(&m->blob, (size_t)n_floats);
  if (!rc) {
    const hipError_t he = hipMemcpy(m->blob, w, sizeof(float) * n_floats, hipMemcpyHostToDevice);
    if (he != hipSuccess) rc = lb_fail(LB_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(he));
  }
  if (rc) {
    lb_linear_destroy(m);
    return rc;
  }
  m->w = m->blob;
  *out = m;
  return LB_OK;
}

// node features of the current window -> xnode ([BN][64]; null: the model's own rows), the model -> out (rows of ldo
// floats).  A caller that keeps the rows (the training step's saved activation) passes a buffer of its own, so that another
// forward on the same model does not overwrite them.
int lbk_linear_forward(lb_engine* e, lb_linear* m, float* xnode, float* out, int ldo) {
  const int64_t BN = e->BN;
  if (!xnode) xnode = m->xnode;
  lb_tic(e, LB_T_NODEFEAT);
  LB_TRY(lbk_node_features_raw(e, xnode, LN_KPAD));
  lb_toc(e);
  lb_tic(e, LB_T_DECODER);
  const unsigned nb = (unsigned)std::min<int64_t>((BN + 15) / 16, 4096);
  hipLaunchKernelGGL(k_ln_forward, dim3(nb ? nb : 1), dim3(LN_WG), 0, e->stream, e->ctrl, BN, m->desc.n_in - 1, m->desc.out_dim,
                     xnode, e->ptype, m->w, out, ldo);
  lb_toc(e);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

extern "C" int lb_linear_forward(lb_engine* e, lb_linear* m, float* acc_out_dev) {
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  if (e->g.force_kind == LB_FORCE_BUFFER && !e->force)
    return lb_fail(LB_ERR_STATE, "LB_FORCE_BUFFER engine: call lb_set_force first");
  LB_TRY(lbk_linear_forward(e, m, nullptr, e->acc, 4));
  if (acc_out_dev) LB_TRY(lb_export_rows(e, e->acc, acc_out_dev, true));
  // the model reads no edges, but the feature and model kernels are no-ops once a list build has overflowed (the poison
  // that stops a rollout): nothing was written then, and the caller must hear of it
  LB_HIP(hipMemcpyAsync(e->ctrl_host, e->ctrl, sizeof(lb_ctrl), hipMemcpyDeviceToHost, e->stream));
  LB_HIP(hipStreamSynchronize(e->stream));
  if (e->ctrl_host->overflow_step >= 0) return lb_fail(LB_ERR_STATE, "neighbor list overflowed: re-allocate first");
  return LB_OK;
}

// The whole step loop on the device: features -> model -> integrator.  The model reads no edges, so no step builds the
// neighbor list (the generic loop builds one per step and gets the same positions): nothing can overflow, *n_realloc_out = 0.
// Like lb_rollout it leaves an allocated list behind: an engine without one, or one whose last build overflowed (every
// kernel of a step is a no-op then), allocates once before the loop - the latter counts as one re-allocation.
extern "C" int lb_linear_rollout(lb_engine* e, lb_linear* m, const double* traj_dev, int32_t T, int32_t n_steps,
                                 double* pred_out_dev, int32_t* n_realloc_out) {
  if (!traj_dev || !pred_out_dev) return lb_fail(LB_ERR_ARG, "null argument");
  LB_TRY(lb_model_check(e, m ? m->eng : nullptr));
  if (T < e->g.isl) return lb_fail(LB_ERR_ARG, "trajectory shorter than input_seq_length");
  if (e->g.force_kind == LB_FORCE_BUFFER)
    return lb_fail(LB_ERR_UNSUPPORTED, "lb_rollout with LB_FORCE_BUFFER: drive the steps from the host");
  LB_TRY(lbk_load_window(e, traj_dev, T, 0, 0));
  int n_realloc = 0;
  if (e->e_cap <= 0) {
    LB_TRY(lb_nl_allocate(e, nullptr, nullptr, nullptr));
  } else {
    LB_HIP(hipMemcpyAsync(e->ctrl_host, e->ctrl, sizeof(lb_ctrl), hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    if (e->ctrl_host->overflow_step >= 0) {
      LB_TRY(lb_nl_allocate(e, nullptr, nullptr, nullptr));
      n_realloc = 1;
    }
  }
  for (int s = 0; s < n_steps; ++s) {
    LB_TRY(lbk_linear_forward(e, m, nullptr, e->acc, 4));
    LB_TRY(lbk_integrate(e, e->acc, 4, nullptr, traj_dev, T, pred_out_dev, n_steps));
  }
  LB_HIP(hipStreamSynchronize(e->stream));
  if (n_realloc_out) *n_realloc_out = n_realloc;
  return LB_OK;
}
