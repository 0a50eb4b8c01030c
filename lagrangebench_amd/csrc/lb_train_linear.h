// lb_train_linear.h - the training step of the Linear baseline (models/linear.py; trainer.py:35-89), part of lb_train.hip.
//
// The handle is an lb_gns_train on the common frame (train_step_begin / train_ensure / train_step_end): its device blob is
// lb_linear_create's, w (F + 1, dim) row-major then b (dim), with no padding (cmap empty).
//   forward   the inference kernel (lb_linear.hip: k_ln_forward) on t->ln, a view of t->w: the prediction is Linear.apply's
//             bit for bit; the node rows go to the handle's own t->xnode, the saved activation (a forward or rollout on the
//             view between lb_train_forward and lb_train_backward writes the view's rows, not these)
//   loss      the masked _mse of every "acc" model (train_loss)
//   backward  [dW ; db] = [X | type | 1]^T dY, dY only dim columns wide: k_ln_dw forms the partial sums of a contiguous chunk
//             of rows - thread c < F owns column c of the node rows, thread F the type column (read from ptype), thread
//             F + 1 the bias - and k_part_reduce adds the chunks in ascending order.  The (F + 2) x dim partial of a chunk
//             has the layout of the blob, so one descriptor covers W and b.
// Exact fp32, fixed order, no atomics: two calls give the same bits.
#pragma once

__global__ void __launch_bounds__(128) k_ln_dw(const float* __restrict__ X, int ldx, int F, const int32_t* __restrict__ ptype,
                                               const float* __restrict__ dY, int M, int64_t rows, int64_t chunk,
                                               float* __restrict__ part) {
  const int c = threadIdx.x;
  if (c >= F + 2) return;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0; r < r1; ++r) {
    const float x = c < F ? X[r * ldx + c] : (c == F ? (float)ptype[r] : 1.f);
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (m < M) acc[m] += x * dY[r * M + m];
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (m < M) part[((int64_t)blockIdx.x * (F + 2) + c) * M + m] = acc[m];
}

static void lnt_free(lb_gns_train* t) {
  if (t->ln) lb_linear_destroy(t->ln);
  t->ln = nullptr;
}

static int lnt_ensure(lb_gns_train* t, int64_t BN, int64_t E) {
  return train_ensure(t, BN, E, [t](int64_t cn, int64_t, int64_t) -> int {
    LB_TRY(t->mem.get(&t->xnode, (size_t)cn * 64));
    LB_TRY(t->mem.get(&t->pred, (size_t)cn * 4));
    LB_TRY(t->mem.get(&t->dy, (size_t)cn * 4));
    // one slot: a partial of (F + 2) x dim floats per chunk of >= 64 rows (linear_backward_part)
    t->red_cap = std::min<int64_t>(DW_MAX_G, (cn + 63) / 64 + 1) * (int64_t)(t->ln_desc.n_in + 1) * t->ln_desc.out_dim + 4096;
    return LB_OK;
  });
}

extern "C" int lb_linear_train_create(lb_engine* e, const lb_linear_desc* d, const float* w, int64_t n_floats, lb_gns_train** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  lb_gns_train* t = new lb_gns_train();
  t->eng = e;
  t->f16x2 = false;   // exact fp32 throughout (the reference's fp32 policy; there is no tall-skinny product here)
  t->ln_desc = *d;
  t->n_floats = t->n_compact = (int64_t)(d->n_in + 1) * d->out_dim;
  int rc = d->n_in >= 1 && d->out_dim >= 1 ? LB_OK : lb_fail(LB_ERR_ARG, "Linear (%d, %d): bad widths", d->n_in, d->out_dim);
  if (!rc) rc = train_handle_init(t, "linear weight blob", w, n_floats);
  if (!rc) rc = lbk_linear_view_create(e, d, t->w, &t->ln);   // (checks the description against the engine)
  if (rc) {
    lb_gns_train_destroy(t);
    return rc;
  }
  *out = t;
  return LB_OK;
}

// The inference view of the handle: lb_linear_forward / lb_linear_rollout on it run on the CURRENT weights.  Borrowed: it
// lives and dies with t.
extern "C" int lb_linear_train_model(lb_gns_train* t, lb_linear** out) {
  if (!t || !out) return lb_fail(LB_ERR_ARG, "null argument");
  if (!t->ln) return lb_fail(LB_ERR_ARG, "not a Linear training handle");
  *out = t->ln;
  return LB_OK;
}

static int linear_forward_part(lb_gns_train* t, const char* entry, float* pred_out_dev) {
  lb_engine* e = t->eng;
  int64_t E = 0, BN = 0;
  LB_TRY(train_step_begin(t, entry, &E, &BN));
  t->fwd_E = E;
  t->fwd_BN = BN;
  LB_TRY(lnt_ensure(t, BN, 0));   // (no edge-sized scratch: the model reads no edges)
  const int dim = t->ln_desc.out_dim;
  LB_TRY(lbk_linear_forward(e, t->ln, t->xnode, t->pred, dim));
  if (pred_out_dev)
    LB_HIP(hipMemcpyAsync(pred_out_dev, t->pred, sizeof(float) * BN * dim, hipMemcpyDeviceToDevice, e->stream));
  return LB_OK;
}
// from d loss / d pred in t->dy (BN x dim)
static int linear_backward_part(lb_gns_train* t) {
  lb_engine* e = t->eng;
  const int64_t BN = t->fwd_BN;
  const int F = t->ln_desc.n_in - 1, dim = t->ln_desc.out_dim;
  if (BN > 0) {
    int64_t chunk = (BN + DW_MAX_G - 1) / DW_MAX_G, off = 0;
    if (chunk < 64) chunk = 64;
    const int G = (int)((BN + chunk - 1) / chunk);
    const int64_t n = (int64_t)(F + 2) * dim;
    float* part = red_slot(t, (int64_t)G * n, &off);
    if (!part) return LB_ERR_STATE;
    hipLaunchKernelGGL(k_ln_dw, dim3(G), dim3(128), 0, e->stream, t->xnode, 64, F, e->ptype, t->dy, dim, BN, chunk,
                       part);
    red_push(t, off, G, n, (int)n, 0, 0, t->g, nullptr);
  }
  return train_step_end(t);
}
static int linear_train_loss_grad_once(lb_gns_train* t, const float* target_dev, float loss_weight, float* pred_out_dev) {
  LB_TRY(linear_forward_part(t, "lb_gns_train_loss_grad", pred_out_dev));
  LB_TRY(train_loss(t, t->pred, target_dev, loss_weight, t->dy));
  return linear_backward_part(t);
}
// lb_gns_train_loss_grad on a Linear handle.  The guard never fires (no f16x2 product, no sender view): one attempt.
static int linear_train_loss_grad(lb_gns_train* t, const float* target_dev, float loss_weight, double* loss_out,
                                  float* pred_out_dev) {
  t->fwd_live = false;
  return train_loss_grad_guarded(t, loss_out, [&] { return linear_train_loss_grad_once(t, target_dev, loss_weight, pred_out_dev); });
}
