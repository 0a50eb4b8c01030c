// lb_train_linear.h - the training step of the Linear baseline (models/linear.py; trainer.py:35-89), part of lb_train.hip.
//
// The handle is an lb_gns_train on the common frame (train_step_begin / train_ensure / train_step_end): its device blob is
// lb_linear_create's, w (F + 1, dim) row-major then b (dim), with no padding (cmap empty).
//   forward   the inference kernel (lb_linear.hip: k_ln_forward) on lb_lnt::view, a view of t->w: the prediction is Linear.apply's
//             bit for bit; the node rows go to the handle's own lb_lnt::xnode, the saved activation (a forward or rollout on the
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

struct lb_lnt {
  lb_linear_desc desc{};
  lb_linear* view = nullptr;   // the inference forward on t->w
  float* xnode = nullptr;      // [cap_n][64]: the node rows of the step's forward
};

static void lnt_free(lb_gns_train* t) {
  lb_lnt* g = t->ln;
  if (!g) return;
  if (g->view) lb_linear_destroy(g->view);
  delete g;  // (its buffers are the handle arena's)
  t->ln = nullptr;
}

static int lnt_ensure(lb_gns_train* t, int64_t BN, int64_t) {   // (no edge-sized scratch: the model reads no edges)
  return train_ensure(t, BN, 0, [t](int64_t cn, int64_t, int64_t) -> int {
    lb_lnt* g = t->ln;
    LB_TRY(t->mem.get(&g->xnode, (size_t)cn * 64));
    LB_TRY(t->mem.get(&t->pred, (size_t)cn * 4));
    LB_TRY(t->mem.get(&t->dy, (size_t)cn * 4));
    // one slot: a partial of (F + 2) x dim floats per chunk of >= 64 rows (k_ln_dw in linear_backward, split as dw_narrow's)
    t->red_cap = dw_groups_max(cn) * (int64_t)(g->desc.n_in + 1) * g->desc.out_dim + 4096;
    return LB_OK;
  });
}

// The model's halves of the step: the inference kernel with the node rows kept -> t->pred ...
static int linear_forward(lb_gns_train* t, const float**) {
  lb_lnt* g = t->ln;
  return lbk_linear_forward(t->eng, g->view, g->xnode, t->pred, g->desc.out_dim);
}
// ... and, from d loss / d pred in t->dy (BN x dim)
static int linear_backward(lb_gns_train* t, double*) {
  lb_engine* e = t->eng;
  lb_lnt* g = t->ln;
  const int64_t BN = t->fwd_BN;
  const int F = g->desc.n_in - 1, dim = g->desc.out_dim;
  if (BN > 0) {
    int64_t chunk = (BN + DW_MAX_G - 1) / DW_MAX_G, off = 0;
    if (chunk < 64) chunk = 64;
    const int G = (int)((BN + chunk - 1) / chunk);
    const int64_t n = (int64_t)(F + 2) * dim;
    float* part = red_slot(t, (int64_t)G * n, &off);
    if (!part) return LB_ERR_STATE;
    hipLaunchKernelGGL(k_ln_dw, dim3(G), dim3(128), 0, e->stream, g->xnode, 64, F, e->ptype, t->dy, dim, BN, chunk,
                       part);
    red_push(t, off, G, n, (int)n, 0, 0, t->g, nullptr);
  }
  return LB_OK;
}
// (lb_gns_train_loss_grad is its loss entry; the guard never fires - no f16x2 product, no sender view: one attempt)
static const lb_train_model linear_model = {"Linear", "lb_gns_train_loss_grad", false, false, true, lnt_free, lnt_ensure,
                                            linear_forward, linear_backward, nullptr};

extern "C" int lb_linear_train_create(lb_engine* e, const lb_linear_desc* d, const float* w, int64_t n_floats, lb_gns_train** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  *out = nullptr;
  lb_gns_train* t = new lb_gns_train();
  lb_lnt* g = new lb_lnt();
  t->model = &linear_model;
  t->ln = g;
  t->eng = e;
  t->f16x2 = false;   // exact fp32 throughout (the reference's fp32 policy; there is no tall-skinny product here)
  g->desc = *d;
  t->n_floats = t->n_compact = (int64_t)(d->n_in + 1) * d->out_dim;
  int rc = d->n_in >= 1 && d->out_dim >= 1 ? LB_OK : lb_fail(LB_ERR_ARG, "Linear (%d, %d): bad widths", d->n_in, d->out_dim);
  if (!rc) rc = train_handle_init(t, "linear weight blob", w, n_floats);
  if (!rc) rc = lbk_linear_view_create(e, d, t->w, &g->view);   // (checks the description against the engine)
  return train_create_finish(t, rc, out);
}

// The inference view of the handle: lb_linear_forward / lb_linear_rollout on it run on the CURRENT weights.  Borrowed: it
// lives and dies with t.
extern "C" int lb_linear_train_model(lb_gns_train* t, lb_linear** out) {
  if (!t || !out) return lb_fail(LB_ERR_ARG, "null argument");
  if (t->model != &linear_model) return lb_fail(LB_ERR_ARG, "not a Linear training handle");
  *out = t->ln->view;
  return LB_OK;
}
