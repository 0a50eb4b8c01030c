// lb_gns_weights.hip - GNS weight loading (host only): the flat blob of models/gns.py GNS.flatten -> the packed
// device images the network kernels read (struct lb_gns, lb_internal.h).
//
//   lb_gns_walk    the ONE statement of the blob's layout: a view of every Linear, in module order
//   lb_stage       the host copy of the device blob: 256-byte aligned images, upload, pointer fix-up
//   lb_pack_fused  num_mlp_layers == 2: one lb_mlp_w per MLP, each image packed for the kernels that read it
//   lb_pack_dense  any other depth: one 128 x 128 image per Linear and input block (lb_gns_generic.hip)
//
// A latent narrower than the 128-wide tiles (GNS-5-64, docs/pages/baselines.rst:54) runs on the same kernels: the
// packers zero-fill k >= K and m >= M, biases and LayerNorm scale / offset are stored padded with zeros (the padded
// features stay exactly 0 through every layer) and the kernels divide by the true width (lb_ctrl::ln_inv_d / ln_pad).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "lb_msplit.h"

// ------------------------------------------------------------------------------------------- blob layout
struct lb_lin_view {   // one Linear: w is (blocks * rows, out) row-major over `blocks` concatenated inputs, b is [out]
  const float* w;
  int blocks, rows, out;
  const float* b;
  const float* block(int i) const { return w + (size_t)i * rows * out; }
};
struct lb_mlp_view {
  std::vector<lb_lin_view> lin;
  const float* ln_s = nullptr;  // [out of the last Linear], null = no LayerNorm
  const float* ln_o = nullptr;
};
struct lb_gns_view {
  const float* embed = nullptr;  // [types][emb] or null
  lb_mlp_view enc_node, enc_edge, dec;
  std::vector<lb_mlp_view> proc_edge, proc_node;
};

// Blob order (models/gns.py GNS.flatten): [embed] then per MLP, in module-creation order (node encoder, edge encoder,
// per step the edge MLP over [sender | receiver | edge] and the node MLP over [node | aggregate], decoder),
// linear_0 .. linear_{n-1} as (w [in][out], b [out]) and, except for the decoder, LayerNorm scale, offset.
static int lb_gns_walk(const lb_gns_desc* d, const float* w, int64_t n_floats, lb_gns_view* v) {
  const int dl = d->latent_size, nl = d->blocks_per_step;
  const int emb = d->num_particle_types > 1 ? d->embedding_size : 0;
  int64_t off = 0;
  auto take = [&](int64_t n) {  // (nothing is read before the length check below)
    const float* p = off + n <= n_floats ? w + off : nullptr;
    off += n;
    return p;
  };
  auto mlp = [&](int blocks, int rows, int out, bool ln) {
    lb_mlp_view m;
    for (int li = 0; li < nl; ++li) {
      lb_lin_view l;
      l.blocks = li ? 1 : blocks;
      l.rows = li ? dl : rows;
      l.out = li == nl - 1 ? out : dl;
      l.w = take((int64_t)l.blocks * l.rows * l.out);
      l.b = take(l.out);
      m.lin.push_back(l);
    }
    if (ln) {
      m.ln_s = take(out);
      m.ln_o = take(out);
    }
    return m;
  };
  if (emb) v->embed = take((int64_t)d->num_particle_types * emb);
  v->enc_node = mlp(1, d->node_in + emb, dl, true);
  v->enc_edge = mlp(1, d->edge_in, dl, true);
  for (int k = 0; k < d->num_mp_steps; ++k) {
    v->proc_edge.push_back(mlp(3, dl, dl, true));
    v->proc_node.push_back(mlp(2, dl, dl, true));
  }
  v->dec = mlp(1, dl, d->out_dim, false);
  if (off != n_floats) {
    if (nl == 2)
      return lb_fail(LB_ERR_ARG, "weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)off);
    return lb_fail(LB_ERR_ARG, "weight blob has %lld floats, the model (num_mlp_layers %d, latent %d) needs %s",
                   (long long)n_floats, nl, dl, off > n_floats ? "more" : "fewer");
  }
  return LB_OK;
}

// A Linear with every input block zero-padded to 128 rows and 128 columns: for the images that hold several input blocks
// as ONE matrix (a processor node MLP's first Linear; lb_pack_ms interleaves the blocks).  Every other image is packed
// straight from the blob.
static std::vector<float> lb_lin_padded(const lb_lin_view& l) {
  std::vector<float> o((size_t)l.blocks * LB_D * LB_D, 0.f);
  for (int b = 0; b < l.blocks; ++b)
    for (int r = 0; r < l.rows; ++r)
      memcpy(&o[((size_t)b * LB_D + r) * LB_D], l.block(b) + (size_t)r * l.out, sizeof(float) * l.out);
  return o;
}

// ------------------------------------------------------------------------------------------- staging
struct lb_stage {
  std::vector<float> host;                            // the device blob as it will be uploaded
  std::vector<std::pair<const float**, size_t>> fix;  // image pointers to set once the device address is known
  double w_rms_min = 1e30;

  // n floats at the next 256-byte boundary, the first n_src copied from src and the rest 0; *field will point at their
  // device copy.  The returned host pointer is valid until the next put.
  float* put(const float** field, size_t n, const float* src = nullptr, size_t n_src = 0) {
    const size_t off = (host.size() + 63) & ~(size_t)63;
    host.resize(off + n, 0.f);
    if (src) memcpy(host.data() + off, src, n_src * sizeof(float));
    fix.push_back({field, off});
    return host.data() + off;
  }
  // f16x2 carries a weight as fp16 hi + fp16 lo with an ABSOLUTE floor of 2^-25 on the pair: a matrix whose entries
  // are uniformly small (rms < 2^-7) would lose the 1e-5 class - noted here, acted on by lb_gns_create
  void note_rms(const lb_lin_view& l) {
    const size_t n = (size_t)l.blocks * l.rows * l.out;
    double s2 = 0;
    size_t nz = 0;
    for (size_t i = 0; i < n; ++i) {
      s2 += (double)l.w[i] * l.w[i];
      nz += l.w[i] != 0.f;
    }
    if (nz) w_rms_min = std::min(w_rms_min, std::sqrt(s2 / (double)nz));
  }
  int upload(float** blob) {
    if (hipMalloc((void**)blob, host.size() * sizeof(float)) != hipSuccess) {
      *blob = nullptr;
      return lb_fail(LB_ERR_HIP, "hipMalloc(weights) failed");
    }
    if (hipMemcpy(*blob, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return lb_fail(LB_ERR_HIP, "weight upload failed");
    for (const auto& f : fix) *f.first = *blob + f.second;
    return LB_OK;
  }
};

// ------------------------------------------------------------------------------------------- packing policies
// num_mlp_layers == 2 (lb_gns.hip, lbk_decoder16).  Which MLP gets which image: the lb_mlp_w comment in lb_internal.h.
static void lb_pack_fused(lb_stage& st, const lb_gns_view& v, lb_gns* g) {
  const int D = LB_D, L = g->desc.num_mp_steps, dl = g->desc.latent_size, od = g->desc.out_dim;
  // one (K, M) matrix -> one image of Kp x Mp
  auto p32 = [&](const float** f, const float* w, int K, int M, int Kp, int Mp) {
    lb_pack_weight(w, K, M, Kp, Mp, st.put(f, (size_t)Kp * Mp));
  };
  auto p16 = [&](const float** f, const float* w, int K, int M, int Kp) {
    lb_pack_weight16(w, K, M, Kp, st.put(f, (size_t)Kp * 128));
  };
  auto p16h = [&](const float** f, const float* w, int K, int M, int Kp, int Mp = 128) {
    lb_pack_weight16h(w, K, M, Kp, st.put(f, (size_t)Kp * Mp), Mp);
  };
  // b0, b1 (padded to b1_pad) and the LayerNorm parameters
  auto vecs = [&](lb_mlp_w& m, const lb_mlp_view& s, bool b0, int b1_pad = LB_D) {
    if (b0) st.put(&m.b0, D, s.lin[0].b, dl);
    st.put(&m.b1, b1_pad, s.lin[1].b, s.lin[1].out);
    if (s.ln_s) {
      st.put(&m.ln_s, D, s.ln_s, dl);
      st.put(&m.ln_o, D, s.ln_o, dl);
    }
  };
  // M-split image (lb_msplit.hip): the matrices of one launch back to back; keep = floats kept of a piece (0 = all)
  struct ms_piece { const float* w; int K, M, nkb, npw; bool perm; size_t keep; };
  auto put_ms = [&](const float** f, const std::vector<ms_piece>& pieces) {
    std::vector<float> img, tmp;
    for (const ms_piece& m : pieces) {
      tmp.assign((size_t)m.nkb * m.npw * 4096, 0.f);
      lb_pack_ms(m.w, m.K, m.M, m.nkb, m.npw, m.perm, tmp.data());
      img.insert(img.end(), tmp.begin(), m.keep ? tmp.begin() + m.keep : tmp.end());
    }
    st.put(f, img.size(), img.data(), img.size());
  };
  // (128, 256) = [Ws | Wr]: the sender and receiver rows of an edge MLP's first Linear, applied per NODE by the node
  // kernel of the layer before (gns.py:97-100)
  auto ws_wr = [&](const lb_lin_view& l) {
    std::vector<float> o((size_t)D * 2 * D, 0.f);
    for (int r = 0; r < dl; ++r) {
      memcpy(&o[(size_t)r * 2 * D], l.block(0) + (size_t)r * dl, sizeof(float) * dl);
      memcpy(&o[(size_t)r * 2 * D + D], l.block(1) + (size_t)r * dl, sizeof(float) * dl);
    }
    return o;
  };

  // decoder (k_decoder16; its biases also feed the last M-split node launch).  The f16x2 copy of the head is packed times
  // 2^s (max |w| -> [0.25, 0.5)) and the kernels multiply the result by 2^-s: exact, and independent of the output
  // normalisation a checkpoint was trained with
  const lb_lin_view &d0 = v.dec.lin[0], &d1 = v.dec.lin[1];
  std::vector<float> d1s(d1.w, d1.w + (size_t)dl * od);
  {
    float mx = 0.f;
    for (float x : d1s) mx = std::max(mx, std::fabs(x));
    int sh = 0;
    if (mx > 0.f && std::isfinite(mx)) sh = std::max(-60, std::min(60, (int)std::floor(std::log2(0.5 / (double)mx))));
    for (float& x : d1s) x = std::ldexp(x, sh);
    g->dec_unscale = std::ldexp(1.f, -sh);
  }
  st.note_rms(d0);  // (the head is rescaled instead)
  p16(&g->dec.w0_16, d0.w, dl, dl, D);
  p16h(&g->dec.w0_16h, d0.w, dl, dl, D);
  p16(&g->dec.w1_16, d1.w, dl, od, D);
  p16h(&g->dec.w1_16h, d1s.data(), dl, od, D, 16);
  vecs(g->dec, v.dec, true, 32);

  // edge encoder
  {
    const lb_lin_view &l0 = v.enc_edge.lin[0], &l1 = v.enc_edge.lin[1];
    lb_mlp_w& m = g->enc_edge;
    st.note_rms(l0);
    st.note_rms(l1);
    p16(&m.w0_16, l0.w, l0.rows, dl, 16);
    p16h(&m.w0_16h, l0.w, l0.rows, dl, 32);
    p16(&m.w1_16, l1.w, dl, dl, D);
    p16h(&m.w1_16h, l1.w, dl, dl, D);
    vecs(m, v.enc_edge, true);
    put_ms(&m.ms, {{l0.w, l0.rows, dl, 1, 1, false, 0}, {l1.w, dl, dl, 4, 1, true, 0}});
  }

  // a node MLP whose first Linear is the (K0, M0) matrix w0, padded to K0p rows; ms = what its M-split launch applies
  // after the MLP itself
  auto node_mlp = [&](lb_mlp_w& m, const lb_mlp_view& s, const float* w0, int K0, int M0, int K0p,
                      std::vector<ms_piece> ms) {
    const lb_lin_view& l1 = s.lin[1];
    st.note_rms(s.lin[0]);
    st.note_rms(l1);
    p32(&m.w0, w0, K0, M0, K0p, D);
    p16h(&m.w0_16h, w0, K0, M0, K0p);
    p32(&m.w1, l1.w, dl, dl, D, D);
    p16h(&m.w1_16h, l1.w, dl, dl, D);
    vecs(m, s, true);
    ms.insert(ms.begin(), {{w0, K0, M0, K0p / 32, 1, true, 0}, {l1.w, dl, dl, 4, 1, true, 0}});
    put_ms(&m.ms, ms);
  };
  auto proj_piece = [&](const std::vector<float>& wsr) { return std::vector<ms_piece>{{wsr.data(), D, 2 * D, 4, 2, true, 0}}; };

  std::vector<float> wsr, wsr_next;  // [Ws | Wr] of this layer's edge MLP and of the next one's
  if (L) wsr = ws_wr(v.proc_edge[0].lin[0]);
  node_mlp(g->enc_node, v.enc_node, v.enc_node.lin[0].w, v.enc_node.lin[0].rows, dl, g->kq_node * 8,
           L ? proj_piece(wsr) : std::vector<ms_piece>());
  g->proc_edge.resize(L);
  g->proc_node.resize(L);
  for (int k = 0; k < L; ++k) {
    {  // edge MLP: the node kernel before it applies [Ws | Wr] (+ b0), its own kernels the edge rows of W0
      const lb_lin_view &l0 = v.proc_edge[k].lin[0], &l1 = v.proc_edge[k].lin[1];
      lb_mlp_w& m = g->proc_edge[k];
      p32(&m.proj_w, wsr.data(), D, 2 * D, D, 2 * D);
      float* two = st.put(&m.proj_w_h2, (size_t)2 * D * D);
      lb_pack_weight16h(l0.block(0), dl, dl, D, two, D);
      lb_pack_weight16h(l0.block(1), dl, dl, D, two + (size_t)D * D, D);
      memcpy(st.put(&m.proj_b, 2 * D) + D, l0.b, sizeof(float) * dl);
      p16(&m.w0_16, l0.block(2), dl, dl, D);
      p16h(&m.w0_16h, l0.block(2), dl, dl, D);
      p16(&m.w1_16, l1.w, dl, dl, D);
      p16h(&m.w1_16h, l1.w, dl, dl, D);
      vecs(m, v.proc_edge[k], false);
      put_ms(&m.ms, {{l0.block(2), dl, dl, 4, 1, true, 0}, {l1.w, dl, dl, 4, 1, true, 0}});
    }
    // node MLP; its M-split launch goes on with the next layer's projection or, after the last layer, with the decoder
    // (k_node_ms<DEC>: W0 and output block 0 of the scaled head)
    const std::vector<float> w0 = lb_lin_padded(v.proc_node[k].lin[0]);
    std::vector<ms_piece> ms = {{d0.w, dl, dl, 4, 1, true, 0}, {d1s.data(), dl, od, 4, 1, true, 2048}};
    if (k + 1 < L) {
      wsr_next = ws_wr(v.proc_edge[k + 1].lin[0]);
      ms = proj_piece(wsr_next);
    }
    node_mlp(g->proc_node[k], v.proc_node[k], w0.data(), 2 * D, D, 2 * D, ms);
    wsr.swap(wsr_next);
  }
}

// any other depth (lb_gns_generic.hip): every Linear as one 128 x 128 image per input block, in both packings
static void lb_pack_dense(lb_stage& st, const lb_gns_view& v, lb_gns* g) {
  const int D = LB_D, L = g->desc.num_mp_steps;
  auto mlp = [&](lb_gen_mlp& m, const lb_mlp_view& s) {
    m.lin.resize(s.lin.size());
    for (size_t li = 0; li < s.lin.size(); ++li) {
      const lb_lin_view& l = s.lin[li];
      lb_gen_lin& x = m.lin[li];
      st.note_rms(l);
      x.wh.resize(l.blocks);
      x.wf.resize(l.blocks);
      for (int b = 0; b < l.blocks; ++b) {
        lb_pack_weight16h(l.block(b), l.rows, l.out, D, st.put(&x.wh[b], (size_t)D * D), D);
        lb_pack_weight16(l.block(b), l.rows, l.out, D, st.put(&x.wf[b], (size_t)D * D));
      }
      st.put(&x.b, D, l.b, l.out);
    }
    if (s.ln_s) {
      st.put(&m.ln_s, D, s.ln_s, s.lin.back().out);
      st.put(&m.ln_o, D, s.ln_o, s.lin.back().out);
    }
  };
  mlp(g->g_enc_node, v.enc_node);
  mlp(g->g_enc_edge, v.enc_edge);
  g->g_proc_edge.resize(L);
  g->g_proc_node.resize(L);
  for (int k = 0; k < L; ++k) {
    mlp(g->g_proc_edge[k], v.proc_edge[k]);
    mlp(g->g_proc_node[k], v.proc_node[k]);
  }
  mlp(g->g_dec, v.dec);
}

// ------------------------------------------------------------------------------------------- API
extern "C" int lb_gns_create(lb_engine* e, const lb_gns_desc* d, const float* w, int64_t n_floats, lb_gns** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  const int dl = d->latent_size, nl = d->blocks_per_step;
  if (dl < 16 || dl > LB_D || dl % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "latent_size %d not built (multiples of 16 up to 128)", dl);
  if (d->out_dim != e->g.dim) return lb_fail(LB_ERR_ARG, "out_dim %d != case dim %d", d->out_dim, e->g.dim);
  if (d->node_in != e->g.node_in) return lb_fail(LB_ERR_ARG, "node_in %d != case feature width %d", d->node_in, e->g.node_in);
  if (d->edge_in != e->g.dim + 1) return lb_fail(LB_ERR_ARG, "edge_in %d != dim+1", d->edge_in);
  if (d->num_mp_steps < 0 || d->num_mp_steps > 64) return lb_fail(LB_ERR_ARG, "bad num_mp_steps");
  if (nl < 1 || nl > 16) return lb_fail(LB_ERR_ARG, "num_mlp_layers %d out of range (1..16)", nl);
  const int nin = d->node_in + (d->num_particle_types > 1 ? d->embedding_size : 0);
  if (nin > 128) return lb_fail(LB_ERR_UNSUPPORTED, "node input width %d > 128 not built", nin);
  lb_gns_view v;
  LB_TRY(lb_gns_walk(d, w, n_floats, &v));

  lb_gns* g = new lb_gns();
  g->desc = *d;
  g->eng = e;
  g->generic = nl != 2;  // any depth other than the published two Linears runs on the one-Linear-per-launch kernels
  g->kq_node = (nin + 31) / 32 * 4;
  g->lnc[0] = 1.0f / (float)dl;  // LayerNorm width of this model (lb_gns_bind)
  g->lnc[1] = (float)(LB_D - dl);
  lb_stage st;
  if (v.embed) st.put(&g->embed, (size_t)d->num_particle_types * d->embedding_size, v.embed,
                      (size_t)d->num_particle_types * d->embedding_size);
  if (g->generic)
    lb_pack_dense(st, v, g);
  else
    lb_pack_fused(st, v, g);
  int rc = st.upload(&g->blob);
  if (!rc && st.w_rms_min < 0.0078125 && e->f16x2 && e->math_auto) {
    fprintf(stderr, "[lbhip] a weight matrix has rms %.3g < 2^-7: its fp16 hi/lo split would fall short of the 1e-5 class - "
                    "this engine uses exact-fp32 MFMA arithmetic\n", st.w_rms_min);
    e->f16x2 = 0;
  }
  if (!rc) rc = lb_ensure_node_scratch(e);
  if (!rc) rc = lb_gns_bind(e, g);
  for (int i = 0; i < 3 && g->generic && !rc; ++i) rc = lb_alloc(&g->gen_hn[i], (size_t)e->BN * LB_D);  // hidden rows
  if (rc) {
    lb_gns_destroy(g);
    return rc;
  }
  *out = g;
  return LB_OK;
}

// Per-model constants that live in engine-wide state (the LayerNorm width in the control block, the node feature
// row stride in the geometry): re-applied whenever another model of the same engine runs.
int lb_gns_bind(lb_engine* e, lb_gns* g) {
  if (e->bound_model == g) return LB_OK;
  LB_HIP(hipMemcpyAsync(&e->ctrl->ln_inv_d, g->lnc, sizeof(g->lnc), hipMemcpyHostToDevice, e->stream));
  e->g.kpad = g->kq_node * 8;
  e->bound_model = g;
  return LB_OK;
}

extern "C" void lb_gns_destroy(lb_gns* g) {
  if (!g) return;
  if (g->eng && g->eng->bound_model == g) g->eng->bound_model = nullptr;
  if (g->blob) (void)hipFree(g->blob);
  for (float* b : g->gen_hn)
    if (b) (void)hipFree(b);
  if (g->gen_he) (void)hipFree(g->gen_he);
  delete g;
}

extern "C" int lb_gns_set_tap(lb_gns* g, float* tap) {
  if (!g) return lb_fail(LB_ERR_ARG, "null model");
  g->tap = tap;
  return LB_OK;
}
