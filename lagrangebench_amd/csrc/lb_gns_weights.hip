// lb_gns_weights.hip - GNS weight loading (host only): the flat blob of models/gns.py GNS.flatten -> the packed
// device images the network kernels read (struct lb_gns, lb_internal.h).
//
//   lb_gns_walk    the ONE statement of the blob's layout: a view of every Linear, in module order
//   lb_stage       the host copy of the device blob: 256-byte aligned images, upload, pointer fix-up
//   lb_pack_fused  num_mlp_layers == 2: one lb_mlp_w per MLP, each image packed for the kernels that read it
//   lb_pack_dense  any other depth: one 128 x 128 image per Linear and input block (lb_gns_generic.hip)
//   lb_gns_pack_plan_build  the same policies run against the RECORDING stage: the images as a job table over a training
//                  handle's device blob (lb_gns_repack.h), replayed by lb_gns_repack.hip or, for the test, on the host
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

#include "lb_gns_repack.h"
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

// ------------------------------------------------------------------------------------------- sources
// The (K, M) matrix an image is packed from, as rectangles of the blob (lb_pack_piece with a pointer for the offset); what
// no rectangle covers is 0.  One rectangle: a Linear's block as it lies in the blob.  Several: the matrices that hold
// input blocks side by side or padded to 128 rows.
struct lb_src_piece {
  const float* w;
  int row0, rows, stride, col0, cols;
};
struct lb_src {
  std::vector<lb_src_piece> pc;
  int K = 0, M = 0;
  bool scaled = false;  // times the decoder head's power of two (lb_stage::head_shift)
};
static lb_src lb_src_plain(const float* w, int K, int M) { return {{{w, 0, K, M, 0, M}}, K, M, false}; }
// every input block of a Linear zero-padded to 128 rows and 128 columns, as ONE (blocks * 128, 128) matrix (a processor
// node MLP's first Linear; lb_pack_ms interleaves the blocks)
static lb_src lb_src_padded(const lb_lin_view& l) {
  lb_src s;
  s.K = l.blocks * LB_D;
  s.M = LB_D;
  for (int b = 0; b < l.blocks; ++b) s.pc.push_back({l.block(b), b * LB_D, l.rows, l.out, 0, l.out});
  return s;
}
// (128, 256) = [Ws | Wr]: the sender and receiver rows of an edge MLP's first Linear, applied per NODE by the node
// kernel of the layer before (gns.py:97-100)
static lb_src lb_src_ws_wr(const lb_lin_view& l) {
  lb_src s;
  s.K = LB_D;
  s.M = 2 * LB_D;
  for (int b = 0; b < 2; ++b) s.pc.push_back({l.block(b), 0, l.rows, l.out, b * LB_D, l.out});
  return s;
}

// ------------------------------------------------------------------------------------------- staging
// One image of an M-split launch (lb_msplit.hip); keep = floats kept of it (0 = all)
struct lb_ms_piece {
  lb_src s;
  int nkb, npw;
  bool perm;
  size_t keep;
};

// The device blob of a model in the making: 256-byte aligned images in the order the policies ask for them.
//   direct (rec == null): the host copy of the blob, packed from host weights by the host packers; upload, pointer fix-up
//   recording:            no weights are read; every image becomes a lb_pack_job of rec (lb_gns_repack.h) whose source
//                         offsets are those of the blob at `base` seen through `cmap`
struct lb_stage {
  std::vector<float> host;                            // direct: the device blob as it will be uploaded
  std::vector<std::pair<const float**, size_t>> fix;  // image pointers to set once the device address is known
  double w_rms_min = 1e30;
  int sh = 0;  // direct: the decoder head is packed times 2^sh
  lb_pack_plan* rec = nullptr;
  const float* base = nullptr;
  const std::vector<int64_t>* cmap = nullptr;
  size_t n = 0;  // floats so far

  size_t next(const float** field, size_t count) {
    const size_t off = (n + 63) & ~(size_t)63;
    n = off + count;
    if (!rec) host.resize(n, 0.f);
    if (field) fix.push_back({field, off});
    return off;
  }
  // recording: the pieces of a source, translated.  A piece lies within one input block of a Linear, whose rows keep a
  // constant distance in the padded layout as well.
  int rec_pieces(const std::vector<lb_src_piece>& pc) {
    auto at = [&](int64_t i) { return cmap ? (*cmap)[(size_t)i] : i; };
    for (const lb_src_piece& p : pc) {
      const int64_t o = p.w - base;
      const int stride = p.rows > 1 ? (int)(at(o + p.stride) - at(o)) : p.stride;
      rec->pieces.push_back({at(o), p.row0, p.rows, stride, p.col0, p.cols, 0});
    }
    return (int)pc.size();
  }
  void rec_job(size_t off, int kind, const lb_src& s, int Kpad, int Mpad, int nkb, bool perm, int at, size_t floats) {
    lb_pack_job j{};
    j.dst = (int64_t)off;
    j.kind = kind;
    j.K = s.K;
    j.M = s.M;
    j.Kpad = Kpad;
    j.Mpad = Mpad;
    j.nkb = nkb;
    j.perm = perm;
    j.at = at;
    j.scaled = s.scaled;
    j.n_ent = (int32_t)((floats + 3) / 4);
    j.piece0 = (int32_t)rec->pieces.size();
    j.n_pieces = rec_pieces(s.pc);
    rec->jobs.push_back(j);
  }
  // direct: the source as a dense (K, M) matrix
  std::vector<float> dense(const lb_src& s) const {
    std::vector<float> o((size_t)s.K * s.M, 0.f);
    for (const lb_src_piece& p : s.pc)
      for (int r = 0; r < p.rows; ++r)
        memcpy(&o[(size_t)(p.row0 + r) * s.M + p.col0], p.w + (size_t)r * p.stride, sizeof(float) * p.cols);
    if (s.scaled)
      for (float& x : o) x = std::ldexp(x, sh);
    return o;
  }

  // n floats at the next 256-byte boundary: n_src floats of src from float `at` on, the rest 0; *field will point at them
  void vec(const float** field, size_t count, const float* src = nullptr, size_t n_src = 0, size_t at = 0) {
    const size_t off = next(field, count);
    if (rec)
      rec_job(off, LB_PK_VEC, src ? lb_src_plain(src, 1, (int)n_src) : lb_src(), 1, (int)count, 0, false, (int)at, count);
    else if (src)
      memcpy(host.data() + off + at, src, n_src * sizeof(float));
  }
  // one (K, M) matrix -> one image of Kp x Mp in packing `kind` (LB_PK_P32 / P16 / P16H); field null: the image continues
  // the one before it (its size is a multiple of the alignment)
  void img(const float** field, int kind, const lb_src& s, int Kp, int Mp) {
    const size_t off = next(field, (size_t)Kp * Mp);
    if (rec) return rec_job(off, kind, s, Kp, Mp, 0, false, 0, (size_t)Kp * Mp);
    const std::vector<float> w = dense(s);
    float* out = host.data() + off;
    if (kind == LB_PK_P32) lb_pack_weight(w.data(), s.K, s.M, Kp, Mp, out);
    else if (kind == LB_PK_P16) lb_pack_weight16(w.data(), s.K, s.M, Kp, out);
    else lb_pack_weight16h(w.data(), s.K, s.M, Kp, out, Mp);
  }
  // M-split image: the matrices of one launch back to back
  void ms(const float** field, const std::vector<lb_ms_piece>& pieces) {
    size_t total = 0;
    for (const lb_ms_piece& m : pieces) total += m.keep ? m.keep : (size_t)m.nkb * m.npw * 4096;
    size_t off = next(field, total);
    std::vector<float> tmp;
    for (const lb_ms_piece& m : pieces) {
      const size_t full = (size_t)m.nkb * m.npw * 4096, kept = m.keep ? m.keep : full;
      if (rec) {
        rec_job(off, LB_PK_MS, m.s, 32 * m.nkb, 128 * m.npw, m.nkb, m.perm, 0, kept);
      } else {
        tmp.assign(full, 0.f);
        lb_pack_ms(dense(m.s).data(), m.s.K, m.s.M, m.nkb, m.npw, m.perm, tmp.data());
        memcpy(host.data() + off, tmp.data(), kept * sizeof(float));
      }
      off += kept;
    }
  }
  // f16x2 carries a weight as fp16 hi + fp16 lo with an ABSOLUTE floor of 2^-25 on the pair: a matrix whose entries
  // are uniformly small (rms < 2^-7) would lose the 1e-5 class - noted here, acted on by lb_gns_create
  void note_rms(const lb_lin_view& l) {
    if (rec) {
      std::vector<lb_src_piece> pc;
      for (int b = 0; b < l.blocks; ++b) pc.push_back({l.block(b), 0, l.rows, l.out, 0, l.out});
      const int32_t p0 = (int32_t)rec->pieces.size();
      rec->rms.push_back({p0, rec_pieces(pc)});
      return;
    }
    const size_t cnt = (size_t)l.blocks * l.rows * l.out;
    double s2 = 0;
    size_t nz = 0;
    for (size_t i = 0; i < cnt; ++i) {
      s2 += (double)l.w[i] * l.w[i];
      nz += l.w[i] != 0.f;
    }
    if (nz) w_rms_min = std::min(w_rms_min, std::sqrt(s2 / (double)nz));
  }
  // the power of two the (K, M) decoder head is packed with: max |w| -> [0.25, 0.5) (lb_head_shift)
  void head_shift(const lb_lin_view& l) {
    if (rec) {
      const int32_t p0 = (int32_t)rec->pieces.size();
      rec->head = {p0, rec_pieces({{l.w, 0, l.rows, l.out, 0, l.out}})};
      return;
    }
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)l.rows * l.out; ++i) mx = std::max(mx, std::fabs(l.w[i]));
    sh = lb_head_shift(mx);
  }
  int upload(lb_arena& mem, float** blob) {
    LB_TRY(mem.get(blob, host.size()));
    if (hipMemcpy(*blob, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return lb_fail(LB_ERR_HIP, "weight upload failed");
    for (const auto& f : fix) *f.first = *blob + f.second;
    return LB_OK;
  }
};

// ------------------------------------------------------------------------------------------- packing policies
// num_mlp_layers == 2 (lb_gns.hip, lbk_decoder16).  Which MLP gets which image: the lb_mlp_w comment in lb_internal.h.
static void lb_pack_fused(lb_stage& st, const lb_gns_view& v, lb_gns* g) {
  const int D = LB_D, L = g->desc.num_mp_steps, dl = g->desc.latent_size;
  auto p32 = [&](const float** f, const lb_src& s, int Kp, int Mp) { st.img(f, LB_PK_P32, s, Kp, Mp); };
  auto p16 = [&](const float** f, const lb_src& s, int Kp) { st.img(f, LB_PK_P16, s, Kp, 128); };
  auto p16h = [&](const float** f, const lb_src& s, int Kp, int Mp = 128) { st.img(f, LB_PK_P16H, s, Kp, Mp); };
  auto lin = [&](const lb_lin_view& l, int b = 0) { return lb_src_plain(l.block(b), l.rows, l.out); };
  // b0, b1 (padded to b1_pad) and the LayerNorm parameters
  auto vecs = [&](lb_mlp_w& m, const lb_mlp_view& s, bool b0, int b1_pad = LB_D) {
    if (b0) st.vec(&m.b0, D, s.lin[0].b, dl);
    st.vec(&m.b1, b1_pad, s.lin[1].b, s.lin[1].out);
    if (s.ln_s) {
      st.vec(&m.ln_s, D, s.ln_s, dl);
      st.vec(&m.ln_o, D, s.ln_o, dl);
    }
  };

  // decoder (k_decoder16; its biases also feed the last M-split node launch).  The f16x2 copy of the head is packed times
  // 2^s (max |w| -> [0.25, 0.5)) and the kernels multiply the result by 2^-s: exact, and independent of the output
  // normalisation a checkpoint was trained with
  const lb_lin_view &d0 = v.dec.lin[0], &d1 = v.dec.lin[1];
  st.head_shift(d1);
  g->dec_unscale = std::ldexp(1.f, -st.sh);
  lb_src d1s = lin(d1);
  d1s.scaled = true;
  st.note_rms(d0);  // (the head is rescaled instead)
  p16(&g->dec.w0_16, lin(d0), D);
  p16h(&g->dec.w0_16h, lin(d0), D);
  p16(&g->dec.w1_16, lin(d1), D);
  p16h(&g->dec.w1_16h, d1s, D, 16);
  vecs(g->dec, v.dec, true, 32);

  // edge encoder
  {
    const lb_lin_view &l0 = v.enc_edge.lin[0], &l1 = v.enc_edge.lin[1];
    lb_mlp_w& m = g->enc_edge;
    st.note_rms(l0);
    st.note_rms(l1);
    p16(&m.w0_16, lin(l0), 16);
    p16h(&m.w0_16h, lin(l0), 32);
    p16(&m.w1_16, lin(l1), D);
    p16h(&m.w1_16h, lin(l1), D);
    vecs(m, v.enc_edge, true);
    st.ms(&m.ms, {{lin(l0), 1, 1, false, 0}, {lin(l1), 4, 1, true, 0}});
  }

  // a node MLP whose first Linear is the matrix w0, padded to K0p rows; ms = what its M-split launch applies after the
  // MLP itself
  auto node_mlp = [&](lb_mlp_w& m, const lb_mlp_view& s, const lb_src& w0, int K0p, std::vector<lb_ms_piece> ms) {
    const lb_lin_view& l1 = s.lin[1];
    st.note_rms(s.lin[0]);
    st.note_rms(l1);
    p32(&m.w0, w0, K0p, D);
    p16h(&m.w0_16h, w0, K0p);
    p32(&m.w1, lin(l1), D, D);
    p16h(&m.w1_16h, lin(l1), D);
    vecs(m, s, true);
    ms.insert(ms.begin(), {{w0, K0p / 32, 1, true, 0}, {lin(l1), 4, 1, true, 0}});
    st.ms(&m.ms, ms);
  };
  auto proj_piece = [&](const lb_src& wsr) { return std::vector<lb_ms_piece>{{wsr, 4, 2, true, 0}}; };

  lb_src wsr, wsr_next;  // [Ws | Wr] of this layer's edge MLP and of the next one's
  if (L) wsr = lb_src_ws_wr(v.proc_edge[0].lin[0]);
  node_mlp(g->enc_node, v.enc_node, lin(v.enc_node.lin[0]), g->kq_node * 8, L ? proj_piece(wsr) : std::vector<lb_ms_piece>());
  g->proc_edge.resize(L);
  g->proc_node.resize(L);
  for (int k = 0; k < L; ++k) {
    {  // edge MLP: the node kernel before it applies [Ws | Wr] (+ b0), its own kernels the edge rows of W0
      const lb_lin_view &l0 = v.proc_edge[k].lin[0], &l1 = v.proc_edge[k].lin[1];
      lb_mlp_w& m = g->proc_edge[k];
      p32(&m.proj_w, wsr, D, 2 * D);
      p16h(&m.proj_w_h2, lin(l0, 0), D, D);
      p16h(nullptr, lin(l0, 1), D, D);
      st.vec(&m.proj_b, 2 * D, l0.b, dl, D);
      p16(&m.w0_16, lin(l0, 2), D);
      p16h(&m.w0_16h, lin(l0, 2), D);
      p16(&m.w1_16, lin(l1), D);
      p16h(&m.w1_16h, lin(l1), D);
      vecs(m, v.proc_edge[k], false);
      st.ms(&m.ms, {{lin(l0, 2), 4, 1, true, 0}, {lin(l1), 4, 1, true, 0}});
    }
    // node MLP; its M-split launch goes on with the next layer's projection or, after the last layer, with the decoder
    // (k_node_ms<DEC>: W0 and output block 0 of the scaled head)
    std::vector<lb_ms_piece> ms = {{lin(d0), 4, 1, true, 0}, {d1s, 4, 1, true, 2048}};
    if (k + 1 < L) {
      wsr_next = lb_src_ws_wr(v.proc_edge[k + 1].lin[0]);
      ms = proj_piece(wsr_next);
    }
    node_mlp(g->proc_node[k], v.proc_node[k], lb_src_padded(v.proc_node[k].lin[0]), 2 * D, ms);
    std::swap(wsr, wsr_next);
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
        st.img(&x.wh[b], LB_PK_P16H, lb_src_plain(l.block(b), l.rows, l.out), D, D);
        st.img(&x.wf[b], LB_PK_P16, lb_src_plain(l.block(b), l.rows, l.out), D, D);
      }
      st.vec(&x.b, D, l.b, l.out);
    }
    if (s.ln_s) {
      st.vec(&m.ln_s, D, s.ln_s, s.lin.back().out);
      st.vec(&m.ln_o, D, s.ln_o, s.lin.back().out);
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

// everything lb_gns_create stages, in its order
static void lb_gns_stage_all(lb_stage& st, const lb_gns_view& v, lb_gns* g) {
  const lb_gns_desc* d = &g->desc;
  if (v.embed) st.vec(&g->embed, (size_t)d->num_particle_types * d->embedding_size, v.embed,
                      (size_t)d->num_particle_types * d->embedding_size);
  if (g->generic)
    lb_pack_dense(st, v, g);
  else
    lb_pack_fused(st, v, g);
}

// ------------------------------------------------------------------------------------------- API
// e: the engine the model is made for, or null (the job table and its self-test need none)
static int lb_gns_check_desc(const lb_gns_desc* d, const lb_engine* e) {
  const int dl = d->latent_size, nl = d->blocks_per_step;
  if (dl < 16 || dl > LB_D || dl % 16)
    return lb_fail(LB_ERR_UNSUPPORTED, "latent_size %d not built (multiples of 16 up to 128)", dl);
  if (e && d->out_dim != e->g.dim) return lb_fail(LB_ERR_ARG, "out_dim %d != case dim %d", d->out_dim, e->g.dim);
  if (e && d->node_in != e->g.node_in) return lb_fail(LB_ERR_ARG, "node_in %d != case feature width %d", d->node_in, e->g.node_in);
  if (e && d->edge_in != e->g.dim + 1) return lb_fail(LB_ERR_ARG, "edge_in %d != dim+1", d->edge_in);
  if (!e && (d->out_dim < 1 || d->out_dim > 3 || d->node_in < 1 || d->edge_in < 1 || d->edge_in > 16))
    return lb_fail(LB_ERR_ARG, "bad input / output widths");
  if (d->num_mp_steps < 0 || d->num_mp_steps > 64) return lb_fail(LB_ERR_ARG, "bad num_mp_steps");
  if (nl < 1 || nl > 16) return lb_fail(LB_ERR_ARG, "num_mlp_layers %d out of range (1..16)", nl);
  const int nin = d->node_in + (d->num_particle_types > 1 ? d->embedding_size : 0);
  if (nin > 128) return lb_fail(LB_ERR_UNSUPPORTED, "node input width %d > 128 not built", nin);
  return LB_OK;
}
// the host-side fields of a model that the packing policies read
static void lb_gns_init(lb_gns* g, const lb_gns_desc* d, lb_engine* e, int kq_node) {
  const int nin = d->node_in + (d->num_particle_types > 1 ? d->embedding_size : 0);
  g->desc = *d;
  g->eng = e;
  g->generic = d->blocks_per_step != 2;  // any depth other than the published two Linears runs on the one-Linear-per-launch kernels
  g->kq_node = kq_node > 0 ? kq_node : (nin + 31) / 32 * 4;
  g->lnc[0] = 1.0f / (float)d->latent_size;  // LayerNorm width of this model (lb_gns_bind)
  g->lnc[1] = (float)(LB_D - d->latent_size);
}

extern "C" int lb_gns_create(lb_engine* e, const lb_gns_desc* d, const float* w, int64_t n_floats, lb_gns** out) {
  if (!e || !d || !w || !out) return lb_fail(LB_ERR_ARG, "null argument");
  LB_TRY(lb_gns_check_desc(d, e));
  lb_gns_view v;
  LB_TRY(lb_gns_walk(d, w, n_floats, &v));

  lb_gns* g = new lb_gns();
  lb_gns_init(g, d, e, 0);
  lb_stage st;
  lb_gns_stage_all(st, v, g);
  g->blob_floats = (int64_t)st.host.size();
  int rc = st.upload(g->mem, &g->blob);
  if (!rc) lb_gns_rms_guard(e, st.w_rms_min);
  if (!rc) rc = lb_ensure_node_scratch(e);
  if (!rc) rc = lb_gns_bind(e, g);
  for (int i = 0; i < 3 && g->generic && !rc; ++i) rc = g->mem.get(&g->gen_hn[i], (size_t)e->BN * LB_D);  // hidden rows
  if (rc) {
    lb_gns_destroy(g);
    return rc;
  }
  *out = g;
  return LB_OK;
}

// the consequence of lb_stage::note_rms (lb_gns_create, lb_gns_train_sync_model)
void lb_gns_rms_guard(lb_engine* e, double w_rms_min) {
  if (w_rms_min < 0.0078125 && e->f16x2 && e->math_auto) {
    fprintf(stderr, "[lbhip] a weight matrix has rms %.3g < 2^-7: its fp16 hi/lo split would fall short of the 1e-5 class - "
                    "this engine uses exact-fp32 MFMA arithmetic\n", w_rms_min);
    e->f16x2 = 0;
  }
}

// ------------------------------------------------------------------------------------------- job table
// The recording run of the policies: no weights are read (the walk is over a blob of the right length that is never
// dereferenced), the model the image pointers go to is a scratch one.
int lb_gns_pack_plan_build(const lb_gns_desc* d, int kq_node, const std::vector<int64_t>* cmap, int64_t n_compact,
                           int64_t n_src, lb_pack_plan* plan) {
  LB_TRY(lb_gns_check_desc(d, nullptr));
  if (cmap && (int64_t)cmap->size() != n_compact) return lb_fail(LB_ERR_ARG, "index map of %lld entries for %lld weights",
                                                                 (long long)cmap->size(), (long long)n_compact);
  const std::vector<float> dummy((size_t)std::max<int64_t>(n_compact, 1));
  lb_gns_view v;
  LB_TRY(lb_gns_walk(d, dummy.data(), n_compact, &v));
  lb_gns g{};
  lb_gns_init(&g, d, nullptr, kq_node);
  *plan = lb_pack_plan();
  lb_stage st;
  st.rec = plan;
  st.base = dummy.data();
  st.cmap = cmap;
  lb_gns_stage_all(st, v, &g);
  plan->blob_floats = (int64_t)st.n;
  plan->src_floats = n_src;
  // bounds, checked HERE once so that no replay has to: every source rectangle inside the source blob, every image inside
  // the device blob; then the workgroups of the pack kernel
  for (const lb_pack_piece& p : plan->pieces)
    if (p.off < 0 || p.rows < 1 || p.cols < 1 || p.stride < p.cols ||
        p.off + (int64_t)(p.rows - 1) * p.stride + p.cols > n_src)
      return lb_fail(LB_ERR_STATE, "repack table: a source rectangle leaves the weight blob");
  for (size_t ji = 0; ji < plan->jobs.size(); ++ji) {
    const lb_pack_job& j = plan->jobs[ji];
    if (j.dst % 4 || j.dst < 0 || j.dst + (int64_t)4 * j.n_ent > ((plan->blob_floats + 3) & ~(int64_t)3))
      return lb_fail(LB_ERR_STATE, "repack table: an image leaves the packed blob");
    for (int e0 = 0; e0 < j.n_ent; e0 += LB_PACK_LANES) plan->blocks.push_back({(int32_t)ji, e0});
  }
  if (plan->blob_floats % 4) return lb_fail(LB_ERR_UNSUPPORTED, "repack table: packed blob of %lld floats", (long long)plan->blob_floats);
  return LB_OK;
}

// The table replayed on the host: what lbk_gns_repack's kernels do, entry by entry, through the same functions
static void lb_pack_plan_interpret(const lb_pack_plan& plan, const float* w, float* out, lb_pack_stats* stats) {
  const lb_pack_piece* pc = plan.pieces.data();
  std::vector<double> s2(LB_PACK_LANES), nz(LB_PACK_LANES);
  uint32_t mxb = 0, m;
  stats->rms_min = 1e30;
  for (const lb_pack_red& r : plan.rms) {
    for (int l = 0; l < LB_PACK_LANES; ++l) lb_pack_red_lane(r, pc, w, l, &s2[l], &nz[l], &m);
    stats->rms_min = std::min(stats->rms_min, lb_pack_red_rms(s2.data(), nz.data()));
  }
  for (int l = 0; l < LB_PACK_LANES && plan.head.n_pieces; ++l) {
    lb_pack_red_lane(plan.head, pc, w, l, &s2[l], &nz[l], &m);
    mxb = std::max(mxb, m);
  }
  const int sh = lb_head_shift(__builtin_bit_cast(float, mxb));
  stats->scale = lb_pow2f(sh);
  stats->unscale = lb_pow2f(-sh);
  for (const lb_pack_job& j : plan.jobs)
    for (int ent = 0; ent < j.n_ent; ++ent)
      lb_pack_entry(j, pc, w, stats->scale, ent, reinterpret_cast<uint32_t*>(out + j.dst + (int64_t)4 * ent));
}

extern "C" int64_t lb_gns_pack_selftest(const lb_gns_desc* d, int32_t node_in_kq, const float* w, int64_t n_floats,
                                        int64_t* n_bytes_out) {
  if (!d || !w) return lb_fail(LB_ERR_ARG, "null argument");
  LB_TRY(lb_gns_check_desc(d, nullptr));
  if (node_in_kq < 0 || node_in_kq > 16 || node_in_kq % 4) return lb_fail(LB_ERR_ARG, "node_in_kq %d: 0 or 4, 8, 12, 16", (int)node_in_kq);
  // (a) lb_gns_create's staging
  lb_gns_view v;
  LB_TRY(lb_gns_walk(d, w, n_floats, &v));
  lb_gns ga{};
  lb_gns_init(&ga, d, nullptr, node_in_kq);
  if (node_in_kq && node_in_kq < (d->node_in + (d->num_particle_types > 1 ? d->embedding_size : 0) + 7) / 8)
    return lb_fail(LB_ERR_ARG, "node_in_kq %d is narrower than the node input", (int)node_in_kq);
  lb_stage st;
  lb_gns_stage_all(st, v, &ga);
  // (b) the job table over the training handle's 128-padded layout, replayed on the host
  std::vector<int64_t> cmap;
  int64_t n_dev = 0, n_compact = 0;
  LB_TRY(lb_gns_train_padded_map(d, &cmap, &n_dev, &n_compact));
  if (n_compact != n_floats) return lb_fail(LB_ERR_ARG, "weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)n_compact);
  std::vector<float> padded;
  const float* src = w;
  if (!cmap.empty()) {
    padded.assign((size_t)n_dev, 0.f);
    for (int64_t i = 0; i < n_floats; ++i) padded[(size_t)cmap[(size_t)i]] = w[i];
    src = padded.data();
  }
  lb_pack_plan plan;
  LB_TRY(lb_gns_pack_plan_build(d, ga.kq_node, cmap.empty() ? nullptr : &cmap, n_compact, n_dev, &plan));
  if (plan.blob_floats != (int64_t)st.host.size())
    return lb_fail(LB_ERR_STATE, "the recorded blob has %lld floats, the packed one %lld", (long long)plan.blob_floats, (long long)st.host.size());
  std::vector<float> img((size_t)plan.blob_floats, 0.f);
  lb_pack_stats stats;
  lb_pack_plan_interpret(plan, src, img.data(), &stats);
  int64_t diff = 0;
  const unsigned char *a = reinterpret_cast<const unsigned char*>(st.host.data()), *b = reinterpret_cast<const unsigned char*>(img.data());
  for (size_t i = 0; i < img.size() * sizeof(float); ++i) diff += a[i] != b[i];
  // the scalars beside the images: dec_unscale (4 bytes), and the rms decision up to the summation order
  diff += 4 * (int64_t)(__builtin_bit_cast(uint32_t, stats.unscale) != __builtin_bit_cast(uint32_t, ga.dec_unscale));
  const double r0 = st.w_rms_min, r1 = stats.rms_min;
  diff += 8 * (int64_t)(std::fabs(r0 - r1) > 1e-12 * std::max(r0, r1));
  if (n_bytes_out) *n_bytes_out = (int64_t)(img.size() * sizeof(float));
  return diff;
}

extern "C" int64_t lb_gns_image_bytes(lb_gns* g) { return g ? g->blob_floats * (int64_t)sizeof(float) : -1; }
extern "C" int lb_gns_image_read(lb_gns* g, void* out_host, int64_t n_bytes) {
  if (!g || !out_host || n_bytes != g->blob_floats * (int64_t)sizeof(float)) return lb_fail(LB_ERR_ARG, "bad argument");
  LB_HIP(hipStreamSynchronize(g->eng->stream));
  LB_HIP(hipMemcpy(out_host, g->blob, (size_t)n_bytes, hipMemcpyDeviceToHost));
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
  lb_repack_free(g->repack);
  delete g;
}

extern "C" int lb_gns_set_tap(lb_gns* g, float* tap) {
  if (!g) return lb_fail(LB_ERR_ARG, "null model");
  g->tap = tap;
  return LB_OK;
}
