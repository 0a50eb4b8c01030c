// lb_gns_repack.hip - lb_gns_train_sync_model: the packed inference images of a GNS (lb_gns::blob) re-made ON THE DEVICE from
// the weight blob of a training handle, so that a push-forward unroll runs on the weights the optimiser has just written
// without a device-to-host copy of the blob, a host parameter tree and a host repack (lb_gns_create: ~14 MB of images for
// GNS-10-128).
//
// Nothing here knows which image goes where: lb_gns_weights.hip records its packing policies as a job table
// (lb_gns_pack_plan_build, lb_gns_repack.h) once per model; the table is uploaded and replayed at every call:
//   k_repack_stats   one workgroup per noted Linear: its non-zero rms (fp64, fixed order) - and one for max |w| of the decoder head
//   k_repack_finish  one lane: the smallest rms, the head's power of two (lb_head_shift) -> lb_pack_stats, on the device
//   k_repack         one lane per 16-byte destination entry (lb_pack_entry), 256 consecutive entries of one image per
//                    workgroup: the job is uniform over the workgroup (scalar loads), the stores are full dwordx4 lines in
//                    lane order, the reads are gathers from <= 384 x 128 sources that the stats pass has just pulled into L2.
//                    No atomics, no LDS; ~3.6 k workgroups for GNS-10-128.
// The host reads back lb_pack_stats (16 bytes) for lb_gns::dec_unscale and the rms guard - never the weights.
// Bounds: every source rectangle and destination image of the table is checked against the two blobs when the table is built.
#include "lb_gns_repack.h"
#include "lb_internal.h"

struct lb_repack {
  lb_arena mem;  // owns every buffer below
  lb_pack_job* jobs = nullptr;
  lb_pack_piece* pieces = nullptr;
  lb_pack_block* blocks = nullptr;
  lb_pack_red* reds = nullptr;  // the noted Linears, then the head (if any)
  double* rms = nullptr;        // [n_rms]
  uint32_t* head_mx = nullptr;
  lb_pack_stats* stats = nullptr;       // device
  lb_pack_stats* stats_host = nullptr;  // pinned
  int n_blocks = 0, n_rms = 0, has_head = 0;
  int64_t src_floats = 0;
};

void lb_repack_free(lb_repack* r) {
  delete r;
}

__global__ void __launch_bounds__(LB_PACK_LANES) k_repack_stats(const lb_pack_red* __restrict__ reds, const lb_pack_piece* __restrict__ pc,
                                                                 const float* __restrict__ w, int n_rms, double* __restrict__ rms,
                                                                 uint32_t* __restrict__ head_mx) {
  __shared__ double s2[LB_PACK_LANES], nz[LB_PACK_LANES];
  __shared__ uint32_t mx[LB_PACK_LANES];
  const int t = threadIdx.x, r = blockIdx.x;
  lb_pack_red_lane(reds[r], pc, w, t, &s2[t], &nz[t], &mx[t]);
  __syncthreads();
  if (t) return;
  if (r < n_rms) {
    rms[r] = lb_pack_red_rms(s2, nz);
  } else {
    uint32_t m = 0;
    for (int i = 0; i < LB_PACK_LANES; ++i) m = mx[i] > m ? mx[i] : m;
    *head_mx = m;
  }
}

__global__ void k_repack_finish(const double* __restrict__ rms, int n_rms, const uint32_t* __restrict__ head_mx, int has_head,
                                lb_pack_stats* __restrict__ stats) {
  if (threadIdx.x || blockIdx.x) return;
  double mn = 1e30;
  for (int i = 0; i < n_rms; ++i) mn = rms[i] < mn ? rms[i] : mn;
  const int sh = has_head ? lb_head_shift(__builtin_bit_cast(float, *head_mx)) : 0;
  stats->scale = lb_pow2f(sh);
  stats->unscale = lb_pow2f(-sh);
  stats->rms_min = mn;
}

__global__ void __launch_bounds__(LB_PACK_LANES) k_repack(const lb_pack_job* __restrict__ jobs, const lb_pack_piece* __restrict__ pc,
                                                          const lb_pack_block* __restrict__ blocks, const float* __restrict__ w,
                                                          const lb_pack_stats* __restrict__ stats, float* __restrict__ blob) {
  const lb_pack_block b = blocks[blockIdx.x];
  const lb_pack_job j = jobs[b.job];
  const int ent = b.ent0 + (int)threadIdx.x;
  if (ent >= j.n_ent) return;
  uint32_t o[4];
  lb_pack_entry(j, pc, w, stats->scale, ent, o);
  reinterpret_cast<uint4*>(blob + j.dst)[ent] = make_uint4(o[0], o[1], o[2], o[3]);
}

template <typename T>
static int repack_upload(lb_arena& mem, T** dev, const std::vector<T>& v) {
  LB_TRY(mem.get(dev, v.size()));
  if (!v.empty()) LB_HIP(hipMemcpy(*dev, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return LB_OK;
}

static int repack_build(lb_gns* g, const std::vector<int64_t>& cmap, int64_t n_compact, int64_t n_src) {
  lb_pack_plan plan;
  LB_TRY(lb_gns_pack_plan_build(&g->desc, g->kq_node, cmap.empty() ? nullptr : &cmap, n_compact, n_src, &plan));
  if (plan.blob_floats != g->blob_floats)
    return lb_fail(LB_ERR_STATE, "repack table: %lld floats of images, the model holds %lld", (long long)plan.blob_floats,
                   (long long)g->blob_floats);
  lb_repack* r = new lb_repack();
  g->repack = r;  // (freed by lb_gns_destroy, also after a failure below)
  r->n_blocks = (int)plan.blocks.size();
  r->n_rms = (int)plan.rms.size();
  r->has_head = plan.head.n_pieces > 0;
  r->src_floats = n_src;
  std::vector<lb_pack_red> reds = plan.rms;
  if (r->has_head) reds.push_back(plan.head);
  LB_TRY(repack_upload(r->mem, &r->jobs, plan.jobs));
  LB_TRY(repack_upload(r->mem, &r->pieces, plan.pieces));
  LB_TRY(repack_upload(r->mem, &r->blocks, plan.blocks));
  LB_TRY(repack_upload(r->mem, &r->reds, reds));
  LB_TRY(r->mem.get(&r->rms, (size_t)r->n_rms));
  LB_TRY(r->mem.get(&r->head_mx, 1));
  LB_TRY(r->mem.get(&r->stats, 1));
  return r->mem.get_pinned(&r->stats_host, 1);
}

int lbk_gns_repack(lb_engine* e, lb_gns* g, const float* w_dev, const std::vector<int64_t>& cmap, int64_t n_compact,
                   int64_t n_src) {
  if (g->repack && g->repack->src_floats != n_src) {
    lb_repack_free(g->repack);
    g->repack = nullptr;
  }
  if (!g->repack) {
    const int rc = repack_build(g, cmap, n_compact, n_src);
    if (rc) {
      lb_repack_free(g->repack);
      g->repack = nullptr;
      return rc;
    }
  }
  lb_repack* r = g->repack;
  hipStream_t s = e->stream;
  const int n_red = r->n_rms + r->has_head;
  if (n_red)
    hipLaunchKernelGGL(k_repack_stats, dim3(n_red), dim3(LB_PACK_LANES), 0, s, r->reds, r->pieces, w_dev, r->n_rms, r->rms, r->head_mx);
  hipLaunchKernelGGL(k_repack_finish, dim3(1), dim3(64), 0, s, r->rms, r->n_rms, r->head_mx, r->has_head, r->stats);
  if (r->n_blocks)
    hipLaunchKernelGGL(k_repack, dim3(r->n_blocks), dim3(LB_PACK_LANES), 0, s, r->jobs, r->pieces, r->blocks, w_dev, r->stats, g->blob);
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(r->stats_host, r->stats, sizeof(lb_pack_stats), hipMemcpyDeviceToHost, s));
  LB_HIP(hipStreamSynchronize(s));
  if (r->has_head) g->dec_unscale = r->stats_host->unscale;
  lb_gns_rms_guard(e, r->stats_host->rms_min);
  return LB_OK;
}
