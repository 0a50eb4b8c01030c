// lb_graph.hip - the two graph primitives a message-passing network written OUTSIDE this library needs on the engine's
// current neighbor list (lagrangebench_amd/graph.py wraps them as torch autograd functions):
//
//   lb_graph_gather(role, x (B*N, C))         -> out (B*E_cap, C)   out[slot] = x[role index of the slot], pads +0.0
//   lb_graph_segment_sum(role, msg (B*E_cap, C)) -> out (B*N, C)    out[i]    = sum of the real slots whose role index is i
//
// in the PADDED layout of lb_nl_read_idx: slot (b, j), j < n_edges[b], is compact edge row_ptr[b N] + j of the engine's
// receiver-sorted list.  They are each other's adjoints, so the backward of either is the other one: the same kernels,
// the same bits.
//
// Order contract of the sum: the first term, then one fp32 add per further term in ASCENDING SLOT ORDER - a numpy float32
// loop gives the same bits.  Receivers: the slots of node i are the contiguous CSR row of i.  Senders: the slots come from
// the sender-sorted view (lb_sender_view.h): per sender its compact edges in ascending order, built by transposing the
// receiver rows, or by a stable radix sort of (sender, edge) when the list holds an edge without its transpose.  The view
// lives in the engine's arena and is rebuilt at the first sender sum after a list build (lb_engine::nl_gen).  No atomics on
// floats anywhere; two calls give the same bits.
//
// Kernel shape.  Both are streaming kernels with no reuse: a group of LPR lanes (a power of two, 1 .. 64) owns one output
// row, a lane owns column units u = lane, lane + LPR, ...: 16-byte units (f32x4) when C % 4 == 0 and the pointers are
// 16-byte aligned, single floats otherwise.  C = 128 is half a wave per row with one 16-byte access per lane - the shape
// of k_segment_sum (lb_gns.hip) - so a row's slots are read as whole 512-byte lines.  Four independent loads are in flight
// per lane; the adds stay sequential.  Rows of one output are summed by ONE lane per column: no cross-lane step, no LDS.
// Grids are capped at 2048 workgroups of 256 threads and stride over the rows.  Addresses are int64 throughout.
#include <algorithm>

#include "lb_device.h"
#include "lb_sender_view.h"

#include <hipcub/hipcub.hpp>  // header-only device radix sort (the sender view of a list with one-directional edges)

#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

template <bool VEC>
struct lb_unit {
  typedef float type;
};
template <>
struct lb_unit<true> {
  typedef f32x4 type;
};
template <typename T>
__device__ __forceinline__ T lb_zero_unit();
template <>
__device__ __forceinline__ float lb_zero_unit<float>() {
  return 0.f;
}
template <>
__device__ __forceinline__ f32x4 lb_zero_unit<f32x4>() {
  return f32x4{0.f, 0.f, 0.f, 0.f};
}

// out[slot][:] = x[idx[compact edge of the slot]][:] for the real slots, +0.0 for the pads.  U units per row.
template <bool VEC>
__global__ void __launch_bounds__(256) k_graph_gather(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ x, float* __restrict__ out, int64_t BN, int N,
                                                      int B, int e_cap, int E, int U, int lpr_shift) {
  typedef typename lb_unit<VEC>::type T;
  const int lpr = 1 << lpr_shift, lane = threadIdx.x & (lpr - 1);
  const int64_t rows = (int64_t)B * e_cap, stride = (int64_t)gridDim.x * (256 >> lpr_shift);
  const T* __restrict__ xs = reinterpret_cast<const T*>(x);
  T* __restrict__ os = reinterpret_cast<T*>(out);
  for (int64_t r = (int64_t)blockIdx.x * (256 >> lpr_shift) + (threadIdx.x >> lpr_shift); r < rows; r += stride) {
    const int b = (int)(r / e_cap), j = (int)(r - (int64_t)b * e_cap);
    const int base = row_ptr[(int64_t)b * N], nb = row_ptr[(int64_t)(b + 1) * N] - base;
    const bool real = j < nb && base + j < E;
    int64_t node = real ? idx[base + j] : 0;
    node = node < 0 ? 0 : (node >= BN ? BN - 1 : node);   // (an index of the list is a node of the batch: never clamps)
    for (int u = lane; u < U; u += lpr) os[r * U + u] = real ? xs[node * U + u] : lb_zero_unit<T>();
  }
}

// out[i][:] = msg[slot of p0][:] + msg[slot of p0 + 1][:] + ... over the positions p of row i of (seg_ptr, perm): compact edge
// k = perm ? perm[p] : p, padded slot = b E_cap + k - row_ptr[b N].  +0.0 for an empty row.  Pad slots are never read.
template <bool VEC>
__global__ void __launch_bounds__(256) k_graph_segment_sum(const int32_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ seg_ptr,
                                                           const int32_t* __restrict__ perm, const float* __restrict__ msg,
                                                           float* __restrict__ out, int64_t BN, int N, int e_cap, int E, int U,
                                                           int lpr_shift) {
  typedef typename lb_unit<VEC>::type T;
  const int lpr = 1 << lpr_shift, lane = threadIdx.x & (lpr - 1);
  const int64_t stride = (int64_t)gridDim.x * (256 >> lpr_shift);
  const T* __restrict__ ms = reinterpret_cast<const T*>(msg);
  T* __restrict__ os = reinterpret_cast<T*>(out);
  for (int64_t i = (int64_t)blockIdx.x * (256 >> lpr_shift) + (threadIdx.x >> lpr_shift); i < BN; i += stride) {
    const int64_t b = i / N;
    const int base = row_ptr[b * N];
    int last = row_ptr[(b + 1) * N];   // one past the trajectory's compact edges, capped by the list and by its E_cap slots
    last = last < E ? last : E;
    last = last - base < e_cap ? last : base + e_cap;
    int p0 = seg_ptr[i], p1 = seg_ptr[i + 1];
    p0 = p0 < E ? p0 : E;
    p1 = p1 < E ? p1 : E;
    const int64_t slot0 = b * e_cap - base;   // padded slot of compact edge k = slot0 + k
    // compact edge at position p; a sender view is a permutation of the trajectory's own edges, the clamp never acts on one
    auto edge = [&](int p) -> int64_t {
      int k = perm ? perm[p] : p;
      k = k < base ? base : k;
      k = k >= last ? last - 1 : k;
      return slot0 + k;
    };
    if (last <= base) p1 = p0;   // (a trajectory without edges has empty rows)
    for (int u = lane; u < U; u += lpr) {
      T s = lb_zero_unit<T>();
      int p = p0;
      if (p < p1) s = ms[edge(p++) * U + u];   // the sum STARTS from the first term (-0.0 stays -0.0)
      for (; p + 4 <= p1; p += 4) {
        const T a0 = ms[edge(p + 0) * U + u];
        const T a1 = ms[edge(p + 1) * U + u];
        const T a2 = ms[edge(p + 2) * U + u];
        const T a3 = ms[edge(p + 3) * U + u];
        s = s + a0;
        s = s + a1;
        s = s + a2;
        s = s + a3;
      }
      for (; p < p1; ++p) s = s + ms[edge(p) * U + u];
      os[i * U + u] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// What the ops need to know about the current list, read back ONCE per list build (one stream synchronisation): whether
// it overflowed, its edge count, and that every trajectory's edges fit its E_cap slots.
static int graph_begin(lb_engine* e, const char* entry) {
  if (e->e_cap <= 0) return lb_fail(LB_ERR_STATE, "%s before lb_nl_allocate", entry);
  if (!e->graph_seen || e->graph_gen != e->nl_gen || e->graph_ecap != e->e_cap) {
    std::vector<int32_t> nb((size_t)e->g.B);
    LB_HIP(hipMemcpyAsync(e->ctrl_host, e->ctrl, sizeof(lb_ctrl), hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipMemcpyAsync(nb.data(), e->nedges_b, sizeof(int32_t) * nb.size(), hipMemcpyDeviceToHost, e->stream));
    LB_HIP(hipStreamSynchronize(e->stream));
    e->graph_bad = e->ctrl_host->overflow_step >= 0;
    for (int32_t n : nb) e->graph_bad = e->graph_bad || n > e->e_cap;
    e->graph_E = e->ctrl_host->n_edges_total;
    e->graph_gen = e->nl_gen;
    e->graph_ecap = e->e_cap;
    e->graph_seen = true;
  }
  if (e->graph_bad) return lb_fail(LB_ERR_STATE, "%s: the neighbor list overflowed: re-allocate first", entry);
  return LB_OK;
}

// The sender view of the current list -> e->snd_perm (E), e->snd_ptr (BN + 1): what train_sender_sort (lb_train.hip) builds
// per step, here once per list build.  The transposition's flag is read right away; a list with an edge in one direction
// only goes to the radix sort, whose buffers are allocated at that first use.
static int graph_sender_view(lb_engine* e) {
  if (e->snd_seen && e->snd_gen == e->nl_gen) return LB_OK;
  hipStream_t s = e->stream;
  const int64_t E = e->graph_E, BN = e->BN;
  e->snd_seen = false;
  if (E > e->snd_cap || BN + 1 > e->snd_cap)
    LB_TRY(lb_regrow(s, &e->snd_cap, std::max<int64_t>(E + E / 8 + 1024, BN + 2), [&](int64_t n) {
      e->snd_radix = false;
      e->snd_tmp_bytes = 0;
      LB_TRY(e->mem.drop(&e->snd_key));
      LB_TRY(e->mem.drop(&e->snd_iota));
      LB_TRY(e->mem.drop(&e->snd_tmp));
      LB_TRY(e->mem.get(&e->snd_perm, (size_t)n));
      LB_TRY(e->mem.get(&e->snd_ptr, (size_t)n));
      return e->snd_flag ? LB_OK : e->mem.get(&e->snd_flag, 1);
    }));
  int32_t flag = 0;
  LB_HIP(hipMemsetAsync(e->snd_flag, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_sender_transpose, GRID1(std::max(E, BN + 1)), 0, s, e->row_ptr, e->senders, e->receivers, E, BN,
                     e->snd_perm, e->snd_ptr, e->snd_flag);
  LB_HIP(hipGetLastError());
  LB_HIP(hipMemcpyAsync(&flag, e->snd_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LB_HIP(hipStreamSynchronize(s));
  if (flag && E > 0) {
    if (!e->snd_radix) {   // the radix sort's set, sized with the view (snd_cap entries)
      const int64_t n = e->snd_cap;
      LB_TRY(e->mem.get(&e->snd_key, (size_t)n));
      LB_TRY(e->mem.get(&e->snd_iota, (size_t)n));
      hipLaunchKernelGGL(k_iota, GRID1(n), 0, s, e->snd_iota, n);
      e->snd_tmp_bytes = 0;
      LB_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, e->snd_tmp_bytes, e->senders, e->snd_key, e->snd_iota, e->snd_perm,
                                                (int)n, 0, 32, s));
      LB_TRY(e->mem.get(&e->snd_tmp, e->snd_tmp_bytes));
      e->snd_radix = true;   // (last: set only when all three exist)
    }
    size_t bytes = e->snd_tmp_bytes;
    LB_HIP(hipcub::DeviceRadixSort::SortPairs(e->snd_tmp, bytes, e->senders, e->snd_key, e->snd_iota, e->snd_perm, (int)E, 0, 32,
                                              s));
    hipLaunchKernelGGL(k_lower_bounds, GRID1(BN + 1), 0, s, e->snd_key, E, BN, e->snd_ptr);
    LB_HIP(hipGetLastError());
    e->snd_sorts += 1;
  }
  e->snd_gen = e->nl_gen;
  e->snd_seen = true;
  return LB_OK;
}

// lanes per row for U units: the next power of two, 64 at most
static int graph_lpr_shift(int U) {
  int sh = 0;
  while (sh < 6 && (1 << sh) < U) ++sh;
  return sh;
}
static bool graph_vec(const void* a, const void* b, int C) {
  return C % 4 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
}
static unsigned graph_blocks(int64_t rows, int lpr_shift) {
  const int64_t per_block = 256 >> lpr_shift;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + per_block - 1) / per_block, 2048));
}

extern "C" int lb_graph_gather(lb_engine* e, int32_t role, const float* x_dev, float* out_dev, int32_t C) {
  if (!e || !x_dev || !out_dev) return lb_fail(LB_ERR_ARG, "null argument");
  if ((role != 0 && role != 1) || C < 1) return lb_fail(LB_ERR_ARG, "lb_graph_gather: role %d (0 receivers, 1 senders), C %d", role, C);
  LB_TRY(graph_begin(e, "lb_graph_gather"));
  const int32_t* idx = role ? e->senders : e->receivers;
  const bool vec = graph_vec(x_dev, out_dev, C);
  const int U = vec ? C / 4 : C, sh = graph_lpr_shift(U);
  const unsigned blocks = graph_blocks((int64_t)e->g.B * e->e_cap, sh);
  if (vec)
    hipLaunchKernelGGL(k_graph_gather<true>, dim3(blocks), dim3(256), 0, e->stream, e->row_ptr, idx, x_dev, out_dev, e->BN,
                       e->g.N, e->g.B, e->e_cap, (int)e->graph_E, U, sh);
  else
    hipLaunchKernelGGL(k_graph_gather<false>, dim3(blocks), dim3(256), 0, e->stream, e->row_ptr, idx, x_dev, out_dev, e->BN,
                       e->g.N, e->g.B, e->e_cap, (int)e->graph_E, U, sh);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

extern "C" int lb_graph_segment_sum(lb_engine* e, int32_t role, const float* msg_dev, float* out_dev, int32_t C) {
  if (!e || !msg_dev || !out_dev) return lb_fail(LB_ERR_ARG, "null argument");
  if ((role != 0 && role != 1) || C < 1)
    return lb_fail(LB_ERR_ARG, "lb_graph_segment_sum: role %d (0 receivers, 1 senders), C %d", role, C);
  LB_TRY(graph_begin(e, "lb_graph_segment_sum"));
  if (role) LB_TRY(graph_sender_view(e));
  const int32_t* seg = role ? e->snd_ptr : e->row_ptr;
  const int32_t* perm = role ? e->snd_perm : nullptr;
  const bool vec = graph_vec(msg_dev, out_dev, C);
  const int U = vec ? C / 4 : C, sh = graph_lpr_shift(U);
  const unsigned blocks = graph_blocks(e->BN, sh);
  if (vec)
    hipLaunchKernelGGL(k_graph_segment_sum<true>, dim3(blocks), dim3(256), 0, e->stream, e->row_ptr, seg, perm, msg_dev, out_dev,
                       e->BN, e->g.N, e->e_cap, (int)e->graph_E, U, sh);
  else
    hipLaunchKernelGGL(k_graph_segment_sum<false>, dim3(blocks), dim3(256), 0, e->stream, e->row_ptr, seg, perm, msg_dev, out_dev,
                       e->BN, e->g.N, e->e_cap, (int)e->graph_E, U, sh);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

extern "C" int32_t lb_graph_sender_sorts(lb_engine* e) { return e ? e->snd_sorts : -1; }
