// lb_graph.hip - the graph primitives a message-passing network written OUTSIDE this library needs on the engine's
// current neighbor list (lagrangebench_amd/graph.py wraps them as torch autograd functions):
//
//   lb_graph_gather(role, x (B*N, C))         -> out (B*E_cap, C)   out[slot] = x[role index of the slot], pads +0.0
//   lb_graph_segment_sum(role, msg (B*E_cap, C)) -> out (B*N, C)    out[i]    = sum of the real slots whose role index is i
//
// and, for attention and pooling layers (further down: "attention ops"), lb_graph_degree, lb_graph_segment_max / _min,
// lb_graph_segment_softmax and the fused lb_graph_attend with their backward entries; for filter x neighbour messages ("edge
// messages") the fused lb_graph_conv and the edge-shaped lb_graph_pair_mul / lb_graph_pair_add, and the equivariant couplings
// through a per-edge vector, lb_graph_conv_vec / lb_graph_conv_dot with lb_graph_conv_vec_edge_grad; the continuous-filter
// convolution with its Linear inside, lb_graph_filter_conv with lb_graph_filter_conv_grad; the multi-aggregator
// lb_graph_aggregate (sum, mean, max, min, std, var of one message from one walk) with its backward; the reverse-edge map
// lb_graph_reverse with swap / symmetrize / antisymmetrize on it, lb_graph_edge_pair_t ("edge pairs"); and lb_graph_features_backward
// ("feature transpose"): d loss / d window from the cotangents of the features such a network was handed.
//
// All work in the PADDED layout of lb_nl_read_idx: slot (b, j), j < n_edges[b], is compact edge row_ptr[b N] + j of the engine's
// receiver-sorted list.  Gather and segment_sum are each other's adjoints, so the backward of either is the other one: the
// same kernels, the same bits.
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
//
// Element types.  The text above and the kernels' comments speak of float32; every op also runs on bfloat16 tensors (the
// lb_graph_*_t entries) through the same kernels - "element types" below: a 16-byte unit is then 8 elements (C % 8 == 0), the
// arithmetic stays fp32 and each stored element is rounded once.
#include <algorithm>
#include <type_traits>

#include "lb_device.h"
#include "lb_features.h"
#include "lb_sender_view.h"

#include <hipcub/hipcub.hpp>  // header-only device radix sort (the sender view of a list with one-directional edges)

#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

// ---- element types.  Every op runs on float32 or bfloat16 tensors (include/lbhip.h: the lb_graph_*_t entries); the kernels are
// templates over the element type E (float, or lb_bf16: the 16 bits of a bfloat16) and the elements W of one access - 16
// bytes (4 floats, 8 bf16), 8 bytes (4 bf16, attend only) or one element.  Only the load and the store of a unit differ: the
// load widens to fp32 registers (exact), the store rounds to nearest even ONCE; everything between them is the fp32 arithmetic.
// So a bf16 op is round(fp32 op(upcast inputs)) bit for bit, and no partial result is ever held in bf16.
typedef uint16_t lb_bf16;
typedef uint32_t lb_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lb_u32x2 __attribute__((ext_vector_type(2)));
typedef int32_t lb_i32x4 __attribute__((ext_vector_type(4)));
typedef float lb_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 lb_bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float lb_widen(uint32_t bits16) { return __uint_as_float(bits16 << 16); }
// two fp32 -> two bf16 in one word (lo in bits 0..15): the compiler's conversion, v_cvt_pk_bf16_f32 on gfx950 - round to
// nearest even, NaN stays NaN, overflow to inf, subnormals kept (the kernel mode keeps fp32 subnormals)
__device__ __forceinline__ uint32_t lb_round2(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(lb_f32x2{lo, hi}, lb_bf16x2));
}
__device__ __forceinline__ lb_bf16 lb_round1(float f) { return __builtin_bit_cast(lb_bf16, (__bf16)f); }

template <typename E>
__device__ __forceinline__ float lb_ld1(const E* p) {
  if constexpr (sizeof(E) == 4)
    return *p;
  else
    return lb_widen(*p);
}
template <typename E>
__device__ __forceinline__ void lb_st1(E* p, float f) {
  if constexpr (sizeof(E) == 4)
    *p = f;
  else
    *p = lb_round1(f);
}
template <typename E, int W>
__device__ __forceinline__ void lb_ld(const E* p, float (&a)[W]) {
  static_assert(sizeof(E) == 4 ? (W == 4 || W == 1) : (W == 8 || W == 4 || W == 1), "unit width");
  if constexpr (W == 1) {
    a[0] = lb_ld1<E>(p);
  } else if constexpr (sizeof(E) == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    a[0] = t[0], a[1] = t[1], a[2] = t[2], a[3] = t[3];
  } else if constexpr (W == 8) {
    const lb_u32x4 t = *reinterpret_cast<const lb_u32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[2 * k] = lb_widen(t[k]), a[2 * k + 1] = __uint_as_float(t[k] & 0xffff0000u);
  } else {
    const lb_u32x2 t = *reinterpret_cast<const lb_u32x2*>(p);
#pragma unroll
    for (int k = 0; k < 2; ++k) a[2 * k] = lb_widen(t[k]), a[2 * k + 1] = __uint_as_float(t[k] & 0xffff0000u);
  }
}
template <typename E, int W>
__device__ __forceinline__ void lb_st(E* p, const float (&a)[W]) {
  if constexpr (W == 1)
    lb_st1<E>(p, a[0]);
  else if constexpr (sizeof(E) == 4)
    *reinterpret_cast<f32x4*>(p) = f32x4{a[0], a[1], a[2], a[3]};
  else if constexpr (W == 8)
    *reinterpret_cast<lb_u32x4*>(p) =
        lb_u32x4{lb_round2(a[0], a[1]), lb_round2(a[2], a[3]), lb_round2(a[4], a[5]), lb_round2(a[6], a[7])};
  else
    *reinterpret_cast<lb_u32x2*>(p) = lb_u32x2{lb_round2(a[0], a[1]), lb_round2(a[2], a[3])};
}
// W int32 (the winning slots of segment_max): 16-byte accesses when W > 1
template <int W>
__device__ __forceinline__ void lb_ldi(const int32_t* p, int32_t (&a)[W]) {
  if constexpr (W == 1) {
    a[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4) {
      const lb_i32x4 t = *reinterpret_cast<const lb_i32x4*>(p + q);
      a[q] = t[0], a[q + 1] = t[1], a[q + 2] = t[2], a[q + 3] = t[3];
    }
  }
}
template <int W>
__device__ __forceinline__ void lb_sti(int32_t* p, const int32_t (&a)[W]) {
  if constexpr (W == 1) {
    *p = a[0];
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4) *reinterpret_cast<lb_i32x4*>(p + q) = lb_i32x4{a[q], a[q + 1], a[q + 2], a[q + 3]};
  }
}

// ---- the list, a slot, a row.  Every kernel takes the list it works on as ONE descriptor by value: the CSR of the engine's
// receiver-sorted list and the sizes of the padded layout, with the op's units per row (U) and lanes per row (2^lpr_shift).
// The node-parallel kernels also take the walk - the rows of their role.  Members are only ever read by name (uniform values
// in scalar registers); a run-time index into a by-value argument would go to scratch (see lb_sel3 in k_graph_features_bwd).
struct lb_glist {
  const int32_t* row_ptr;
  int64_t BN;
  int N, B, e_cap, E;
  int U, lpr_shift;
};
struct lb_gwalk {
  const int32_t *seg_ptr, *perm;   // receivers: (row_ptr, null); senders: the sender view (snd_ptr, snd_perm)
};
// a node index of the list, clamped into the batch (an index of the list is a node of the batch: never clamps)
__device__ __forceinline__ int64_t graph_clamp(const lb_glist& L, int64_t node) {
  return node < 0 ? 0 : (node >= L.BN ? L.BN - 1 : node);
}

// Padded slot r (flat over the batch): whether it is real, the slot j within its trajectory, its compact edge k, and the nodes
// idx / oidx (oidx may be null) hold for it - node 0 for a pad.
struct lb_gslot {
  bool real;
  int j, k;
  int64_t node, other;
};
__device__ __forceinline__ lb_gslot graph_slot(const lb_glist& L, int64_t r, const int32_t* __restrict__ idx,
                                              const int32_t* __restrict__ oidx = nullptr) {
  lb_gslot s;
  const int b = (int)(r / L.e_cap);
  s.j = (int)(r - (int64_t)b * L.e_cap);
  const int base = L.row_ptr[(int64_t)b * L.N], nb = L.row_ptr[(int64_t)(b + 1) * L.N] - base;
  s.k = base + s.j;
  s.real = s.j < nb && s.k < L.E;
  s.node = graph_clamp(L, s.real ? idx[s.k] : 0);
  s.other = oidx ? graph_clamp(L, s.real ? oidx[s.k] : 0) : 0;
  return s;
}

// Row i of (seg_ptr, perm): positions p0 .. p1 - 1; edge(p) is the padded slot (flat over the batch) of position p - compact
// edge k = perm ? perm[p] : p, padded slot = b E_cap + k - row_ptr[b N] - clamped into the trajectory's own E_cap slots (a
// sender view is a permutation of the trajectory's own edges: the clamp never acts on one); first is the trajectory's slot 0,
// so edge(p) - first is the slot j within it.  Pad slots are never reached.
struct lb_row {
  const int32_t* perm;
  int base, last, p0, p1;
  int64_t slot0, first;
  __device__ __forceinline__ int64_t edge(int p) const {
    int k = perm ? perm[p] : p;
    k = k < base ? base : k;
    k = k >= last ? last - 1 : k;
    return slot0 + k;
  }
};
__device__ __forceinline__ lb_row graph_row(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ seg_ptr,
                                            const int32_t* __restrict__ perm, int64_t i, int N, int e_cap, int E) {
  lb_row R;
  const int64_t b = i / N;
  R.perm = perm;
  R.base = row_ptr[b * N];
  int last = row_ptr[(b + 1) * N];   // one past the trajectory's compact edges, capped by the list and by its E_cap slots
  last = last < E ? last : E;
  R.last = last - R.base < e_cap ? last : R.base + e_cap;
  int p0 = seg_ptr[i], p1 = seg_ptr[i + 1];
  R.p0 = p0 < E ? p0 : E;
  R.p1 = p1 < E ? p1 : E;
  // a trajectory without edges has empty rows; p1 < p0 cannot happen on a valid list (seg_ptr ascends), so that guard never acts
  if (R.last <= R.base || R.p1 < R.p0) R.p1 = R.p0;
  R.first = b * e_cap;
  R.slot0 = R.first - R.base;
  return R;
}
__device__ __forceinline__ lb_row graph_row(const lb_glist& L, const lb_gwalk& walk, int64_t i) {
  return graph_row(L.row_ptr, walk.seg_ptr, walk.perm, i, L.N, L.e_cap, L.E);
}

// The loop nest of the row-shaped kernels: a group of lpr = 2^lpr_shift lanes owns row r = first, first + stride, ..., a lane
// of it the units u = lane, lane + lpr, ... of the row.  head(r) runs once per row, body(r, its result, u) per unit.
struct lb_glanes {
  int lpr, lane;
  int64_t first, stride;
};
__device__ __forceinline__ lb_glanes graph_lanes(const lb_glist& L) {
  const int lpr = 1 << L.lpr_shift;
  return {lpr, (int)threadIdx.x & (lpr - 1), (int64_t)blockIdx.x * (256 >> L.lpr_shift) + (threadIdx.x >> L.lpr_shift),
          (int64_t)gridDim.x * (256 >> L.lpr_shift)};
}
template <typename Head, typename Body>
__device__ __forceinline__ void graph_for(const lb_glist& L, int64_t rows, Head head, Body body) {
  const lb_glanes G = graph_lanes(L);
  for (int64_t r = G.first; r < rows; r += G.stride) {
    const auto h = head(r);
    for (int u = G.lane; u < L.U; u += G.lpr) body(r, h, u);
  }
}
// node-parallel: body(node i, its lb_row, u); edge-parallel: body(padded slot r, its lb_gslot, u)
template <typename Body>
__device__ __forceinline__ void graph_for_nodes(const lb_glist& L, const lb_gwalk& walk, Body body) {
  graph_for(L, L.BN, [&](int64_t i) { return graph_row(L, walk, i); }, body);
}
template <typename Body>
__device__ __forceinline__ void graph_for_slots(const lb_glist& L, const int32_t* __restrict__ idx,
                                                const int32_t* __restrict__ oidx, Body body) {
  graph_for(L, (int64_t)L.B * L.e_cap, [&](int64_t r) { return graph_slot(L, r, idx, oidx); }, body);
}

// out[slot][:] = x[idx[compact edge of the slot]][:] for the real slots, +0.0 for the pads: a bit copy of U units of type T per
// row - f32x4 (16 bytes of either element type), float, or lb_bf16; all bits zero is +0.0 in both.
template <typename T>
__global__ void __launch_bounds__(256) k_graph_gather(lb_glist L, const int32_t* __restrict__ idx, const void* __restrict__ x,
                                                      void* __restrict__ out) {
  const T* __restrict__ xs = reinterpret_cast<const T*>(x);
  T* __restrict__ os = reinterpret_cast<T*>(out);
  const int U = L.U;
  graph_for_slots(L, idx, nullptr,
                  [&](int64_t r, const lb_gslot& s, int u) { os[r * U + u] = s.real ? xs[s.node * U + u] : T{}; });
}

// out[i][:] = msg[slot of p0][:] + msg[slot of p0 + 1][:] + ... over the positions p of row i of (seg_ptr, perm): compact edge
// k = perm ? perm[p] : p, padded slot = b E_cap + k - row_ptr[b N].  +0.0 for an empty row.  Pad slots are never read.
// The adds are fp32 on the widened terms; the sum is rounded to E once, at the store.
// This kernel, the hottest of the file, keeps its own text - scalar arguments, the caps and clamps of graph_row inline, the loop
// nest of graph_for written out: through the shared descriptor and helpers it compiled to the same loop but ran 2 - 5 % slower on
// the large case, and the cause was not found in the ISA.  graph_row states the same caps (its p1 < p0 guard never acts on a
// valid list); a change to one goes into the other.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_segment_sum(const int32_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ seg_ptr,
                                                           const int32_t* __restrict__ perm, const T* __restrict__ ms,
                                                           T* __restrict__ os, int64_t BN, int N, int e_cap, int E, int U,
                                                           int lpr_shift) {
  const int lpr = 1 << lpr_shift, lane = threadIdx.x & (lpr - 1);
  const int64_t stride = (int64_t)gridDim.x * (256 >> lpr_shift);
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
      float s[W], a0[W], a1[W], a2[W], a3[W];
#pragma unroll
      for (int k = 0; k < W; ++k) s[k] = 0.f;
      int p = p0;
      if (p < p1) lb_ld<T, W>(ms + (edge(p++) * U + u) * W, s);   // the sum STARTS from the first term (-0.0 stays -0.0)
      for (; p + 4 <= p1; p += 4) {
        lb_ld<T, W>(ms + (edge(p + 0) * U + u) * W, a0);
        lb_ld<T, W>(ms + (edge(p + 1) * U + u) * W, a1);
        lb_ld<T, W>(ms + (edge(p + 2) * U + u) * W, a2);
        lb_ld<T, W>(ms + (edge(p + 3) * U + u) * W, a3);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          s[k] = s[k] + a0[k];
          s[k] = s[k] + a1[k];
          s[k] = s[k] + a2[k];
          s[k] = s[k] + a3[k];
        }
      }
      for (; p < p1; ++p) {
        lb_ld<T, W>(ms + (edge(p) * U + u) * W, a0);
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = s[k] + a0[k];
      }
      lb_st<T, W>(os + (i * U + u) * W, s);
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention ops
// degree, segment max / min, segment softmax and the fused attend, forward and backward (the contracts
// are in include/lbhip.h).  The node-parallel kernels walk a row as k_graph_segment_sum does (graph_for_nodes), the edge-parallel
// ones address a slot as k_graph_gather does (graph_slot).  A unit is W = 4 floats (one 16-byte access) or W = 1.
// -ffp-contract=off holds for this file (build.py); the attend sum spells its roundings out with __fmul_rn / __fadd_rn anyway.

// a replaces the running s: strictly greater (MIN: smaller), or a is the first NaN (np.maximum / np.minimum keep a NaN)
template <bool MIN>
__device__ __forceinline__ bool lb_beats(float a, float s) {
  return (MIN ? a < s : a > s) || (a != a && s == s);
}

__global__ void __launch_bounds__(256) k_graph_degree(lb_glist L, lb_gwalk walk, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.BN) return;
  const lb_row R = graph_row(L, walk, i);
  out[i] = R.p1 - R.p0;
}

// out[i][c] = the first real slot's value, replaced by each further slot in ascending slot order that beats it (MIN: the
// smallest); win[i][c] = the slot j (within the trajectory) that won, -1 and +0.0 for an empty row.
template <typename T, int W, bool MIN>
__global__ void __launch_bounds__(256) k_graph_segment_max(lb_glist L, lb_gwalk walk, const T* __restrict__ msg,
                                                           T* __restrict__ out, int32_t* __restrict__ win) {
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t i, const lb_row& R, int u) {
    float s[W], a[W];
    int32_t w[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = 0.f, w[k] = -1;
    int p = R.p0;
    if (p < R.p1) {
      const int64_t e = R.edge(p++);
      lb_ld<T, W>(msg + (e * U + u) * W, s);
#pragma unroll
      for (int k = 0; k < W; ++k) w[k] = (int32_t)(e - R.first);
    }
#pragma unroll 4
    for (; p < R.p1; ++p) {
      const int64_t e = R.edge(p);
      lb_ld<T, W>(msg + (e * U + u) * W, a);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (lb_beats<MIN>(a[k], s[k])) s[k] = a[k], w[k] = (int32_t)(e - R.first);
    }
    lb_st<T, W>(out + (i * U + u) * W, s);
    lb_sti<W>(win + (i * U + u) * W, w);
  });
}

// d_msg[slot][c] = d_out[node][c] where the slot won column c of its node, +0.0 in every other real slot and in the pads.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_segment_max_bwd(lb_glist L, const int32_t* __restrict__ idx,
                                                               const T* __restrict__ d_out, const int32_t* __restrict__ win,
                                                               T* __restrict__ d_msg) {
  const int U = L.U;
  graph_for_slots(L, idx, nullptr, [&](int64_t r, const lb_gslot& s, int u) {
    float d[W], g[W];
    int32_t w[W];
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = 0.f;
    if (s.real) {
      lb_ld<T, W>(d_out + (s.node * U + u) * W, g);
      lb_ldi<W>(win + (s.node * U + u) * W, w);
#pragma unroll
      for (int k = 0; k < W; ++k) d[k] = w[k] == s.j ? g[k] : 0.f;
    }
    lb_st<T, W>(d_msg + (r * U + u) * W, d);
  });
}

// y[slot][c] = expf(x[slot][c] - m) / s over the slots of node i: m the maximum as in k_graph_segment_max, s the ordered sum of
// the exponentials.  The group that owns the node writes the node's slots; the pad slots were zeroed before the launch.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_softmax(lb_glist L, lb_gwalk walk, const T* __restrict__ x, T* __restrict__ y) {
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t, const lb_row& R, int u) {
    if (R.p0 >= R.p1) return;
    float m[W], s[W], a[W];
    lb_ld<T, W>(x + (R.edge(R.p0) * U + u) * W, m);
#pragma unroll 4
    for (int p = R.p0 + 1; p < R.p1; ++p) {
      lb_ld<T, W>(x + (R.edge(p) * U + u) * W, a);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (lb_beats<false>(a[k], m[k])) m[k] = a[k];
    }
    lb_ld<T, W>(x + (R.edge(R.p0) * U + u) * W, a);
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = expf(a[k] - m[k]);
#pragma unroll 4
    for (int p = R.p0 + 1; p < R.p1; ++p) {
      lb_ld<T, W>(x + (R.edge(p) * U + u) * W, a);
#pragma unroll
      for (int k = 0; k < W; ++k) s[k] = __fadd_rn(s[k], expf(a[k] - m[k]));
    }
#pragma unroll 4
    for (int p = R.p0; p < R.p1; ++p) {
      const int64_t o = (R.edge(p) * U + u) * W;
      lb_ld<T, W>(x + o, a);
#pragma unroll
      for (int k = 0; k < W; ++k) a[k] = expf(a[k] - m[k]) / s[k];
      lb_st<T, W>(y + o, a);
    }
  });
}

// d_x[slot][c] = y (d_y - sum_k d_y[k] y[k]) over the slots of node i, the sum ordered; the pads were zeroed before the launch.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_softmax_bwd(lb_glist L, lb_gwalk walk, const T* __restrict__ y,
                                                           const T* __restrict__ d_y, T* __restrict__ d_x) {
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t, const lb_row& R, int u) {
    if (R.p0 >= R.p1) return;
    float dot[W], a[W], g[W];
    {
      const int64_t o = (R.edge(R.p0) * U + u) * W;
      lb_ld<T, W>(y + o, a);
      lb_ld<T, W>(d_y + o, g);
#pragma unroll
      for (int k = 0; k < W; ++k) dot[k] = __fmul_rn(g[k], a[k]);
    }
#pragma unroll 4
    for (int p = R.p0 + 1; p < R.p1; ++p) {
      const int64_t o = (R.edge(p) * U + u) * W;
      lb_ld<T, W>(y + o, a);
      lb_ld<T, W>(d_y + o, g);
#pragma unroll
      for (int k = 0; k < W; ++k) dot[k] = __fadd_rn(dot[k], __fmul_rn(g[k], a[k]));
    }
#pragma unroll 4
    for (int p = R.p0; p < R.p1; ++p) {
      const int64_t o = (R.edge(p) * U + u) * W;
      lb_ld<T, W>(y + o, a);
      lb_ld<T, W>(d_y + o, g);
#pragma unroll
      for (int k = 0; k < W; ++k) a[k] = __fmul_rn(a[k], g[k] - dot[k]);
      lb_st<T, W>(d_x + o, a);
    }
  });
}

// out[i][h][:] = sum over the slots of node i of alpha[slot][h] v[slot][h][:], alpha = expf(l - m) / s as k_graph_softmax computes
// it: the product rounded, the adds in ascending slot order from the first term.  A lane owns units of the H D row and runs the
// max and the sum pass over its head's logits itself (kept from one unit of the row to the next while the head stays: hc, m,
// s); the lane of a head's first unit stores that head's m and s.  That state lives across the units of a row, so this kernel
// spells the two loops of graph_for out: carried through graph_for's callables (in a struct the head returns, or in captured
// locals) the same source compiled to a bfloat16 sender walk 4 % slower.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_attend(lb_glist L, lb_gwalk walk, const T* __restrict__ logits,
                                                      const T* __restrict__ values, T* __restrict__ out,
                                                      float* __restrict__ m_out, float* __restrict__ s_out, int H, int D) {
  const int U = L.U;
  const lb_glanes G = graph_lanes(L);
  for (int64_t i = G.first; i < L.BN; i += G.stride) {
    const lb_row R = graph_row(L, walk, i);
    int hc = -1;
    float m = 0.f, s = 1.f;
    for (int u = G.lane; u < U; u += G.lpr) {
      const int h = (u * W) / D;
      float acc[W], v[W];
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] = 0.f;
      if (R.p0 < R.p1) {
        if (h != hc) {
          hc = h;
          m = lb_ld1<T>(logits + R.edge(R.p0) * H + h);
#pragma unroll 4
          for (int p = R.p0 + 1; p < R.p1; ++p) {
            const float a = lb_ld1<T>(logits + R.edge(p) * H + h);
            if (lb_beats<false>(a, m)) m = a;
          }
          s = expf(lb_ld1<T>(logits + R.edge(R.p0) * H + h) - m);
#pragma unroll 4
          for (int p = R.p0 + 1; p < R.p1; ++p) s = __fadd_rn(s, expf(lb_ld1<T>(logits + R.edge(p) * H + h) - m));
        }
        {
          const int64_t e = R.edge(R.p0);
          const float al = expf(lb_ld1<T>(logits + e * H + h) - m) / s;
          lb_ld<T, W>(values + (e * U + u) * W, v);
#pragma unroll
          for (int k = 0; k < W; ++k) acc[k] = __fmul_rn(al, v[k]);
        }
#pragma unroll 4
        for (int p = R.p0 + 1; p < R.p1; ++p) {
          const int64_t e = R.edge(p);
          const float al = expf(lb_ld1<T>(logits + e * H + h) - m) / s;
          lb_ld<T, W>(values + (e * U + u) * W, v);
#pragma unroll
          for (int k = 0; k < W; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(al, v[k]));
        }
      }
      lb_st<T, W>(out + (i * U + u) * W, acc);
      if ((u * W) % D == 0) m_out[i * H + h] = m, s_out[i * H + h] = s;
    }
  }
}

// d_values[slot][h][:] = alpha[slot][h] d_out[node][h][:] (one multiplication), +0.0 in the pads; alpha recomputed from the
// saved m and s of the node.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_attend_dvalues(lb_glist L, const int32_t* __restrict__ idx,
                                                              const T* __restrict__ logits, const float* __restrict__ m_in,
                                                              const float* __restrict__ s_in, const T* __restrict__ d_out,
                                                              T* __restrict__ d_values, int H, int D) {
  const int U = L.U;
  graph_for_slots(L, idx, nullptr, [&](int64_t r, const lb_gslot& s, int u) {
    float d[W], g[W];
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = 0.f;
    if (s.real) {
      const int h = (u * W) / D;
      const float al = expf(lb_ld1<T>(logits + r * H + h) - m_in[s.node * H + h]) / s_in[s.node * H + h];
      lb_ld<T, W>(d_out + (s.node * U + u) * W, g);
#pragma unroll
      for (int k = 0; k < W; ++k) d[k] = __fmul_rn(al, g[k]);
    }
    lb_st<T, W>(d_values + (r * U + u) * W, d);
  });
}

// t[slot][h] = sum_d d_out[node][h][d] v[slot][h][d], one lane per (slot, head), d ascending; +0.0 in the pads.  t is fp32:
// for float tensors it IS the d_logits buffer; for bf16 ones it is the engine's buffer, and every slot of d_logits gets +0.0
// here (k_graph_attend_dlogits then writes the real slots).
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_attend_t(lb_glist L, const int32_t* __restrict__ idx, const T* __restrict__ values,
                                                        const T* __restrict__ d_out, float* __restrict__ t, T* d_logits, int H,
                                                        int D) {
  const int64_t total = (int64_t)L.B * L.e_cap * H, stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
    const int64_t r = q / H;
    const int h = (int)(q - r * H);
    const lb_gslot s = graph_slot(L, r, idx);
    float acc = 0.f;
    if (s.real) {
      const T* __restrict__ vp = values + (r * H + h) * D;
      const T* __restrict__ gp = d_out + (s.node * H + h) * D;
      float v[W], g[W];
      bool first = true;
      for (int d = 0; d < D; d += W) {
        lb_ld<T, W>(vp + d, v);
        lb_ld<T, W>(gp + d, g);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const float pr = __fmul_rn(g[k], v[k]);
          acc = first ? pr : __fadd_rn(acc, pr);
          first = false;
        }
      }
    }
    t[q] = acc;
    if constexpr (sizeof(T) != 4) d_logits[q] = 0;
  }
}

// d_logits[slot][h] = alpha (t[slot][h] - sum_k alpha[k] t[k][h]) over the slots of node i, t (B E_cap, H) fp32, the sum ordered;
// one lane per (node, head).  In place on t for float tensors (d_logits == t); rounded once into d_logits for bf16 ones.  The
// pad slots hold the +0.0 k_graph_attend_t wrote.
template <typename T>
__global__ void __launch_bounds__(256) k_graph_attend_dlogits(lb_glist L, lb_gwalk walk, const T* __restrict__ logits,
                                                              const float* __restrict__ m_in, const float* __restrict__ s_in,
                                                              const float* t, T* d_logits, int H) {
  const int64_t total = L.BN * H, stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
    const int64_t i = q / H;
    const int h = (int)(q - i * H);
    const lb_row R = graph_row(L, walk, i);
    if (R.p0 >= R.p1) continue;
    const float m = m_in[q], s = s_in[q];
    float dot;
    {
      const int64_t o = R.edge(R.p0) * H + h;
      dot = __fmul_rn(expf(lb_ld1<T>(logits + o) - m) / s, t[o]);
    }
    for (int p = R.p0 + 1; p < R.p1; ++p) {
      const int64_t o = R.edge(p) * H + h;
      dot = __fadd_rn(dot, __fmul_rn(expf(lb_ld1<T>(logits + o) - m) / s, t[o]));
    }
    for (int p = R.p0; p < R.p1; ++p) {
      const int64_t o = R.edge(p) * H + h;
      lb_st1<T>(d_logits + o, __fmul_rn(expf(lb_ld1<T>(logits + o) - m) / s, t[o] - dot));
    }
  }
}

// ------------------------------------------------------------------------------------------------ edge messages
// conv, pair_mul and pair_add (the contracts are in include/lbhip.h): the "filter x neighbour" message of a
// continuous-filter or equivariant network without its edge-shaped intermediates.  conv walks the rows of its role as
// k_graph_segment_sum does and reads, per slot, the w row of the slot and the x row of the slot's OTHER node (oidx: the compact
// list of the other role, at the compact edge lb_row::edge resolved); pair_mul / pair_add address a slot as k_graph_gather does
// and read one node row per role.  x, a and b are (B N, K, C), w and the edge-shaped outputs (B E_cap, C): a unit divides C, so
// a lane holds one w unit per slot and loops k.  Every product is one __fmul_rn, every sum starts from its first term and adds
// one __fadd_rn per further term - slots ascending in conv, k ascending in pair_mul.
//
// One slot's loads for k-chunk k0 .. k0 + KT - 1: the w unit and KT x units (a k past K - 1 re-reads row K - 1; never stored).
template <typename T, int W, int KT>
__device__ __forceinline__ void graph_conv_load(const lb_row& R, int p, const int32_t* __restrict__ oidx, const T* __restrict__ x,
                                                const T* __restrict__ w, const lb_glist& L, int K, int k0, int U, int u,
                                                float (&f)[W], float (&a)[KT][W]) {
  const int64_t e = R.edge(p);
  const int64_t node = graph_clamp(L, oidx[e - R.slot0]);
  lb_ld<T, W>(w + (e * U + u) * W, f);
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const int k = k0 + q < K ? k0 + q : K - 1;
    lb_ld<T, W>(x + ((node * K + k) * U + u) * W, a[q]);
  }
}
// out[i][k][:] = sum over the slots of row i, ascending, of fl32(x[other node of the slot][k][:] * w[slot][:]); +0.0 for an empty
// row.  KT accumulator rows per pass over the slots (1 for K = 1; 3 for K > 1: a vector feature), SU slots' loads in flight; the
// adds sequential.
template <typename T, int W, int KT>
__global__ void __launch_bounds__(256) k_graph_conv(lb_glist L, lb_gwalk walk, const int32_t* __restrict__ oidx,
                                                    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ out, int K) {
  constexpr int SU = KT == 1 ? 4 : 2;
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t i, const lb_row& R, int u) {
    for (int k0 = 0; k0 < K; k0 += KT) {
      float s[KT][W], f[SU][W], a[SU][KT][W];
#pragma unroll
      for (int q = 0; q < KT; ++q)
#pragma unroll
        for (int c = 0; c < W; ++c) s[q][c] = 0.f;
      int p = R.p0;
      if (p < R.p1) {   // the sum STARTS from the first product
        graph_conv_load<T, W, KT>(R, p++, oidx, x, w, L, K, k0, U, u, f[0], a[0]);
#pragma unroll
        for (int q = 0; q < KT; ++q)
#pragma unroll
          for (int c = 0; c < W; ++c) s[q][c] = __fmul_rn(a[0][q][c], f[0][c]);
      }
      for (; p + SU <= R.p1; p += SU) {
#pragma unroll
        for (int t = 0; t < SU; ++t) graph_conv_load<T, W, KT>(R, p + t, oidx, x, w, L, K, k0, U, u, f[t], a[t]);
#pragma unroll
        for (int t = 0; t < SU; ++t)
#pragma unroll
          for (int q = 0; q < KT; ++q)
#pragma unroll
            for (int c = 0; c < W; ++c) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(a[t][q][c], f[t][c]));
      }
      for (; p < R.p1; ++p) {
        graph_conv_load<T, W, KT>(R, p, oidx, x, w, L, K, k0, U, u, f[0], a[0]);
#pragma unroll
        for (int q = 0; q < KT; ++q)
#pragma unroll
          for (int c = 0; c < W; ++c) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(a[0][q][c], f[0][c]));
      }
#pragma unroll
      for (int q = 0; q < KT; ++q)
        if (k0 + q < K) lb_st<T, W>(out + ((i * K + k0 + q) * U + u) * W, s[q]);
    }
  });
}

// The pair ops: a, b (B N, K, C), one unit of a's row of the slot's a node combined with b's of its b node, +0.0 in the pads.
//   MUL: out[slot][:] = fl32(a[a node][0][:] * b[b node][0][:]) + fl32(a[..][1][:] * b[..][1][:]) + ... (k ascending, the first
//        product starts the sum).  SUM_K false is K = 1, the plain product (no k loop, its registers); true is conv's d_w.
//   ADD: out[slot][:] = fl32(a[a node][:] + b[b node][:]) (K = 1).
template <typename T, int W, bool MUL, bool SUM_K>
__device__ __forceinline__ void graph_pair_body(const lb_glist& L, const int32_t* __restrict__ aidx,
                                                const int32_t* __restrict__ bidx, const T* __restrict__ a,
                                                const T* __restrict__ b, T* __restrict__ out, int K_) {
  const int K = SUM_K ? K_ : 1, U = L.U;
  graph_for_slots(L, aidx, bidx, [&](int64_t r, const lb_gslot& t, int u) {
    const int64_t na = t.node, nn = t.other;
    float s[W], fa[W], fb[W];
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] = 0.f;
    if (t.real) {
      lb_ld<T, W>(a + (na * K * U + u) * W, fa);
      lb_ld<T, W>(b + (nn * K * U + u) * W, fb);
#pragma unroll
      for (int c = 0; c < W; ++c) s[c] = MUL ? __fmul_rn(fa[c], fb[c]) : __fadd_rn(fa[c], fb[c]);
#pragma unroll 4
      for (int k = 1; k < K; ++k) {
        lb_ld<T, W>(a + ((na * K + k) * U + u) * W, fa);
        lb_ld<T, W>(b + ((nn * K + k) * U + u) * W, fb);
#pragma unroll
        for (int c = 0; c < W; ++c) s[c] = __fadd_rn(s[c], __fmul_rn(fa[c], fb[c]));
      }
    }
    lb_st<T, W>(out + (r * U + u) * W, s);
  });
}
template <typename T, int W, bool SUM_K>
__global__ void __launch_bounds__(256) k_graph_pair_mul(lb_glist L, const int32_t* __restrict__ aidx,
                                                        const int32_t* __restrict__ bidx, const T* __restrict__ a,
                                                        const T* __restrict__ b, T* __restrict__ out, int K) {
  graph_pair_body<T, W, true, SUM_K>(L, aidx, bidx, a, b, out, K);
}
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_pair_add(lb_glist L, const int32_t* __restrict__ aidx,
                                                        const int32_t* __restrict__ bidx, const T* __restrict__ a,
                                                        const T* __restrict__ b, T* __restrict__ out) {
  graph_pair_body<T, W, false, false>(L, aidx, bidx, a, b, out, 1);
}

// ---- edge pairs: an edge (s -> r) beside its transpose (r -> s).
// The reverse map, rev (B E_cap) int32: for the real slot of (receiver r, sender s) the slot j' within its trajectory of the edge
// (receiver s, sender r), -1 where the list does not hold that edge (tests/_asym.py) and in every pad slot; a self-edge maps to
// itself.  One lane per padded slot bisects the CSR row of its sender for its receiver - the arithmetic of k_sender_transpose
// (lb_sender_view.h); a row holds a sender at most once (lb_neighbor.hip: a receiver meets every particle of its stencil once), so
// the first position whose sender is >= r is the only candidate - and turns the compact edge it finds into a padded slot as
// lb_row::edge does: k - row_ptr[b N], here refused (-1) rather than clamped when it falls outside the trajectory's own real
// slots, which a valid list never does.  By construction rev[rev[j]] == j wherever rev[j] >= 0.  No flag, no atomics.
__global__ void __launch_bounds__(256) k_graph_reverse(lb_glist L, const int32_t* __restrict__ senders,
                                                       const int32_t* __restrict__ receivers, int32_t* __restrict__ rev) {
  const int64_t rows = (int64_t)L.B * L.e_cap;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows; q += (int64_t)gridDim.x * 256) {
    const lb_gslot t = graph_slot(L, q, receivers, senders);   // node: the receiver r, other: the sender s (both clamped)
    int32_t found = -1;
    if (t.real) {
      const int r = (int)t.node, s = (int)t.other;
      int lo = L.row_ptr[s], hi = L.row_ptr[s + 1];   // first position of row s whose sender is >= r
      hi = hi < L.E ? hi : L.E;
      lo = lo < 0 ? 0 : lo;
      const int end = hi;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (senders[mid] < r) lo = mid + 1; else hi = mid;
      }
      if (lo < end && senders[lo] == r) {
        const int base = t.k - t.j, jr = lo - base;   // the trajectory's first compact edge; the transpose's slot within it
        int nb = L.row_ptr[(int64_t)(q / L.e_cap + 1) * L.N] - base;
        nb = nb < L.e_cap ? nb : L.e_cap;
        if (jr >= 0 && jr < nb) found = jr;
      }
    }
    rev[q] = found;
  }
}

// swap / symmetrize / antisymmetrize, one kernel with a mode: out[slot][:] = msg[partner][:] (a bit copy), fl32(msg[slot][:] +
// msg[partner][:]) or fl32(msg[slot][:] - msg[partner][:]) for a real slot whose rev entry names a partner; +0.0 for a slot
// without one and for every pad.  Edge-parallel in the shape of the pair ops: a lane group per padded slot, one scattered row
// read (the partner's) beside the streamed one.  rev is -1 in the pads, so a pad slot of msg is never read; the partner of a real
// slot is a real slot of the same trajectory (v < E_cap is checked: no address leaves the tensor).
struct lb_gpartner {
  bool paired;
  int64_t q;   // the partner's padded slot, flat over the batch
};
template <typename T, int W, int MODE>
__global__ void __launch_bounds__(256) k_graph_edge_pair(lb_glist L, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ rev, const T* __restrict__ msg,
                                                         T* __restrict__ out) {
  const int U = L.U;
  graph_for(
      L, (int64_t)L.B * L.e_cap,
      [&](int64_t r) {
        const lb_gslot t = graph_slot(L, r, idx);
        const int v = t.real ? rev[r] : -1;
        const bool paired = v >= 0 && v < L.e_cap;
        return lb_gpartner{paired, r - t.j + (paired ? v : 0)};
      },
      [&](int64_t r, const lb_gpartner& p, int u) {
        if constexpr (MODE == LB_GRAPH_PAIR_SWAP) {   // the bits as they are: 16 bytes of either element type, or one element
          using V = std::conditional_t<(W > 1), f32x4, T>;
          const V* __restrict__ ms = reinterpret_cast<const V*>(msg);
          V* __restrict__ os = reinterpret_cast<V*>(out);
          os[r * U + u] = p.paired ? ms[p.q * U + u] : V{};
        } else {
          float s[W], fa[W], fb[W];
#pragma unroll
          for (int c = 0; c < W; ++c) s[c] = 0.f;
          if (p.paired) {
            lb_ld<T, W>(msg + (r * U + u) * W, fa);
            lb_ld<T, W>(msg + (p.q * U + u) * W, fb);
#pragma unroll
            for (int c = 0; c < W; ++c) s[c] = MODE == LB_GRAPH_PAIR_SYM ? __fadd_rn(fa[c], fb[c]) : __fsub_rn(fa[c], fb[c]);
          }
          lb_st<T, W>(out + (r * U + u) * W, s);
        }
      });
}

// conv_vec and conv_dot: the scalar <-> vector couplings of an equivariant layer through a per-edge vector u (B E_cap, K), K <= 9
// (rel_disp, or spherical harmonics up to l = 2), without the (B E_cap, K, C) product.  Both walk the rows of their role as conv
// does; u rows are K elements wide (12 bytes at K = 3), so u is read with scalar loads - one address per lane group, a broadcast.
//
// One slot's loads of conv_vec for k-chunk k0 .. k0 + KT - 1: the w unit, the x unit of the other node and KT scalars of u (a k
// past K - 1 re-reads column K - 1; never stored).
template <typename T, int W, int KT>
__device__ __forceinline__ void graph_conv_vec_load(const lb_row& R, int p, const int32_t* __restrict__ oidx,
                                                    const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ uv,
                                                    const lb_glist& L, int K, int k0, int U, int u, float (&f)[W], float (&a)[W],
                                                    float (&g)[KT]) {
  const int64_t e = R.edge(p);
  const int64_t node = graph_clamp(L, oidx[e - R.slot0]);
  lb_ld<T, W>(w + (e * U + u) * W, f);
  lb_ld<T, W>(x + (node * U + u) * W, a);
#pragma unroll
  for (int q = 0; q < KT; ++q) g[q] = lb_ld1<T>(uv + e * K + (k0 + q < K ? k0 + q : K - 1));
}
// out[i][k][:] = sum over the slots of row i, ascending, of fl32(fl32(x[other node of the slot][:] * w[slot][:]) * u[slot][k]);
// +0.0 for an empty row.  KT accumulator rows per pass over the slots (1 for K = 1, 3 for K > 1, as k_graph_conv: nine rows of a
// bf16 unit would be 72 accumulators beside the loads in flight; K = 3, the common case, is one pass), SU slots' loads in flight;
// the adds sequential.
template <typename T, int W, int KT>
__global__ void __launch_bounds__(256) k_graph_conv_vec(lb_glist L, lb_gwalk walk, const int32_t* __restrict__ oidx,
                                                        const T* __restrict__ x, const T* __restrict__ w,
                                                        const T* __restrict__ uv, T* __restrict__ out, int K) {
  constexpr int SU = KT == 1 ? 4 : 2;
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t i, const lb_row& R, int u) {
    for (int k0 = 0; k0 < K; k0 += KT) {
      float s[KT][W], f[SU][W], a[SU][W], g[SU][KT];
#pragma unroll
      for (int q = 0; q < KT; ++q)
#pragma unroll
        for (int c = 0; c < W; ++c) s[q][c] = 0.f;
      int p = R.p0;
      if (p < R.p1) {   // the sum STARTS from the first product
        graph_conv_vec_load<T, W, KT>(R, p++, oidx, x, w, uv, L, K, k0, U, u, f[0], a[0], g[0]);
#pragma unroll
        for (int c = 0; c < W; ++c) {
          const float xw = __fmul_rn(a[0][c], f[0][c]);
#pragma unroll
          for (int q = 0; q < KT; ++q) s[q][c] = __fmul_rn(xw, g[0][q]);
        }
      }
      for (; p + SU <= R.p1; p += SU) {
#pragma unroll
        for (int t = 0; t < SU; ++t) graph_conv_vec_load<T, W, KT>(R, p + t, oidx, x, w, uv, L, K, k0, U, u, f[t], a[t], g[t]);
#pragma unroll
        for (int t = 0; t < SU; ++t)
#pragma unroll
          for (int c = 0; c < W; ++c) {
            const float xw = __fmul_rn(a[t][c], f[t][c]);
#pragma unroll
            for (int q = 0; q < KT; ++q) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(xw, g[t][q]));
          }
      }
      for (; p < R.p1; ++p) {
        graph_conv_vec_load<T, W, KT>(R, p, oidx, x, w, uv, L, K, k0, U, u, f[0], a[0], g[0]);
#pragma unroll
        for (int c = 0; c < W; ++c) {
          const float xw = __fmul_rn(a[0][c], f[0][c]);
#pragma unroll
          for (int q = 0; q < KT; ++q) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(xw, g[0][q]));
        }
      }
#pragma unroll
      for (int q = 0; q < KT; ++q)
        if (k0 + q < K) lb_st<T, W>(out + ((i * K + k0 + q) * U + u) * W, s[q]);
    }
  });
}

// t[:] = fl32(v[node][0][:] * u[slot][0]) + fl32(v[node][1][:] * u[slot][1]) + ... (k ascending, the first product starts the
// sum): one unit of the per-edge contraction of a vector feature with u (the edge gradients form the same t from the V units
// they hold anyway).
template <typename T, int W>
__device__ __forceinline__ void graph_vec_dot(const T* __restrict__ v, const T* __restrict__ uv, int64_t node, int64_t e, int K,
                                              int U, int u, float (&t)[W]) {
  float a[W];
  lb_ld<T, W>(v + (node * K * U + u) * W, a);
  float g = lb_ld1<T>(uv + e * K);
#pragma unroll
  for (int c = 0; c < W; ++c) t[c] = __fmul_rn(a[c], g);
#pragma unroll 4
  for (int k = 1; k < K; ++k) {
    lb_ld<T, W>(v + ((node * K + k) * U + u) * W, a);
    g = lb_ld1<T>(uv + e * K + k);
#pragma unroll
    for (int c = 0; c < W; ++c) t[c] = __fadd_rn(t[c], __fmul_rn(a[c], g));
  }
}
// out[i][:] = sum over the slots of row i, ascending, of fl32(w[slot][:] * t[slot][:]), t of the slot's other node as above; +0.0
// for an empty row.  One accumulator row; two slots' loads (a w unit, K v units, K scalars of u each) in flight, the adds sequential.
template <typename T, int W>
__global__ void __launch_bounds__(256) k_graph_conv_dot(lb_glist L, lb_gwalk walk, const int32_t* __restrict__ oidx,
                                                        const T* __restrict__ v, const T* __restrict__ w,
                                                        const T* __restrict__ uv, T* __restrict__ out, int K) {
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t i, const lb_row& R, int u) {
    float s[W], f[2][W], t[2][W];
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] = 0.f;
    auto term = [&](int p, float (&fw)[W], float (&tt)[W]) {
      const int64_t e = R.edge(p);
      lb_ld<T, W>(w + (e * U + u) * W, fw);
      graph_vec_dot<T, W>(v, uv, graph_clamp(L, oidx[e - R.slot0]), e, K, U, u, tt);
    };
    int p = R.p0;
    if (p < R.p1) {   // the sum STARTS from the first product
      term(p++, f[0], t[0]);
#pragma unroll
      for (int c = 0; c < W; ++c) s[c] = __fmul_rn(f[0][c], t[0][c]);
    }
    for (; p + 2 <= R.p1; p += 2) {
      term(p, f[0], t[0]);
      term(p + 1, f[1], t[1]);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        s[c] = __fadd_rn(s[c], __fmul_rn(f[0][c], t[0][c]));
        s[c] = __fadd_rn(s[c], __fmul_rn(f[1][c], t[1][c]));
      }
    }
    if (p < R.p1) {
      term(p, f[0], t[0]);
#pragma unroll
      for (int c = 0; c < W; ++c) s[c] = __fadd_rn(s[c], __fmul_rn(f[0][c], t[0][c]));
    }
    lb_st<T, W>(out + (i * U + u) * W, s);
  });
}

// The edge gradients of both ops, from a scalar-side node tensor S (B N, C), read at the slot's node of `idx`, and a vector-side
// one V (B N, K, C), read at its node of `oidx`:
//   d_w[slot][c] = fl32(S[c] * t[c]), t the contraction of V with u above;
//   d_u[slot][k] = sum over c of fl32(fl32(S[c] * w[slot][c]) * V[k][c]) in the FIXED order of LB_GRAPH_DU_BLOCK (include/lbhip.h):
//                  consecutive blocks of 16 columns, c ascending inside a block from its first product, the block sums added in
//                  ascending block order from the first one - whatever the unit width, the lanes per slot or the element type.
// +0.0 in the pad slots of both.  A group of 2^lpr_shift lanes owns a slot and a lane the units lane, lane + lpr, ... as in the
// pair kernels, so every load and the d_w store is one contiguous run per slot.  A block of 16 columns is BL = 16 / W
// neighbouring lanes (W divides C and 16: a unit lies in one block; the last block may be short).  Its sum is a chain along
// those lanes: the block's first lane adds its W products from the first one, each further lane takes its neighbour's partial
// sum (one shuffle per k) and adds its own W products to it, c ascending - BL - 1 steps, every block of the wave at once.  The
// block sums, held by each block's last lane, are then added in ascending block order (one shuffle per block and k); every
// lane of the group holds the running sum, which carries over the rounds of a row wider than the group; lane 0 stores it.
// (Lanes that own whole blocks need no chain, but read 16 bytes at a stride of 64, four times the cache lines per load: that
// form ran clearly slower.)  Both outputs share the loads of S, V, w
// and u; a null output is not computed.  KM: the k rows held in registers - 3 for K <= 3, LB_GRAPH_MAX_K otherwise.  The
// slot's state lives across its units, so this kernel spells graph_for's two loops out, as k_graph_attend does.
#define LB_GRAPH_MAX_K 9
template <typename T, int W, int KM>
__global__ void __launch_bounds__(256) k_graph_vec_edge_grad(lb_glist L, const int32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ oidx, const T* __restrict__ S,
                                                             const T* __restrict__ V, const T* __restrict__ w,
                                                             const T* __restrict__ uv, T* __restrict__ d_w, T* __restrict__ d_u,
                                                             int K) {
  static_assert(LB_GRAPH_DU_BLOCK % W == 0, "a unit lies in one block");
  constexpr int BL = LB_GRAPH_DU_BLOCK / W;   // lanes of one block
  const int U = L.U;
  const lb_glanes G = graph_lanes(L);
  const int lane0 = ((int)threadIdx.x & 63) - G.lane, pos = G.lane & (BL - 1);   // the group's first lane; this lane in its block
  const int64_t rows = (int64_t)L.B * L.e_cap;
  for (int64_t r = G.first; r < rows; r += G.stride) {
    const lb_gslot sl = graph_slot(L, r, idx, oidx);   // (uniform over the group)
    float tot[KM], g[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) tot[k] = 0.f, g[k] = 0.f;
    if (sl.real) {
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) g[k] = lb_ld1<T>(uv + r * K + k);
    }
    for (int u0 = 0; u0 < U; u0 += G.lpr) {   // one round: unit u0 + lane of every lane (uniform trip count)
      const int u = u0 + G.lane, live = U - u0 < G.lpr ? U - u0 : G.lpr;   // live: the round's units
      float du[KM][W], part[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        part[k] = 0.f;
#pragma unroll
        for (int c = 0; c < W; ++c) du[k][c] = 0.f;
      }
      if (u < U) {
        float dw[W];
#pragma unroll
        for (int c = 0; c < W; ++c) dw[c] = 0.f;
        if (sl.real) {
          float s[W], f[W], t[W];
          lb_ld<T, W>(S + (sl.node * U + u) * W, s);
          lb_ld<T, W>(w + (r * U + u) * W, f);
#pragma unroll
          for (int k = 0; k < KM; ++k)
            if (k < K) lb_ld<T, W>(V + ((sl.other * K + k) * U + u) * W, du[k]);
#pragma unroll
          for (int c = 0; c < W; ++c) f[c] = __fmul_rn(s[c], f[c]), t[c] = 0.f;   // fl32(S w)
#pragma unroll
          for (int k = 0; k < KM; ++k)
            if (k < K) {
#pragma unroll
              for (int c = 0; c < W; ++c) {
                const float tv = __fmul_rn(du[k][c], g[k]);
                t[c] = k == 0 ? tv : __fadd_rn(t[c], tv);
                du[k][c] = __fmul_rn(f[c], du[k][c]);
              }
            }
#pragma unroll
          for (int c = 0; c < W; ++c) dw[c] = __fmul_rn(s[c], t[c]);
        }
        if (d_w) lb_st<T, W>(d_w + (r * U + u) * W, dw);
      }
      if (d_u && sl.real) {
        // the chain along the lanes of a block: step j is the block's lane j (all blocks of the wave at once)
#pragma unroll
        for (int j = 0; j < BL; ++j) {
          if (j < live) {   // (uniform; a round shorter than a block ends its chain early)
#pragma unroll
            for (int k = 0; k < KM; ++k)
              if (k < K) {
                float v = j == 0 ? 0.f : __shfl_up(part[k], 1);
                if (pos == j) {
                  v = j == 0 ? du[k][0] : __fadd_rn(v, du[k][0]);
#pragma unroll
                  for (int c = 1; c < W; ++c) v = __fadd_rn(v, du[k][c]);
                  part[k] = v;
                }
              }
          }
        }
        // the block sums in ascending block order, from each block's last live lane
        for (int b = 0; b * BL < live; ++b) {
          const int end = ((b + 1) * BL < live ? (b + 1) * BL : live) - 1;
#pragma unroll
          for (int k = 0; k < KM; ++k)
            if (k < K) {
              const float v = __shfl(part[k], lane0 + end);
              tot[k] = (u0 == 0 && b == 0) ? v : __fadd_rn(tot[k], v);
            }
        }
      }
    }
    if (d_u && G.lane == 0) {
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) lb_st1<T>(d_u + r * K + k, tot[k]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ filter_conv
// conv with its filter formed in registers: wf[slot][c] = fl32(f[slot][0] * weight[0][c]) + fl32(f[slot][1] * weight[1][c]) + ...
// (r ascending, the first product starts the sum) from a per-edge basis f (B E_cap, R), R <= LB_GRAPH_MAX_R, and a weight (R, C)
// shared by the batch (the contract is in include/lbhip.h).  wf never reaches memory.
//
// Where the weight lives.  A lane owns unit u of a row and needs the R x W weight columns of that unit - at most 32 x 4 floats,
// which it keeps in registers (bfloat16 rows are read in 8-byte units here, W = 4, so that they fit).  A lane's unit does not change
// from one row to the next while a row is no wider than its lane group (C <= 256), so the weight is loaded once per lane and
// kernel; a wider row reloads it per unit from L1 / L2, once per row, not per slot.  That state lives across rows, so the kernel
// spells graph_for's two loops out, as k_graph_attend does.  RM: the r rows held (20 - PaiNN's n_rbf - or 32); rows past R are zero, their
// terms are formed and dropped by a select - no branch in the slot loop, and every f load of a slot is issued before its use.
// f rows are R elements wide (80 bytes at R = 20): one address per lane group, a broadcast, as u is read in conv_vec - four
// elements per load when R % 4 == 0 and f is 16-byte aligned (FV), scalar loads otherwise; an r past R - 1 re-reads the row's end.
template <typename T, int W, int RM>
__device__ __forceinline__ void graph_filter_unit(const float (&fr)[RM], const float (&wt)[RM][W], int R, float (&wf)[W]) {
#pragma unroll
  for (int c = 0; c < W; ++c) wf[c] = __fmul_rn(fr[0], wt[0][c]);
#pragma unroll
  for (int r = 1; r < RM; ++r)
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const float t = __fadd_rn(wf[c], __fmul_rn(fr[r], wt[r][c]));
      wf[c] = r < R ? t : wf[c];
    }
}
// One slot's loads for k-chunk k0 .. k0 + KT - 1: the R scalars of f and KT x units of the slot's other node.
template <typename T, int W, int KT, int RM, bool FV>
__device__ __forceinline__ void graph_filter_load(const lb_row& Rw, int p, const int32_t* __restrict__ oidx,
                                                  const T* __restrict__ x, const T* __restrict__ f, const lb_glist& L, int K, int k0,
                                                  int R, int U, int u, float (&fr)[RM], float (&a)[KT][W]) {
  const int64_t e = Rw.edge(p);
  const int64_t node = graph_clamp(L, oidx[e - Rw.slot0]);
  if constexpr (FV) {   // R % 4 == 0 and f aligned: four elements per load; a group past R re-reads the last one
    static_assert(RM % 4 == 0, "groups of four");
#pragma unroll
    for (int r = 0; r < RM; r += 4) {
      float t[4];
      lb_ld<T, 4>(f + e * R + (r < R ? r : R - 4), t);
      fr[r] = t[0], fr[r + 1] = t[1], fr[r + 2] = t[2], fr[r + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int r = 0; r < RM; ++r) fr[r] = lb_ld1<T>(f + e * R + (r < R ? r : R - 1));
  }
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const int k = k0 + q < K ? k0 + q : K - 1;
    lb_ld<T, W>(x + ((node * K + k) * U + u) * W, a[q]);
  }
}
// out[i][k][:] = sum over the slots of row i, ascending, of fl32(x[other node of the slot][k][:] * wf[slot][:]); +0.0 for an empty
// row: k_graph_conv's sum on the filter above.  KT accumulator rows per pass over the slots (1 for K = 1, 3 for K > 1), two slots'
// loads in flight; the adds sequential.
template <typename T, int W, int KT, int RM, bool FV>
__global__ void __launch_bounds__(256) k_graph_filter_conv(lb_glist L, lb_gwalk walk, const int32_t* __restrict__ oidx,
                                                           const T* __restrict__ x, const T* __restrict__ f,
                                                           const T* __restrict__ weight, T* __restrict__ out, int K, int R) {
  const int U = L.U;
  const lb_glanes G = graph_lanes(L);
  float wt[RM][W];
  int held = -1;   // the unit whose weight columns wt holds
  for (int64_t i = G.first; i < L.BN; i += G.stride) {
    const lb_row Rw = graph_row(L, walk, i);
    for (int u = G.lane; u < U; u += G.lpr) {
      if (u != held) {
        held = u;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
#pragma unroll
          for (int c = 0; c < W; ++c) wt[r][c] = 0.f;
          if (r < R) lb_ld<T, W>(weight + ((int64_t)r * U + u) * W, wt[r]);
        }
      }
      for (int k0 = 0; k0 < K; k0 += KT) {
        float s[KT][W], fr[2][RM], a[2][KT][W], wf[2][W];
#pragma unroll
        for (int q = 0; q < KT; ++q)
#pragma unroll
          for (int c = 0; c < W; ++c) s[q][c] = 0.f;
        int p = Rw.p0;
        if (p < Rw.p1) {   // the sum STARTS from the first product
          graph_filter_load<T, W, KT, RM, FV>(Rw, p++, oidx, x, f, L, K, k0, R, U, u, fr[0], a[0]);
          graph_filter_unit<T, W, RM>(fr[0], wt, R, wf[0]);
#pragma unroll
          for (int q = 0; q < KT; ++q)
#pragma unroll
            for (int c = 0; c < W; ++c) s[q][c] = __fmul_rn(a[0][q][c], wf[0][c]);
        }
        for (; p + 2 <= Rw.p1; p += 2) {
#pragma unroll
          for (int t = 0; t < 2; ++t) graph_filter_load<T, W, KT, RM, FV>(Rw, p + t, oidx, x, f, L, K, k0, R, U, u, fr[t], a[t]);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            graph_filter_unit<T, W, RM>(fr[t], wt, R, wf[t]);
#pragma unroll
            for (int q = 0; q < KT; ++q)
#pragma unroll
              for (int c = 0; c < W; ++c) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(a[t][q][c], wf[t][c]));
          }
        }
        if (p < Rw.p1) {
          graph_filter_load<T, W, KT, RM, FV>(Rw, p, oidx, x, f, L, K, k0, R, U, u, fr[0], a[0]);
          graph_filter_unit<T, W, RM>(fr[0], wt, R, wf[0]);
#pragma unroll
          for (int q = 0; q < KT; ++q)
#pragma unroll
            for (int c = 0; c < W; ++c) s[q][c] = __fadd_rn(s[q][c], __fmul_rn(a[0][q][c], wf[0][c]));
        }
#pragma unroll
        for (int q = 0; q < KT; ++q)
          if (k0 + q < K) lb_st<T, W>(out + ((i * K + k0 + q) * U + u) * W, s[q]);
      }
    }
  }
}

// The edge gradients of filter_conv, from g[slot][c] = fl32(x[o][0][c] * d[n][0][c]) + fl32(x[o][1][c] * d[n][1][c]) + ... (k
// ascending, the first product starts the sum; o the slot's other node, n its `role` node: conv's d_w), which is never stored:
//   d_f[slot][r]   = the sum over c of fl32(weight[r][c] * g[slot][c]) in the order of LB_GRAPH_DU_BLOCK: consecutive blocks of 16
//                    columns, c ascending inside a block from its first product, the block sums added in ascending block order from
//                    the first one; +0.0 in the pad slots;
//   d_weight[r][c] = the sum over every real slot of the batch of fl32(f[slot][r] * g[slot][c]) in the two-level order of
//                    LB_GRAPH_FILTER_CHUNK: per chunk of consecutive flat padded slots a partial sum from +0.0 over its real slots,
//                    ascending (k_graph_filter_dw); the total from +0.0 over the partials, ascending (k_graph_filter_finish).
// Both are small dense products against an edge-shaped operand that exists only tile by tile: a workgroup forms g for a tile of
// LB_GF_TILE slots and LB_GF_COLS columns in LDS - a lane per unit of a slot's row, so x and d rows are read as whole lines as in
// k_graph_pair_mul - and every lane then owns outputs whose sums it runs alone, in order, from LDS: no shuffle, no atomics.
#define LB_GF_TILE 32    // slots of a tile
#define LB_GF_COLS 128   // columns of a tile: a multiple of LB_GRAPH_DU_BLOCK, and 256 lanes make whole slots of its units
static_assert(LB_GF_COLS % LB_GRAPH_DU_BLOCK == 0 && LB_GRAPH_FILTER_CHUNK % LB_GF_TILE == 0 && LB_GRAPH_MAX_R <= 32, "tile sizes");
struct lb_gf_slots {
  int real[LB_GF_TILE];
  int64_t node[LB_GF_TILE], other[LB_GF_TILE];
};
// the tile's slots from flat padded slot r0 (a slot past the batch is a pad), by the first LB_GF_TILE lanes
__device__ __forceinline__ void graph_filter_slots(const lb_glist& L, int64_t r0, int64_t total, const int32_t* __restrict__ idx,
                                                   const int32_t* __restrict__ oidx, lb_gf_slots& S) {
  if (threadIdx.x < LB_GF_TILE) {
    const int64_t r = r0 + threadIdx.x;
    lb_gslot s{};
    if (r < total) s = graph_slot(L, r, idx, oidx);
    S.real[threadIdx.x] = s.real, S.node[threadIdx.x] = s.node, S.other[threadIdx.x] = s.other;
  }
}
// g of the tile's real slots for columns c0 .. c0 + LB_GF_COLS - 1 (those below C) -> gs; a pad slot's row is left as it was
template <typename T, int W>
__device__ __forceinline__ void graph_filter_g(const T* __restrict__ x, const T* __restrict__ d, int K, int C, int c0,
                                               const lb_gf_slots& S, float (*gs)[LB_GF_COLS + 1]) {
  constexpr int UC = LB_GF_COLS / W;   // units of a tile row
  const int u = (int)threadIdx.x % UC, col = c0 + u * W;
  if (col >= C) return;
  for (int s = (int)threadIdx.x / UC; s < LB_GF_TILE; s += 256 / UC) {
    if (!S.real[s]) continue;
    const T* __restrict__ xp = x + S.other[s] * K * C + col;
    const T* __restrict__ dp = d + S.node[s] * K * C + col;
    float g[W], a[W], b[W];
    lb_ld<T, W>(xp, a);
    lb_ld<T, W>(dp, b);
#pragma unroll
    for (int c = 0; c < W; ++c) g[c] = __fmul_rn(a[c], b[c]);
#pragma unroll 4
    for (int k = 1; k < K; ++k) {
      lb_ld<T, W>(xp + (int64_t)k * C, a);
      lb_ld<T, W>(dp + (int64_t)k * C, b);
#pragma unroll
      for (int c = 0; c < W; ++c) g[c] = __fadd_rn(g[c], __fmul_rn(a[c], b[c]));
    }
#pragma unroll
    for (int c = 0; c < W; ++c) gs[s][u * W + c] = g[c];
  }
}

// d_f: lane (s, rg) of the workgroup owns slot s of the tile and the rows r = rg, rg + 8, ... (RN of them) and runs their blocked
// sums over the columns - all passes of LB_GF_COLS columns of a tile before the next tile, the running totals in registers.  The
// weight columns of a pass are staged in LDS (rows past R zero; once per workgroup when C is one pass); g is read at an odd
// row stride (no bank conflict across s), the weight as a broadcast.
template <typename T, int W, int RN>
__global__ void __launch_bounds__(256) k_graph_filter_df(lb_glist L, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ oidx, const T* __restrict__ x,
                                                         const T* __restrict__ d, const T* __restrict__ weight, T* __restrict__ d_f,
                                                         int K, int R, int C) {
  __shared__ float gs[LB_GF_TILE][LB_GF_COLS + 1];
  __shared__ __attribute__((aligned(16))) float ws[8 * RN][LB_GF_COLS];
  __shared__ lb_gf_slots S;
  const int64_t total = (int64_t)L.B * L.e_cap, tiles = (total + LB_GF_TILE - 1) / LB_GF_TILE;
  const int s = threadIdx.x & (LB_GF_TILE - 1), rg = threadIdx.x / LB_GF_TILE;
  const int passes = (C + LB_GF_COLS - 1) / LB_GF_COLS;
  bool staged = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * LB_GF_TILE;
    __syncthreads();   // (the last tile's readers are done)
    graph_filter_slots(L, r0, total, idx, oidx, S);
    float tot[RN];
#pragma unroll
    for (int n = 0; n < RN; ++n) tot[n] = 0.f;
    for (int pass = 0; pass < passes; ++pass) {
      const int c0 = pass * LB_GF_COLS, cn = C - c0 < LB_GF_COLS ? C - c0 : LB_GF_COLS;
      if (pass) __syncthreads();   // (the last pass's readers are done)
      if (passes > 1 || !staged) {
        staged = true;
        for (int q = threadIdx.x; q < 8 * RN * LB_GF_COLS; q += 256) {
          const int r = q / LB_GF_COLS, c = q % LB_GF_COLS;
          ws[r][c] = (r < R && c < cn) ? lb_ld1<T>(weight + (int64_t)r * C + c0 + c) : 0.f;
        }
      }
      __syncthreads();
      graph_filter_g<T, W>(x, d, K, C, c0, S, gs);
      __syncthreads();
      if (S.real[s]) {
        for (int cb = 0; cb < cn; cb += LB_GRAPH_DU_BLOCK) {
          const int bn = cn - cb;   // the block's columns (LB_GRAPH_DU_BLOCK or more: a full block)
          float gv[LB_GRAPH_DU_BLOCK];
#pragma unroll
          for (int c = 0; c < LB_GRAPH_DU_BLOCK; ++c) gv[c] = gs[s][cb + c];   // (past bn: whatever LDS holds, dropped below)
#pragma unroll
          for (int n = 0; n < RN; ++n) {
            const float* __restrict__ wr = ws[rg + 8 * n] + cb;
            float part = __fmul_rn(wr[0], gv[0]);
#pragma unroll
            for (int c = 1; c < LB_GRAPH_DU_BLOCK; ++c) {
              const float t = __fadd_rn(part, __fmul_rn(wr[c], gv[c]));
              part = c < bn ? t : part;
            }
            tot[n] = (pass == 0 && cb == 0) ? part : __fadd_rn(tot[n], part);
          }
        }
      }
    }
    if (r0 + s < total) {
#pragma unroll
      for (int n = 0; n < RN; ++n)
        if (rg + 8 * n < R) lb_st1<T>(d_f + (r0 + s) * R + rg + 8 * n, tot[n]);
    }
  }
}

// The partial sums of d_weight: workgroup (q, pass) owns chunk q of `chunk` flat padded slots and columns c0 .. c0 + LB_GF_COLS - 1;
// lane (cl, rg) of it the outputs r = rg, rg + 8, ... x c = c0 + cl, c0 + cl + 32, ...: RN x 4 accumulators from +0.0, fed tile by
// tile with the real slots in ascending order - f and g of the tile from LDS.  partials is (chunks, R, C) fp32, every element
// written (+0.0 by a chunk of pads).
template <typename T, int W, int RN>
__global__ void __launch_bounds__(256) k_graph_filter_dw(lb_glist L, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ oidx, const T* __restrict__ x,
                                                         const T* __restrict__ d, const T* __restrict__ f,
                                                         float* __restrict__ partials, int K, int R, int C, int chunk) {
  __shared__ float gs[LB_GF_TILE][LB_GF_COLS + 1];
  __shared__ float fs[LB_GF_TILE][8 * RN + 1];
  __shared__ lb_gf_slots S;
  const int64_t total = (int64_t)L.B * L.e_cap, q = blockIdx.x;
  const int c0 = blockIdx.y * LB_GF_COLS;
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int64_t end = (q + 1) * chunk < total ? (q + 1) * chunk : total;
  float acc[RN][4];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[n][m] = 0.f;
  for (int64_t r0 = q * chunk; r0 < end; r0 += LB_GF_TILE) {
    __syncthreads();   // (the last tile's readers are done)
    graph_filter_slots(L, r0, total, idx, oidx, S);
    __syncthreads();
    graph_filter_g<T, W>(x, d, K, C, c0, S, gs);
    for (int t = threadIdx.x; t < LB_GF_TILE * 8 * RN; t += 256) {
      const int s = t / (8 * RN), r = t % (8 * RN);
      if (S.real[s] && r < R) fs[s][r] = lb_ld1<T>(f + (r0 + s) * R + r);   // (a pad slot's f is never read)
    }
    __syncthreads();
    for (int s = 0; s < LB_GF_TILE; ++s) {
      if (!S.real[s]) continue;   // (uniform)
      float gv[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) gv[m] = gs[s][cl + 32 * m];
#pragma unroll
      for (int n = 0; n < RN; ++n) {
        const float fr = fs[s][rg + 8 * n];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[n][m] = __fadd_rn(acc[n][m], __fmul_rn(fr, gv[m]));
      }
    }
  }
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int r = rg + 8 * n, c = c0 + cl + 32 * m;
      if (r < R && c < C) partials[(q * R + r) * C + c] = acc[n][m];
    }
}
// d_weight[r][c] = +0.0 + partials[0][r][c] + partials[1][r][c] + ...: one lane per element, the chunks ascending.
template <typename T>
__global__ void __launch_bounds__(256) k_graph_filter_finish(const float* __restrict__ partials, int64_t chunks, int64_t RC,
                                                             T* __restrict__ d_weight) {
  const int64_t stride = (int64_t)gridDim.x * 256;   // (the grid is capped: graph_blocks1)
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < RC; q += stride) {
    float tot = 0.f, v[16];
    int64_t k = 0;
    for (; k + 16 <= chunks; k += 16) {   // sixteen loads in flight; the adds stay sequential
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = partials[(k + j) * RC + q];
#pragma unroll
      for (int j = 0; j < 16; ++j) tot = __fadd_rn(tot, v[j]);
    }
    for (; k < chunks; ++k) tot = __fadd_rn(tot, partials[k * RC + q]);
    lb_st1<T>(d_weight + q, tot);
  }
}

// ------------------------------------------------------------------------------------------------ multi-aggregator
// aggregate: sum, mean, max, min, std and var of one message from one walk of the row (the contract is in
// include/lbhip.h above lb_graph_aggregate).  out is (B N, A, C): plane a of node i is row i A + a of C columns.  Where each op
// stores its plane comes as a named member of lb_gagg (-1: not asked for) - uniform values in scalar registers, never an array
// indexed at run time (see lb_glist).  EXT: max / min and their winners are wanted; MOM: the centred second moment is (std / var),
// which costs the second walk of the row - cache-hot, the lane re-reads the lines it just read.
struct lb_gagg {
  int A;
  int sum, mean, max, min, std, var;   // plane of the op among the A of out, -1 when it was not asked for
  float eps;
};
// The correctly rounded root of the contract.  Not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define it as
// the native approximation (1 ulp).  sqrtf compiles to the correctly rounded expansion - hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt, which also makes __fdiv_rn (there: x / y) the correctly rounded quotient.
__device__ __forceinline__ float lb_sqrt_rn(float x) { return sqrtf(x); }
// W fp32 (the saved mean and std): 16-byte accesses when W > 1
template <int W>
__device__ __forceinline__ void lb_ldf(const float* p, float (&a)[W]) {
  if constexpr (W == 1) {
    a[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + q);
      a[q] = t[0], a[q + 1] = t[1], a[q + 2] = t[2], a[q + 3] = t[3];
    }
  }
}
template <int W>
__device__ __forceinline__ void lb_stf(float* p, const float (&a)[W]) {
  if constexpr (W == 1) {
    *p = a[0];
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4) *reinterpret_cast<f32x4*>(p + q) = f32x4{a[q], a[q + 1], a[q + 2], a[q + 3]};
  }
}

// Per node i and column c over the real slots j1 < ... < jd of the row: s = the ordered sum (k_graph_segment_sum's bits), the
// maximum and the minimum with their winning slots (k_graph_segment_max's), m = s / max(d, 1), and with MOM the second walk:
// q = the ordered sum of fl32(t t), t = fl32(x - m); var = q / max(d, 1), std = sqrt(var + eps).  An empty row stores +0.0 in
// every plane (std included), -1 in win and +0.0 in stats.  win (B N, 2, C): max plane, min plane; stats (B N, 2, C) fp32: m, std.
template <typename T, int W, bool EXT, bool MOM>
__global__ void __launch_bounds__(256) k_graph_aggregate(lb_glist L, lb_gwalk walk, lb_gagg G, const T* __restrict__ msg,
                                                         T* __restrict__ out, int32_t* __restrict__ win,
                                                         float* __restrict__ stats) {
  const int U = L.U;
  graph_for_nodes(L, walk, [&](int64_t i, const lb_row& R, int u) {
    float s[W], hi[W], lo[W], a[W];
    int32_t whi[W], wlo[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = 0.f, hi[k] = 0.f, lo[k] = 0.f, whi[k] = -1, wlo[k] = -1;
    int p = R.p0;
    if (p < R.p1) {   // every reduction STARTS from the first slot
      const int64_t e = R.edge(p++);
      lb_ld<T, W>(msg + (e * U + u) * W, s);
#pragma unroll
      for (int k = 0; k < W; ++k) hi[k] = s[k], lo[k] = s[k], whi[k] = wlo[k] = (int32_t)(e - R.first);
    }
#pragma unroll 4
    for (; p < R.p1; ++p) {
      const int64_t e = R.edge(p);
      lb_ld<T, W>(msg + (e * U + u) * W, a);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        s[k] = __fadd_rn(s[k], a[k]);
        if constexpr (EXT) {
          if (lb_beats<false>(a[k], hi[k])) hi[k] = a[k], whi[k] = (int32_t)(e - R.first);
          if (lb_beats<true>(a[k], lo[k])) lo[k] = a[k], wlo[k] = (int32_t)(e - R.first);
        }
      }
    }
    const int d = R.p1 - R.p0;
    const float dd = (float)(d > 1 ? d : 1);
    const int64_t o = i * G.A * U + u;   // unit u of plane 0 of node i; plane a is a U units further
    float m[W];
#pragma unroll
    for (int k = 0; k < W; ++k) m[k] = __fdiv_rn(s[k], dd);
    if (G.sum >= 0) lb_st<T, W>(out + (o + (int64_t)G.sum * U) * W, s);
    if (G.mean >= 0) lb_st<T, W>(out + (o + (int64_t)G.mean * U) * W, m);
    if constexpr (EXT) {
      if (G.max >= 0) lb_st<T, W>(out + (o + (int64_t)G.max * U) * W, hi);
      if (G.min >= 0) lb_st<T, W>(out + (o + (int64_t)G.min * U) * W, lo);
      lb_sti<W>(win + ((i * 2 + 0) * U + u) * W, whi);
      lb_sti<W>(win + ((i * 2 + 1) * U + u) * W, wlo);
    }
    if constexpr (MOM) {
      float q[W], sd[W];
#pragma unroll
      for (int k = 0; k < W; ++k) q[k] = 0.f, sd[k] = 0.f;
      p = R.p0;
      if (p < R.p1) {
        lb_ld<T, W>(msg + (R.edge(p++) * U + u) * W, a);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const float t = __fsub_rn(a[k], m[k]);
          q[k] = __fmul_rn(t, t);
        }
      }
#pragma unroll 4
      for (; p < R.p1; ++p) {
        lb_ld<T, W>(msg + (R.edge(p) * U + u) * W, a);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const float t = __fsub_rn(a[k], m[k]);
          q[k] = __fadd_rn(q[k], __fmul_rn(t, t));
        }
      }
#pragma unroll
      for (int k = 0; k < W; ++k) q[k] = __fdiv_rn(q[k], dd);   // (q is var from here)
      if (G.std >= 0 && d > 0) {   // a node without slots keeps +0.0, not sqrt(eps)
#pragma unroll
        for (int k = 0; k < W; ++k) sd[k] = lb_sqrt_rn(__fadd_rn(q[k], G.eps));
      }
      if (G.var >= 0) lb_st<T, W>(out + (o + (int64_t)G.var * U) * W, q);
      if (G.std >= 0) lb_st<T, W>(out + (o + (int64_t)G.std * U) * W, sd);
      lb_stf<W>(stats + ((i * 2 + 0) * U + u) * W, m);
      lb_stf<W>(stats + ((i * 2 + 1) * U + u) * W, sd);
    }
  });
}

// d_msg[slot j of node n][c] = the present terms added in this fixed order, the first present one starting the sum (d the
// degree of n, t = fl32(x_j - m) from msg and the saved mean): g_sum; fl32(g_mean / d); g_max if j won the maximum of (n, c);
// g_min likewise; fl32(fl32(g_std t) / fl32(d std)); fl32(fl32(fl32(2 g_var) t) / d).  A real slot without a present term (an
// extremum it did not win, nothing else asked for) and every pad slot get +0.0.  The head of a slot adds the degree of its node,
// read from the role's seg_ptr as graph_row caps it.
struct lb_gslot_deg {
  lb_gslot s;
  int d;
};
template <typename T, int W, bool EXT, bool MOM>
__global__ void __launch_bounds__(256) k_graph_aggregate_bwd(lb_glist L, lb_gwalk walk, lb_gagg G,
                                                             const int32_t* __restrict__ idx, const T* __restrict__ d_out,
                                                             const T* __restrict__ msg, const int32_t* __restrict__ win,
                                                             const float* __restrict__ stats, T* __restrict__ d_msg) {
  const int U = L.U;
  graph_for(
      L, (int64_t)L.B * L.e_cap,
      [&](int64_t r) {
        lb_gslot_deg h;
        h.s = graph_slot(L, r, idx);
        h.d = 1;
        if (h.s.real) {
          const lb_row R = graph_row(L, walk, h.s.node);
          h.d = R.p1 - R.p0;
        }
        return h;
      },
      [&](int64_t r, const lb_gslot_deg& h, int u) {
        float acc[W], g[W];
        bool any[W];
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] = 0.f, any[k] = false;
        if (h.s.real) {
          const float dd = (float)(h.d > 1 ? h.d : 1);
          const int64_t o = h.s.node * G.A * U + u;
          if (G.sum >= 0) {
            lb_ld<T, W>(d_out + (o + (int64_t)G.sum * U) * W, g);
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] = g[k], any[k] = true;
          }
          if (G.mean >= 0) {
            lb_ld<T, W>(d_out + (o + (int64_t)G.mean * U) * W, g);
#pragma unroll
            for (int k = 0; k < W; ++k) {
              const float t = __fdiv_rn(g[k], dd);
              acc[k] = any[k] ? __fadd_rn(acc[k], t) : t, any[k] = true;
            }
          }
          if constexpr (EXT) {
            int32_t w[W];
            if (G.max >= 0) {
              lb_ld<T, W>(d_out + (o + (int64_t)G.max * U) * W, g);
              lb_ldi<W>(win + ((h.s.node * 2 + 0) * U + u) * W, w);
#pragma unroll
              for (int k = 0; k < W; ++k)
                if (w[k] == h.s.j) acc[k] = any[k] ? __fadd_rn(acc[k], g[k]) : g[k], any[k] = true;
            }
            if (G.min >= 0) {
              lb_ld<T, W>(d_out + (o + (int64_t)G.min * U) * W, g);
              lb_ldi<W>(win + ((h.s.node * 2 + 1) * U + u) * W, w);
#pragma unroll
              for (int k = 0; k < W; ++k)
                if (w[k] == h.s.j) acc[k] = any[k] ? __fadd_rn(acc[k], g[k]) : g[k], any[k] = true;
            }
          }
          if constexpr (MOM) {
            float x[W], m[W], sd[W];
            lb_ld<T, W>(msg + (r * U + u) * W, x);
            lb_ldf<W>(stats + ((h.s.node * 2 + 0) * U + u) * W, m);
#pragma unroll
            for (int k = 0; k < W; ++k) x[k] = __fsub_rn(x[k], m[k]);   // (x is t from here)
            if (G.std >= 0) {
              lb_ld<T, W>(d_out + (o + (int64_t)G.std * U) * W, g);
              lb_ldf<W>(stats + ((h.s.node * 2 + 1) * U + u) * W, sd);
#pragma unroll
              for (int k = 0; k < W; ++k) {
                const float t = __fdiv_rn(__fmul_rn(g[k], x[k]), __fmul_rn(dd, sd[k]));
                acc[k] = any[k] ? __fadd_rn(acc[k], t) : t, any[k] = true;
              }
            }
            if (G.var >= 0) {
              lb_ld<T, W>(d_out + (o + (int64_t)G.var * U) * W, g);
#pragma unroll
              for (int k = 0; k < W; ++k) {
                const float t = __fdiv_rn(__fmul_rn(__fmul_rn(2.f, g[k]), x[k]), dd);
                acc[k] = any[k] ? __fadd_rn(acc[k], t) : t, any[k] = true;
              }
            }
          }
        }
        lb_st<T, W>(d_msg + (r * U + u) * W, acc);
      });
}

// ------------------------------------------------------------------------------------------------ feature transpose
// d loss / d window (B N, isl, dim) fp64 from the cotangents of the features a TorchModel module receives: the transpose of the
// feature builder as the comment above k_feat_bwd (lb_train.hip) states it, on the engine's current window and list, in the
// layouts of the module's feature dict (node arrays (B N, .), edge arrays in the padded slots).  One lane per (particle, axis),
// axis minor: the lanes of a particle read neighbouring floats of an edge row, the per-axis sums are independent and share only
// the scalar d_rel_dist / rel_dist.  Every sum in fp64 over terms formed from the fp32 inputs, in a fixed order: frames
// ascending (velocity terms, then d_abs_pos); on the newest frame the walls, the particle's receiver row in ascending slot
// order, the edges it sends in ascending sender-view order.  No atomics.  Forward values: rel_disp / rel_dist are read from the
// engine's fp32 edge features (as k_feat_bwd does); the engine holds no fp32 node features outside a GNS handle, so the
// normalised velocities, their magnitudes and the wall distances are recomputed from the fp64 window by the operations of
// lb_node_features_body and rounded to fp32 - the values the module was handed.  Null cotangents are zero and skip their reads.
struct lb_gfb_args {
  int64_t BN;
  int e_cap, E;
  const double* win;
  const lb_ctrl* ctrl;
  const int32_t *ptype, *row_ptr, *snd_ptr, *snd_perm;
  const float* efeat;
  const float *d_abs, *d_vh, *d_vm, *d_bd, *d_rd, *d_rr;
  double* out;
};
__device__ __forceinline__ double lb_gfb_nvel(const lb_geom& g, int64_t BN, const double* __restrict__ win, int step, int f,
                                              int d, int64_t i, double box, double half, double mean, double sd) {
  const double v = lb_disp1(lb_pos(win, g, BN, step, f + 1, d, i), lb_pos(win, g, BN, step, f, d, i), box, half, g.periodic);
  return (v - mean) / sd;
}
// h_e along axis d of the edge in padded slot `slot` (compact edge slot - slot0)
__device__ __forceinline__ double lb_gfb_edge(const lb_gfb_args& a, int dim, int d, int64_t slot, int64_t slot0, double rc) {
  const float* __restrict__ f = a.efeat + (slot - slot0) * 8;
  const float dist = f[dim];
  const double w = (a.d_rr && dist != 0.f) ? (double)a.d_rr[slot] / (double)dist : 0.0;
  const double dd = a.d_rd ? (double)a.d_rd[slot * dim + d] : 0.0;
  return (dd + w * (double)f[d]) / rc;
}
__global__ void __launch_bounds__(256) k_graph_features_bwd(lb_geom g, lb_gfb_args a) {
  const int dim = g.dim, isl = g.isl, K = g.isl - 1;
  const int64_t total = a.BN * dim, stride = (int64_t)gridDim.x * 256;
  int step = a.ctrl->step;
  step = step < 0 ? 0 : step;
  const bool edges = a.d_rd || a.d_rr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
    const int64_t i = q / dim;
    const int d = (int)(q - i * dim);
    double* __restrict__ out = a.out + i * isl * dim + d;
    if (a.ptype[i] == LB_PAD_TYPE) {
      for (int f = 0; f <= K; ++f) out[f * dim] = 0.0;
      continue;
    }
    // this lane's axis constants (selected with compares: a run-time index into the by-value geometry would go to scratch)
    const double box = lb_sel3(d, g.box[0], g.box[1], g.box[2]), half = lb_sel3(d, g.half_box[0], g.half_box[1], g.half_box[2]);
    const double mean = lb_sel3(d, g.vel_mean[0], g.vel_mean[1], g.vel_mean[2]);
    const double sd = lb_sel3(d, g.vel_std[0], g.vel_std[1], g.vel_std[2]), inv_std = 1.0 / sd;
    double prev = 0.0;   // what velocity f - 1 sends to its later frame f
    for (int f = 0; f <= K; ++f) {
      double cur = 0.0;
      if (f < K && (a.d_vh || a.d_vm)) {
        const float gv = a.d_vh ? a.d_vh[(i * K + f) * dim + d] : 0.f;
        double wm = 0.0;
        float x = 0.f;
        if (a.d_vm) {
          double s2 = 0.0, nd = 0.0;
#pragma nounroll   // (one copy of the periodic displacement's fmod; c is uniform, so g.box[c] is a scalar load)
          for (int c = 0; c < dim; ++c) {
            const double nv = lb_gfb_nvel(g, a.BN, a.win, step, f, c, i, g.box[c], g.half_box[c], g.vel_mean[c], g.vel_std[c]);
            s2 = c == 0 ? nv * nv : s2 + nv * nv;
            nd = c == d ? nv : nd;
          }
          const float m = (float)sqrt(s2);
          x = (float)nd;
          wm = m != 0.f ? (double)a.d_vm[i * K + f] / (double)m : 0.0;
        }
        cur = ((double)gv + wm * (double)x) * inv_std;
      }
      double acc = prev - cur;
      prev = cur;
      if (a.d_abs) acc += (double)a.d_abs[(i * isl + f) * dim + d];
      if (f == K) {
        if (a.d_bd) {
          const double p = lb_pos(a.win, g, a.BN, step, K, d, i);
          const double b_lo = lb_sel3(d, g.bound_lo[0], g.bound_lo[1], g.bound_lo[2]);
          const double b_hi = lb_sel3(d, g.bound_hi[0], g.bound_hi[1], g.bound_hi[2]);
          const float lo = (float)fmin(fmax((p - b_lo) / g.rc, -1.0), 1.0), hi = (float)fmin(fmax((b_hi - p) / g.rc, -1.0), 1.0);
          if (lo > -1.f && lo < 1.f) acc += (double)a.d_bd[i * 2 * dim + d] / g.rc;
          if (hi > -1.f && hi < 1.f) acc -= (double)a.d_bd[i * 2 * dim + dim + d] / g.rc;
        }
        if (edges) {
          const lb_row R = graph_row(a.row_ptr, a.row_ptr, nullptr, i, g.N, a.e_cap, a.E);
#pragma unroll 4
          for (int p = R.p0; p < R.p1; ++p) acc += lb_gfb_edge(a, dim, d, R.edge(p), R.slot0, g.rc);
          const lb_row S = graph_row(a.row_ptr, a.snd_ptr, a.snd_perm, i, g.N, a.e_cap, a.E);
#pragma unroll 4
          for (int p = S.p0; p < S.p1; ++p) acc -= lb_gfb_edge(a, dim, d, S.edge(p), S.slot0, g.rc);
        }
      }
      out[f * dim] = acc;
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
static unsigned graph_blocks(int64_t rows, int lpr_shift) {
  const int64_t per_block = 256 >> lpr_shift;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + per_block - 1) / per_block, 2048));
}
static unsigned graph_blocks1(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536)); }
static bool graph_aligned(std::initializer_list<const void*> ptrs) {
  uintptr_t a = 0;
  for (const void* p : ptrs) a |= (uintptr_t)p;
  return a % 16 == 0;
}
static size_t graph_esize(int32_t dtype) { return dtype == LB_DTYPE_BF16 ? 2 : 4; }
// Elements of one access for rows whose units must divide `span` columns (C; D for attend, where a unit lies in one head):
// 16 bytes - 4 floats, 8 bf16 - when span allows it and every pointer is 16-byte aligned; for bf16 and `half_units` (attend)
// 8 bytes when span % 4 == 0; one element otherwise.
static int graph_width(int32_t dtype, int span, bool half_units, std::initializer_list<const void*> ptrs) {
  if (!graph_aligned(ptrs)) return 1;
  if (dtype == LB_DTYPE_F32) return span % 4 == 0 ? 4 : 1;
  return span % 8 == 0 ? 8 : (half_units && span % 4 == 0 ? 4 : 1);
}
// The checks every entry makes, the list's status, the sender view for role 1 (`view`: the op walks rows of the role).
static int graph_entry(lb_engine* e, const char* entry, int32_t role, int32_t dtype, bool ptrs_ok, int32_t c0, int32_t c1,
                       bool view = true) {
  if (!e || !ptrs_ok) return lb_fail(LB_ERR_ARG, "null argument");
  if ((role != 0 && role != 1) || c0 < 1 || c1 < 1)
    return lb_fail(LB_ERR_ARG, "%s: role %d (0 receivers, 1 senders), columns %d x %d", entry, role, c0, c1);
  if (dtype != LB_DTYPE_F32 && dtype != LB_DTYPE_BF16)
    return lb_fail(LB_ERR_ARG, "%s: dtype %d (0 float32, 1 bfloat16)", entry, dtype);
  LB_TRY(graph_begin(e, entry));
  if (role && view) LB_TRY(graph_sender_view(e));
  return LB_OK;
}

// One launch's plan: the list descriptor with the op's units (U = cols / W) and lanes per row, the walk of `role` and its two
// compact index lists, the unit width W (graph_width over `span` and `ptrs`) and the grid.  Rows: a lane group per node or per
// padded slot.  (The flat kernels - degree, attend_t, attend_dlogits: one lane per output element - take graph_list /
// graph_walk as they are.)
enum lb_grows { LB_NODES, LB_SLOTS };
struct lb_gplan {
  lb_glist L;
  lb_gwalk walk;
  const int32_t *idx, *oidx;   // the node of `role` per compact edge, and the other one
  int W;
  unsigned blocks;
};
static lb_glist graph_list(const lb_engine* e, int U, int lpr_shift) {
  return lb_glist{e->row_ptr, e->BN, e->g.N, e->g.B, e->e_cap, (int)e->graph_E, U, lpr_shift};
}
static lb_gwalk graph_walk(const lb_engine* e, int32_t role) {
  return lb_gwalk{role ? e->snd_ptr : e->row_ptr, role ? e->snd_perm : nullptr};
}
static lb_gplan graph_plan(const lb_engine* e, int32_t role, int32_t dtype, lb_grows rows, int cols, int span, bool half_units,
                           std::initializer_list<const void*> ptrs) {
  const int64_t n = rows == LB_NODES ? e->BN : (int64_t)e->g.B * e->e_cap;
  lb_gplan P{};
  P.W = graph_width(dtype, span, half_units, ptrs);
  const int U = cols / P.W, sh = graph_lpr_shift(U);
  P.L = graph_list(e, U, sh);
  P.walk = graph_walk(e, role);
  P.idx = role ? e->senders : e->receivers;
  P.oidx = role ? e->receivers : e->senders;
  P.blocks = graph_blocks(n, sh);
  return P;
}
// f(T{}, lb_w<W>{}) with the element type and the unit width of the call as types: (float, 4 | 1), (lb_bf16, 8 | 1) and, for the
// ops that have them (HALF: attend), the 8-byte bf16 units (lb_bf16, 4).  f launches; its launch error is the result.
template <int W>
using lb_w = std::integral_constant<int, W>;
template <bool HALF = false, typename F>
static int graph_dispatch(int32_t dtype, int W, F f) {
  if (dtype == LB_DTYPE_F32 && W == 4) {
    f(float{}, lb_w<4>{});
  } else if (dtype == LB_DTYPE_F32) {
    f(float{}, lb_w<1>{});
  } else if (W == 8) {
    f(lb_bf16{}, lb_w<8>{});
  } else if (HALF && W == 4) {
    if constexpr (HALF) f(lb_bf16{}, lb_w<4>{});
  } else {
    f(lb_bf16{}, lb_w<1>{});
  }
  LB_HIP(hipGetLastError());
  return LB_OK;
}
template <typename Kernel, typename... Args>
static void graph_launch(lb_engine* e, unsigned blocks, Kernel kernel, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, e->stream, args...);
}

static int graph_gather(lb_engine* e, const char* entry, int32_t role, const void* x, void* out, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, x && out, C, 1, false));
  // a bit copy: 16-byte units (4 floats, 8 bf16) when the row is made of them and the pointers are aligned, elements otherwise
  const lb_gplan P = graph_plan(e, role, dtype, LB_SLOTS, C, C, false, {x, out});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using V = std::conditional_t<(decltype(w)::value > 1), f32x4, decltype(t)>;
    graph_launch(e, P.blocks, k_graph_gather<V>, P.L, P.idx, x, out);
  });
}
extern "C" int lb_graph_gather_t(lb_engine* e, int32_t role, const void* x_dev, void* out_dev, int32_t C, int32_t dtype) {
  return graph_gather(e, "lb_graph_gather_t", role, x_dev, out_dev, C, dtype);
}
extern "C" int lb_graph_gather(lb_engine* e, int32_t role, const float* x_dev, float* out_dev, int32_t C) {
  return graph_gather(e, "lb_graph_gather", role, x_dev, out_dev, C, LB_DTYPE_F32);
}

static int graph_segment_sum(lb_engine* e, const char* entry, int32_t role, const void* msg, void* out, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, msg && out, C, 1));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {msg, out});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_segment_sum<T, decltype(w)::value>, e->row_ptr, P.walk.seg_ptr, P.walk.perm, (const T*)msg,
                 (T*)out, e->BN, e->g.N, e->e_cap, (int)e->graph_E, P.L.U, P.L.lpr_shift);
  });
}
extern "C" int lb_graph_segment_sum_t(lb_engine* e, int32_t role, const void* msg_dev, void* out_dev, int32_t C, int32_t dtype) {
  return graph_segment_sum(e, "lb_graph_segment_sum_t", role, msg_dev, out_dev, C, dtype);
}
extern "C" int lb_graph_segment_sum(lb_engine* e, int32_t role, const float* msg_dev, float* out_dev, int32_t C) {
  return graph_segment_sum(e, "lb_graph_segment_sum", role, msg_dev, out_dev, C, LB_DTYPE_F32);
}

extern "C" int32_t lb_graph_sender_sorts(lb_engine* e) { return e ? e->snd_sorts : -1; }

// ---- the attention ops' entries
extern "C" int lb_graph_degree(lb_engine* e, int32_t role, int32_t* out_dev) {
  LB_TRY(graph_entry(e, "lb_graph_degree", role, LB_DTYPE_F32, out_dev != nullptr, 1, 1));
  hipLaunchKernelGGL(k_graph_degree, GRID1(e->BN), 0, e->stream, graph_list(e, 0, 0), graph_walk(e, role), out_dev);
  LB_HIP(hipGetLastError());
  return LB_OK;
}

static int graph_segment_max(lb_engine* e, const char* entry, bool minimum, int32_t role, const void* msg, void* out, int32_t* win,
                             int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, msg && out && win, C, 1));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {msg, out, win});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    graph_launch(e, P.blocks, minimum ? k_graph_segment_max<T, W, true> : k_graph_segment_max<T, W, false>, P.L, P.walk,
                 (const T*)msg, (T*)out, win);
  });
}
extern "C" int lb_graph_segment_max_t(lb_engine* e, int32_t role, const void* msg_dev, void* out_dev, int32_t* win_dev, int32_t C,
                                      int32_t dtype) {
  return graph_segment_max(e, "lb_graph_segment_max_t", false, role, msg_dev, out_dev, win_dev, C, dtype);
}
extern "C" int lb_graph_segment_min_t(lb_engine* e, int32_t role, const void* msg_dev, void* out_dev, int32_t* win_dev, int32_t C,
                                      int32_t dtype) {
  return graph_segment_max(e, "lb_graph_segment_min_t", true, role, msg_dev, out_dev, win_dev, C, dtype);
}
extern "C" int lb_graph_segment_max(lb_engine* e, int32_t role, const float* msg_dev, float* out_dev, int32_t* win_dev, int32_t C) {
  return graph_segment_max(e, "lb_graph_segment_max", false, role, msg_dev, out_dev, win_dev, C, LB_DTYPE_F32);
}
extern "C" int lb_graph_segment_min(lb_engine* e, int32_t role, const float* msg_dev, float* out_dev, int32_t* win_dev, int32_t C) {
  return graph_segment_max(e, "lb_graph_segment_min", true, role, msg_dev, out_dev, win_dev, C, LB_DTYPE_F32);
}

static int graph_segment_max_backward(lb_engine* e, const char* entry, int32_t role, const void* d_out, const int32_t* win,
                                      void* d_msg, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, d_out && win && d_msg, C, 1));
  const lb_gplan P = graph_plan(e, role, dtype, LB_SLOTS, C, C, false, {d_out, win, d_msg});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_segment_max_bwd<T, decltype(w)::value>, P.L, P.idx, (const T*)d_out, win, (T*)d_msg);
  });
}
extern "C" int lb_graph_segment_max_backward_t(lb_engine* e, int32_t role, const void* d_out_dev, const int32_t* win_dev,
                                               void* d_msg_dev, int32_t C, int32_t dtype) {
  return graph_segment_max_backward(e, "lb_graph_segment_max_backward_t", role, d_out_dev, win_dev, d_msg_dev, C, dtype);
}
extern "C" int lb_graph_segment_max_backward(lb_engine* e, int32_t role, const float* d_out_dev, const int32_t* win_dev,
                                             float* d_msg_dev, int32_t C) {
  return graph_segment_max_backward(e, "lb_graph_segment_max_backward", role, d_out_dev, win_dev, d_msg_dev, C, LB_DTYPE_F32);
}

static int graph_segment_softmax(lb_engine* e, const char* entry, int32_t role, const void* logits, void* out, int32_t C,
                                 int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, logits && out, C, 1));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {logits, out});
  LB_HIP(hipMemsetAsync(out, 0, graph_esize(dtype) * (size_t)e->g.B * e->e_cap * C, e->stream));   // the pad slots: +0.0
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_softmax<T, decltype(w)::value>, P.L, P.walk, (const T*)logits, (T*)out);
  });
}
extern "C" int lb_graph_segment_softmax_t(lb_engine* e, int32_t role, const void* logits_dev, void* out_dev, int32_t C,
                                          int32_t dtype) {
  return graph_segment_softmax(e, "lb_graph_segment_softmax_t", role, logits_dev, out_dev, C, dtype);
}
extern "C" int lb_graph_segment_softmax(lb_engine* e, int32_t role, const float* logits_dev, float* out_dev, int32_t C) {
  return graph_segment_softmax(e, "lb_graph_segment_softmax", role, logits_dev, out_dev, C, LB_DTYPE_F32);
}

static int graph_segment_softmax_backward(lb_engine* e, const char* entry, int32_t role, const void* y, const void* d_y, void* d_x,
                                          int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, y && d_y && d_x, C, 1));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {y, d_y, d_x});
  LB_HIP(hipMemsetAsync(d_x, 0, graph_esize(dtype) * (size_t)e->g.B * e->e_cap * C, e->stream));
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_softmax_bwd<T, decltype(w)::value>, P.L, P.walk, (const T*)y, (const T*)d_y, (T*)d_x);
  });
}
extern "C" int lb_graph_segment_softmax_backward_t(lb_engine* e, int32_t role, const void* y_dev, const void* d_y_dev,
                                                   void* d_x_dev, int32_t C, int32_t dtype) {
  return graph_segment_softmax_backward(e, "lb_graph_segment_softmax_backward_t", role, y_dev, d_y_dev, d_x_dev, C, dtype);
}
extern "C" int lb_graph_segment_softmax_backward(lb_engine* e, int32_t role, const float* y_dev, const float* d_y_dev,
                                                 float* d_x_dev, int32_t C) {
  return graph_segment_softmax_backward(e, "lb_graph_segment_softmax_backward", role, y_dev, d_y_dev, d_x_dev, C, LB_DTYPE_F32);
}

static int graph_attend(lb_engine* e, const char* entry, int32_t role, const void* logits, const void* values, void* out,
                        float* m, float* s, int32_t H, int32_t D, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, logits && values && out && m && s, H, D));
  if ((int64_t)H * D > INT32_MAX) return lb_fail(LB_ERR_ARG, "%s: H %d x D %d columns", entry, H, D);
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, H * D, D, true, {values, out});
  return graph_dispatch<true>(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_attend<T, decltype(w)::value>, P.L, P.walk, (const T*)logits, (const T*)values, (T*)out, m,
                 s, H, D);
  });
}
extern "C" int lb_graph_attend_t(lb_engine* e, int32_t role, const void* logits_dev, const void* values_dev, void* out_dev,
                                 float* m_dev, float* s_dev, int32_t H, int32_t D, int32_t dtype) {
  return graph_attend(e, "lb_graph_attend_t", role, logits_dev, values_dev, out_dev, m_dev, s_dev, H, D, dtype);
}
extern "C" int lb_graph_attend(lb_engine* e, int32_t role, const float* logits_dev, const float* values_dev, float* out_dev,
                               float* m_dev, float* s_dev, int32_t H, int32_t D) {
  return graph_attend(e, "lb_graph_attend", role, logits_dev, values_dev, out_dev, m_dev, s_dev, H, D, LB_DTYPE_F32);
}

static int graph_attend_backward(lb_engine* e, const char* entry, int32_t role, const void* logits, const void* values,
                                 const float* m, const float* s, const void* d_out, void* d_logits, void* d_values, int32_t H,
                                 int32_t D, int32_t dtype) {
  LB_TRY(graph_entry(e, entry, role, dtype, logits && values && m && s && d_out && d_logits && d_values, H, D));
  if ((int64_t)H * D > INT32_MAX) return lb_fail(LB_ERR_ARG, "%s: H %d x D %d columns", entry, H, D);
  const int64_t slots = (int64_t)e->g.B * e->e_cap;
  // t (slots, H) fp32: the d_logits buffer itself for float tensors, the engine's buffer for bf16 ones (t is never rounded)
  float* t = (float*)d_logits;
  if (dtype != LB_DTYPE_F32) {
    if (slots * H > e->graph_t_cap)
      LB_TRY(lb_regrow(e->stream, &e->graph_t_cap, slots * H + slots * H / 8, [&](int64_t n) { return e->mem.get(&e->graph_t, (size_t)n); }));
    t = e->graph_t;
  }
  const lb_gplan Pv = graph_plan(e, role, dtype, LB_SLOTS, H * D, D, true, {d_out, d_values});
  LB_TRY(graph_dispatch<true>(dtype, Pv.W, [&](auto t_, auto w) {
    using T = decltype(t_);
    graph_launch(e, Pv.blocks, k_graph_attend_dvalues<T, decltype(w)::value>, Pv.L, Pv.idx, (const T*)logits, m, s, (const T*)d_out,
                 (T*)d_values, H, D);
  }));
  // the two flat kernels - one lane per (slot, head), then per (node, head): no units, no lanes per row
  const lb_glist L = graph_list(e, 0, 0);
  LB_TRY(graph_dispatch<true>(dtype, graph_width(dtype, D, true, {values, d_out}), [&](auto t_, auto w) {
    using T = decltype(t_);
    graph_launch(e, graph_blocks1(slots * H), k_graph_attend_t<T, decltype(w)::value>, L, Pv.idx, (const T*)values,
                 (const T*)d_out, t, (T*)d_logits, H, D);
  }));
  return graph_dispatch(dtype, 1, [&](auto t_, auto) {
    using T = decltype(t_);
    graph_launch(e, graph_blocks1(e->BN * H), k_graph_attend_dlogits<T>, L, graph_walk(e, role), (const T*)logits, m, s,
                 (const float*)t, (T*)d_logits, H);
  });
}
extern "C" int lb_graph_attend_backward_t(lb_engine* e, int32_t role, const void* logits_dev, const void* values_dev,
                                          const float* m_dev, const float* s_dev, const void* d_out_dev, void* d_logits_dev,
                                          void* d_values_dev, int32_t H, int32_t D, int32_t dtype) {
  return graph_attend_backward(e, "lb_graph_attend_backward_t", role, logits_dev, values_dev, m_dev, s_dev, d_out_dev,
                               d_logits_dev, d_values_dev, H, D, dtype);
}
extern "C" int lb_graph_attend_backward(lb_engine* e, int32_t role, const float* logits_dev, const float* values_dev,
                                        const float* m_dev, const float* s_dev, const float* d_out_dev, float* d_logits_dev,
                                        float* d_values_dev, int32_t H, int32_t D) {
  return graph_attend_backward(e, "lb_graph_attend_backward", role, logits_dev, values_dev, m_dev, s_dev, d_out_dev, d_logits_dev,
                               d_values_dev, H, D, LB_DTYPE_F32);
}

// ---- the edge-message entries (float32 or bfloat16 by dtype; no float32-only twins)
extern "C" int lb_graph_conv(lb_engine* e, int32_t role, const void* x_dev, const void* w_dev, void* out_dev, int32_t K, int32_t C,
                             int32_t dtype) {
  // the sender view only where sender rows are walked (role 1); the other node of a slot comes from the compact list
  LB_TRY(graph_entry(e, "lb_graph_conv", role, dtype, x_dev && w_dev && out_dev, K, C));
  if ((int64_t)K * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "lb_graph_conv: K %d x C %d columns", K, C);
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {x_dev, w_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;   // K > 1: three k at a time
    graph_launch(e, P.blocks, K == 1 ? k_graph_conv<T, W, 1> : k_graph_conv<T, W, 3>, P.L, P.walk, P.oidx, (const T*)x_dev,
                 (const T*)w_dev, (T*)out_dev, K);
  });
}

// K and C of the vector ops: 1 <= K <= LB_GRAPH_MAX_K (u rows are read as scalars into registers), C >= 1
static int graph_vec_sizes(const char* entry, int32_t K, int32_t C) {
  if (K < 1 || K > LB_GRAPH_MAX_K || C < 1)
    return lb_fail(LB_ERR_ARG, "%s: K %d (1 .. %d), C %d (>= 1)", entry, K, LB_GRAPH_MAX_K, C);
  if ((int64_t)K * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "%s: K %d x C %d columns", entry, K, C);
  return LB_OK;
}

extern "C" int lb_graph_conv_vec(lb_engine* e, int32_t role, const void* x_dev, const void* w_dev, const void* u_dev,
                                 void* out_dev, int32_t K, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_conv_vec", role, dtype, x_dev && w_dev && u_dev && out_dev, 1, 1));
  LB_TRY(graph_vec_sizes("lb_graph_conv_vec", K, C));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {x_dev, w_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;   // K > 1: three k at a time
    graph_launch(e, P.blocks, K == 1 ? k_graph_conv_vec<T, W, 1> : k_graph_conv_vec<T, W, 3>, P.L, P.walk, P.oidx, (const T*)x_dev,
                 (const T*)w_dev, (const T*)u_dev, (T*)out_dev, K);
  });
}

extern "C" int lb_graph_conv_dot(lb_engine* e, int32_t role, const void* v_dev, const void* w_dev, const void* u_dev,
                                 void* out_dev, int32_t K, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_conv_dot", role, dtype, v_dev && w_dev && u_dev && out_dev, 1, 1));
  LB_TRY(graph_vec_sizes("lb_graph_conv_dot", K, C));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {v_dev, w_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_conv_dot<T, decltype(w)::value>, P.L, P.walk, P.oidx, (const T*)v_dev, (const T*)w_dev,
                 (const T*)u_dev, (T*)out_dev, K);
  });
}

extern "C" int lb_graph_conv_vec_edge_grad(lb_engine* e, int32_t s_role, const void* s_dev, const void* v_dev, const void* w_dev,
                                           const void* u_dev, void* d_w_dev, void* d_u_dev, int32_t K, int32_t C, int32_t dtype) {
  // edge-parallel: no view.  Either output may be null (not wanted), not both.
  LB_TRY(graph_entry(e, "lb_graph_conv_vec_edge_grad", s_role, dtype, s_dev && v_dev && w_dev && u_dev && (d_w_dev || d_u_dev), 1,
                     1, false));
  LB_TRY(graph_vec_sizes("lb_graph_conv_vec_edge_grad", K, C));
  const lb_gplan P = graph_plan(e, s_role, dtype, LB_SLOTS, C, C, false, {s_dev, v_dev, w_dev, d_w_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;   // K <= 3 (a vector in space): three k rows in registers
    graph_launch(e, P.blocks, K <= 3 ? k_graph_vec_edge_grad<T, W, 3> : k_graph_vec_edge_grad<T, W, LB_GRAPH_MAX_K>, P.L, P.idx,
                 P.oidx, (const T*)s_dev, (const T*)v_dev, (const T*)w_dev, (const T*)u_dev, (T*)d_w_dev, (T*)d_u_dev, K);
  });
}

// ---- filter_conv's entries.  K, R and C: K >= 1, 1 <= R <= LB_GRAPH_MAX_R (the weight columns of a unit live in registers), C >= 1
static int graph_filter_sizes(const char* entry, int32_t K, int32_t R, int32_t C) {
  if (K < 1 || R < 1 || R > LB_GRAPH_MAX_R || C < 1)
    return lb_fail(LB_ERR_ARG, "%s: K %d (>= 1), R %d (1 .. %d), C %d (>= 1)", entry, K, R, LB_GRAPH_MAX_R, C);
  if ((int64_t)K * C > INT32_MAX || (int64_t)R * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "%s: K %d, R %d x C %d columns", entry, K, R, C);
  return LB_OK;
}
// the span graph_width is asked for: units of at most 4 elements - bfloat16 rows in 8-byte units - so that the R x W weight columns
// of a unit fit a lane's registers
static int graph_filter_span(int32_t dtype, int C) { return dtype == LB_DTYPE_BF16 && C % 4 == 0 ? 4 : C; }
// f(lb_w<N>{}) with a compile-time bound N >= n out of the list
template <int... Ns, typename F>
static void graph_at_most(int n, F f) {
  bool done = false;
  ((!done && n <= Ns ? (f(lb_w<Ns>{}), done = true) : false), ...);
}

extern "C" int lb_graph_filter_conv(lb_engine* e, int32_t role, const void* x_dev, const void* f_dev, const void* weight_dev,
                                    void* out_dev, int32_t K, int32_t R, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_filter_conv", role, dtype, x_dev && f_dev && weight_dev && out_dev, 1, 1));
  LB_TRY(graph_filter_sizes("lb_graph_filter_conv", K, R, C));
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, graph_filter_span(dtype, C), true, {x_dev, weight_dev, out_dev});
  return graph_dispatch<true>(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    if constexpr (W <= 4)
      graph_at_most<20, 32>(R, [&](auto rm) {
        constexpr int RM = decltype(rm)::value;   // K > 1: three k at a time; f in groups of four where its rows allow it
        auto kernel = K == 1 ? k_graph_filter_conv<T, W, 1, RM, false> : k_graph_filter_conv<T, W, 3, RM, false>;
        if (R % 4 == 0 && graph_aligned({f_dev})) kernel = K == 1 ? k_graph_filter_conv<T, W, 1, RM, true> : k_graph_filter_conv<T, W, 3, RM, true>;
        graph_launch(e, P.blocks, kernel, P.L, P.walk, P.oidx, (const T*)x_dev, (const T*)f_dev, (const T*)weight_dev, (T*)out_dev,
                     K, R);
      });
  });
}

extern "C" int64_t lb_graph_filter_partials(lb_engine* e, int32_t R, int32_t C) {
  if (!e || e->e_cap <= 0 || R < 1 || C < 1) return 0;
  const int64_t slots = (int64_t)e->g.B * e->e_cap;
  return (slots + LB_GRAPH_FILTER_CHUNK - 1) / LB_GRAPH_FILTER_CHUNK * R * C;
}

extern "C" int lb_graph_filter_conv_grad(lb_engine* e, int32_t role, const void* x_dev, const void* d_dev, const void* f_dev,
                                         const void* weight_dev, void* d_f_dev, void* d_weight_dev, float* partials_dev,
                                         int64_t partials_len, int32_t K, int32_t R, int32_t C, int32_t dtype) {
  // edge-parallel: no view.  Either output may be null (not wanted), not both; the partials go with d_weight.
  const char* entry = "lb_graph_filter_conv_grad";
  LB_TRY(graph_entry(e, entry, role, dtype,
                     x_dev && d_dev && f_dev && weight_dev && (d_f_dev || d_weight_dev) && (partials_dev || !d_weight_dev), 1, 1,
                     false));
  LB_TRY(graph_filter_sizes(entry, K, R, C));
  const int64_t slots = (int64_t)e->g.B * e->e_cap, chunks = (slots + LB_GRAPH_FILTER_CHUNK - 1) / LB_GRAPH_FILTER_CHUNK;
  const int passes = (C + LB_GF_COLS - 1) / LB_GF_COLS;
  if (d_weight_dev && (partials_len < chunks * R * C || passes > 65535 || chunks > INT32_MAX))
    return lb_fail(LB_ERR_ARG, "%s: partials of %lld floats, %lld chunks x R %d x C %d needed", entry, (long long)partials_len,
                   (long long)chunks, R, C);
  const lb_gplan P = graph_plan(e, role, dtype, LB_SLOTS, C, graph_filter_span(dtype, C), true, {x_dev, d_dev});
  const lb_glist L = graph_list(e, 0, 0);   // (the tile kernels lay their lanes out themselves)
  const int64_t tiles = (slots + LB_GF_TILE - 1) / LB_GF_TILE;
  return graph_dispatch<true>(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    if constexpr (W <= 4)
      graph_at_most<1, 2, 3, 4>((R + 7) / 8, [&](auto rn) {
        constexpr int RN = decltype(rn)::value;
        if (d_f_dev)
          graph_launch(e, (unsigned)std::min<int64_t>(tiles, 2048), k_graph_filter_df<T, W, RN>, L, P.idx, P.oidx, (const T*)x_dev,
                       (const T*)d_dev, (const T*)weight_dev, (T*)d_f_dev, K, R, C);
        if (d_weight_dev) {
          hipLaunchKernelGGL((k_graph_filter_dw<T, W, RN>), dim3((unsigned)chunks, (unsigned)passes), dim3(256), 0, e->stream, L,
                             P.idx, P.oidx, (const T*)x_dev, (const T*)d_dev, (const T*)f_dev, partials_dev, K, R, C,
                             (int)LB_GRAPH_FILTER_CHUNK);
          graph_launch(e, graph_blocks1((int64_t)R * C), k_graph_filter_finish<T>, (const float*)partials_dev, chunks,
                       (int64_t)R * C, (T*)d_weight_dev);
        }
      });
  });
}

extern "C" int lb_graph_pair_mul(lb_engine* e, int32_t a_role, const void* a_dev, const void* b_dev, void* out_dev, int32_t K,
                                 int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_pair_mul", a_role, dtype, a_dev && b_dev && out_dev, K, C, false));   // edge-parallel: no view
  if ((int64_t)K * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "lb_graph_pair_mul: K %d x C %d columns", K, C);
  const lb_gplan P = graph_plan(e, a_role, dtype, LB_SLOTS, C, C, false, {a_dev, b_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    graph_launch(e, P.blocks, K == 1 ? k_graph_pair_mul<T, W, false> : k_graph_pair_mul<T, W, true>, P.L, P.idx, P.oidx,
                 (const T*)a_dev, (const T*)b_dev, (T*)out_dev, K);
  });
}

extern "C" int lb_graph_pair_add(lb_engine* e, int32_t a_role, const void* a_dev, const void* b_dev, void* out_dev, int32_t C,
                                 int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_pair_add", a_role, dtype, a_dev && b_dev && out_dev, C, 1, false));
  const lb_gplan P = graph_plan(e, a_role, dtype, LB_SLOTS, C, C, false, {a_dev, b_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    graph_launch(e, P.blocks, k_graph_pair_add<T, decltype(w)::value>, P.L, P.idx, P.oidx, (const T*)a_dev, (const T*)b_dev,
                 (T*)out_dev);
  });
}

// ---- edge pairs.  The reverse map of the current list -> e->rev (B E_cap): built at its first use after a list build, keyed on
// nl_gen and E_cap as the sender view is (whose buffers and flag it does not touch); one launch, nothing read back.
static int graph_reverse_map(lb_engine* e) {
  if (e->rev_seen && e->rev_gen == e->nl_gen && e->rev_ecap == e->e_cap) return LB_OK;
  const int64_t rows = (int64_t)e->g.B * e->e_cap;
  e->rev_seen = false;
  if (rows > e->rev_cap)
    LB_TRY(lb_regrow(e->stream, &e->rev_cap, rows, [&](int64_t n) { return e->mem.get(&e->rev, (size_t)n); }));
  hipLaunchKernelGGL(k_graph_reverse, dim3(graph_blocks1(rows)), dim3(256), 0, e->stream, graph_list(e, 0, 0), e->senders,
                     e->receivers, e->rev);
  LB_HIP(hipGetLastError());
  e->rev_gen = e->nl_gen;
  e->rev_ecap = e->e_cap;
  e->rev_seen = true;
  return LB_OK;
}

extern "C" int lb_graph_reverse(lb_engine* e, int32_t* out_dev) {
  LB_TRY(graph_entry(e, "lb_graph_reverse", 0, LB_DTYPE_F32, out_dev != nullptr, 1, 1, false));
  LB_TRY(graph_reverse_map(e));
  LB_HIP(hipMemcpyAsync(out_dev, e->rev, sizeof(int32_t) * (size_t)e->g.B * (size_t)e->e_cap, hipMemcpyDeviceToDevice, e->stream));
  return LB_OK;
}

extern "C" int lb_graph_edge_pair_t(lb_engine* e, int32_t mode, const void* msg_dev, void* out_dev, int32_t C, int32_t dtype) {
  LB_TRY(graph_entry(e, "lb_graph_edge_pair_t", 0, dtype, msg_dev && out_dev, C, 1, false));   // edge-parallel: no sender view
  if (mode < LB_GRAPH_PAIR_SWAP || mode > LB_GRAPH_PAIR_ANTISYM)
    return lb_fail(LB_ERR_ARG, "lb_graph_edge_pair_t: mode %d (0 swap, 1 symmetrize, 2 antisymmetrize)", mode);
  if (msg_dev == out_dev) return lb_fail(LB_ERR_ARG, "lb_graph_edge_pair_t: out must not be msg (a slot reads its partner's row)");
  LB_TRY(graph_reverse_map(e));
  const lb_gplan P = graph_plan(e, 0, dtype, LB_SLOTS, C, C, false, {msg_dev, out_dev});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    auto kernel = mode == LB_GRAPH_PAIR_SWAP ? k_graph_edge_pair<T, W, LB_GRAPH_PAIR_SWAP>
                  : mode == LB_GRAPH_PAIR_SYM ? k_graph_edge_pair<T, W, LB_GRAPH_PAIR_SYM>
                                              : k_graph_edge_pair<T, W, LB_GRAPH_PAIR_ANTISYM>;
    graph_launch(e, P.blocks, kernel, P.L, P.idx, (const int32_t*)e->rev, (const T*)msg_dev, (T*)out_dev);
  });
}

// ---- the multi-aggregator's entries.  `ops`: one nibble per plane of out from the low end, an op code LB_AGG_SUM .. LB_AGG_VAR,
// 0 ends the list; every code at most once, at least one, nothing after the end.
static int graph_aggregate_ops(const char* entry, int32_t ops, float eps, bool need_eps, lb_gagg* G) {
  int* const pos[6] = {&G->sum, &G->mean, &G->max, &G->min, &G->std, &G->var};
  *G = lb_gagg{0, -1, -1, -1, -1, -1, -1, eps};
  bool ended = false, ok = ops > 0;
  for (int a = 0; a < 8 && ok; ++a) {
    const int code = (ops >> (4 * a)) & 15;
    if (code == 0) {
      ended = true;
    } else if (ended || code > LB_AGG_VAR || *pos[code - 1] >= 0) {
      ok = false;
    } else {
      *pos[code - 1] = a;
      G->A = a + 1;
    }
  }
  if (!ok || G->A < 1) return lb_fail(LB_ERR_ARG, "%s: ops 0x%x (a nibble per plane: distinct codes 1 .. 6, 0 ends)", entry, ops);
  if (need_eps && G->std >= 0 && !(eps > 0.f)) return lb_fail(LB_ERR_ARG, "%s: eps %g with std (> 0)", entry, (double)eps);
  return LB_OK;
}
// <EXT, MOM> of the call as types, like graph_dispatch's (T, W)
template <typename F>
static void graph_aggregate_flags(bool ext, bool mom, F f) {
  using yes = std::true_type;
  using no = std::false_type;
  if (ext && mom) f(yes{}, yes{});
  else if (ext) f(yes{}, no{});
  else if (mom) f(no{}, yes{});
  else f(no{}, no{});
}

extern "C" int lb_graph_aggregate(lb_engine* e, int32_t role, const void* msg_dev, void* out_dev, int32_t* win_dev,
                                  float* stats_dev, int32_t C, int32_t ops, float eps, int32_t dtype) {
  if (!e) return lb_fail(LB_ERR_ARG, "null argument");
  lb_gagg G;
  LB_TRY(graph_aggregate_ops("lb_graph_aggregate", ops, eps, true, &G));
  const bool ext = G.max >= 0 || G.min >= 0, mom = G.std >= 0 || G.var >= 0;
  LB_TRY(graph_entry(e, "lb_graph_aggregate", role, dtype, msg_dev && out_dev && (win_dev || !ext) && (stats_dev || !mom), C, 1));
  if ((int64_t)G.A * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "lb_graph_aggregate: %d planes x C %d columns", G.A, C);
  const lb_gplan P = graph_plan(e, role, dtype, LB_NODES, C, C, false, {msg_dev, out_dev, ext ? win_dev : nullptr,
                                                                        mom ? stats_dev : nullptr});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    graph_aggregate_flags(ext, mom, [&](auto x, auto m) {
      graph_launch(e, P.blocks, k_graph_aggregate<T, W, decltype(x)::value, decltype(m)::value>, P.L, P.walk, G, (const T*)msg_dev,
                   (T*)out_dev, win_dev, stats_dev);
    });
  });
}

extern "C" int lb_graph_aggregate_backward(lb_engine* e, int32_t role, const void* d_out_dev, const void* msg_dev,
                                           const int32_t* win_dev, const float* stats_dev, void* d_msg_dev, int32_t C, int32_t ops,
                                           int32_t dtype) {
  if (!e) return lb_fail(LB_ERR_ARG, "null argument");
  lb_gagg G;
  LB_TRY(graph_aggregate_ops("lb_graph_aggregate_backward", ops, 0.f, false, &G));
  const bool ext = G.max >= 0 || G.min >= 0, mom = G.std >= 0 || G.var >= 0;
  // edge-parallel, but the degree of a slot's node comes from the rows of the role: the sender view for role 1
  LB_TRY(graph_entry(e, "lb_graph_aggregate_backward", role, dtype,
                     d_out_dev && d_msg_dev && (win_dev || !ext) && ((msg_dev && stats_dev) || !mom), C, 1));
  if ((int64_t)G.A * C > INT32_MAX) return lb_fail(LB_ERR_ARG, "lb_graph_aggregate_backward: %d planes x C %d columns", G.A, C);
  const lb_gplan P = graph_plan(e, role, dtype, LB_SLOTS, C, C, false, {d_out_dev, d_msg_dev, ext ? win_dev : nullptr,
                                                                        mom ? msg_dev : nullptr, mom ? stats_dev : nullptr});
  return graph_dispatch(dtype, P.W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W = decltype(w)::value;
    graph_aggregate_flags(ext, mom, [&](auto x, auto m) {
      graph_launch(e, P.blocks, k_graph_aggregate_bwd<T, W, decltype(x)::value, decltype(m)::value>, P.L, P.walk, G, P.idx,
                   (const T*)d_out_dev, (const T*)msg_dev, win_dev, stats_dev, (T*)d_msg_dev);
    });
  });
}

extern "C" int lb_graph_features_backward(lb_engine* e, const float* d_abs_pos, const float* d_vel_hist, const float* d_vel_mag,
                                          const float* d_bound, const float* d_rel_disp, const float* d_rel_dist,
                                          double* d_window_out) {
  if (!e || !d_window_out) return lb_fail(LB_ERR_ARG, "null argument");
  if (d_vel_mag && !e->g.has_vel_mag) return lb_fail(LB_ERR_ARG, "lb_graph_features_backward: d_vel_mag on an engine without vel_mag");
  if (d_bound && !e->g.has_bound) return lb_fail(LB_ERR_ARG, "lb_graph_features_backward: d_bound on an engine without bound");
  if (e->g.f32) return lb_fail(LB_ERR_UNSUPPORTED, "lb_graph_features_backward: float32 geometry");
  const bool edges = d_rel_disp || d_rel_dist;   // (only these need the sender view)
  LB_TRY(graph_entry(e, "lb_graph_features_backward", edges ? 1 : 0, LB_DTYPE_F32, true, 1, 1));
  lb_gfb_args a{};
  a.BN = e->BN; a.e_cap = e->e_cap; a.E = (int)e->graph_E;
  a.win = e->win; a.ctrl = e->ctrl; a.ptype = e->ptype; a.row_ptr = e->row_ptr;
  a.snd_ptr = edges ? e->snd_ptr : e->row_ptr; a.snd_perm = edges ? e->snd_perm : nullptr;
  a.efeat = e->efeat;
  a.d_abs = d_abs_pos; a.d_vh = d_vel_hist; a.d_vm = d_vel_mag; a.d_bd = d_bound; a.d_rd = d_rel_disp; a.d_rr = d_rel_dist;
  a.out = d_window_out;
  hipLaunchKernelGGL(k_graph_features_bwd, dim3(graph_blocks(e->BN * e->g.dim, 0)), dim3(256), 0, e->stream, e->g, a);
  LB_HIP(hipGetLastError());
  return LB_OK;
}
