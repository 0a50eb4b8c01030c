// lb_sender_view.h - the kernels that build the sender-sorted view of the engine's edge list: per sender, the compact edge
// numbers of the edges it sends, in ascending order (snd_perm), and the row starts (snd_ptr).  Shared by the training step
// (lb_train.hip: train_sender_sort, a view per step in the handle's arena) and the graph ops (lb_graph.hip: a view per list
// build in the engine's arena).  Each translation unit gets its own copy (static); the hosts differ in who owns the buffers
// and in when the "edge without a transpose" flag is read.
#pragma once
#include "lb_internal.h"

// Sender-sorted view of the step's edge list WITHOUT a sort (round 6; hipcub::DeviceRadixSort until then: three rocprim
// kernels + a lower-bound pass per step).  The neighbor relation is symmetric - (r, s) is an edge iff (s, r) is - and the list
// is sorted by (receiver, sender): the edges SENT by node s are the transposes of row s, so s sends as many edges as it
// receives (snd_ptr == row_ptr) and, among the edges sent by s in ascending edge order (= ascending receiver), edge (r, s)
// has the rank that r has among the senders of row s.  One thread per edge: a bisection of row s (a dozen L2-resident
// integers) for r, then snd_perm[row_ptr[s] + rank] = edge.  The periodic displacement is antisymmetric only up to one
// rounding of (x + L/2), so a pair within ~1e-16 of the cutoff CAN be an edge in one direction only: a thread that does
// not find its transpose raises bit 4 of the step's guard flag - the reductions then add nothing and the step is repeated
// with the radix sort (lb_train.hip: train_loss_grad_guarded; lb_graph.hip reads the flag
// right after the launch and sorts).
static __global__ void k_sender_transpose(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ senders,
                                   const int32_t* __restrict__ receivers, int64_t E, int64_t BN, int32_t* __restrict__ snd_perm,
                                   int32_t* __restrict__ snd_ptr, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= BN) snd_ptr[i] = row_ptr[i];
  if (i >= E) return;
  const int r = receivers[i], s = senders[i];
  int lo = row_ptr[s], hi = row_ptr[s + 1];   // first position of row s whose sender is >= r
  const int end = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (senders[mid] < r) lo = mid + 1; else hi = mid;
  }
  if (lo < end && senders[lo] == r)
    snd_perm[lo] = (int32_t)i;
  else
    atomicOr(flag, 4);
}
static __global__ void k_iota(int32_t* __restrict__ x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = (int32_t)i;
}
// snd_ptr[s] = first position of key >= s in the sorted sender keys (lower bound), s = 0 .. N
static __global__ void k_lower_bounds(const int32_t* __restrict__ keys, int64_t E, int64_t N, int32_t* __restrict__ ptr) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > N) return;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < (int32_t)s) lo = mid + 1; else hi = mid;
  }
  ptr[s] = (int32_t)lo;
}
