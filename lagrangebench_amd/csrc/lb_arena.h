// lb_arena.h - the only place of liblbhip.so that allocates or frees device and pinned host memory.
//
// Ownership: every object that keeps buffers (engine, model, training handle, a solver's locals) has ONE lb_arena.  Its
// fields stay raw pointers; the arena records the pointer VALUES it handed out, and frees what is left when it is
// destroyed.  A destroy function therefore lists no buffers.
// Capacity last: a set of buffers that grows with a capacity goes through lb_regrow, which zeroes the capacity before the
// first allocation and writes it back only after the last one has succeeded.  The "is it large enough" tests key on the
// capacity alone.
//
// The primitives sit behind three macros, so that a host program without HIP can compile this header with its own
// (tools/arena_check.cpp): LB_ARENA_ALLOC(void** pp, size_t bytes, bool pinned, unsigned flags) -> true on success,
// LB_ARENA_FREE(void* p, bool pinned), and LB_ARENA_SYNC(stream) -> true on success.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/lbhip.h"

#ifndef LB_ARENA_ALLOC
#include <hip/hip_runtime.h>
#define LB_ARENA_ALLOC(pp, bytes, pinned, flags) \
  (((pinned) ? hipHostMalloc((pp), (bytes), (flags)) : hipMalloc((pp), (bytes))) == hipSuccess)
#define LB_ARENA_FREE(p, pinned) ((pinned) ? (void)hipHostFree(p) : (void)hipFree(p))
#define LB_ARENA_SYNC(stream) (hipStreamSynchronize(stream) == hipSuccess)
#endif

int lb_fail(int code, const char* fmt, ...);

template <typename T>
struct lb_arena_elem {
  static constexpr size_t size = sizeof(T);
};
template <>
struct lb_arena_elem<void> {  // a byte buffer (radix-sort scratch)
  static constexpr size_t size = 1;
};

struct lb_arena {
  lb_arena() = default;
  lb_arena(const lb_arena&) = delete;
  lb_arena& operator=(const lb_arena&) = delete;
  ~lb_arena() { clear(); }

  // *p = n elements of device memory (n == 0: one).  A non-null *p must be this arena's and is freed first.
  // On failure *p is null and the arena holds what it held before, less the old *p.
  template <typename T>
  int get(T** p, size_t n) {
    return take((void**)p, (n ? n : 1) * lb_arena_elem<T>::size, false, 0);
  }
  // ... of pinned host memory (hipHostMalloc flags)
  template <typename T>
  int get_pinned(T** p, size_t n, unsigned flags = 0) {
    return take((void**)p, (n ? n : 1) * lb_arena_elem<T>::size, true, flags);
  }
  // free *p and null it; null is a no-op, a pointer this arena does not own is refused and left alone
  template <typename T>
  int drop(T** p) {
    return release((void**)p);
  }
  void clear() {
    for (const rec& r : owned) LB_ARENA_FREE(r.p, r.pinned);
    owned.clear();
  }
  size_t live() const { return owned.size(); }

 private:
  struct rec {
    void* p;
    bool pinned;
  };
  std::vector<rec> owned;

  int release(void** p) {
    if (!*p) return LB_OK;
    for (size_t i = 0; i < owned.size(); ++i)
      if (owned[i].p == *p) {
        LB_ARENA_FREE(owned[i].p, owned[i].pinned);
        owned[i] = owned.back();
        owned.pop_back();
        *p = nullptr;
        return LB_OK;
      }
    return lb_fail(LB_ERR_ARG, "lb_arena: %p is not owned by this arena", *p);
  }
  int take(void** p, size_t bytes, bool pinned, unsigned flags) {
    if (int rc = release(p)) return rc;
    owned.reserve(owned.size() + 1);  // (the record of a successful allocation cannot fail to be kept)
    void* q = nullptr;
    if (!LB_ARENA_ALLOC(&q, bytes, pinned, flags))
      return lb_fail(LB_ERR_HIP, "%s of %zu bytes failed", pinned ? "hipHostMalloc" : "hipMalloc", bytes);
    owned.push_back({q, pinned});
    *p = q;
    return LB_OK;
  }
};

// The one regrow frame: wait for the stream's readers of the old buffers, capacity = 0, alloc(want) calls arena.get for every
// buffer of the set (get frees the old one), capacity = want only when all of them succeeded.
template <typename S, typename C, typename F>
int lb_regrow(S stream, C* cap, C want, F alloc) {
  if (!LB_ARENA_SYNC(stream)) return lb_fail(LB_ERR_HIP, "hipStreamSynchronize failed before a regrow");
  *cap = 0;
  if (int rc = alloc(want)) return rc;
  *cap = want;
  return LB_OK;
}
