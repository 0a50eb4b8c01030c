// arena_check.cpp - host-only check of csrc/lb_arena.h (no HIP): the allocation primitives are a counting malloc / free that
// can be told to fail on the k-th allocation.
//   c++ -std=c++17 -Wall -o arena_check tools/arena_check.cpp && ./arena_check
// (tests/test_device_memory.py builds and runs it; a -fsanitize=address,undefined build is run by hand)
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

static int g_live = 0;       // allocations not yet freed
static int g_allocs = 0;     // allocations asked for since the last arm()
static int g_fail_at = 0;    // fail the k-th of them (1-based; 0 = none)
static int g_syncs = 0;
static size_t g_last_bytes = 0;
static bool g_last_pinned = false;
static unsigned g_last_flags = 0;

static bool check_alloc(void** pp, size_t bytes, bool pinned, unsigned flags) {
  g_last_bytes = bytes;
  g_last_pinned = pinned;
  g_last_flags = flags;
  if (++g_allocs == g_fail_at) return false;
  *pp = malloc(bytes);
  if (!*pp) return false;
  ++g_live;
  return true;
}
static void check_free(void* p, bool) {
  free(p);
  --g_live;
}
static void arm(int k) {
  g_allocs = 0;
  g_fail_at = k;
}

#define LB_ARENA_ALLOC(pp, bytes, pinned, flags) check_alloc((pp), (bytes), (pinned), (flags))
#define LB_ARENA_FREE(p, pinned) check_free((p), (pinned))
#define LB_ARENA_SYNC(stream) (++g_syncs, (stream) == 0)
#include "../lagrangebench_amd/csrc/lb_arena.h"

static char g_msg[512];
int lb_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return code;
}

static int g_bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      ++g_bad;                                                     \
    }                                                              \
  } while (0)

struct three {  // a set of buffers under one capacity
  float* a = nullptr;
  double* b = nullptr;
  int* c = nullptr;
  long cap = 0;
};
static int grow(lb_arena& m, three& s, long want, int stream = 0) {
  return lb_regrow(stream, &s.cap, want, [&](long n) {
    if (int rc = m.get(&s.a, (size_t)n)) return rc;
    if (int rc = m.get(&s.b, (size_t)n)) return rc;
    return m.get(&s.c, (size_t)n + 1);
  });
}
static void touch(three& s) {  // every buffer of a complete set is writable over its whole length
  for (long i = 0; i < s.cap; ++i) s.a[i] = 1.f, s.b[i] = 2.0, s.c[i] = 3;
  s.c[s.cap] = 4;
}

int main() {
  arm(0);
  {  // get, regrow by get, drop, clear, destructor
    lb_arena m;
    float* x = nullptr;
    double* y = nullptr;
    int* pin = nullptr;
    CHECK(m.get(&x, 10) == LB_OK && x && g_live == 1 && m.live() == 1 && g_last_bytes == 10 * sizeof(float) && !g_last_pinned);
    x[9] = 1.f;
    CHECK(m.get(&y, 3) == LB_OK && y && g_live == 2 && g_last_bytes == 3 * sizeof(double));
    CHECK(m.get(&x, 100) == LB_OK && x && g_live == 2 && m.live() == 2);  // the old x is freed
    x[99] = 1.f;
    CHECK(m.get_pinned(&pin, 4, 2u) == LB_OK && pin && g_live == 3 && g_last_pinned && g_last_flags == 2u &&
          g_last_bytes == 4 * sizeof(int));
    CHECK(m.get_pinned(&pin, 8) == LB_OK && g_live == 3 && g_last_flags == 0u);
    CHECK(m.drop(&y) == LB_OK && !y && g_live == 2 && m.live() == 2);
    CHECK(m.drop(&y) == LB_OK && g_live == 2);  // null: nothing to do
    // n == 0 allocates one element
    char* z = nullptr;
    void* raw = nullptr;
    CHECK(m.get(&z, 0) == LB_OK && z && g_last_bytes == 1 && g_live == 3);
    z[0] = 1;
    CHECK(m.get(&raw, 0) == LB_OK && raw && g_last_bytes == 1);
    CHECK(m.get(&raw, 24) == LB_OK && raw && g_last_bytes == 24 && g_live == 4);  // void: bytes
    // an unowned pointer is refused by drop and by get, and left alone
    float local = 0.f, *foreign = &local;
    CHECK(m.drop(&foreign) == LB_ERR_ARG && foreign == &local && g_live == 4 && m.live() == 4);
    CHECK(m.get(&foreign, 4) == LB_ERR_ARG && foreign == &local && g_live == 4);
    lb_arena other;
    CHECK(other.drop(&x) == LB_ERR_ARG && x && g_live == 4);
    // a failed get: null pointer, nothing leaked, the old buffer of that pointer gone, the arena usable
    arm(1);
    CHECK(m.get(&x, 1000) == LB_ERR_HIP && !x && g_live == 3 && m.live() == 3);
    arm(1);
    double* w = nullptr;
    CHECK(m.get(&w, 5) == LB_ERR_HIP && !w && g_live == 3 && m.live() == 3);
    arm(0);
    CHECK(m.get(&x, 7) == LB_OK && x && g_live == 4);
    m.clear();
    CHECK(g_live == 0 && m.live() == 0);
    x = nullptr;  // (clear() leaves the caller's pointers dangling)
    CHECK(m.get(&x, 2) == LB_OK && m.get(&w, 2) == LB_OK && g_live == 2);
  }
  CHECK(g_live == 0);  // the destructor

  // lb_regrow over a three-buffer set, a failure at each position in turn
  for (int k = 1; k <= 3; ++k)
    for (int had_old = 0; had_old < 2; ++had_old) {
      lb_arena m;
      three s;
      arm(0);
      if (had_old) {
        CHECK(grow(m, s, 8) == LB_OK && s.cap == 8 && g_live == 3);
        touch(s);
      }
      const int syncs = g_syncs;
      arm(k);
      CHECK(grow(m, s, 64) == LB_ERR_HIP);
      CHECK(g_syncs == syncs + 1);
      CHECK(s.cap == 0);
      // every pointer is null or a live buffer of the arena: k - 1 new ones, the failed one null, the rest old (or null)
      const int want_live = (k - 1) + (had_old ? 3 - k : 0);
      CHECK(g_live == want_live && (int)m.live() == want_live);
      void* ptrs[3] = {s.a, s.b, s.c};
      CHECK(ptrs[k - 1] == nullptr);
      for (int i = 0; i < 3; ++i) CHECK((ptrs[i] != nullptr) == (i < k - 1 || (had_old && i > k - 1)));
      arm(0);
      CHECK(grow(m, s, 64) == LB_OK && s.cap == 64 && s.a && s.b && s.c && g_live == 3 && m.live() == 3);
      touch(s);
    }
  CHECK(g_live == 0);
  {  // a failed synchronisation allocates nothing and leaves the set as it was
    lb_arena m;
    three s;
    arm(0);
    CHECK(grow(m, s, 8) == LB_OK);
    float* a0 = s.a;
    CHECK(grow(m, s, 16, 1) == LB_ERR_HIP && s.cap == 8 && s.a == a0 && g_live == 3);
  }
  CHECK(g_live == 0);
  printf(g_bad ? "arena_check: %d FAILED\n" : "arena_check: ok\n", g_bad);
  return g_bad ? 1 : 0;
}
