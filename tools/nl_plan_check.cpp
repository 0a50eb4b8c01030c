// nl_plan_check.cpp - host-only run of csrc/lb_nl_plan.h (no HIP): which launches a neighbor-list build would consist of.
//   c++ -std=c++17 -Wall -o nl_plan_check tools/nl_plan_check.cpp && ./nl_plan_check < cases
// (tests/test_nl_plan.py builds and runs it; a -fsanitize=address,undefined build is run by hand)
// One build per input line, 22 integers: the fields of lb_nl_in in the order of FIELDS below, then the two facts an allocation
// (e_cap == 0) reads back from its count sweep - the largest number of candidates in one stencil (the staged k_nl flags a
// stencil above its capacity; the other kernels stage nothing) and the largest degree.  Per line, the text lb_nl_route would
// give after that build.
#include "../lagrangebench_amd/csrc/lb_nl_plan.h"

static const char* const FIELDS =
    "B N dim f32 use_cell_list ncell0 ncell1 ncell2 ncells nstencil cell_capacity e_cap nl_dense nl_one_off wg_sum maxd "
    "tmp_send tmp_feat64 want_efeat64 fused max_stencil max_deg";

// The build as lbk_nl_build runs it; the read-back of an allocation acts on in.nl_dense as the engine's does on e->nl_dense.
static lb_nl_plan build(lb_nl_in& in, long long max_stencil, long long max_deg) {
  lb_nl_plan p = lb_nl_make_plan(in);
  if (in.e_cap > 0 || p.single) return p;
  if (p.count == 0 && max_stencil > p.count_cand && !in.nl_dense) {  // density_error == 1
    in.nl_dense = true;
    const int8_t first = (int8_t)(p.count + 1);
    p = build(in, max_stencil, max_deg);
    p.reentry = first;
    return p;
  }
  if (max_deg > LB_MAX_ROW) in.nl_dense = true;
  lb_nl_plan_sweep(p, in, false);
  return p;
}

int main() {
  long long v[22];
  char text[512];
  for (int line = 1;; ++line) {
    int n = 0;
    while (n < 22 && scanf("%lld", &v[n]) == 1) ++n;
    if (n == 0) return 0;
    if (n < 22) {
      fprintf(stderr, "nl_plan_check: case %d has %d of the 22 fields: %s\n", line, n, FIELDS);
      return 1;
    }
    lb_nl_in in{(int)v[0], (int)v[1], (int)v[2], v[0] * v[1], v[3] != 0, v[4] != 0, {(int)v[5], (int)v[6], (int)v[7]}, (int)v[8],
                (int)v[9], (int32_t)v[10], (int32_t)v[11], v[12] != 0, v[13] != 0, v[14] != 0, (int32_t)v[15], v[16] != 0,
                v[17] != 0, v[18] != 0, v[19] != 0};
    const lb_nl_plan p = build(in, v[20], v[21]);
    lb_nl_route_text(text, sizeof(text), p, (int)in.f32, in.dim, (int)in.use_cell_list, (int)in.nl_dense);
    puts(text);
  }
}
