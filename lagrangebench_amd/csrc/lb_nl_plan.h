// lb_nl_plan.h - which launches a neighbor-list build consists of, decided from a dozen host integers: lbk_nl_build
// (lb_neighbor.hip) fills an lb_nl_in, makes the plan and launches what it says; lb_nl_route prints it.  Plain C++ without HIP:
// tools/nl_plan_check.cpp includes this header alone, and tests/test_nl_plan.py checks the route table and every threshold
// from both sides without a GPU.  Every routing threshold lives here; the kernels of lb_neighbor.hip use the same names.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

// The staged-stencil and row-buffer limits belong to lb_internal.h (lb_api.hip reads them too); a host-only program gets
// them from here, and lb_neighbor.hip asserts that the two statements agree.
constexpr int lb_nl_stencil_cand = 2048, lb_nl_max_row = 256, lb_nl_max_row_dense = 4096;
#ifndef LB_MAX_STENCIL_CAND
#define LB_MAX_STENCIL_CAND lb_nl_stencil_cand
#define LB_MAX_ROW lb_nl_max_row
#define LB_MAX_ROW_DENSE lb_nl_max_row_dense
#endif

#define SCAN_THREADS 256
#define SCAN_CHUNK (SCAN_THREADS * 8)
// `small` = staged-candidate capacity of the one-wave k_nl variant to use (a multiple of 128 up to NL_SMALL_MAXC), or 0 for the
// 256-thread / 2048-candidate variant.  The LDS footprint of the staged stencil (28 B per candidate) sets how many cells a CU
// keeps in flight - the search is latency bound, so the smallest variant that holds cell_capacity * 3^dim candidates is used.
#define NL_SMALL_MAXC 1024
// (the comments in front of the kernels named here, lb_neighbor.hip, have the launches each limit saves and their timings)
#define LB_SMALL_N 4096   // nodes k_rows_small scans in one workgroup; nodes and cells k_cells_small<LB_SMALL_N / LB_SMALL_T> bins
#define LB_SMALL_T 1024   // threads of the one-workgroup kernels
#define LB_CELLS1_PER 8   // k_cells_small<LB_CELLS1_PER> (one mid-size trajectory), k_cells_traj: particles per thread
#define LB_CELLS1_N (LB_SMALL_T * LB_CELLS1_PER)
#define LB_CELLS1_NCELL 32768   // ... and the cells whose counters fit their dynamic LDS
#define NLW_WAVES 4       // k_nlw: receivers (waves) per workgroup
#define NLC_WAVES 4       // k_nlc: cells (waves) per workgroup
#define LB_CSCAN_N 16384  // nodes up to which k_nl_compact_scan is the update path's scan + finish + compaction
#define NLS_WAVES 16  // at most; the launch uses ceil(N / 256) waves so that every CU gets at most one workgroup
#define NLS_CAND 512  // stencil candidates per receiver (row buffer entries; >= LB_MAX_ROW)
#define NLM_N 8192
#define NLM_WAVES 16
#define NLM_RPW 2
#define NLM_ROWBUF 1024  // row buffer per wave: the hits of the receivers done (<= 256 each) + 768 candidates
#define LB_NLS_MAX_LDS (150 * 1024)  // dynamic LDS the single-launch builds may use
static_assert(NLS_CAND >= LB_MAX_ROW, "k_nl_small's row buffer holds a full row");

// What the decision reads, as lbk_nl_build finds it in the engine.
struct lb_nl_in {
  int B, N, dim;
  int64_t BN;
  bool f32, use_cell_list;
  int ncell[3], ncells, nstencil;
  int32_t cell_capacity, e_cap;   // frozen capacities (e_cap == 0: an allocation)
  bool nl_dense, nl_one_off, wg_sum;
  int32_t maxd;                   // per-node slots of the single-sweep update path, and whether its row buffers exist
  bool tmp_send, tmp_feat64, want_efeat64, fused;   // fused: lb_fused_launches(), false under LB_SMALL_FUSED=0
};

// What a build launches.  single: 0 none, 1 k_nl_small, 2 k_nl_mid.  cells, finish: the enums below (0 none).  search /
// count: the kernel of the NL_ROWS or NL_FILL sweep / of the NL_COUNT sweep, -1 none, else lb_nl_search_kind (an allocation
// that turns dense between the two sweeps counts with one kernel and fills with another).  cand / count_cand: staged
// capacity of k_nl (0 otherwise).  rows: NL_ROWS sweep.  compact: k_nl_compact follows.  reentry: an allocation counted with
// kernel kind reentry - 1 first, hit the stencil limit and ran again dense (lbk_nl_build writes it).
enum { LB_CELLS_STRIDED = 1, LB_CELLS_SMALL, LB_CELLS_TRAJ, LB_CELLS_MID, LB_CELLS_SORT };
enum { LB_FINISH_COMPACT_SCAN = 1, LB_FINISH_ROWS_SMALL, LB_FINISH_SCAN };
struct lb_nl_plan {
  int8_t single = 0, cells = 0, search = -1, count = -1, rows = 0, finish = 0, compact = 0, reentry = 0;
  int16_t cand = 0, count_cand = 0;
  int small = 0;                  // staged capacity of the one-wave k_nl variant, 0 = the 256-thread one
  bool strided = false;           // fixed-stride cell slots,
  int64_t strided_slots = 0;      // ... of all cells
  int npad = 0, nls_waves = 0;    // single-launch builds: N padded to 64, waves of k_nl_small,
  size_t single_lds = 0;          // ... dynamic LDS bytes,
  int single_blocks = 0, single_threads = 0;   // ... grid
  int ncell_tot = 0;              // grids: cells of the batch,
  int nb_cells = 0, nb_nodes = 0;    // ... workgroups of 256 cells (k_cell_zero) / nodes (k_cell_bin, k_cell_count, k_cell_fill),
  int nsb_cells = 0, nsb_rows = 0;   // ... scan chunks over the cells / the nodes,
  int64_t nb_search = 0;          // ... search workgroups of the sweep to launch,
  int search_waves = 0;           // ... their waves,
  int nb_rows16 = 0;              // ... workgroups of 16 rows (k_nl_compact_scan, k_nl_compact)
};

// Which search kernel a build uses, from the input alone: 0 = k_nl (workgroup per cell, staged stencil), 1 = k_nlw (wave per
// receiver), 2 = k_nlc (wave per cell).  Measured (MI355X, B = 8): 3^3-cell stencils favour the per-wave kernels (TGV3D 0.28
// -> 0.18 -> 0.12 ms per step), 3^2-cell stencils the staged per-cell kernel (DAM2D 0.11 vs 0.15 ms).  The dense fall-back
// (nl_dense, sticky) exceeds the staged kernels' LB_MAX_STENCIL_CAND candidates or LB_MAX_ROW neighbors: k_nlw with a row
// buffer sized from the largest degree runs (the reference re-allocates for ANY occupancy, rollout.py:134-151).
inline int lb_nl_search_kind(const lb_nl_in& in) {
  if (in.use_cell_list && !in.nl_dense && (in.dim == 3 || in.f32)) return 2;
  return in.nl_dense || in.f32 ? 1 : 0;
}

// The count sweep (count) or the NL_ROWS / NL_FILL sweep of plan p: kernel, staged capacity, grid.  lb_nl_make_plan calls it;
// an allocation calls it again for its fill sweep, after the count's read-back may have set in.nl_dense.
inline void lb_nl_plan_sweep(lb_nl_plan& p, const lb_nl_in& in, bool count) {
  const int kind = lb_nl_search_kind(in);
  (count ? p.count : p.search) = (int8_t)kind;
  (count ? p.count_cand : p.cand) = (int16_t)(kind ? 0 : p.small ? p.small : LB_MAX_STENCIL_CAND);
  p.search_waves = kind == 2 ? NLC_WAVES : kind == 1 ? NLW_WAVES : p.small ? 1 : 4;
  p.nb_search = kind == 2 ? (in.B * in.ncells + NLC_WAVES - 1) / NLC_WAVES : kind == 1 ? (in.BN + NLW_WAVES - 1) / NLW_WAVES
                                                                                       : in.B * in.ncells;
}

inline lb_nl_plan lb_nl_make_plan(const lb_nl_in& in) {
  lb_nl_plan p{};
  const int64_t BN = in.BN;
  const int ncell_tot = in.B * in.ncells;
  const int frozen = in.e_cap > 0;
  // LB_SMALL_FUSED=0: always the multi-launch bookkeeping (lb_fused_launches, lb_internal.h)
  const bool small_ok = in.fused;
  const bool small_rows = small_ok && BN <= LB_SMALL_N;
  const bool small_cells = small_rows && ncell_tot <= LB_SMALL_N;
  // one trajectory on the update path: the whole build is ONE launch - k_nl_small up to LB_SMALL_N particles, k_nl_mid with
  // a cell list whose masks fit LDS up to NLM_N
  const bool one_traj = small_ok && frozen && in.B == 1 && !in.nl_dense && !in.nl_one_off && in.wg_sum &&
                        in.ncell[0] < 2048 && in.ncell[1] < 2048 && in.ncell[2] < 1024;
  const int npad = (int)((BN + 63) / 64 * 64);
  const int64_t tab = in.use_cell_list ? (int64_t)(in.ncell[0] + in.ncell[1] + (in.dim == 3 ? in.ncell[2] : 0)) * (npad / 64) : 0;
  const int nls_waves = (int)std::min<int64_t>(NLS_WAVES, std::max<int64_t>(1, (BN + 255) / 256));
  const size_t nls_lds = (size_t)npad * (8 * in.dim + 4) + 8 * (size_t)tab + sizeof(int) * ((size_t)nls_waves * NLS_CAND + 32);
  const bool nls = one_traj && BN <= LB_SMALL_N && nls_lds <= LB_NLS_MAX_LDS &&
                   (!in.use_cell_list || (int64_t)in.cell_capacity * in.nstencil <= NLS_CAND);
  const size_t nlm_lds = 8 * (size_t)tab + sizeof(int) * ((size_t)npad + NLM_WAVES * NLM_ROWBUF + 48);
  const bool nlm = one_traj && BN > LB_SMALL_N && BN <= NLM_N && in.use_cell_list && nlm_lds <= LB_NLS_MAX_LDS &&
                   (int64_t)in.cell_capacity * in.nstencil <= NLM_ROWBUF - LB_MAX_ROW * (NLM_RPW - 1);
  p.npad = npad;
  p.nls_waves = nls_waves;
  if (nls || nlm) {
    p.single = nls ? 1 : 2;
    p.single_lds = nls ? nls_lds : nlm_lds;
    p.single_blocks = nls ? (int)((BN + nls_waves - 1) / nls_waves) : (int)((BN + NLM_WAVES * NLM_RPW - 1) / (NLM_WAVES * NLM_RPW));
    p.single_threads = 64 * (nls ? nls_waves : NLM_WAVES);
    return p;
  }
  // (one mid-size trajectory that the single-launch builds above refused, e.g. DAM2D: binning still in one launch)
  const bool mid_cells = small_ok && frozen && in.B == 1 && BN <= LB_CELLS1_N && ncell_tot <= LB_CELLS1_NCELL;
  // batches: one workgroup per trajectory, one launch (LB_SMALL_FUSED=0: the five-launch counting sort)
  // (measured, profiles/r04_ab_cells_traj.txt: 2.5 k particles x 8 23.1 -> 17.5 us, 5.7 k x 8 27.7 -> 22.7 us, 8 k x 8 30.8 -> 32.5 us -
  // one workgroup per trajectory is bound by its scattered stores from ONE CU; above 6 k particles the five launches stay)
  const bool traj_cells = small_ok && frozen && !small_cells && in.B > 1 && in.use_cell_list && in.N <= 6144 &&
                          in.ncells <= LB_CELLS1_NCELL;
  // frozen capacities + a search kernel that walks CELLS: fixed-stride slots, two launches (k_cell_zero, k_cell_bin)
  p.strided_slots = (int64_t)ncell_tot * in.cell_capacity;
#ifdef LB_NO_STRIDED   // (A/B builds: tools/build_variant.sh csr -DLB_NO_STRIDED)
  p.strided = false;
#else
  p.strided = small_ok && frozen && in.use_cell_list && in.cell_capacity > 0 && lb_nl_search_kind(in) != 1 &&
              p.strided_slots < ((int64_t)1 << 30);
#endif
  p.cells = p.strided ? LB_CELLS_STRIDED : small_cells ? LB_CELLS_SMALL : traj_cells ? LB_CELLS_TRAJ :
            mid_cells ? LB_CELLS_MID : LB_CELLS_SORT;
  p.ncell_tot = ncell_tot;
  p.nb_cells = (ncell_tot + 255) / 256;
  p.nb_nodes = (int)((BN + 255) / 256);
  p.nsb_cells = (ncell_tot + SCAN_CHUNK - 1) / SCAN_CHUNK;
  // one wave per cell when the frozen cell capacity bounds the stencil (a cell holding more than
  // cell_capacity particles flags overflow anyway); the 256-thread / 2048-candidate variant otherwise
  // (the LDS footprint of the staged stencil sets how many cells a CU keeps in flight)
  const int64_t cand_cap = (int64_t)in.cell_capacity * in.nstencil;
  p.small = (frozen && in.use_cell_list && cand_cap <= NL_SMALL_MAXC) ? (int)std::max<int64_t>(128, (cand_cap + 127) / 128 * 128) : 0;
  p.rows = frozen && in.maxd > 0 && in.tmp_send && (!in.want_efeat64 || in.tmp_feat64);
  // update path: ONE sweep writes the rows.  Otherwise count, finish and fill - an allocation reads the count back in
  // between and plans its fill sweep then (lbk_nl_build)
  if (!p.rows) lb_nl_plan_sweep(p, in, true);
  if (p.rows || frozen) lb_nl_plan_sweep(p, in, false);
  // update path of a small batch: scan + finish + compaction in one launch (LB_SMALL_FUSED=0: the separate launches)
  p.nb_rows16 = (int)((BN + 15) / 16);
  p.nsb_rows = (int)((BN + SCAN_CHUNK - 1) / SCAN_CHUNK);
  if (p.rows && small_ok && BN <= LB_CSCAN_N && in.B <= 64) {
    p.finish = LB_FINISH_COMPACT_SCAN;
  } else {
    p.finish = small_rows ? LB_FINISH_ROWS_SMALL : LB_FINISH_SCAN;
    p.compact = p.rows;
  }
  return p;
}

// The text of lb_nl_route (include/lbhip.h).
inline void lb_nl_route_text(char* out, size_t cap, const lb_nl_plan& r, int f32, int dim, int cell_list, int dense) {
  static const char* const single[] = {"multi", "k_nl_small", "k_nl_mid"};
  static const char* const cells[] = {"none", "strided", "cells_small", "cells_traj", "cells_mid", "sort"};
  static const char* const search[] = {"none", "k_nl", "k_nlw", "k_nlc"};
  static const char* const finish[] = {"none", "compact_scan", "rows_small", "scan+finish"};
  snprintf(out, cap,
           "build=%s;cells=%s;search=%s;cand=%d;count=%s;count_cand=%d;mode=%s;finish=%s%s;reentry=%s;f32=%d;dim=%d;cell_list=%d;"
           "dense=%d",
           single[r.single], cells[r.cells], search[r.search + 1], (int)r.cand, search[r.count + 1], (int)r.count_cand,
           r.rows ? "rows" : r.count >= 0 ? "count+fill" : "none", finish[r.finish], r.compact ? "+compact" : "",
           search[r.reentry], f32, dim, cell_list, dense);
}
