// lb_gns_repack.h - the packed GNS inference images as a JOB TABLE, and the one function that fills a destination entry.
//
// lb_gns_weights.hip states which image of which MLP goes where (lb_pack_fused / lb_pack_dense) against an lb_stage.  The
// direct stage packs host weights with the host packers (lb_gns_create).  The RECORDING stage runs the same policy code
// without weights and writes down, per image, a lb_pack_job: where it lies in lb_gns::blob, its packing kind and sizes and
// where its source matrix lies in a training handle's DEVICE weight blob (lb_train.hip; a latent below 128 is stored
// 128-padded there, the padding is zero and stays zero).  lb_gns_repack.hip replays the table on the device
// (lb_gns_train_sync_model); lb_gns_pack_selftest replays it on the host.  Both call lb_pack_entry below, so the index maps
// of the four packings and the fp16 hi / lo split exist once beside the host packers they are tested against.
//
// The decoder head's power-of-two scale and the rms guard of lb_gns_create are derived from the current weights by
// lb_pack_red_lane / lb_pack_red_rms / lb_head_shift (same header, same sharing).  The guard's rms is an fp64 sum in a FIXED order that differs from
// lb_stage::note_rms's (256 strided lanes, then lane order): the two can disagree about "rms < 2^-7" only for a matrix whose
// rms lies within rounding (a few ulp of fp64) of the threshold.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/lbhip.h"

#if defined(__HIPCC__)
#define LB_HD __host__ __device__
#else
#define LB_HD
#endif

// ------------------------------------------------------------------------------------------- fp16 conversion
// fp32 -> fp16 bits, round to nearest even, in integer arithmetic (fp16 subnormals included: the `lo` half of a weight
// below 2^-3 is one).  Equal to the compiler's (_Float16) conversion; written out so that host and device agree by construction.
LB_HD static inline uint16_t lb_f32_to_f16_rne(float f) {
  uint32_t x = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x47800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));  // inf / nan
  if (x < 0x38800000u) {  // subnormal half (or zero): value * 2^24 rounded to nearest even
    if (x < 0x33000000u) return (uint16_t)sign;
    const int shift = 126 - (int)(x >> 23);  // 14 .. 24
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    const uint32_t lsb = 1u << shift, half = lsb >> 1;
    uint32_t r = m >> shift;
    const uint32_t rem = m & (lsb - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    return (uint16_t)(sign | r);
  }
  uint32_t r = x - 0x38000000u;  // rebias exponent 127 -> 15
  const uint32_t rem = r & 0x1fffu;
  r >>= 13;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
  return (uint16_t)(sign | r);
}
LB_HD static inline float lb_f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0) {
    if (m == 0) {
      x = sign;
    } else {
      int k = 0;
      uint32_t mm = m;
      while (!(mm & 0x400u)) {
        mm <<= 1;
        ++k;
      }
      x = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ffu) << 13);
    }
  } else if (e == 31) {
    x = sign | 0x7f800000u | (m << 13);
  } else {
    x = sign | ((e + 112) << 23) | (m << 13);
  }
  return __builtin_bit_cast(float, x);
}

// ------------------------------------------------------------------------------------------- job table
enum lb_pack_kind {
  LB_PK_VEC = 0,  // a padded vector: Mpad floats, M of them from the source, the first at float `at`
  LB_PK_P32,      // lb_pack_weight     (Kpad x Mpad)
  LB_PK_P16,      // lb_pack_weight16   (Kpad x 128)
  LB_PK_P16H,     // lb_pack_weight16h  (Kpad x Mpad, hi | lo)
  LB_PK_MS        // lb_pack_ms         (Kpad = 32 nkb, Mpad = 128 npw, hi | lo), the first n_ent entries kept
};
// a rectangle of the (K, M) source matrix: element (row0 + r, col0 + c) = w[off + r * stride + c], r < rows, c < cols.
// What no piece covers is 0 (the zero padding the host assembles for [Ws | Wr] and the two-block node Linear).
struct lb_pack_piece {
  int64_t off;  // floats into the weight blob the table was recorded for
  int32_t row0, rows, stride, col0, cols, pad_;
};
struct lb_pack_job {
  int64_t dst;  // floats into lb_gns::blob; a multiple of 4
  int32_t kind, K, M, Kpad, Mpad;
  int32_t nkb;     // LB_PK_MS: k-blocks of 32
  int32_t perm;    // LB_PK_MS: the C-layout k permutation
  int32_t at;      // LB_PK_VEC
  int32_t scaled;  // source times the decoder head's power of two (lb_pack_stats::scale)
  int32_t n_ent;   // 16-byte destination entries
  int32_t piece0, n_pieces;
};
// the non-zero rms of one Linear (lb_stage::note_rms) / the largest |w| of the decoder head: sums over these pieces
struct lb_pack_red {
  int32_t piece0, n_pieces;
};
// 256 consecutive entries of one job = one workgroup of the pack kernel
struct lb_pack_block {
  int32_t job, ent0;
};
struct lb_pack_plan {
  std::vector<lb_pack_job> jobs;
  std::vector<lb_pack_piece> pieces;
  std::vector<lb_pack_red> rms;  // one per noted Linear
  lb_pack_red head{0, 0};        // n_pieces 0: no scaled head (num_mlp_layers != 2)
  std::vector<lb_pack_block> blocks;
  int64_t blob_floats = 0;  // floats of lb_gns::blob
  int64_t src_floats = 0;   // floats of the weight blob the offsets refer to
};
// what the device derives from the current weights before it packs
struct lb_pack_stats {
  float scale;     // 2^sh of the decoder head (1 without one)
  float unscale;   // 2^-sh = lb_gns::dec_unscale
  double rms_min;  // smallest non-zero rms over the noted Linears (1e30: none)
};
#define LB_PACK_LANES 256  // lanes of one reduction (the order of the fp64 sums is part of the result)

// ------------------------------------------------------------------------------------------- the element function
LB_HD static inline float lb_pack_src(const lb_pack_job& j, const lb_pack_piece* pc, const float* w, int k, int m) {
  if (k >= j.K || m >= j.M) return 0.f;
  for (int i = 0; i < j.n_pieces; ++i) {
    const lb_pack_piece& p = pc[j.piece0 + i];
    const int r = k - p.row0, c = m - p.col0;
    if (r >= 0 && r < p.rows && c >= 0 && c < p.cols) return w[p.off + (int64_t)r * p.stride + c];
  }
  return 0.f;
}

// The 16 bytes of destination entry `ent` of job j: four floats, or eight fp16 halves of the hi (part 0) or lo (part 1)
// image.  The index maps are those of lb_pack_weight (lb_gns.hip), lb_pack_weight16 / 16h (lb_edge16.hip) and lb_pack_ms
// (lb_msplit.hip) with the loops turned inside out: entry -> (k, m) of each of its elements.
LB_HD static inline void lb_pack_entry(const lb_pack_job& j, const lb_pack_piece* pc, const float* w, float scale, int ent,
                                       uint32_t out[4]) {
  const int lane = ent & 63, blk = ent >> 6;
  auto src = [&](int k, int m) {
    const float x = lb_pack_src(j, pc, w, k, m);
    return j.scaled ? x * scale : x;  // a power of two: exact
  };
  if (j.kind == LB_PK_VEC) {
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * ent + i - j.at;
      out[i] = __builtin_bit_cast(uint32_t, (c >= 0 && c < j.M) ? src(0, c) : 0.f);
    }
    return;
  }
  if (j.kind == LB_PK_P32) {  // entry = (kq * NMB + mb) * 64 + lane
    const int NMB = j.Mpad / 32, kq = blk / NMB, mb = blk % NMB;
    for (int i = 0; i < 4; ++i) out[i] = __builtin_bit_cast(uint32_t, src(8 * kq + 4 * (lane >> 5) + i, 32 * mb + (lane & 31)));
    return;
  }
  if (j.kind == LB_PK_P16) {  // entry = (((mbk * 4 + jj) * 2 + hf) * 64 + lane
    const int hf = blk & 1, jj = (blk >> 1) & 3, mbk = blk >> 3;
    for (int c = 0; c < 4; ++c)
      out[c] = __builtin_bit_cast(uint32_t, src(16 * mbk + 4 * (lane >> 4) + jj, 16 * (4 * hf + c) + (lane & 15)));
    return;
  }
  // the two fp16 kinds: entry = ((outer * 2) + part) * 64 + lane, eight halves
  const int part = blk & 1, outer = blk >> 1, g = lane >> 4;
  int kb, m;
  bool perm = true;
  if (j.kind == LB_PK_P16H) {  // outer = p * NMBO + mbo
    const int NMBO = j.Mpad / 16;
    kb = outer / NMBO;
    m = 16 * (outer % NMBO) + (lane & 15);
  } else {  // LB_PK_MS: outer = mb * nkb + kb
    kb = outer % j.nkb;
    m = 16 * (outer / j.nkb) + (lane & 15);
    perm = j.perm != 0;
  }
  uint16_t h[8];
  for (int i = 0; i < 8; ++i) {
    const int k = perm ? 32 * kb + 16 * (i >> 2) + 4 * g + (i & 3) : 32 * kb + 8 * g + i;
    const float x = src(k, m);
    const uint16_t hi = lb_f32_to_f16_rne(x);
    h[i] = part ? lb_f32_to_f16_rne(x - lb_f16_to_f32(hi)) : hi;
  }
  for (int i = 0; i < 4; ++i) out[i] = (uint32_t)h[2 * i] | ((uint32_t)h[2 * i + 1] << 16);
}

// ------------------------------------------------------------------------------------------- head scale, rms guard
// The power of two that brings max |w| of the decoder head into [0.25, 0.5): floor(log2(0.5 / mx)) for a finite non-zero
// mx, clamped to +-60, else 0 - from the bits of mx (mx = f 2^e, 1 <= f < 2: -1 - e when f = 1, else -2 - e), so that host
// and device need no log2 to agree.
LB_HD static inline int lb_head_shift(float mx) {
  const uint32_t b = __builtin_bit_cast(uint32_t, mx) & 0x7fffffffu;
  const int ef = (int)(b >> 23);
  if (b == 0 || ef == 255) return 0;
  if (ef == 0) return 60;  // an fp32 subnormal: far below 2^-61
  const int sh = ((b & 0x7fffffu) ? -2 : -1) - (ef - 127);
  return sh < -60 ? -60 : sh > 60 ? 60 : sh;
}
LB_HD static inline float lb_pow2f(int sh) { return __builtin_bit_cast(float, (uint32_t)(127 + sh) << 23); }  // |sh| <= 126

// lane `lane` of LB_PACK_LANES over the elements of a reduction's pieces, in (piece, row, column) order: the sum of squares
// and the count of its non-zero elements, and the largest |w| bits of its non-NaN elements
LB_HD static inline void lb_pack_red_lane(const lb_pack_red& r, const lb_pack_piece* pc, const float* w, int lane, double* s2,
                                          double* nz, uint32_t* mx) {
  double s = 0, n = 0;
  uint32_t m = 0;
  for (int i = 0; i < r.n_pieces; ++i) {
    const lb_pack_piece& p = pc[r.piece0 + i];
    const int cnt = p.rows * p.cols;  // (at most 128 x 128)
    for (int q = lane; q < cnt; q += LB_PACK_LANES) {
      const float x = w[p.off + (int64_t)(q / p.cols) * p.stride + (q % p.cols)];
      s += (double)x * x;
      n += x != 0.f;
      const uint32_t a = __builtin_bit_cast(uint32_t, x) & 0x7fffffffu;
      if (a <= 0x7f800000u && a > m) m = a;
    }
  }
  *s2 = s;
  *nz = n;
  *mx = m;
}
// ... and the lanes of one reduction combined in lane order: rms over the non-zero elements (1e30: all zero)
LB_HD static inline double lb_pack_red_rms(const double* s2, const double* nz) {
  double s = 0, n = 0;
  for (int i = 0; i < LB_PACK_LANES; ++i) {
    s += s2[i];
    n += nz[i];
  }
  return n > 0 ? __builtin_sqrt(s / n) : 1e30;
}

// ------------------------------------------------------------------------------------------- host entry points
struct lb_gns;
struct lb_engine;
// lb_gns_weights.hip: the job table of a model with this description (kq_node as lb_gns_create derives it), recorded by
// the packing policies; cmap (or null: identity) maps an index of the GNS.flatten blob to the source blob's
int lb_gns_pack_plan_build(const lb_gns_desc* d, int kq_node, const std::vector<int64_t>* cmap, int64_t n_compact,
                           int64_t n_src, lb_pack_plan* plan);
// lb_train.hip: the device layout of a training handle's blobs for this description (no HIP call)
int lb_gns_train_padded_map(const lb_gns_desc* d, std::vector<int64_t>* cmap, int64_t* n_dev, int64_t* n_compact);
// lb_gns_repack.hip: replay g's table on the device from w_dev (a blob in the layout cmap describes), on the engine's stream
struct lb_repack;
int lbk_gns_repack(lb_engine* e, lb_gns* g, const float* w_dev, const std::vector<int64_t>& cmap, int64_t n_compact,
                   int64_t n_src);
void lb_repack_free(lb_repack* r);
