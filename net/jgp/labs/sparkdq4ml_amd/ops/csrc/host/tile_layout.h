// The MFMA-fragment tile formats of an assembled feature matrix, in ONE place: the tall bf16 tiles
// (TiledBF16, d <= 64) and the wide bf16 / wide fp8 tiles (TiledWide).  The packers (rowops.hip,
// gram_wide.hip), the row readers (rowops.hip), the lsq passes (lsq.hip, lsq_qn.hip) and every
// launcher that sizes a tiled buffer take the format from here; ops/layout.py (tiled_offsets,
// wide_offsets) is the specification, and tests/test_tile_layout_host.py compares the two on the
// CPU through the host module.  The Gram inner loops (gram.hip's tall kernels, gram_stream.hip,
// gram_folds.hip, glm_irls.hip, WideTraits and the SYRK main loop of gram_wide.hip) still carry
// their own addressing (docs/DESIGN.md, "Tile layouts").
//
// A matrix is a [superstep s][tile t] grid of chunks, t < tiles(layout, d): 64 rows x 32 features,
// 2048 elements.  Inside a chunk a feature's 8 consecutive rows (a *run*: q = (r >> 3) & 7 of
// feature lane fl = f & 31) are contiguous, and an MFMA lane's 16-byte fragment is one run (bf16)
// or two runs 16 rows apart (fp8):
//   tall bf16   [4 k-steps i][64 lanes][8]:  lane 32h + fl holds rows 32h + 8i + j   (q = 4h + i)
//   wide bf16   [4 k-steps ki][64 lanes][8]: lane 32h + fl holds rows 16ki + 8h + j  (q = 2ki + h)
//   wide fp8    [2 halves][64 lanes][16]:    a lane's 32 bytes are its k-steps 0..3, half = ki >> 1
//
// The shared part is scalar constexpr code with no thread index: it compiles for the host (g++)
// and, under hipcc, for the device.  The fragment / run loads and stores below it are device code.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include "common.h"
#define DQ_TL_FN __host__ __device__ __forceinline__ constexpr
#else
#define DQ_TL_FN constexpr
#endif

namespace dq4ml {
namespace tile {

// layout codes (the ``tiled`` argument of rowops, LsqX::layout)
enum Layout : int { kPlain = 0, kTall = 1, kWide = 2, kWideFp8 = 3 };

constexpr int kSupRows = 64;      // rows per superstep
constexpr int kTileFeats = 32;    // features per tile
constexpr int kChunkElems = kSupRows * kTileFeats;

// the wide layout of TiledWide's ``eb`` (bytes of a lane's 8-row run: 16 bf16, 8 fp8; the
// launchers reject any other value before they get here)
DQ_TL_FN int wide_layout(int eb) { return eb == 8 ? kWideFp8 : kWide; }
DQ_TL_FN int elem_bytes(int layout) { return layout == kWideFp8 ? 1 : 2; }
DQ_TL_FN int frag_elems(int layout) { return 16 / elem_bytes(layout); }  // of a lane's 16 bytes
DQ_TL_FN int64_t chunk_bytes(int layout) { return (int64_t)kChunkElems * elem_bytes(layout); }
// a *unit* is what one wave reads with one 16-byte load per lane: 16 rows (bf16) / 32 rows (fp8)
DQ_TL_FN int units_per_sup(int layout) { return (int)(chunk_bytes(layout) / (64 * 16)); }

DQ_TL_FN int live_tiles(int d) { return (d + 31) >> 5; }
// tile stride NT of a superstep: tall = the live tiles, wide = whole 256-feature panels (kPlain has
// no tiles: callers branch on it first)
DQ_TL_FN int tiles(int layout, int d) { return layout == kTall ? live_tiles(d) : ((d + 255) >> 8) * 8; }
DQ_TL_FN int64_t supersteps(int64_t n) { return (n + 63) >> 6; }
DQ_TL_FN int64_t bytes(int layout, int d, int64_t n) { return supersteps(n) * tiles(layout, d) * chunk_bytes(layout); }

// Run q of feature lane fl in chunk `chunk` (= s * NT + t).  In the bf16 layouts a run is one
// 16-byte slot of the matrix, run_slot; run_offset is the element offset of a run's first row in
// any layout.  (The sums stay 64-bit and in this order: the shape the packers and the row readers
// compiled from.)
DQ_TL_FN int64_t run_slot(int layout, int64_t chunk, int q, int fl) {
  return layout == kTall ? chunk * 256 + (q & 3) * 64 + (q >> 2) * 32 + fl
                         : chunk * 256 + (q >> 1) * 64 + 32 * (q & 1) + fl;
}
DQ_TL_FN int64_t run_offset(int layout, int64_t chunk, int q, int fl) {
  if (layout != kWideFp8) return run_slot(layout, chunk, q, fl) << 3;
  const int lane = 32 * (q & 1) + fl, ki = q >> 1;  // k-step ki -> half ki >> 1, byte 8 * (ki & 1)
  return chunk * 2048 + (((ki >> 1) * 64 + lane) << 4) + ((ki & 1) << 3);
}

// element offset of (feature f, row r): the twin of layout.py's tiled_offsets / wide_offsets
DQ_TL_FN int64_t elem_offset(int layout, int f, int64_t r, int NT) {
  const int64_t s = r >> 6;
  if (layout == kTall) {
    const int h = (int)((r >> 5) & 1), i = (int)((r >> 3) & 3), j = (int)(r & 7);
    const int t = f >> 5, lane = 32 * h + (f & 31);
    return ((((s * NT + t) * 4 + i) * 64 + lane) << 3) + j;
  }
  const int ki = (int)((r >> 4) & 3), h = (int)((r >> 3) & 1), j = (int)(r & 7);
  const int t = f >> 5, lane = 32 * h + (f & 31);
  if (layout == kWide) return ((((s * NT + t) * 4 + ki) * 64 + lane) << 3) + j;
  return (s * NT + t) * 2048 + (((ki >> 1) * 64 + lane) << 4) + ((ki & 1) << 3) + j;
}

// the 16-byte fragment of `lane` in unit `sub` of chunk (s * NT + t), from `base`: a byte offset
// (frag_byte) or the matrix pointer (frag_ptr, below).  The chunk is added first and the 32-bit
// slot second: the order the lsq passes compiled from.
template <typename B>
DQ_TL_FN B frag_at(B base, int layout, int64_t chunk, int sub, int lane) {
  return base + chunk * chunk_bytes(layout) + ((sub * 64 + lane) << 4);
}
DQ_TL_FN int64_t frag_byte(int layout, int64_t chunk, int sub, int lane) {
  return frag_at<int64_t>(0, layout, chunk, sub, lane);
}

// the inverse map: row of element e of the fragment of lane half h in unit `sub` of superstep s
DQ_TL_FN int64_t frag_row(int layout, int64_t s, int sub, int h, int e) {
  return layout == kTall   ? s * 64 + 32 * h + 8 * sub + e
         : layout == kWide ? s * 64 + 16 * sub + 8 * h + e
                           : s * 64 + 16 * (2 * sub + (e >> 3)) + 8 * h + (e & 7);
}

// a wrong edit fails here, in both compilers: every chunk is filled exactly from its first to its
// last element, and a fragment's elements sit where frag_row says their rows are
static_assert(tiles(kTall, 33) == 2 && tiles(kWide, 257) == 16 && live_tiles(257) == 9, "tile strides");
static_assert(bytes(kTall, 33, 130) == 3 * 2 * 4096 && bytes(kWideFp8, 257, 130) == 3 * 16 * 2048, "sizes");
static_assert(units_per_sup(kTall) == 4 && units_per_sup(kWide) == 4 && units_per_sup(kWideFp8) == 2, "units");
static_assert(elem_offset(kTall, 0, 0, 2) == 0 && elem_offset(kTall, 31, 63, 2) == 2047, "tall chunk");
static_assert(elem_offset(kWide, 0, 0, 8) == 0 && elem_offset(kWide, 31, 63, 8) == 2047, "wide bf16 chunk");
static_assert(elem_offset(kWideFp8, 0, 0, 8) == 0 && elem_offset(kWideFp8, 31, 63, 8) == 2047, "wide fp8 chunk");
static_assert(elem_offset(kTall, 32, 64, 2) == 3 * 2048 && elem_offset(kWide, 32, 64, 8) == 9 * 2048, "chunk grid");
static_assert(elem_offset(kTall, 5, frag_row(kTall, 2, 3, 1, 7), 2) * 2 == frag_byte(kTall, 4, 3, 37) + 14, "tall inverse");
static_assert(elem_offset(kWide, 5, frag_row(kWide, 2, 3, 1, 7), 8) * 2 == frag_byte(kWide, 16, 3, 37) + 14, "wide inverse");
static_assert(elem_offset(kWideFp8, 5, frag_row(kWideFp8, 2, 1, 1, 15), 8) == frag_byte(kWideFp8, 16, 1, 37) + 15,
              "fp8 inverse");

#if defined(__HIPCC__)
// ---- device side: fragments and runs as f32 -------------------------------------------------
__device__ __forceinline__ void fp8x8_to_f32(unsigned lo, unsigned hi, float x[8]) {
  x[0] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 0);
  x[1] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 1);
  x[2] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 2);
  x[3] = __builtin_amdgcn_cvt_f32_fp8((int)lo, 3);
  x[4] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 0);
  x[5] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 1);
  x[6] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 2);
  x[7] = __builtin_amdgcn_cvt_f32_fp8((int)hi, 3);
}

// where the lsq passes read
template <int L>
__device__ __forceinline__ const unsigned char* frag_ptr(const unsigned char* base, int64_t chunk, int sub,
                                                         int lane) {
  return frag_at(base, L, chunk, sub, lane);
}

// a lane's 16-byte fragment -> its frag_elems(L) values
template <int L>
__device__ __forceinline__ void unpack(const u32x4 q, float* x) {
  if constexpr (L == kWideFp8) {
    fp8x8_to_f32(q[0], q[1], x);
    fp8x8_to_f32(q[2], q[3], x + 8);
  } else {
    bf16x8_to_f32(q, x);
  }
}

// one element as f32 (the scalar row readers); NT = tiles(L, d)
template <int L>
__device__ __forceinline__ float load_elem(const void* X, int f, int64_t r, int NT) {
  const int64_t o = elem_offset(L, f, r, NT);
  if constexpr (L == kWideFp8) return __builtin_amdgcn_cvt_f32_fp8((int)reinterpret_cast<const uint8_t*>(X)[o], 0);
  else return bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(X)[o]);
}

// run q of feature lane fl of chunk `chunk` (= s * NT + t): its 8 rows as f32 ...
template <int L>
__device__ __forceinline__ void load_run(const unsigned char* X, int64_t chunk, int q, int fl, float x[8]) {
  if constexpr (L == kWideFp8) {
    const uint64_t v = *gptr<uint64_t>(X + run_offset(L, chunk, q, fl));
    fp8x8_to_f32((unsigned)v, (unsigned)(v >> 32), x);
  } else {
    bf16x8_to_f32(gptr<u32x4>(X)[run_slot(L, chunk, q, fl)], x);
  }
}

// ... and stored from 8 floats: a bf16 cast, or an e4m3 pack of values already scaled and clamped
// to [-448, 448] (the conversion maps overflow to NaN)
template <int L>
__device__ __forceinline__ void store_run(unsigned char* out, int64_t chunk, int q, int fl, const float x[8]) {
  if constexpr (L == kWideFp8) {
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
    *reinterpret_cast<u32x2*>(out + run_offset(L, chunk, q, fl)) = u32x2{(unsigned)lo, (unsigned)hi};
  } else {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)x[j];
    reinterpret_cast<u32x4*>(out)[run_slot(L, chunk, q, fl)] = __builtin_bit_cast(u32x4, v);
  }
}
#endif

}  // namespace tile
}  // namespace dq4ml

#undef DQ_TL_FN
