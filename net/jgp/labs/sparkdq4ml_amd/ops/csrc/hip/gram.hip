// K5 — WLS sufficient statistics ("Gram") of a feature-major matrix on MFMA.
//
// Replaces Spark's per-row ``WeightedLeastSquares.Aggregator.add`` (BLAS.spr of every row into a
// packed Gram) triggered by LinearRegression.fit at
// DataQuality4MachineLearningApp.java:126.  One streaming pass over
//     X  [d, ld]  feature-major (bf16 / f32 / f64),  y [n],  optional w [n] and selection sel [n]
// produces   count, Σw, Σw², Σwy, Σwy², Σw·x (d), Σw·x·y (d), Σ w·x·xᵀ (upper)   in f64.
//
// Tall-skinny design (d <= 64, memory bound: 1e8 x 32 bf16 = 6.4 GB per pass):
//  * "superstep" = 64 consecutive rows.  Lane l of a wave owns feature f = l & 31 (bf16/f32
//    modes) and the row half h = l >> 5, and loads ITS 32 rows of ITS feature as contiguous
//    16-byte vectors — in feature-major storage that is exactly the A/B fragment of
//    v_mfma_f32_32x32x16_bf16 (A[i=l&31][k=8h+j]) with the K index permuted (allowed: Σ_k is
//    order-free as long as A and B use the same permutation, and they are the same registers).
//    No LDS transpose, no shuffles: 4 loads + 4 MFMAs per 32-feature tile per superstep.
//  * Upper tile pairs only (d <= 32: 1 pair, d <= 64: 3 pairs).
//  * Column sums and Xᵀy ride on a second MFMA with B = [w_hi, w_lo, wy_hi, wy_lo, 0...]: the
//    per-row scalars are computed lane = row (coalesced), split hi/lo into bf16 (≈16-bit
//    mantissa for the label) and handed to the fragment layout through a 512-byte LDS stripe.
//  * f64 mode (Spark-parity path): d <= 8 takes the lane-per-row skinny kernel below, d > 8 the
//    stream kernel (gram_stream.hip: v_mfma_f64_16x16x4_f64 on 16-feature tiles), which also takes
//    the f32 modes and bf16 mode on row-major f32 storage.  This file's MFMA kernels are bf16 only.
//  * Per-wave f32 (bf16 mode) / f64 accumulators -> deterministic in-block wave reduction in
//    LDS -> one f64 partial slab per block (format: gram_slab.h) -> ``gram_reduce`` sums slabs in
//    a fixed order (no atomics: bit-reproducible run to run).
#include <hip/hip_runtime.h>

#include "common.h"
#include "gram.h"
#include "gram_slab.h"
#include "scan.h"
#include "tile_layout.h"

namespace dq4ml {

namespace {

// bf16 kernel: 8 waves per block -- one per CU at <= 256 VGPRs for d <= 64, and for d <= 32
// unmasked (NT 1, XMODE 0) two co-resident per CU at <= 128 VGPRs (since round 5 -- the 16-wave
// block lost), so one block's ramp and reduction overlap the other's stream and the next pass's
// blocks start beside this pass's last ones.  Same box, two reps (profiles/r5_shard_drain.md):
// 1.25e7-row shard 0.1297 / 0.1292 vs 0.1347 / 0.1365 ms per fit, 1e8 headline 0.987 / 0.989 vs
// 0.994 / 0.992 ms.
constexpr int kBf16Block = 512;
template <int NT, int XMODE>
struct BF16Geom {
  static constexpr int kBlock = kBf16Block;
  static constexpr int kWaves = kBlock / kWave;
  static constexpr int kMinBlocks = (NT == 1 && XMODE == 0) ? 2 : 1;
};

// The 12-bit companion of the tiled storage that a bf16 kernel reads (gram.h: pack_tiles /
// patch_tiles; GramArgs::xpack with xdir or with xrec + xovf)
enum class Companion { kRaw, kMixed, kPatched };

__device__ __forceinline__ double load_as_f64(const void* p, int dt, int64_t i) {
  switch (dt) {
    case DT_F64: return reinterpret_cast<const double*>(p)[i];
    case DT_F32: return (double)reinterpret_cast<const float*>(p)[i];
    case DT_BF16: return (double)bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(p)[i]);
    case DT_I32: return (double)reinterpret_cast<const int32_t*>(p)[i];
    case DT_I64: return (double)reinterpret_cast<const int64_t*>(p)[i];
    case DT_U8: return (double)reinterpret_cast<const uint8_t*>(p)[i];
    default: return 0.0;
  }
}

// per-row scalars of row r (lane = row): liveness, weight, label
__device__ __forceinline__ RowVals row_vals(const GramArgs& a, int64_t r) {
  RowVals v{false, 0.0, 0.0, 0.0};
  if (r < a.n) {
    bool live = a.sel ? (a.sel[r] != 0) : true;
    if (live) {
      double w = a.w ? load_as_f64(a.w, a.wdt, r) : 1.0;
      double y = load_as_f64(a.y, a.ydt, r);
      v.live = true;
      v.w = w;
      v.y = y;
      v.wy = w * y;
    }
  }
  return v;
}

// The label of row r as loaded bits (f32 or f64 labels only), converted where it is used: a load
// issued a superstep ahead then waits for nothing where it is issued.  row_vals with the label
// taken from such bits: the same values through the same operations.
struct LabelBits {
  uint32_t lo, hi;
};

__device__ __forceinline__ LabelBits label_bits(const GramArgs& a, int64_t r) {
  LabelBits b{0u, 0u};
  if (r < a.n) {
    if (a.ydt == DT_F64) {
      const u32x2 v = reinterpret_cast<const u32x2*>(a.y)[r];
      b.lo = v[0];
      b.hi = v[1];
    } else {
      b.lo = reinterpret_cast<const uint32_t*>(a.y)[r];
    }
  }
  return b;
}

// (WEIGHTS = false: a.w is null -- no weight load whose wait would also drain the loads in flight)
template <bool WEIGHTS>
__device__ __forceinline__ RowVals row_vals(const GramArgs& a, int64_t r, LabelBits b) {
  RowVals v{false, 0.0, 0.0, 0.0};
  if (r < a.n) {
    bool live = a.sel ? (a.sel[r] != 0) : true;
    if (live) {
      double w = 1.0;
      if constexpr (WEIGHTS) w = a.w ? load_as_f64(a.w, a.wdt, r) : 1.0;
      double y = a.ydt == DT_F64 ? __longlong_as_double(((long long)b.hi << 32) | (long long)b.lo)
                                 : (double)__uint_as_float(b.lo);
      v.live = true;
      v.w = w;
      v.y = y;
      v.wy = w * y;
    }
  }
  return v;
}

// ---- 32 rows of one feature as 4 bf16x8 fragments --------------------------------------------
template <typename T>
__device__ __forceinline__ void load_rows32_bf16(const T* p, int64_t rows_left, bf16x8 (&fr)[4]);

template <>
__device__ __forceinline__ void load_rows32_bf16<uint16_t>(const uint16_t* p, int64_t rows_left, bf16x8 (&fr)[4]) {
  if (rows_left >= 32) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 u = __builtin_nontemporal_load(q + i);
      fr[i] = __builtin_bit_cast(bf16x8, u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = 8 * i + j;
        uint16_t b = e < rows_left ? p[e] : uint16_t(0);
        fr[i][j] = __builtin_bit_cast(__bf16, b);
      }
    }
  }
}

template <>
__device__ __forceinline__ void load_rows32_bf16<double>(const double* p, int64_t rows_left, bf16x8 (&fr)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = 8 * i + j;
      fr[i][j] = (__bf16)(float)(e < rows_left ? p[e] : 0.0);
    }
}

// zero the elements of dead rows (binary mask): bits = liveness of the lane's 32 rows
__device__ __forceinline__ void mask_frags(bf16x8 (&fr)[4], uint32_t bits) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!((bits >> (8 * i + j)) & 1u)) fr[i][j] = (__bf16)0.0f;
}

__device__ __forceinline__ void weight_frags(bf16x8 (&fr)[4], const float* wl /* lane's 32 row weights in LDS */) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) fr[i][j] = (__bf16)((float)fr[i][j] * wl[8 * i + j]);
}

// slab element o (storage order: head, then T x T tiles of the row-major upper pairs I <= J < NT)
// -> its packed-upper destination; lower halves of the diagonal tiles and padding features drop
__device__ __forceinline__ void fold_store(int o, double t, int d, int T, int NT, double* __restrict__ out) {
  const int head = slab_head(d);
  if (o < head) {
    out[o] = t;
    return;
  }
  const int e = o - head, pr = e / (T * T), w = e - pr * T * T, r = w / T, cc = w - (w / T) * T;
  int I = 0, rem = pr;
  while (rem >= NT - I) {
    rem -= NT - I;
    ++I;
  }
  const int J = I + rem;
  const int64_t i = (int64_t)I * T + r, j = (int64_t)J * T + cc;
  if (i <= j && j < d) out[head + i + j * (j + 1) / 2] = t;
}

// ---- 12-bit packed tiles (gram.h: pack_tiles) -------------------------------------------------
// One lane's three 16-byte pieces of a packed entry -> its four raw fragments.  B2 = base << 7 in
// both halfwords; code + B2 <= 0x7FFF per halfword, so the add never reaches a sign bit.
// (NP: the caller's pieces per buffer -- four where an entry may also be raw, three where not)
template <int NP>
__device__ __forceinline__ void unpack_tile(const u32x4 (&raw)[NP], uint32_t B2, bf16x8 (&fr)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t d0 = raw[0][i], d1 = raw[1][i], d2 = raw[2][i];
    uint32_t q = (d0 >> 11) & 0x000F000Fu;
    q |= (d1 >> 7) & 0x00F000F0u;
    q |= (d2 >> 3) & 0x07000700u;
    q |= (d2 & 0x40004000u) << 1;
    u32x4 r;
    r[0] = (d0 & 0x87FF87FFu) + B2;
    r[1] = (d1 & 0x87FF87FFu) + B2;
    r[2] = (d2 & 0x87FF87FFu) + B2;
    r[3] = q + B2;
    fr[i] = __builtin_bit_cast(bf16x8, r);
  }
}

// One exception record of the patched companion (gram.h: patch_tiles) into the decoded fragments:
// the owning lane writes the record's 16 bits over the named halfword of the named dword (a
// select on every dword; the record is wave-uniform, so the comparisons are scalar).
__device__ __forceinline__ void patch_frags(bf16x8 (&fr)[4], uint32_t rec, int lane) {
  const uint32_t dw = (rec >> 17) & 15u;
  const bool hi = ((rec >> 16) & 1u) != 0;
  const uint32_t keep = hi ? 0x0000FFFFu : 0xFFFF0000u;
  const uint32_t val = hi ? rec << 16 : rec & 0xFFFFu;
  const bool mine = (int)(rec >> 21) == lane;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32x4 u = __builtin_bit_cast(u32x4, fr[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = (mine && dw == (uint32_t)(4 * i + j)) ? ((u[j] & keep) | val) : u[j];
    fr[i] = __builtin_bit_cast(bf16x8, u);
  }
}

// =============================================================================================
// bf16 MFMA kernel
// =============================================================================================
// COMP kPatched (tiled storage, XMODE 0, no weights, no selection, f32 label): every full
// superstep is read from the patched companion, the ragged tail from the raw tiles.
template <typename TX, int NT, int XMODE, bool TILED, Companion COMP = Companion::kRaw>
__global__ __launch_bounds__((BF16Geom<NT, XMODE>::kBlock), (BF16Geom<NT, XMODE>::kMinBlocks)) void
gram_tall_bf16_kernel(GramArgs a) {
  constexpr bool PACKED = COMP == Companion::kMixed, PATCHED = COMP == Companion::kPatched;
  static_assert(COMP == Companion::kRaw || TILED, "a packed companion belongs to tiled storage");
  static_assert(!PATCHED || XMODE == 0, "the patched companion: XMODE 0");
  typedef BF16Geom<NT, XMODE> Geo;
  constexpr int NPAIR = NT * (NT + 1) / 2;
  // LDS: per wave 4 cols x 64 rows bf16 (W fragments) + 64 f32 row weights; reused for the
  // block reduction afterwards.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int f = lane & 31, h = lane >> 5;
  __bf16* wl = reinterpret_cast<__bf16*>(smem) + wave * (4 * 64);
  float* wrow = reinterpret_cast<float*>(smem + Geo::kWaves * 4 * 64 * 2) + wave * 64;

  f32x16 acc[NPAIR];
  f32x16 accw[NT];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = f32x16{};
#pragma unroll
  for (int t = 0; t < NT; ++t) accw[t] = f32x16{};
  RowAcc ra;

  const TX* X = reinterpret_cast<const TX*>(a.X);
  const TX* fp[NT];
  bool fvalid[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int feat = t * 32 + f;
    fvalid[t] = feat < a.d;
    fp[t] = X + (int64_t)(fvalid[t] ? feat : 0) * a.ld + 32 * h;
  }

  // (packed: the wave index as a scalar, so the superstep loop and its directory branches are
  // scalar control flow)
  const int64_t gw =
      (int64_t)blockIdx.x * Geo::kWaves + ((PACKED || PATCHED) ? __builtin_amdgcn_readfirstlane(wave) : wave);
  const int64_t total_waves = (int64_t)gridDim.x * Geo::kWaves;
  const bool do_tail = (gw == total_waves - 1) && (a.n > a.nsuper * 64);

  // One superstep of compute on already-loaded feature fragments (rv: the row scalars of row
  // r0 + lane).
  auto compute_rv = [&](const RowVals& rv, bf16x8 (&fr)[NT][4]) {
    // 1) per-row scalars, lane = row
    ra.add(rv);
    stage_w_stripe(wl, lane, rv);
    if (XMODE == 2) wrow[lane] = (float)rv.w;
    const uint64_t live_bits = __ballot(rv.live);
    __builtin_amdgcn_wave_barrier();
    // 2) W fragments (lanes f < 4 read their column; everyone else multiplies zeros)
    bf16x8 wf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wf[i] = bf16x8{};
    if (f < 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(wl + f * 64 + 32 * h + 8 * i);
    }
    // 3) masking / weighting of one operand of XᵀX
    bf16x8 frw[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) frw[t][i] = fr[t][i];
    if (XMODE == 1) {
      const uint32_t bits = (uint32_t)(live_bits >> (32 * h));
#pragma unroll
      for (int t = 0; t < NT; ++t) mask_frags(frw[t], bits);
    } else if (XMODE == 2) {
#pragma unroll
      for (int t = 0; t < NT; ++t) weight_frags(frw[t], wrow + 32 * h);
    }
    // 4) MFMAs
    int p = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J, ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[I][i], frw[J][i], acc[p], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) accw[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t][i], wf[i], accw[t], 0, 0, 0);
    __builtin_amdgcn_wave_barrier();
  };
  auto compute = [&](int64_t r0, bf16x8 (&fr)[NT][4]) { compute_rv(row_vals(a, r0 + lane), fr); };
  auto load = [&](int64_t r0, int64_t rows_left, bf16x8 (&fr)[NT][4]) {
    if constexpr (TILED) {
      // MFMA-fragment-ordered storage: superstep s, tile t, k-step i = 1 KiB contiguous
      const u32x4* q = reinterpret_cast<const u32x4*>(a.X) + ((r0 >> 6) * NT) * 4 * 64 + lane;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) fr[t][i] = __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(q + (t * 4 + i) * 64));
      return;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (fvalid[t]) {
        load_rows32_bf16<TX>(fp[t] + r0, rows_left, fr[t]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) fr[t][i] = bf16x8{};
      }
    }
  };

  // Packed companion: entry (s, t) is either three 1 KiB pieces of its slot (decoded at the top of
  // compute, so the packed form is what sits in flight) or today's four loads from the raw tiles.
  // The directory byte is wave-uniform: pk_dir reads the aligned word around it (a scalar load, so
  // it shares no counter with the tile loads; the directory is allocated in whole words) a whole
  // iteration before pk_load branches on it; the byte is cut out of the word only there
  // (dir_bytes), so the load is not waited for where it is issued.  The label of a superstep is
  // loaded with its tiles (pk_y) and converted in compute: nothing between two computes waits for
  // a load issued after the tiles, so the next superstep's loads stay in flight through all of
  // this one's compute.
  auto pk_dir = [&](int64_t s, uint32_t (&dv)[NT]) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(a.xdir);
#pragma unroll
    for (int t = 0; t < NT; ++t) dv[t] = words[(s * NT + t) >> 2];
  };
  auto dir_bytes = [&](int64_t s, const uint32_t (&dv)[NT], int (&db)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      db[t] = (int)((__builtin_amdgcn_readfirstlane(dv[t]) >> (8 * (int)((s * NT + t) & 3))) & 0xFFu);
  };
  auto pk_y = [&](int64_t s) { return label_bits(a, s * 64 + lane); };
  // ln: the lane's 16-byte offset within a piece (its lane index; 0 for the placeholder below)
  auto pk_load = [&](int64_t s, const int (&db)[NT], u32x4 (&raw)[NT][4], int ln) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // both forms are 1 KiB pieces 1 KiB apart: three of the slot, or four of the raw entry
      const bool pk = db[t] != 0xFF;
      const int64_t e = s * NT + t;
      const u32x4* q = (pk ? reinterpret_cast<const u32x4*>(a.xpack) + e * 3 * 64
                           : reinterpret_cast<const u32x4*>(a.X) + e * 4 * 64) + ln;
#pragma unroll
      for (int k = 0; k < 3; ++k) raw[t][k] = __builtin_nontemporal_load(q + k * 64);
      if (!pk) raw[t][3] = __builtin_nontemporal_load(q + 3 * 64);
    }
  };
  auto pk_compute = [&](int64_t s, const int (&db)[NT], const u32x4 (&raw)[NT][4], LabelBits yb) {
    bf16x8 fr[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (db[t] != 0xFF) {
        unpack_tile(raw[t], (uint32_t)db[t] * 0x00800080u, fr[t]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) fr[t][i] = __builtin_bit_cast(bf16x8, raw[t][i]);
      }
    }
    compute_rv(row_vals<XMODE == 2>(a, s * 64 + lane, yb), fr);
  };

  if constexpr (PACKED) {
    // The raw loop's wave -> superstep map, two supersteps per trip: buffers A and B swap roles
    // instead of being copied.  The loads of the next superstep are issued on every path to a
    // compute, so that the waits in it count exactly those as still in flight (a path without
    // them would make every wait drain them): after a wave's last superstep the "next" is a
    // placeholder, three 16-byte loads from slot 0 (the same word for every lane) and the wave's
    // own label again, which nobody reads.
    const int64_t step = total_waves;
    const int64_t end = a.nsuper;
    int64_t s = gw;
    auto pk_next = [&](int64_t s, const uint32_t (&dv)[NT], int (&db)[NT], u32x4 (&raw)[NT][4], LabelBits& yb) {
      const bool more = s + step < end;
      dir_bytes(s + step, dv, db);
#pragma unroll
      for (int t = 0; t < NT; ++t) db[t] = more ? db[t] : 0;
      pk_load(more ? s + step : 0, db, raw, more ? lane : 0);
      yb = pk_y(more ? s + step : s);
      return more;
    };
    if (s < end) {
      u32x4 A[NT][4], B[NT][4];
      int dA[NT], dB[NT];
      uint32_t dv[NT];
      LabelBits yA, yB;
      pk_dir(s, dv);
      dir_bytes(s, dv, dA);
      pk_load(s, dA, A, lane);
      yA = pk_y(s);
      if (s + step < end) pk_dir(s + step, dv);
      for (;;) {
        bool more = pk_next(s, dv, dB, B, yB);
        if (s + 2 * step < end) pk_dir(s + 2 * step, dv);
        pk_compute(s, dA, A, yA);
        if (!more) break;
        s += step;
        more = pk_next(s, dv, dA, A, yA);
        if (s + 2 * step < end) pk_dir(s + 2 * step, dv);
        pk_compute(s, dB, B, yB);
        if (!more) break;
        s += step;
      }
    }
    if (do_tail) {  // the zero-padded last superstep has a directory entry and a slot like any other
      u32x4 A[NT][4];
      int dA[NT];
      uint32_t dv[NT];
      pk_dir(a.nsuper, dv);
      dir_bytes(a.nsuper, dv, dA);
      pk_load(a.nsuper, dA, A, lane);
      pk_compute(a.nsuper, dA, A, pk_y(a.nsuper));
    }
  } else if constexpr (PATCHED) {
    // The all-packed companion: the packed loop's wave -> superstep map and buffer swap with no
    // conditional vector load in it.  Every superstep issues three 1 KiB pieces per tile and its
    // f32 label (s < nsuper implies row < n: no guard), so the waits in front of a decode count
    // exactly the next superstep's loads as still in flight.  After a wave's last superstep the
    // "next" is the packed loop's placeholder: slot 0 at lane offset 0 and the wave's own label
    // again.  An entry's 16-byte directory record comes by a scalar load issued a whole compute
    // ahead (the scalar counter is not the tile loads'); its exceptions are patched into the
    // decoded fragments under a uniform branch on the count, so the MFMA operands are the raw
    // tile's bits.
    const int64_t step = total_waves;
    const int64_t end = a.nsuper;
    int64_t s = gw;
    const u32x4* recs = reinterpret_cast<const u32x4*>(a.xrec);
    const uint32_t* yp = reinterpret_cast<const uint32_t*>(a.y);
    auto pt_dir = [&](int64_t s, u32x4 (&dr)[NT]) {
#pragma unroll
      for (int t = 0; t < NT; ++t) dr[t] = recs[s * NT + t];
    };
    // (the label first: it is the one loaded register that the loop carries under another name
    // than it is loaded to, and a copy on the back edge then waits for the oldest load in flight,
    // not for the tile pieces behind it)
    auto pt_load = [&](int64_t s, u32x4 (&raw)[NT][3], uint32_t& yb, int ln, int64_t sy) {
      yb = yp[sy * 64 + lane];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const u32x4* q = reinterpret_cast<const u32x4*>(a.xpack) + (s * NT + t) * 3 * 64 + ln;
#pragma unroll
        for (int k = 0; k < 3; ++k) raw[t][k] = __builtin_nontemporal_load(q + k * 64);
      }
    };
    auto pt_next = [&](int64_t s, u32x4 (&raw)[NT][3], uint32_t& yb) {
      const bool more = s + step < end;
      pt_load(more ? s + step : 0, raw, yb, more ? lane : 0, more ? s + step : s);
      return more;
    };
    auto pt_compute = [&](const u32x4 (&dr)[NT], const u32x4 (&raw)[NT][3], uint32_t yb) {
      bf16x8 fr[NT][4];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(dr[t][0]);
        const uint32_t cnt = (w0 >> 8) & 0xFFu;
        unpack_tile(raw[t], (w0 & 0xFFu) * 0x00800080u, fr[t]);
        if (cnt != 0) {
          if (cnt <= (uint32_t)kPatchInline) {
            patch_frags(fr[t], __builtin_amdgcn_readfirstlane(dr[t][1]), lane);
            if (cnt > 1) patch_frags(fr[t], __builtin_amdgcn_readfirstlane(dr[t][2]), lane);
            if (cnt > 2) patch_frags(fr[t], __builtin_amdgcn_readfirstlane(dr[t][3]), lane);
          } else {  // rare (about 2.5e-5 of Gaussian entries): the records sit in the overflow table
            const uint32_t* ov = a.xovf + __builtin_amdgcn_readfirstlane(dr[t][1]);
            for (uint32_t c = 0; c < cnt; ++c) patch_frags(fr[t], __builtin_amdgcn_readfirstlane(ov[c]), lane);
          }
        }
      }
      // row_vals of a live, unweighted row: w = 1, wy = y
      const double y = (double)__uint_as_float(yb);
      compute_rv(RowVals{true, 1.0, y, y}, fr);
    };
    if (s < end) {
      u32x4 A[NT][3], B[NT][3], dA[NT], dB[NT], dv[NT];
      uint32_t yA, yB;
      pt_dir(s, dA);
      pt_load(s, A, yA, lane, s);
#pragma unroll
      for (int t = 0; t < NT; ++t) dv[t] = dA[t];
      if (s + step < end) pt_dir(s + step, dv);
      // Whole pairs of supersteps per trip and ONE exit, at the bottom: a second exit between the
      // two computes gets merged with the back edge, and the loop head then waits for every load.
      // A wave's odd last superstep is loaded in the last trip's second slot and computed after
      // the loop.
      bool left = true;  // A holds a superstep that is not computed yet
      if (s + step < end) {
        for (;;) {
#pragma unroll
          for (int t = 0; t < NT; ++t) dB[t] = dv[t];
          pt_load(s + step, B, yB, lane, s + step);
          if (s + 2 * step < end) pt_dir(s + 2 * step, dv);
          pt_compute(dA, A, yA);
          s += step;
#pragma unroll
          for (int t = 0; t < NT; ++t) dA[t] = dv[t];
          left = pt_next(s, A, yA);
          if (s + 2 * step < end) pt_dir(s + 2 * step, dv);
          pt_compute(dB, B, yB);
          s += step;
          if (s + step >= end) break;
        }
      }
      if (left) pt_compute(dA, A, yA);
    }
  } else
  // full supersteps: register double buffer (loads of the wave's next superstep in flight while
  // this one computes).  Wave gw takes supersteps gw, gw + W, gw + 2W, ... (W = total waves), so
  // the whole grid sweeps the rows in step; same-box A/B against one contiguous range per wave
  // (5 alternations): 1e8 rows 1.011-1.015 vs 1.020-1.026 ms, 1.25e7 rows 0.1426-0.1441 vs
  // 0.1471-0.1476 ms per fit.  The packed and patched loops above keep the same map.
  if (gw < a.nsuper) {
    bf16x8 cur[NT][4], nxt[NT][4];
    load(gw * 64, 64, cur);
    for (int64_t s = gw; s < a.nsuper; s += total_waves) {
      if (s + total_waves < a.nsuper) load((s + total_waves) * 64, 64, nxt);
      compute(s * 64, cur);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[t][i] = nxt[t][i];
    }
  }
  // ragged tail (rows not filling a 64-row superstep): last wave only, guarded loads
  if (!PACKED && do_tail) {
    bf16x8 tl[NT][4];
    const int64_t r0 = a.nsuper * 64;
    load(r0, a.n - (r0 + 32 * h), tl);  // tiled storage is zero padded to a whole superstep
    compute(r0, tl);
  }

  // ---- block reduction: fixed-shape tree over the waves (deterministic), 4 rounds ------------
  // (SlabTree32<NT, W>::reduce_and_store of gram_slab.h, kept in line here: behind the call this
  // kernel's main loops get other registers)
  typedef SlabTree32<NT, Geo::kWaves> Tree;
  constexpr int W = Geo::kWaves;
  constexpr int NV = Tree::NV;
  const int d = a.d;
  double sc[kSlabScalars];
  wave_scalars(ra, sc);
  __syncthreads();  // W stripes are dead from here on: reuse the LDS
  float* tr = reinterpret_cast<float*>(smem);
  double* scl = reinterpret_cast<double*>(smem + Tree::kTreeBytes);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSlabScalars; ++k) scl[wave * kSlabScalars + k] = sc[k];
  }
#pragma unroll
  for (int step = W / 2; step >= 1; step >>= 1) {
    if (wave >= step && wave < 2 * step) {
      float* dst = tr + (size_t)(wave - step) * NV * 64 + lane;
      int v = 0;
#pragma unroll
      for (int p = 0; p < NPAIR; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(v++) * 64] = acc[p][r];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(v++) * 64] = accw[t][r];
    }
    __syncthreads();
    if (wave < step) {
      const float* src = tr + (size_t)wave * NV * 64 + lane;
      int v = 0;
#pragma unroll
      for (int p = 0; p < NPAIR; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] += src[(v++) * 64];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) accw[t][r] += src[(v++) * 64];
    }
    __syncthreads();
  }
  if (wave == 0) {
    double* out = a.partials + (int64_t)blockIdx.x * a.P;
    if (lane < kSlabScalars) {
      double t = 0.0;
      for (int w = 0; w < W; ++w) t += scl[w * kSlabScalars + lane];
      slab_put(out + lane, t);
    }
    const int col = mfma32_col(lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // accw[t]: rows = features t*32 + row, cols 0..3 = [w_hi, w_lo, wy_hi, wy_lo]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = accw[t][r];
        const float vn = __shfl_down(v, 1, 64);  // col+1 (same row)
        const int feat = t * 32 + mfma32_row(lane, r);
        if (feat < d) {
          if (col == 0) slab_put(out + kSlabScalars + feat, (double)v + (double)vn);
          if (col == 2) slab_put(out + kSlabScalars + d + feat, (double)v + (double)vn);
        }
      }
    }
    int p = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J, ++p) {
        double* tile = slab_tile<32>(out, d, p);
#pragma unroll
        for (int r = 0; r < 16; ++r) slab_put(tile + mfma32_row(lane, r) * 32 + col, (double)acc[p][r]);
      }
  }
}

// =============================================================================================
// Fused assemble + Gram over SOURCE COLUMNS (d <= 64): the VectorAssembler output is never
// materialized.  Block-cooperative superstep: 256 threads vector-load 64 rows x 32*NT features
// with 16-B loads (thread (f, q) = rows [8q, 8q+8) of feature f: coalesced 256-B column runs),
// convert to bf16 (dead rows of the selection -> 0) and store them in MFMA-fragment order in LDS
// (that octet IS one lane's fragment of k-step q & 3, half q >> 2); wave w then runs k-step w's
// MFMAs for every tile pair.  Next superstep's global loads are in flight during the MFMAs;
// double-buffered LDS, one barrier per superstep.  Partials use the bf16 kernel's slab layout.
// =============================================================================================
template <int NT, int SDT, int YDT>  // SDT: common source dtype (-1 mixed); YDT: label dtype (F32/F64)
__global__ __launch_bounds__(256, (NT == 1 ? 3 : 2)) void gram_cols_kernel(GramArgs a, const PackSrc* __restrict__ srcs) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  constexpr int FR = NT * 4 * 64 * 16;   // fragment bytes per superstep
  constexpr int BUF = FR + 4 * 64 * 2;   // + W stripe [4 cols][64 rows] bf16
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = lane & 31, h = lane >> 5;
  const int fl = tid >> 3, q = tid & 7;

  f32x16 acc[NPAIR];
  f32x16 accw[NT];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = f32x16{};
#pragma unroll
  for (int t = 0; t < NT; ++t) accw[t] = f32x16{};
  RowAcc ra;

  PackSrc src[NT];
  bool fv[NT];
  float sh[NT];  // the thread's feature shifts (GramArgs::xshift; 0 without one)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int feat = t * 32 + fl;
    fv[t] = feat < a.d;
    src[t] = srcs[fv[t] ? feat : 0];  // padding features load column 0 (branch-free) and stage zeros
    sh[t] = (a.xshift && fv[t]) ? a.xshift[feat] : 0.0f;
  }
  const int64_t nsup = (a.n + 63) / 64, nfull = a.n / 64;
  const int64_t s0 = (int64_t)blockIdx.x * a.spw;
  const int64_t s1 = s0 + a.spw < nsup ? s0 + a.spw : nsup;
  const int64_t e1 = s1 < nfull ? s1 : nfull;  // full supersteps of this block: [s0, e1)

  // Everything a superstep needs is PREFETCHED into registers (features, selection bytes, the
  // label of row tid for the 64 row-scalar threads) with branch-free typed loads, so the only
  // vmcnt waits in the loop are the compiler's counted ones at first use — no scalar load in the
  // loop can drain the prefetch.
  struct Pref {
    float x[NT][8];
    uint64_t m;
    double yv;
    uint32_t live;
  };
  auto gload = [&](int64_t s, Pref& p) {
    const int64_t r0 = s * 64 + 8 * q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if constexpr (SDT >= 0) load8_typed<SDT, true>(src[t].ptr, r0, a.n, p.x[t]);
      else load8_f32(src[t].ptr, src[t].dt, r0, a.n, p.x[t]);
    }
    // branch-free: the host always passes a selection (all ones when there is none) and every
    // wave loads the row scalars (only wave 0 uses them) so the compiler can count the loads
    p.m = *gptr<uint64_t>(a.sel + r0);
    const int64_t r = s * 64 + (tid & 63);
    p.yv = YDT == DT_F64 ? gptr<double>(a.y)[r] : (double)gptr<float>(a.y)[r];
    p.live = gptr<uint8_t>(a.sel)[r];
  };
  auto stage_w = [&](unsigned char* base, const RowVals& rv) {
    stage_w_stripe(reinterpret_cast<__bf16*>(base + FR), tid, rv);
  };
  // x - s of the live rows to bf16 (dead rows and padding features exactly 0); sub = false: x
  // is already shifted and masked (the guarded last superstep)
  auto stage_x = [&](unsigned char* base, float (&x)[NT][8], uint64_t m, bool sub = true) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float s_t = sub ? sh[t] : 0.0f;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)(fv[t] && ((m >> (8 * j)) & 0xff) ? x[t][j] - s_t : 0.0f);
      *reinterpret_cast<u32x4*>(base + (((t * 4 + (q & 3)) * 64 + 32 * (q >> 2) + fl) << 4)) = __builtin_bit_cast(u32x4, v);
    }
  };
  auto stage = [&](int buf, Pref& p) {
    unsigned char* base = smem + buf * BUF;
    stage_x(base, p.x, p.m);
    if (tid < 64) {
      RowVals rv{p.live != 0, 0.0, 0.0, 0.0};
      if (rv.live) {
        rv.w = 1.0;
        rv.y = p.yv;
        rv.wy = p.yv;
      }
      ra.add(rv);
      stage_w(base, rv);
    }
  };
  auto compute = [&](int buf) {
    const unsigned char* base = smem + buf * BUF;
    const int i = wave;  // this wave's k-step
    bf16x8 fr[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) fr[t] = *reinterpret_cast<const bf16x8*>(base + (((t * 4 + i) * 64 + lane) << 4));
    bf16x8 wf = bf16x8{};
    if (f < 4) wf = *reinterpret_cast<const bf16x8*>(base + FR + (f * 64 + 32 * h + 8 * i) * 2);
    int p = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J, ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[I], fr[J], acc[p], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) accw[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t], wf, accw[t], 0, 0, 0);
  };

  Pref pa, pb;
  if (s0 < e1) gload(s0, pa);
  if (s0 + 1 < e1) gload(s0 + 1, pb);
  int64_t s = s0;
  // unrolled by two so the register ring has static names; prefetches past the end re-load the
  // last superstep (unconditional, so the compiler counts vmcnt instead of draining to 0)
  for (; s + 1 < e1; s += 2) {
    stage(0, pa);
    gload(s + 2 < e1 ? s + 2 : e1 - 1, pa);
    __syncthreads();
    compute(0);
    stage(1, pb);
    gload(s + 3 < e1 ? s + 3 : e1 - 1, pb);
    __syncthreads();
    compute(1);
  }
  if (s < e1) {
    stage(0, pa);
    __syncthreads();
    compute(0);
    __syncthreads();
  }
  if (s1 > nfull && s0 <= nfull) {  // ragged last superstep: guarded loads (once in the grid)
    const int64_t st = nfull, r0 = st * 64 + 8 * q;
    float x[NT][8];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (fv[t]) load8_f32(src[t].ptr, src[t].dt, r0, a.n, x[t]);
      else
#pragma unroll
        for (int j = 0; j < 8; ++j) x[t][j] = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (r0 + j < a.n) x[t][j] -= sh[t];  // rows past n stay 0
      mask8(a.sel, r0, a.n, x[t]);
    }
    stage_x(smem + BUF, x, ~0ull, false);
    if (tid < 64) {
      const RowVals rv = row_vals(a, st * 64 + tid);
      ra.add(rv);
      stage_w(smem + BUF, rv);
    }
    __syncthreads();
    compute(1);
  }

  // ---- block reduction over the 4 waves (two tree rounds) + partial slab -----------------------
  double sc[kSlabScalars];
  wave_scalars(ra, sc);
  SlabTree32<NT, 4>::reduce_and_store(acc, accw, sc, smem, a.partials + (int64_t)blockIdx.x * a.P, a.d, lane, wave);
}

// =============================================================================================
// f64 "skinny" kernel, d <= 8 (the lab's own shape: d = 1): lane = row, every statistic a running
// f64 register sum on the VALU.  The MFMA kernel maps 16 features to lanes, so at d = 1 15/16 of
// its lanes idle and each load instruction fetches 4 x 8 B (0.9 TB/s measured); here every lane
// streams its own rows' x / y / w / sel with branch-free selects (dead rows contribute exact
// zeros, their garbage never enters a product), 4 rows in flight per thread.  Slab layout = the
// f64 MFMA kernel's (16 x 16 tile), so the slab fold is shared.
// =============================================================================================
// 4 consecutive elements [r0, r0 + 4) of a typed column as f64, ONE vector load (the caller
// guarantees 16-byte-aligned bases and r0 % 4 == 0; the switch is wave-uniform)
__device__ __forceinline__ void load4_as_f64(const void* p, int dt, int64_t r0, double out[4]) {
  typedef __attribute__((ext_vector_type(4))) int i32x4_t;
  typedef __attribute__((ext_vector_type(2))) long long i64x2_t;
  typedef __attribute__((ext_vector_type(4))) unsigned char u8x4_t;
  typedef __attribute__((ext_vector_type(4))) unsigned short u16x4_t;
  switch (dt) {
    case DT_F64: {
      const f64x2 a = reinterpret_cast<const f64x2*>(p)[r0 / 2], b = reinterpret_cast<const f64x2*>(p)[r0 / 2 + 1];
      out[0] = a[0]; out[1] = a[1]; out[2] = b[0]; out[3] = b[1];
      break;
    }
    case DT_F32: {
      const f32x4 v = reinterpret_cast<const f32x4*>(p)[r0 / 4];
      for (int u = 0; u < 4; ++u) out[u] = (double)v[u];
      break;
    }
    case DT_I32: {
      const i32x4_t v = reinterpret_cast<const i32x4_t*>(p)[r0 / 4];
      for (int u = 0; u < 4; ++u) out[u] = (double)v[u];
      break;
    }
    case DT_I64: {
      const i64x2_t a = reinterpret_cast<const i64x2_t*>(p)[r0 / 2], b = reinterpret_cast<const i64x2_t*>(p)[r0 / 2 + 1];
      out[0] = (double)a[0]; out[1] = (double)a[1]; out[2] = (double)b[0]; out[3] = (double)b[1];
      break;
    }
    case DT_U8: {
      const u8x4_t v = reinterpret_cast<const u8x4_t*>(p)[r0 / 4];
      for (int u = 0; u < 4; ++u) out[u] = (double)v[u];
      break;
    }
    case DT_BF16: {
      const u16x4_t v = reinterpret_cast<const u16x4_t*>(p)[r0 / 4];
      for (int u = 0; u < 4; ++u) out[u] = (double)bf16_bits_to_f32(v[u]);
      break;
    }
    default:
      for (int u = 0; u < 4; ++u) out[u] = 0.0;
  }
}

// VEC (columnar sources only, host-checked 16-byte-aligned pointers): each lane owns 4
// CONSECUTIVE rows and reads each column / the label / weights / selection with one vector load
// (the row-strided form moves 1-8 bytes per lane per load); the partial last quad takes clamped
// scalar loads.
template <typename TX, int D, bool COLS = false, bool VEC = false>
__global__ __launch_bounds__(kBlock) void gram_skinny_f64_kernel(GramArgs a) {
  constexpr int NA = D * (D + 1) / 2;
  constexpr int NV = slab_head(D) + NA;  // the slab head (d == D) + the packed upper products
  constexpr int UNR = 4;
  __shared__ double red[kWavesPerBlock][NV];
  double v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  const TX* X = reinterpret_cast<const TX*>(a.X);
  const int64_t n = a.n;
  const int64_t step = (int64_t)gridDim.x * kBlock * UNR;
  const int64_t first = VEC ? ((int64_t)blockIdx.x * kBlock + threadIdx.x) * UNR
                            : (int64_t)blockIdx.x * kBlock * UNR + threadIdx.x;
  for (int64_t r0 = first; r0 < n; r0 += step) {
    double x[UNR][D], yv[UNR], wv[UNR];
    bool live[UNR];
    if (VEC && r0 + UNR <= n) {
      double t[UNR];
      load4_as_f64(a.y, a.ydt, r0, yv);
      if (a.w) {
        load4_as_f64(a.w, a.wdt, r0, wv);
      } else {
#pragma unroll
        for (int u = 0; u < UNR; ++u) wv[u] = 1.0;
      }
      if (a.sel) {
        load4_as_f64(a.sel, DT_U8, r0, t);
#pragma unroll
        for (int u = 0; u < UNR; ++u) live[u] = t[u] != 0.0;
      } else {
#pragma unroll
        for (int u = 0; u < UNR; ++u) live[u] = true;
      }
#pragma unroll
      for (int f = 0; f < D; ++f) {
        load4_as_f64(a.colp[f], a.coldt[f], r0, t);
#pragma unroll
        for (int u = 0; u < UNR; ++u) x[u][f] = t[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {  // loads of all UNR rows first (clamped, unconditional)
        const int64_t r = VEC ? r0 + u : r0 + (int64_t)u * kBlock;
        const int64_t rc = r < n ? r : n - 1;
        live[u] = r < n && (a.sel == nullptr || a.sel[rc] != 0);
        yv[u] = load_as_f64(a.y, a.ydt, rc);
        wv[u] = a.w ? load_as_f64(a.w, a.wdt, rc) : 1.0;
#pragma unroll
        for (int f = 0; f < D; ++f) {
          if constexpr (COLS) {
            x[u][f] = load_as_f64(a.colp[f], a.coldt[f], rc);  // wave-uniform dtype switch
          } else {
            x[u][f] = (double)X[(int64_t)f * a.ld + rc];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const double w = live[u] ? wv[u] : 0.0;
      const double y = live[u] ? yv[u] : 0.0;
      const double wy = w * y;
      v[0] += live[u] ? 1.0 : 0.0;
      v[1] += w;
      v[2] += w * w;
      v[3] += wy;
      v[4] += wy * y;
      int q = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double xi = live[u] ? x[u][i] : 0.0;
        v[kSlabScalars + i] += w * xi;
        v[kSlabScalars + D + i] += wy * xi;
        const double wxi = w * xi;
#pragma unroll
        for (int j = i; j < D; ++j, ++q) v[slab_head(D) + q] += wxi * (live[u] ? x[u][j] : 0.0);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double t = wave_sum_f64(v[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  double* out = a.partials + (int64_t)blockIdx.x * a.P;
  for (int k = threadIdx.x; k < NV; k += kBlock) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) t += red[w][k];
    int64_t dst;
    if (k < slab_head(D)) {
      dst = k;  // scalars, Σw x (D), Σw x y (D): d == D
    } else {
      int q = k - slab_head(D), i = 0;
      while (q >= D - i) {
        q -= D - i;
        ++i;
      }
      dst = slab_tile_offset<16>(D, 0) + i * 16 + (i + q);  // (i, j = i + q) of the 16 x 16 f64 tile
    }
    out[dst] = t;
  }
}

// =============================================================================================
// slab reduction -> packed-upper flat layout
// =============================================================================================

// Storage-order fold: thread = one slab element (consecutive threads read consecutive doubles of
// every slab: 512-B coalesced runs), 16 slab groups per block with independent loads, fixed-order
// LDS combine (deterministic), then the element's packed-upper destination (lower halves of the
// diagonal tiles and padding features are dropped).  The output-order first version gathered
// each packed entry from 256-B-strided tile rows.
__global__ __launch_bounds__(1024) void gram_fold_kernel(const double* __restrict__ partials, int nslab, int P, int d,
                                                        int T, int NT, double* __restrict__ out) {
  __shared__ double part[16][65];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int o = blockIdx.x * 64 + c;
  double s = 0.0;
  if (o < P) {
    const double* p = partials + o;
    int b = g;
    for (; b + 48 < nslab; b += 64) {
      const double v0 = p[(int64_t)b * P], v1 = p[(int64_t)(b + 16) * P];
      const double v2 = p[(int64_t)(b + 32) * P], v3 = p[(int64_t)(b + 48) * P];
      s += (v0 + v1) + (v2 + v3);
    }
    for (; b < nslab; b += 16) s += p[(int64_t)b * P];
  }
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && o < P) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][c];
    fold_store(o, t, d, T, NT, out);
  }
}

// one block per statistic column: thread t sums rows t, t + 256, ... in order, then a fixed LDS
// tree over the 256 partial sums (deterministic run to run)
__global__ __launch_bounds__(256) void window_fold_kernel(const double* __restrict__ part, int64_t rows, int gw,
                                                          double* __restrict__ flat) {
  __shared__ double red[256];
  const int c = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int64_t r = t; r < rows; r += 256) s += part[r * gw + c];
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) {
    if (c == 0) {
      flat[0] = red[0];
      flat[1] = red[0];
      flat[2] = red[0];
    } else {
      flat[c + 2] = red[0];
    }
  }
}

// feature-major [d, ld] (any dtype) -> MFMA-fragment-ordered bf16 tiles (see gram.h)
template <typename TS>
__global__ __launch_bounds__(256) void tile_bf16_kernel(const TS* __restrict__ X, int64_t ld, int d, int64_t n,
                                                       int NT, int64_t nsup, uint16_t* __restrict__ out,
                                                       const float* __restrict__ shift) {
  // one thread = one 16-byte chunk (8 rows of one feature)
  const int64_t nchunks = nsup * NT * 4 * 64;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(c & 63);
    const int i = (int)((c >> 6) & 3);
    const int64_t st = c >> 8;  // superstep * NT + t
    const int t = (int)(st % NT);
    const int64_t s = st / NT;
    const int f = t * 32 + (lane & 31);
    const int64_t r = s * 64 + 32 * (lane >> 5) + 8 * i;
    const float sh = (shift && f < d) ? shift[f] : 0.0f;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = 0.0f;
      if (f < d && r + j < n) {
        if constexpr (sizeof(TS) == 8) x = (float)((double)X[(int64_t)f * ld + r + j] - (double)sh);
        else x = (float)X[(int64_t)f * ld + r + j] - sh;
      }
      v[j] = (__bf16)x;
    }
    reinterpret_cast<u32x4*>(out)[c] = __builtin_bit_cast(u32x4, v);
  }
}

template <>
__global__ __launch_bounds__(256) void tile_bf16_kernel<uint16_t>(const uint16_t* __restrict__ X, int64_t ld, int d,
                                                                 int64_t n, int NT, int64_t nsup,
                                                                 uint16_t* __restrict__ out,
                                                                 const float* __restrict__ shift) {
  const int64_t nchunks = nsup * NT * 4 * 64;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(c & 63);
    const int i = (int)((c >> 6) & 3);
    const int64_t st = c >> 8;
    const int t = (int)(st % NT);
    const int64_t s = st / NT;
    const int f = t * 32 + (lane & 31);
    const int64_t r = s * 64 + 32 * (lane >> 5) + 8 * i;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (f < d) {
      if (r + 8 <= n && ((ld & 7) == 0)) {
        v = *reinterpret_cast<const u32x4*>(X + (int64_t)f * ld + r);
      } else {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (r + j < n) ? X[(int64_t)f * ld + r + j] : (uint16_t)0;
        v = __builtin_bit_cast(u32x4, e);
      }
      if (shift) {  // bf16 source and a bf16-representable shift: x - s is usually exact
        const float sh = shift[f];
        bf16x8 b = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (r + j < n) ? (__bf16)((float)b[j] - sh) : (__bf16)0.0f;
        v = __builtin_bit_cast(u32x4, b);
      }
    }
    reinterpret_cast<u32x4*>(out)[c] = v;
  }
}

// tiles -> directory + 12-bit slots (gram.h: pack_tiles); one wave per (superstep, tile) entry
__global__ __launch_bounds__(256) void pack_tiles_kernel(const u32x4* __restrict__ tiles, int64_t nent,
                                                        uint8_t* __restrict__ dir, u32x4* __restrict__ slots,
                                                        uint32_t* __restrict__ npacked) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  uint32_t mine = 0;
  for (int64_t e = w0; e < nent; e += nw) {
    u32x4 r[4];
    uint32_t emin = 255u, emax = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r[i] = tiles[(e * 4 + i) * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = (r[i][j] >> 7) & 0xFFu, hi = (r[i][j] >> 23) & 0xFFu;
        emin = min(emin, min(lo, hi));
        emax = max(emax, max(lo, hi));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      emin = min(emin, (uint32_t)__shfl_xor((int)emin, o, 64));
      emax = max(emax, (uint32_t)__shfl_xor((int)emax, o, 64));
    }
    const bool ok = emax - emin <= 15u && emin <= 254u;
    if (lane == 0) dir[e] = ok ? (uint8_t)emin : (uint8_t)0xFF;
    u32x4 D[3] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    if (ok) {
      ++mine;
      const uint32_t B2 = emin * 0x00800080u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t p3 = (r[i][3] & 0x7FFF7FFFu) - B2;  // 11-bit codes: no borrow between halfwords
#pragma unroll
        for (int k = 0; k < 3; ++k) D[k][i] = (r[i][k] & 0x80008000u) | ((r[i][k] & 0x7FFF7FFFu) - B2);
        D[0][i] |= (p3 & 0x000F000Fu) << 11;
        D[1][i] |= (p3 & 0x00F000F0u) << 7;
        D[2][i] |= ((p3 & 0x07000700u) << 3) | ((r[i][3] & 0x80008000u) >> 1);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) slots[(e * 3 + k) * 64 + lane] = D[k];
  }
  if (lane == 0 && mine) atomicAdd(npacked, mine);
}

// tiles -> the patched companion (gram.h: patch_tiles); one wave per entry.  FILL = false counts
// the exceptions (per entry, their total and the largest count); FILL = true writes slots,
// directory records and overflow records.  An entry's records are ranked by lane (a wave scan of
// the lanes' counts), then dword, then halfword: the order is a function of the data alone.
template <bool FILL>
__global__ __launch_bounds__(256) void patch_tiles_kernel(const u32x4* __restrict__ tiles, int64_t nent,
                                                         uint32_t* __restrict__ counts,
                                                         unsigned long long* __restrict__ stat,
                                                         const uint32_t* __restrict__ ovoff, u32x4* __restrict__ slots,
                                                         uint32_t* __restrict__ rec, uint32_t* __restrict__ ovf) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long total = 0;
  uint32_t most = 0;
  for (int64_t e = w0; e < nent; e += nw) {
    u32x4 r[4];
    uint32_t emin = 255u, emax = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r[i] = tiles[(e * 4 + i) * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = (r[i][j] >> 7) & 0xFFu, hi = (r[i][j] >> 23) & 0xFFu;
        emin = min(emin, min(lo, hi));
        emax = max(emax, max(lo, hi));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      emin = min(emin, (uint32_t)__shfl_xor((int)emin, o, 64));
      emax = max(emax, (uint32_t)__shfl_xor((int)emax, o, 64));
    }
    const uint32_t base = emax - emin <= 15u ? emin : emax - 15u;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        c += (((r[i][j] >> 7) & 0xFFu) < base ? 1u : 0u) + (((r[i][j] >> 23) & 0xFFu) < base ? 1u : 0u);
    const uint32_t incl = wave_inclusive<AddU32>(c, lane);  // inclusive scan of the lanes' counts
    const uint32_t tot = (uint32_t)__shfl((int)incl, 63, 64);
    if constexpr (!FILL) {
      if (lane == 0) counts[e] = tot;
      total += tot;
      most = max(most, tot);
    } else {
      const bool inl = tot <= (uint32_t)kPatchInline;
      uint32_t* dst = inl ? rec + e * 4 + 1 : ovf + ovoff[e];
      uint32_t rank = incl - c;
      const uint32_t fill = base << 7;  // code 0 in the window
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const uint32_t bits = (r[i][j] >> (16 * hf)) & 0xFFFFu;
            if (((bits >> 7) & 0xFFu) < base) {
              dst[rank++] = ((uint32_t)lane << 21) | ((uint32_t)(4 * i + j) << 17) | ((uint32_t)hf << 16) | bits;
              r[i][j] = (r[i][j] & (hf ? 0x0000FFFFu : 0xFFFF0000u)) | (fill << (16 * hf));
            }
          }
      if (lane == 0) {
        rec[e * 4] = base | (tot << 8);
        if (!inl) rec[e * 4 + 1] = ovoff[e];
      }
      const uint32_t B2 = base * 0x00800080u;
      u32x4 D[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t p3 = (r[i][3] & 0x7FFF7FFFu) - B2;  // 11-bit codes: no borrow between halfwords
#pragma unroll
        for (int k = 0; k < 3; ++k) D[k][i] = (r[i][k] & 0x80008000u) | ((r[i][k] & 0x7FFF7FFFu) - B2);
        D[0][i] |= (p3 & 0x000F000Fu) << 11;
        D[1][i] |= (p3 & 0x00F000F0u) << 7;
        D[2][i] |= ((p3 & 0x07000700u) << 3) | ((r[i][3] & 0x80008000u) >> 1);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) slots[(e * 3 + k) * 64 + lane] = D[k];
    }
  }
  if constexpr (!FILL) {
    if (lane == 0 && total) {
      atomicAdd(stat, total);
      atomicMax(stat + 1, (unsigned long long)most);
    }
  }
}

// Un-shift of the packed statistics (gram.h: stats_unshift).  Pass 1 rewrites the Σxxᵀ entries
// (reading the shifted column sums and Σw, which it does not write), pass 2 the column sums.
__global__ __launch_bounds__(256) void unshift_aa_kernel(double* __restrict__ flat, const float* __restrict__ shift,
                                                        int d) {
  const double W = flat[1];
  const double* as = flat + 5;
  double* aa = flat + 5 + 2 * (int64_t)d;
  const int64_t tot = (int64_t)d * (d + 1) / 2;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
    // packed upper, column-major: e = i + j (j + 1) / 2, i <= j
    int64_t j = (int64_t)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > e) --j;
    while ((j + 1) * (j + 2) / 2 <= e) ++j;
    const int64_t i = e - j * (j + 1) / 2;
    const double si = (double)shift[i], sj = (double)shift[j];
    aa[e] += si * as[j] + sj * as[i] + si * sj * W;
  }
}

__global__ __launch_bounds__(256) void unshift_head_kernel(double* __restrict__ flat, const float* __restrict__ shift,
                                                          int d) {
  const double W = flat[1], B = flat[3];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < d; j += gridDim.x * blockDim.x) {
    const double s = (double)shift[j];
    flat[5 + d + j] += s * B;
    flat[5 + j] += s * W;
  }
}

}  // namespace

void stats_unshift(double* flat, const float* shift, int d, hipStream_t st) {
  if (d < 1) return;
  const int64_t tot = (int64_t)d * (d + 1) / 2;
  int64_t g = (tot + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(unshift_aa_kernel, dim3(g), dim3(256), 0, st, flat, shift, d);
  hipLaunchKernelGGL(unshift_head_kernel, dim3((d + 255) / 256), dim3(256), 0, st, flat, shift, d);
  DQ_HIP_CHECK(hipGetLastError());
}

int64_t tiled_elems(int d, int64_t n) { return tile::bytes(tile::kTall, d, n) / 2; }

void tile_bf16(const void* X, int xdt, int64_t ld, int d, int64_t n, void* out, hipStream_t st, const float* shift) {
  const int NT = tile::tiles(tile::kTall, d);
  const int64_t nsup = tile::supersteps(n);
  const int64_t nchunks = nsup * NT * 256;
  int64_t g = (nchunks + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  switch (xdt) {
    case DT_BF16: hipLaunchKernelGGL(tile_bf16_kernel<uint16_t>, dim3(g), dim3(256), 0, st, (const uint16_t*)X, ld, d, n, NT, nsup, o, shift); break;
    case DT_F32: hipLaunchKernelGGL(tile_bf16_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)X, ld, d, n, NT, nsup, o, shift); break;
    case DT_F64: hipLaunchKernelGGL(tile_bf16_kernel<double>, dim3(g), dim3(256), 0, st, (const double*)X, ld, d, n, NT, nsup, o, shift); break;
    case DT_I32: hipLaunchKernelGGL(tile_bf16_kernel<int32_t>, dim3(g), dim3(256), 0, st, (const int32_t*)X, ld, d, n, NT, nsup, o, shift); break;
    default: throw std::invalid_argument("tile_bf16: unsupported dtype");
  }
  DQ_HIP_CHECK(hipGetLastError());
}

void pack_tiles(const void* tiles, int d, int64_t n, uint8_t* dir, uint32_t* slots, uint32_t* npacked,
                hipStream_t st) {
  if (d < 1 || d > 64) throw std::invalid_argument("pack_tiles: d must be in [1, 64]");
  const int64_t nent = tile::supersteps(n) * tile::tiles(tile::kTall, d);
  if (nent < 1) return;
  int64_t g = (nent + 3) / 4;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(pack_tiles_kernel, dim3(g), dim3(256), 0, st, reinterpret_cast<const u32x4*>(tiles), nent, dir,
                     reinterpret_cast<u32x4*>(slots), npacked);
  DQ_HIP_CHECK(hipGetLastError());
}

static int patch_grid(int64_t nent) {
  int64_t g = (nent + 3) / 4;
  return (int)(g > 16384 ? 16384 : g);
}

void patch_tiles_count(const void* tiles, int64_t nent, uint32_t* counts, unsigned long long* stat, hipStream_t st) {
  if (nent < 1) return;
  hipLaunchKernelGGL(patch_tiles_kernel<false>, dim3(patch_grid(nent)), dim3(256), 0, st,
                     reinterpret_cast<const u32x4*>(tiles), nent, counts, stat, (const uint32_t*)nullptr,
                     (u32x4*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  DQ_HIP_CHECK(hipGetLastError());
}

void patch_tiles_fill(const void* tiles, int64_t nent, const uint32_t* ovoff, uint32_t* slots, uint32_t* rec,
                      uint32_t* ovf, hipStream_t st) {
  if (nent < 1) return;
  hipLaunchKernelGGL(patch_tiles_kernel<true>, dim3(patch_grid(nent)), dim3(256), 0, st,
                     reinterpret_cast<const u32x4*>(tiles), nent, (uint32_t*)nullptr, (unsigned long long*)nullptr, ovoff,
                     reinterpret_cast<u32x4*>(slots), rec, ovf);
  DQ_HIP_CHECK(hipGetLastError());
}

int64_t gram_partial_stride(int mode, int d) {
  return mode == GRAM_F64 ? slab_stride<16>(d) : slab_stride<32>(d);
}

static size_t bf16_lds(int d) {
  const int W = kBf16Block / kWave;
  const int NT = tile::tiles(tile::kTall, d);
  const size_t stripes = (size_t)W * (4 * 64 * 2 + 64 * 4);
  const size_t tree = NT == 1 ? SlabTree32<1, W>::kBytes : SlabTree32<2, W>::kBytes;
  return tree > stripes ? tree : stripes;
}

// Dispatch table of the bf16 kernel: call F with its instantiation for (xdt, d, xmode, storage,
// companion).  Row-major f32 storage is not here: it rides the stream kernel (gram_stream.hip).
template <typename F>
static void with_kernel(int mode, int xdt, int d, int xmode, bool tiled, Companion comp, F&& f) {
  if (mode != GRAM_BF16) throw std::invalid_argument("gram_tall: no kernel for this mode and feature dtype");
  const int NT = tile::tiles(tile::kTall, d);
  constexpr Companion kRaw = Companion::kRaw, kMixed = Companion::kMixed, kPatched = Companion::kPatched;
#define DQ_BF16_CASE(TX, NTV, TL, CO)                                  \
  if (xmode == 0) return f(gram_tall_bf16_kernel<TX, NTV, 0, TL, CO>); \
  if (xmode == 1) return f(gram_tall_bf16_kernel<TX, NTV, 1, TL, CO>); \
  return f(gram_tall_bf16_kernel<TX, NTV, 2, TL, CO>);
  if (comp != kRaw && !(xdt == DT_BF16 && tiled)) throw std::invalid_argument("gram_tall: packed tiles need tiled bf16 storage");
  if (comp == kPatched) {  // (XMODE 0 only: check_companion)
    if (NT == 1) return f(gram_tall_bf16_kernel<uint16_t, 1, 0, true, kPatched>);
    return f(gram_tall_bf16_kernel<uint16_t, 2, 0, true, kPatched>);
  }
  if (comp == kMixed) { if (NT == 1) { DQ_BF16_CASE(uint16_t, 1, true, kMixed) } else { DQ_BF16_CASE(uint16_t, 2, true, kMixed) } }
  if (xdt == DT_BF16 && tiled) { if (NT == 1) { DQ_BF16_CASE(uint16_t, 1, true, kRaw) } else { DQ_BF16_CASE(uint16_t, 2, true, kRaw) } }
  if (tiled) throw std::invalid_argument("gram_tall: tiled storage must be bf16");
  if (xdt == DT_BF16) { if (NT == 1) { DQ_BF16_CASE(uint16_t, 1, false, kRaw) } else { DQ_BF16_CASE(uint16_t, 2, false, kRaw) } }
  if (xdt == DT_F64) { if (NT == 1) { DQ_BF16_CASE(double, 1, false, kRaw) } else { DQ_BF16_CASE(double, 2, false, kRaw) } }
#undef DQ_BF16_CASE
  throw std::invalid_argument("gram_tall(bf16): unsupported feature dtype");
}

constexpr int kSkinnyMaxD = 8;

template <typename F>
static void with_skinny(int xdt, int d, F&& f) {
#define DQ_SKINNY(TX)                                          \
  switch (d) {                                                 \
    case 1: return f(gram_skinny_f64_kernel<TX, 1>);           \
    case 2: return f(gram_skinny_f64_kernel<TX, 2>);           \
    case 3: return f(gram_skinny_f64_kernel<TX, 3>);           \
    case 4: return f(gram_skinny_f64_kernel<TX, 4>);           \
    case 5: return f(gram_skinny_f64_kernel<TX, 5>);           \
    case 6: return f(gram_skinny_f64_kernel<TX, 6>);           \
    case 7: return f(gram_skinny_f64_kernel<TX, 7>);           \
    default: return f(gram_skinny_f64_kernel<TX, 8>);          \
  }
  if (xdt == DT_F64) { DQ_SKINNY(double) }
  if (xdt == DT_F32) { DQ_SKINNY(float) }
#undef DQ_SKINNY
  throw std::invalid_argument("gram_skinny: unsupported feature dtype");
}

template <bool VEC, typename F>
static void with_skinny_cols_t(int d, F&& f) {
  switch (d) {
    case 1: return f(gram_skinny_f64_kernel<double, 1, true, VEC>);
    case 2: return f(gram_skinny_f64_kernel<double, 2, true, VEC>);
    case 3: return f(gram_skinny_f64_kernel<double, 3, true, VEC>);
    case 4: return f(gram_skinny_f64_kernel<double, 4, true, VEC>);
    case 5: return f(gram_skinny_f64_kernel<double, 5, true, VEC>);
    case 6: return f(gram_skinny_f64_kernel<double, 6, true, VEC>);
    case 7: return f(gram_skinny_f64_kernel<double, 7, true, VEC>);
    default: return f(gram_skinny_f64_kernel<double, 8, true, VEC>);
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename F>
static void with_skinny_cols(const GramArgs& a, F&& f) {
  bool vec = aligned16(a.y) && aligned16(a.w) && aligned16(a.sel);
  for (int i = 0; i < a.cols; ++i) vec = vec && aligned16(a.colp[i]);
  if (vec)
    with_skinny_cols_t<true>(a.d, f);
  else
    with_skinny_cols_t<false>(a.d, f);
}

static bool use_skinny(int mode, int d, int xdt, int tiled) {
  return mode == GRAM_F64 && !tiled && d <= kSkinnyMaxD && (xdt == DT_F64 || xdt == DT_F32);
}

int gram_plan_blocks(int mode, int d, int64_t n, int xdt, int xmode) {
  if (mode == GRAM_F32 || mode == GRAM_F32S ||
      (mode == GRAM_F64 && !use_skinny(mode, d, xdt, 0) && (xdt == DT_F64 || xdt == DT_F32)) ||
      (mode == GRAM_BF16 && xdt == DT_F32))
    return gram_stream_blocks(mode, d, n, xdt);
  int nb = 1;
  if (use_skinny(mode, d, xdt, 0)) {
    // >= 8 iterations of 4 rows per thread, at most one resident wave of blocks
    const int64_t want = (n + (int64_t)kBlock * 4 * 8 - 1) / ((int64_t)kBlock * 4 * 8);
    with_skinny(xdt, d, [&](auto kern) { nb = occupancy_grid(kern, kBlock, 0, want); });
    return nb;
  }
  // the bf16 kernel: at least ~4 supersteps per wave, at most one full residency wave of blocks
  const int64_t nsuper = tile::supersteps(n);
  constexpr int wpb = kBf16Block / kWave;
  with_kernel(mode, xdt, d, xmode, false, Companion::kRaw,
              [&](auto kern) { nb = occupancy_grid(kern, kBf16Block, bf16_lds(d), (nsuper + 4 * wpb - 1) / (4 * wpb)); });
  return nb;
}

void gram_window_fold(const double* part, int64_t rows, int gw, double* flat, hipStream_t st) {
  if (gw < 1 || rows < 0) throw std::invalid_argument("gram_window_fold: bad shape");
  hipLaunchKernelGGL(window_fold_kernel, dim3(gw), dim3(256), 0, st, part, rows, gw, flat);
  DQ_HIP_CHECK(hipGetLastError());
}

void gram_reduce(int mode, const double* partials, int blocks, int d, double* out, hipStream_t st) {
  const int T = mode == GRAM_F64 ? 16 : 32;
  const int NT = (d + T - 1) / T;
  const int P = (int)gram_partial_stride(mode, d);
  // output-order gather (first version): 4.4 / 7.9 us at d = 32 / 64; storage order: 3.8 / 3.9 us
  hipLaunchKernelGGL(gram_fold_kernel, dim3((P + 63) / 64), dim3(1024), 0, st, partials, blocks, P, d, T, NT, out);
  DQ_HIP_CHECK(hipGetLastError());
}

// The companion that the pointers of ``a`` name, after checking that the launch can read it.
static Companion check_companion(int mode, const GramArgs& a, int xmode) {
  auto bad = [](const char* what) { throw std::invalid_argument(std::string("gram_tall: ") + what); };
  if (!a.xpack && !a.xdir && !a.xrec) return Companion::kRaw;
  if (!a.xpack) bad("a companion directory without its slot buffer");
  if (!a.xdir && !a.xrec) bad("companion slots without a directory");
  if (a.xdir && a.xrec) bad("companion slots with two directories (mixed and patched)");
  if (!(a.tiled && mode == GRAM_BF16)) bad("packed tiles belong to tiled bf16 storage");
  if (!aligned16(a.xpack)) bad("packed tiles need 16-byte aligned slots");
  if (a.xrec) {
    if (xmode != 0 || a.w || a.sel) bad("patched tiles take unweighted, unselected rows (xmode 0)");
    if (a.ydt != DT_F32) bad("patched tiles need an f32 label");
    if (a.xdt != DT_BF16) bad("patched tiles belong to bf16 storage");
    if (a.d % 32 != 0) bad("patched tiles need d a multiple of 32");
    if (a.nsuper < 1) bad("patched tiles need at least one full superstep");
    if (!a.xovf) bad("patched tiles need an overflow table (any valid pointer when it is empty)");
    if (!aligned16(a.xrec)) bad("patched tiles need 16-byte aligned directory records");
    return Companion::kPatched;
  }
  if (a.w && xmode != 2) bad("packed tiles with weights need xmode 2");
  if (a.ydt != DT_F32 && a.ydt != DT_F64) bad("packed tiles need an f32 / f64 label");
  if (reinterpret_cast<uintptr_t>(a.xdir) & 3) bad("packed tiles need a word-aligned directory");
  return Companion::kMixed;
}

void gram_tall(int mode, GramArgs a, int xmode, int blocks, double* out, hipStream_t st, bool reduce) {
  if (a.d < 1 || a.d > 64) throw std::invalid_argument("gram_tall: d must be in [1, 64]");
  if (blocks < 1) throw std::invalid_argument("gram_tall: blocks must be >= 1");
  a.nsuper = a.n / 64;  // (the bf16 kernel's wave -> superstep map needs no spw)
  a.P = (int)gram_partial_stride(mode, a.d);
  if (a.tiled && mode != GRAM_BF16) throw std::invalid_argument("gram_tall: tiled storage needs bf16 mode");
  const Companion comp = check_companion(mode, a, xmode);
  if (a.xshift) {
    // only the f32 stream kernels subtract a shift (tiled storage is shifted when it is tiled)
    if (!((mode == GRAM_F32 || mode == GRAM_BF16 || mode == GRAM_F32S) && a.xdt == DT_F32 && !a.tiled && a.cols == 0 &&
          gram_stream_ok(mode, a)))
      throw std::invalid_argument("gram_tall: a feature shift needs 16-byte aligned f32 features (stream kernel)");
    gram_stream(mode, a, 1, blocks, out, st, reduce);  // XM = 1: dead / padding rows weigh 0, not -s
    return;
  }
  if (a.cols > 0) {
    if (mode != GRAM_F64 || a.cols != a.d || a.d > kSkinnyMaxD || a.tiled)
      throw std::invalid_argument("gram_tall: columnar sources need f64 mode and d <= 8");
    with_skinny_cols(a, [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), 0, st, a); });
  } else if (use_skinny(mode, a.d, a.xdt, a.tiled)) {
    with_skinny(a.xdt, a.d, [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), 0, st, a); });
  } else if ((mode == GRAM_F32 || mode == GRAM_F32S || mode == GRAM_F64 || (mode == GRAM_BF16 && a.xdt == DT_F32)) &&
             gram_stream_ok(mode, a)) {
    gram_stream(mode, a, xmode, blocks, out, st, reduce);
    return;
  } else if (mode == GRAM_F32 || mode == GRAM_F32S) {
    throw std::invalid_argument("gram_tall(f32): needs 16-byte aligned f32 features and f32/f64 labels");
  } else if (mode == GRAM_F64) {  // (past the skinny kernel the stream kernel is this mode's only one)
    throw std::invalid_argument("gram_tall(f64): needs 16-byte aligned f32/f64 features and f32/f64 labels");
  } else if (mode == GRAM_BF16 && a.xdt == DT_F32) {
    throw std::invalid_argument("gram_tall(bf16): f32 storage needs 16-byte aligned features and f32/f64 labels");
  } else {
    with_kernel(mode, a.xdt, a.d, xmode, a.tiled != 0, comp,
                [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBf16Block), bf16_lds(a.d), st, a); });
  }
  DQ_HIP_CHECK(hipGetLastError());
  if (reduce) gram_reduce(mode, a.partials, blocks, a.d, out, st);
}

static size_t cols_lds(int NT) {
  const size_t bufs = 2 * ((size_t)NT * 4 * 64 * 16 + 4 * 64 * 2);
  const size_t tree = NT == 1 ? SlabTree32<1, 4>::kBytes : SlabTree32<2, 4>::kBytes;
  return bufs > tree ? bufs : tree;
}

template <typename F>
static void with_cols_kernel(int NT, int sdt, int ydt, F&& f) {
#define DQ_COLS(NTV, YT)                                                 \
  switch (sdt) {                                                         \
    case DT_F32: return f(gram_cols_kernel<NTV, DT_F32, YT>);            \
    case DT_F64: return f(gram_cols_kernel<NTV, DT_F64, YT>);            \
    case DT_BF16: return f(gram_cols_kernel<NTV, DT_BF16, YT>);          \
    default: return f(gram_cols_kernel<NTV, -1, YT>);                    \
  }
  if (ydt == DT_F64) {
    if (NT == 1) { DQ_COLS(1, DT_F64) } else { DQ_COLS(2, DT_F64) }
  }
  if (NT == 1) { DQ_COLS(1, DT_F32) } else { DQ_COLS(2, DT_F32) }
#undef DQ_COLS
}

int gram_cols_blocks(int d, int64_t n) {
  const int NT = tile::tiles(tile::kTall, d);
  int nb = 1;
  const int64_t nsup = tile::supersteps(n);
  // >= 4 supersteps per block
  with_cols_kernel(NT, DT_F32, DT_F64, [&](auto k) { nb = occupancy_grid(k, 256, cols_lds(NT), (nsup + 3) / 4); });
  return nb;
}

void gram_cols(GramArgs a, const PackSrc* srcs_dev, int sdt, int blocks, double* out, hipStream_t st) {
  if (a.sel == nullptr) throw std::invalid_argument("gram_cols: pass an all-ones selection when there is none");
  if (a.d < 1 || a.d > 64) throw std::invalid_argument("gram_cols: d must be in [1, 64]");
  if (a.w != nullptr) throw std::invalid_argument("gram_cols: instance weights need the materialized path");
  if (blocks < 1) throw std::invalid_argument("gram_cols: blocks must be >= 1");
  const int64_t nsup = tile::supersteps(a.n);
  a.spw = (nsup + blocks - 1) / blocks;
  if (a.spw < 1) a.spw = 1;
  a.nsuper = nsup;
  a.P = (int)gram_partial_stride(GRAM_BF16, a.d);
  const int NT = tile::tiles(tile::kTall, a.d);
  const size_t lds = cols_lds(NT);
  if (a.ydt != DT_F64 && a.ydt != DT_F32) throw std::invalid_argument("gram_cols: label must be f32 or f64");
  with_cols_kernel(NT, sdt, a.ydt,
                   [&](auto k) { hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, st, a, srcs_dev); });
  DQ_HIP_CHECK(hipGetLastError());
  gram_reduce(GRAM_BF16, a.partials, blocks, a.d, out, st);
}

}  // namespace dq4ml
