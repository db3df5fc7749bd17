// The f64 "partial slab" that every tall Gram kernel (d <= 64) writes once per block, and what
// the kernels share on the way to it.  gram_fold_kernel (gram.hip) folds the slabs of a launch into
// the flat statistics in a fixed order (no atomics: bit-reproducible run to run).
//
//   [count, Σw, Σw², Σwy, Σwy² | Σw·x (d) | Σw·x·y (d) | T x T tiles of the upper tile pairs I <= J]
//
// T = 16 for the f64 MFMA kernels (v_mfma_f64_16x16x4_f64) and 32 for the f32-accumulator kernels
// (v_mfma_f32_32x32x*); the pairs are stored row-major over I <= J < NT = ceil(d / T), each tile
// row-major, lower halves of the diagonal tiles and padding features included (the fold drops them).
// Writers: gram_tall_bf16_kernel, gram_cols_kernel, gram_skinny_f64_kernel (gram.hip),
// gram_folds_f64_kernel (gram_folds.hip), glm_irls_f64_kernel (glm_irls.hip) and the stream
// kernels' two bodies (gram_stream.hip).  Reader: fold_store (gram.hip).
//
// What is NOT here: the serial f64 reduction over the waves (zero an LDS slab, waves 0..NW-1 add
// in order between barriers, copy out) stays written out in its four kernels (the folds and GLM
// kernels and the stream kernels' two bodies), and the tall bf16 kernel keeps
// SlabTree32::reduce_and_store in line.  A call, even force-inlined around the verbatim text, lets
// the compiler order its passes differently, and those kernels' main loops then get other VGPR /
// AGPR / spill counts.  They still take every offset from the functions below.
#pragma once
#ifndef __HIPCC_RTC__  // (ops/streamfuse.py compiles the device part below with hipRTC too)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"
#include "gram.h"
#endif

namespace dq4ml {

// ---- 1. the format ---------------------------------------------------------------------------
constexpr int kSlabScalars = 5;  // count, Σw, Σw², Σwy, Σwy²
// elements in front of the tiles: the scalars, Σw·x (d) at kSlabScalars, Σw·x·y (d) behind it
constexpr int slab_head(int d) { return kSlabScalars + 2 * d; }
// first element of tile pair p (row-major over I <= J)
template <int T>
constexpr int slab_tile_offset(int d, int p) {
  return slab_head(d) + p * T * T;
}
// tile pair p of the slab at `slab`
template <int T>
__device__ __forceinline__ double* slab_tile(double* slab, int d, int p) {
  return slab + kSlabScalars + 2 * d + p * (T * T);
}
// doubles per slab
template <int T>
constexpr int64_t slab_stride(int d) {
  const int NT = (d + T - 1) / T;
  return slab_tile_offset<T>(d, NT * (NT + 1) / 2);
}

// Slab stores: the slabs are folded by gram_fold_kernel after the kernel boundary (an in-kernel
// fold by the last block of each XCD group was measured slower at the 8-GPU shard: 155 us vs
// 142-148 us per fit, profiles/r3_fixed_cost.md; removed in round 4).  Relaxed agent-scope
// stores write through to memory (nothing is left dirty in this XCD's L2 for the fold kernel's
// boundary to flush) -- the form the round-3 headline was measured with.
__device__ __forceinline__ void slab_put(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 2. row scalars --------------------------------------------------------------------------
// per-row scalars of a row (lane = row): liveness, weight, label
struct RowVals {
  bool live;
  double w, y, wy;
};

struct RowAcc {
  double cnt = 0, ws = 0, wws = 0, bs = 0, bbs = 0;
  __device__ __forceinline__ void add(const RowVals& v) {
    if (v.live) {
      cnt += 1.0;
      ws += v.w;
      wws += v.w * v.w;
      bs += v.wy;
      bbs += v.wy * v.y;
    }
  }
};

// per-lane RowAcc -> the slab's scalars as wave sums
__device__ __forceinline__ void wave_scalars(const RowAcc& ra, double (&sc)[kSlabScalars]) {
  sc[0] = ra.cnt, sc[1] = ra.ws, sc[2] = ra.wws, sc[3] = ra.bs, sc[4] = ra.bbs;
#pragma unroll
  for (int k = 0; k < kSlabScalars; ++k) sc[k] = wave_sum_f64(sc[k]);
}

// ---- 3. the bf16 W stripe --------------------------------------------------------------------
// Column sums and Xᵀy ride on a second MFMA with B = [w_hi, w_lo, wy_hi, wy_lo, 0...]: the row's
// scalars split hi/lo into bf16 (≈16-bit mantissa for the label), four 64-row bf16 columns at wl.
__device__ __forceinline__ void stage_w_stripe(__bf16* wl, int row, const RowVals& rv) {
  const float w_hi = (float)(__bf16)(float)rv.w;
  const __bf16 wy_hi = (__bf16)(float)rv.wy;
  wl[0 * 64 + row] = (__bf16)(float)rv.w;
  wl[1 * 64 + row] = (__bf16)(float)(rv.w - (double)w_hi);
  wl[2 * 64 + row] = wy_hi;
  wl[3 * 64 + row] = (__bf16)(float)(rv.wy - (double)(float)wy_hi);
}

// ---- 4. f32 MFMA accumulators: tree over the waves + slab store ------------------------------
// Per-wave f32x16 accumulators of NT 32-feature tiles (acc: the upper pairs; accw: rows =
// features t*32 + row, cols 0..3 = the W stripe's [w_hi, w_lo, wy_hi, wy_lo]) of a W-wave block.
// A fixed-shape tree over the waves through LDS (deterministic; rounds step = W/2 ... 1: waves
// [step, 2 step) store, waves [0, step) add), then wave 0 stores the slab in f64.
template <int NT, int W>
struct SlabTree32 {
  static constexpr int NPAIR = NT * (NT + 1) / 2;
  static constexpr int NV = (NPAIR + NT) * 16;  // f32 accumulator values per lane
  static constexpr size_t kTreeBytes = (size_t)(W / 2) * NV * 64 * sizeof(float);
  static constexpr size_t kBytes = kTreeBytes + (size_t)W * kSlabScalars * sizeof(double);  // LDS at smem

  // sc: the wave's scalars (wave_scalars); smem: the block's LDS, dead from here on and reused
  static __device__ __forceinline__ void reduce_and_store(f32x16 (&acc)[NPAIR], f32x16 (&accw)[NT],
                                                          const double (&sc)[kSlabScalars], unsigned char* smem,
                                                          double* out, int d, int lane, int wave) {
    __syncthreads();  // the loop's LDS is dead from here on: reuse it
    float* tr = reinterpret_cast<float*>(smem);
    double* scl = reinterpret_cast<double*>(smem + kTreeBytes);
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
      if (lane < kSlabScalars) {
        double t = scl[lane];  // waves in order
#pragma unroll
        for (int w = 1; w < W; ++w) t += scl[w * kSlabScalars + lane];
        slab_put(out + lane, t);
      }
      const int col = mfma32_col(lane);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = accw[t][r];
          const float vn = __shfl_down(v, 1, 64);  // col+1 (same row): hi + lo
          const int feat = t * 32 + mfma32_row(lane, r);
          if (feat < d) {
            if (col == 0) slab_put(out + kSlabScalars + feat, (double)v + (double)vn);
            if (col == 2) slab_put(out + kSlabScalars + d + feat, (double)v + (double)vn);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
        double* tile = slab_tile<32>(out, d, p);
#pragma unroll
        for (int r = 0; r < 16; ++r) slab_put(tile + mfma32_row(lane, r) * 32 + col, (double)acc[p][r]);
      }
    }
  }
};

// ---- 5. the staged f64 passes (gram_folds_f64_kernel, glm_irls_f64_kernel): staging + launch plan
// A wave keeps one contiguous range of 64-row supersteps and stages every 16-feature tile of a
// superstep in LDS before the f64 MFMAs.  (The plain f64 statistics took this loop too, in
// gram_tall_f64_kernel, until the stream kernel served every call; the constants keep its name.)
constexpr int kBlock = 256;  // 4 waves
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kStageLd = 66;  // f64 staging row stride (doubles): 2-double pad spreads the banks
// LDS of the loop: per wave 128 row scalars + one staged 16-feature x 64-row tile
constexpr size_t kTallF64LoopBytes = kWavesPerBlock * (128 + 16 * kStageLd) * sizeof(double);

#ifndef __HIPCC_RTC__
// dynamic LDS of a block: the loop's bytes (+ `extra` that the kernel keeps beside them), reused
// for the block reduction's slab
inline size_t staged_f64_lds(int d, size_t extra = 0) {
  const size_t loop = kTallF64LoopBytes + extra, red = (size_t)slab_stride<16>(d) * sizeof(double);
  return red > loop ? red : loop;
}

// grid: a full residency wave of `kern` at that LDS, at least ~4 supersteps per wave
template <typename K>
inline int staged_f64_blocks(K kern, size_t lds, int64_t n) {
  const int64_t nsuper = (n + 63) / 64;
  return occupancy_grid(kern, kBlock, lds, (nsuper + 4 * kWavesPerBlock - 1) / (4 * kWavesPerBlock));
}

// The refusals that the passes share (`who` heads the message), then the fields the kernels plan
// by: nsuper = ceil(n / 64) (the ragged superstep included), spw = supersteps per wave, P.
inline void staged_f64_plan(GramArgs& a, int blocks, const char* who) {
  auto bad = [who](const char* what) { throw std::invalid_argument(std::string(who) + ": " + what); };
  if (a.d < 1 || a.d > 64) bad("d must be in [1, 64]");
  if (blocks < 1) bad("blocks must be >= 1");
  if (a.n < 1) bad("n must be >= 1");
  if (a.ydt != DT_F64 && a.ydt != DT_F32) bad("label must be f32 or f64");
  const int64_t esz = a.xdt == DT_F64 ? 8 : 4;
  if ((reinterpret_cast<uintptr_t>(a.X) & 15) || (a.d > 1 && (a.ld * esz) % 16) || a.ld < a.n)
    bad("feature rows must be 16-byte aligned and ld >= n");
  a.nsuper = (a.n + 63) / 64;
  const int64_t total_waves = (int64_t)blocks * kWavesPerBlock;
  a.spw = (a.nsuper + total_waves - 1) / total_waves;
  if (a.spw < 1) a.spw = 1;
  a.P = (int)slab_stride<16>(a.d);
}
#endif

// Cooperative load of features [f0, f0 + 16) x rows [r0, r0 + 64) of a feature-major matrix into a
// per-wave LDS tile xs[f][row] (f64), zeros for features >= d.  Chunk c = i * 64 + lane.
template <typename TX>
__device__ __forceinline__ void stage_tile(const TX* __restrict__ X, int64_t ld, int d, int f0, int64_t r0, int lane,
                                           double* xs) {
  constexpr int kPer = 16 / sizeof(TX);     // elements per 16-byte chunk
  constexpr int kChunksPerRow = 64 / kPer;  // chunks per feature row segment
  constexpr int kIters = 16 * kChunksPerRow / 64;
  typedef __attribute__((ext_vector_type(kPer))) TX vec;
  vec v[kIters];
#pragma unroll
  for (int i = 0; i < kIters; ++i) {  // all loads in flight first
    const int c = i * 64 + lane;
    const int fl = c / kChunksPerRow, k = c % kChunksPerRow;
    const int feat = f0 + fl;
    const TX* src = X + (int64_t)(feat < d ? feat : 0) * ld + r0 + k * kPer;
    v[i] = feat < d ? __builtin_nontemporal_load(reinterpret_cast<const vec*>(src)) : vec{};
  }
#pragma unroll
  for (int i = 0; i < kIters; ++i) {
    const int c = i * 64 + lane;
    const int fl = c / kChunksPerRow, k = c % kChunksPerRow;
    double* dst = xs + fl * kStageLd + k * kPer;
#pragma unroll
    for (int j = 0; j < kPer; j += 2) *reinterpret_cast<f64x2*>(dst + j) = f64x2{(double)v[i][j], (double)v[i][j + 1]};
  }
}

// The lane's 16 rows [r0 + 16 q, +16) of its feature f of every tile (lane = 16 q + f) as f64.
// full: the wave loads each tile cooperatively — lane-contiguous 16-byte chunks, 512 B (f64) /
// 256 B (f32) runs per feature — and stages it in LDS (xs), then every lane reads its 16 rows of
// its feature back (8 x ds_read_b128).  The per-lane strided scalar loads of the first version
// touched 64 cache lines per instruction (~3 TB/s at d = 16..32).  Else (the ragged superstep):
// guarded loads through the lane's own pointers fp[t] (feature t*16 + f at row 16 q; fvalid[t]:
// that feature exists), zeros from row n on (rows_left = n - (r0 + 16 q)).
template <typename TX, int NT>
__device__ __forceinline__ void load_superstep_f64(const TX* X, int64_t ld, int d, bool full, int64_t r0,
                                                   int64_t rows_left, const TX* const (&fp)[NT],
                                                   const bool (&fvalid)[NT], int lane, double* xs,
                                                   double (&x)[NT][16]) {
  const int f = lane & 15, q = lane >> 4;
  if (full) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      stage_tile<TX>(X, ld, d, t * 16, r0, lane, xs);
      __builtin_amdgcn_wave_barrier();
      const f64x2* src = reinterpret_cast<const f64x2*>(xs + f * kStageLd + 16 * q);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f64x2 v = src[i];
        x[t][2 * i] = v[0];
        x[t][2 * i + 1] = v[1];
      }
      __builtin_amdgcn_wave_barrier();
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        double v = 0.0;
        if (fvalid[t] && e < rows_left) v = (double)fp[t][r0 + e];
        x[t][e] = v;
      }
    }
  }
}

}  // namespace dq4ml
