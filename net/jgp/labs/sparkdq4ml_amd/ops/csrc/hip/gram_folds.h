// Fold-partitioned Gram statistics (see gram_folds.hip): one pass over X yields one flat
// statistics vector per cross-validation fold.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

constexpr int kMaxFolds = 16;

// The fold rule, passed by value in the kernarg.  Granule g (= physical row / G) hashes to a
// uint32 u (splitmix64 of seed + (g + 1) * golden, high word); its fold is the number of
// thresholds thr[0 .. k - 2] that u reaches.
struct FoldRule {
  uint64_t seed;
  int k;
  uint32_t thr[kMaxFolds - 1];
};

__host__ __device__ __forceinline__ uint32_t fold_hash(uint64_t seed, uint64_t g) {
  uint64_t z = seed + (g + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

__host__ __device__ __forceinline__ int fold_of(const FoldRule& fr, uint64_t g) {
  const uint32_t u = fold_hash(fr.seed, g);
  int f = 0;
#pragma unroll
  for (int j = 0; j < kMaxFolds - 1; ++j) f += (j < fr.k - 1 && u >= fr.thr[j]) ? 1 : 0;
  return f;
}

// grid of the one-pass kernel for (d, n, feature dtype): occupancy-sized, >= ~4 granules per wave
int gram_folds_blocks(int d, int64_t n, int xdt);
// One pass, granule = 64 rows: a.partials is [k][blocks][gram_partial_stride(GRAM_F64, d)], out is
// [k][5 + 2d + d(d+1)/2] f64 (each fold's slabs folded by gram_reduce in fixed order).  f32 / f64
// feature-major X with 16-byte aligned feature rows, f32 / f64 label, optional selection, no
// instance weights.
void gram_folds(GramArgs a, const FoldRule& fr, int blocks, double* out, hipStream_t st);
// out[r] = fold of physical row r (granule r / G) for r < n
void fold_ids(int64_t n, int64_t granule, const FoldRule& fr, uint8_t* out, hipStream_t st);

}  // namespace dq4ml
