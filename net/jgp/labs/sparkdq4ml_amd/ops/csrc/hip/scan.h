// Prefix scans on the device: the one home of the wave ladder, the block scan and the row walker
// for the window scans (window.hip), the radix sort (sort.hip), the CSV line ends (csv_scan.hip),
// the block-count scan of scan.hip, the quantile pick (quantile.hip) and the patch ranks
// (gram.hip).  Device code only.
//
// A scan operator S has a trivially copyable S::T of a multiple of 4 bytes, its identity S::id()
// and an associative S::op(earlier, later), which need not commute.
#pragma once
#include "common.h"

namespace dq4ml {

template <class V>
struct Add {
  typedef V T;
  static __device__ __forceinline__ T id() { return 0; }
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
typedef Add<unsigned> AddU32;
typedef Add<long long> AddI64;
typedef Add<unsigned long long> AddU64;

template <class T>
__device__ __forceinline__ T shfl_up_any(T v, int o) {
  static_assert(sizeof(T) % 4 == 0, "shuffled in 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_up(w[k], o, kWave);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// The inclusive scan of v over the lanes of the wave.  Every lane of the wave calls this.
template <class S>
__device__ __forceinline__ typename S::T wave_inclusive(typename S::T v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const typename S::T u = shfl_up_any(v, o);
    if (lane >= o) v = S::op(u, v);
  }
  return v;
}

// The exclusive scan of `agg` over the block's threads in thread order, and the block's total.
// Every thread of the NW-wave block calls this; red: [NW] in LDS.  It syncs before it writes red
// (the last call's readers are done with it), so calls may follow one another with no barrier
// between them.
template <class S, int NW>
__device__ __forceinline__ typename S::T block_exclusive(typename S::T agg, typename S::T& total, typename S::T* red) {
  typedef typename S::T T;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const T inc = wave_inclusive<S>(agg, lane);
  T ex = shfl_up_any(inc, 1);
  if (lane == 0) ex = S::id();
  __syncthreads();
  if (lane == kWave - 1) red[wave] = inc;
  __syncthreads();
  T before = S::id();
  total = S::id();
#pragma unroll(NW <= 8 ? NW : 4)  // (16 int64 totals held at once cost the one-block counts scan two waves per SIMD)
  for (int w = 0; w < NW; ++w) {
    const T x = red[w];
    if (w < wave) before = S::op(before, x);
    total = S::op(total, x);
  }
  return S::op(before, ex);
}

// The row walker: row[0 .. len) becomes carry + its exclusive scan, in place, by the whole NW-wave
// block in trips of kWave * NW * E entries; a thread owns E consecutive ones.  Returns the carry
// with the row's total added.  Where E entries make 16 bytes they move as one vector: the row is
// then 16-byte aligned and padded to a multiple of E entries, and the padding reads as the
// identity whatever it holds.  red: [NW] in LDS.
template <class S, int NW, int E>
__device__ __forceinline__ typename S::T scan_row(typename S::T* row, int64_t len, typename S::T carry, typename S::T* red) {
  typedef typename S::T T;
  constexpr bool kVec = E > 1 && E * sizeof(T) == sizeof(u32x4);
  for (int64_t t0 = 0; t0 < len; t0 += (int64_t)kWave * NW * E) {  // block-uniform
    const int64_t t = t0 + (int64_t)threadIdx.x * E;
    T v[E];
    if (kVec) {
      u32x4 q = {0u, 0u, 0u, 0u};
      if (t < len) q = *reinterpret_cast<const u32x4*>(row + t);
      __builtin_memcpy(v, &q, sizeof(q));
    }
    T agg = S::id();
#pragma unroll
    for (int k = 0; k < E; ++k) {
      if (t + k >= len) v[k] = S::id();
      else if (!kVec) v[k] = row[t + k];
      agg = S::op(agg, v[k]);
    }
    T total;
    T run = S::op(carry, block_exclusive<S, NW>(agg, total, red));
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const T x = v[k];
      v[k] = run;
      run = S::op(run, x);
      if (!kVec && t + k < len) row[t + k] = v[k];
    }
    if (kVec && t < len) {
      u32x4 q;
      __builtin_memcpy(&q, v, sizeof(q));
      *reinterpret_cast<u32x4*>(row + t) = q;
    }
    carry = S::op(carry, total);
  }
  return carry;
}

}  // namespace dq4ml
