// Order-preserving 64-bit keys of typed column values: the one home of the key rule for the
// relational kernels (groupby.hip, join.hip, sort.hip, quantile.hip).  The key column and its
// per-thread reader (KeyCol, KeyRun / load_keys, store_run), the typed raw loaders, the 0/1
// byte-mask loader, order_key and its inverse.  ops/keys.py is the numpy statement of the rule.
#pragma once
#include "common.h"

namespace dq4ml {

typedef __attribute__((ext_vector_type(2))) long long i64x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef unsigned long long u64;

constexpr u64 kSign = 0x8000000000000000ull;
constexpr u64 kNaNBits = 0x7ff8000000000000ull;
constexpr u64 kInfBits = 0x7ff0000000000000ull;
constexpr int kRawRun = 4;  // consecutive rows of one run load

// one key column: valid / sel are 0/1 bytes per row, or null
struct KeyCol {
  const void* col;
  const uint8_t* valid;
  const uint8_t* sel;
  int64_t n;
  int dt;
};

__device__ __forceinline__ bool is_float_dt(int dt) { return dt == DT_F64 || dt == DT_F32; }

__host__ __device__ constexpr bool is_key_dt(int dt) {
  return dt == DT_F64 || dt == DT_F32 || dt == DT_I32 || dt == DT_I64 || dt == DT_U8;
}

// row r of a typed column widened to 64 bits (floats: the bits of the value as a double; integers
// and booleans: the value as an i64)
template <int DT>
__device__ __forceinline__ u64 load_raw(const void* p, int64_t r) {
  if constexpr (DT == DT_F64) return (u64)__double_as_longlong(gptr<double>(p)[r]);
  else if constexpr (DT == DT_I64) return (u64)gptr<long long>(p)[r];
  else if constexpr (DT == DT_F32) return (u64)__double_as_longlong((double)gptr<float>(p)[r]);
  else if constexpr (DT == DT_I32) return (u64)(long long)gptr<int>(p)[r];
  else return gptr<uint8_t>(p)[r] != 0 ? 1ull : 0ull;
}

// (the switch is block-uniform)
__device__ __forceinline__ u64 load_raw(const void* p, int dt, int64_t r) {
  switch (dt) {
    case DT_F64: return load_raw<DT_F64>(p, r);
    case DT_F32: return load_raw<DT_F32>(p, r);
    case DT_I32: return load_raw<DT_I32>(p, r);
    case DT_I64: return load_raw<DT_I64>(p, r);
    default: return load_raw<DT_U8>(p, r);
  }
}

// kRawRun consecutive rows [r0, r0 + 4) of a typed column widened to 64 bits (0 past n).  16-byte
// loads when the run is complete and aligned (r0 is a multiple of 4), else a guarded scalar tail.
template <int DT>
__device__ __forceinline__ void load_run_raw(const void* p, int64_t r0, int64_t n, u64 x[kRawRun]) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  if (aligned && r0 + kRawRun <= n) {
    if constexpr (DT == DT_F64) {
      const f64x2 a = *gptr<f64x2>(reinterpret_cast<const double*>(p) + r0);
      const f64x2 b = *gptr<f64x2>(reinterpret_cast<const double*>(p) + r0 + 2);
      x[0] = (u64)__double_as_longlong(a[0]), x[1] = (u64)__double_as_longlong(a[1]);
      x[2] = (u64)__double_as_longlong(b[0]), x[3] = (u64)__double_as_longlong(b[1]);
    } else if constexpr (DT == DT_I64) {
      const i64x2 a = *gptr<i64x2>(reinterpret_cast<const long long*>(p) + r0);
      const i64x2 b = *gptr<i64x2>(reinterpret_cast<const long long*>(p) + r0 + 2);
      x[0] = (u64)a[0], x[1] = (u64)a[1], x[2] = (u64)b[0], x[3] = (u64)b[1];
    } else if constexpr (DT == DT_F32) {
      const f32x4 a = *gptr<f32x4>(reinterpret_cast<const float*>(p) + r0);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = (u64)__double_as_longlong((double)a[j]);
    } else if constexpr (DT == DT_I32) {
      const i32x4 a = *gptr<i32x4>(reinterpret_cast<const int*>(p) + r0);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = (u64)(long long)a[j];
    } else {
      const uint32_t w = *gptr<uint32_t>(reinterpret_cast<const uint8_t*>(p) + r0);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = ((w >> (8 * j)) & 0xffu) ? 1ull : 0ull;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kRawRun; ++j) {
    const int64_t r = r0 + j;
    x[j] = r < n ? load_raw<DT>(p, r) : 0ull;
  }
}

// (the switch is block-uniform)
__device__ __forceinline__ void load_run(const void* p, int dt, int64_t r0, int64_t n, u64 x[kRawRun]) {
  switch (dt) {
    case DT_F64: load_run_raw<DT_F64>(p, r0, n, x); break;
    case DT_F32: load_run_raw<DT_F32>(p, r0, n, x); break;
    case DT_I32: load_run_raw<DT_I32>(p, r0, n, x); break;
    case DT_I64: load_run_raw<DT_I64>(p, r0, n, x); break;
    default: load_run_raw<DT_U8>(p, r0, n, x); break;
  }
}

// bit j: row r0 + j is inside n and its 0/1 byte is set (null mask: every row inside n)
__device__ __forceinline__ unsigned mask_run(const uint8_t* m, int64_t r0, int64_t n) {
  unsigned out = 0;
  if (m != nullptr && r0 + kRawRun <= n && ((reinterpret_cast<uintptr_t>(m + r0) & 3) == 0)) {
    const uint32_t w = *gptr<uint32_t>(m + r0);
#pragma unroll
    for (int j = 0; j < kRawRun; ++j) out |= ((w >> (8 * j)) & 0xffu) ? (1u << j) : 0u;
    return out;
  }
#pragma unroll
  for (int j = 0; j < kRawRun; ++j) {
    const int64_t r = r0 + j;
    if (r < n && (m == nullptr || gptr<uint8_t>(m)[r] != 0)) out |= 1u << j;
  }
  return out;
}

// order key of the bits of a double that is not NaN; fold: the grouping rule (-0.0 == +0.0), else
// -0.0 < +0.0 (MIN / MAX)
__device__ __forceinline__ u64 float_key(u64 b, bool fold) {
  if (fold && b == kSign) b = 0;
  return (b & kSign) ? ~b : (b | kSign);
}

// order key of a widened value
__device__ __forceinline__ u64 order_key(u64 raw, bool isf, bool fold) {
  if (!isf) return raw ^ kSign;
  // every NaN: one canonical NaN above +inf
  return float_key((raw & ~kSign) > kInfBits ? kNaNBits : raw, fold);
}

// the bits of the double behind a float order key (order_key's inverse for isf)
__host__ __device__ __forceinline__ u64 unkey(u64 k) { return (k & kSign) ? (k ^ kSign) : ~k; }

// a widened value as a double (an i64 rounds to nearest, as a cast does)
__device__ __forceinline__ double raw_as_f64(u64 raw, bool isf) {
  return isf ? __longlong_as_double((long long)raw) : (double)(long long)raw;
}

// The folded keys of the rows [r0, r0 + 4) of a key column.  Bit j of `live`: the row is inside n
// and selected; of `valid`: it is live and its key is not null.
struct KeyRun {
  u64 key[kRawRun];
  unsigned live, valid;
};

__device__ __forceinline__ KeyRun load_keys(const KeyCol& a, int64_t r0) {
  KeyRun k;
  u64 raw[kRawRun];
  load_run(a.col, a.dt, r0, a.n, raw);
  const bool isf = is_float_dt(a.dt);
#pragma unroll
  for (int j = 0; j < kRawRun; ++j) k.key[j] = order_key(raw[j], isf, true);
  k.live = mask_run(a.sel, r0, a.n);
  k.valid = k.live;
  if (a.valid != nullptr) k.valid &= mask_run(a.valid, r0, a.n);
  return k;
}

// out[r0 + j] = v[j] for the rows inside n: one 16-byte store when the run is complete and aligned
__device__ __forceinline__ void store_run(int* out, int64_t r0, int64_t n, const int v[kRawRun]) {
  if (r0 + kRawRun <= n && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
    i32x4 x;
#pragma unroll
    for (int j = 0; j < kRawRun; ++j) x[j] = v[j];
    *reinterpret_cast<i32x4*>(out + r0) = x;
    return;
  }
#pragma unroll
  for (int j = 0; j < kRawRun; ++j)
    if (r0 + j < n) out[r0 + j] = v[j];
}

// launcher-side check of a key column; `who` prefixes the message
inline void check_key_col(const KeyCol& a, int blocks, const char* who) {
  const std::string w(who);
  if (a.n < 0) throw std::invalid_argument(w + ": negative row count");
  if (blocks < 1) throw std::invalid_argument(w + ": blocks must be >= 1");
  if (!is_key_dt(a.dt)) throw std::invalid_argument(w + ": keys must be f64, f32, i32, i64 or u8");
  if (a.col == nullptr && a.n > 0) throw std::invalid_argument(w + ": null column");
}

}  // namespace dq4ml
