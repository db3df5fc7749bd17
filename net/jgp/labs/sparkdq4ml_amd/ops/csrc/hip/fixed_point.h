// The fixed-point cut behind every exact f64 sum on integer accumulators (groupby.hip SUM_F,
// tree.hip's regression histogram).
#pragma once
#include <hip/hip_runtime.h>

namespace dq4ml {

constexpr int kSumLimbs = 4;

// x * 2^(128 - e) as four signed limbs, limb k in units of 2^(e - 32 (k + 1)): with |x| < 2^e every
// step is exact in f64 (|c[k]| < 2^32, all limbs carry the sign of x), so sums of limbs in i64 are
// exact below 2^31 rows.  x must be finite.
__device__ __forceinline__ void cut_limbs(double x, int e, long long c[kSumLimbs]) {
  double t = ldexp(x, 32 - e);
#pragma unroll
  for (int k = 0; k < kSumLimbs; ++k) {
    const double ck = trunc(t);
    c[k] = (long long)ck;
    t = ldexp(t - ck, 32);
  }
}

}  // namespace dq4ml
