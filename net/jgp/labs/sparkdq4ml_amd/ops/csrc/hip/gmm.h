// K5m: one EM pass of a Gaussian mixture (Spark 2.4 ml.clustering.GaussianMixture) over
// feature-major X[d, n] -- the k densities of every row and, fused, the responsibility-weighted
// moments of the M-step (see gmm.hip).  The M-step itself (k eigendecompositions of at most 32 x 32)
// is the host's: ops/gmm.py builds the parameter buffer below from it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

// GMM_STEP: per-block partial statistics of the E-step (no per-row output);
// GMM_ASSIGN: per row the int32 arg-max component (first maximum, -1 for dead rows), the k
// normalised probabilities prob[j * n + row] (0 for dead rows) and, on request, log P (0 for dead rows)
enum GmmMode : int { GMM_STEP = 0, GMM_ASSIGN = 1 };

// The fused range: 1 <= d <= 32, 2 <= k <= 16 and k * dp^2 <= 8192 with dp = 16 ceil(d / 16), that
// is k <= 16 at d <= 16 and k <= 8 at 17 <= d <= 32.  Two budgets end it there:
// * LDS.  A block keeps every W_j (dp x dp, row stride dp + 1) resident: 66 KiB at (dp, k) =
//   (32, 8), beside the staged loop's 37 KiB, the second staged tile (33 KiB, dp = 32 only) and the
//   64 x k responsibilities of each wave (16 KiB): 154 of 160 KiB.  dp = 48 would leave room for
//   k = 2 only.
// * Registers.  The second moments S_j live in accumulators across the supersteps: k upper tile
//   pairs of 8 registers each, 128 at (16, 16) and 192 at (32, 8), beside the 32 / 64 of one
//   component's z = W_j x.  Twice either k does not fit 512 without spilling.
constexpr int kGmmMaxD = 32, kGmmMaxK = 16, kGmmMaxW = 8192;
constexpr int gmm_dp(int d) { return 16 * ((d + 15) / 16); }
constexpr bool gmm_in_range(int d, int k) {
  return d >= 1 && d <= kGmmMaxD && k >= 2 && k <= kGmmMaxK && k * gmm_dp(d) * gmm_dp(d) <= kGmmMaxW;
}

// doubles of the statistics of a pass:
// [k sw, k * d sm (component-major), k * d (d + 1) / 2 S (component-major, packed upper, row-major), loglik, live rows]
constexpr int gmm_stats_size(int k, int d) { return k + k * d + k * (d * (d + 1) / 2) + 2; }
// doubles of the parameter buffer, all component-major:
// [k * dp * dp W (row-major, zero padded), k * dp c = W mu, k weights w, k constants u]
constexpr int gmm_params_size(int k, int d) { return k * gmm_dp(d) * (gmm_dp(d) + 1) + 2 * k; }

// grid of the pass for (d, k, n, feature dtype, mode): occupancy-sized, >= ~4 supersteps per wave
int gmm_blocks(int d, int k, int64_t n, int xdt, int mode);
// One pass over feature-major f32 / f64 X (a.X, a.ld, a.d, a.n, a.xdt, a.sel; 16-byte aligned
// feature rows, ld >= n) inside the fused range, against params = [gmm_params_size].
// GMM_STEP: a.partials = [blocks][gmm_stats_size] slabs for gmm_reduce.
// GMM_ASSIGN: assign = [n] int32, prob = [k][n] f64, logp = [n] f64 or null.
void gmm_pass(GramArgs a, const double* params, int k, int mode, int32_t* assign, double* prob, double* logp,
              int blocks, hipStream_t st);
// stats[i] = sum of partials[b][i] over the blocks in block order
void gmm_reduce(const double* partials, int blocks, int k, int d, double* stats, hipStream_t st);

}  // namespace dq4ml
