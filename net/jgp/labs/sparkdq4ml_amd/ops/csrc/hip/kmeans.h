// K5k: one Lloyd pass of k-means (Spark 2.4 ml.clustering.KMeans, euclidean) over feature-major
// X[d, n] -- nearest centre of every row and, fused, the new centres' sums -- and the one-block
// update that closes an iteration (see kmeans.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

// KM_STEP: per-block partial statistics of the assignment (no per-row output);
// KM_ASSIGN: int32 cluster index per row (-1 for dead rows) and, on request, the f64 row cost
enum KMeansMode : int { KM_STEP = 0, KM_ASSIGN = 1 };

// device state of a fit, f64: [iterations, done, cost, max moved^2]
constexpr int kKMeansState = 4;
constexpr int kKMeansMaxD = 64, kKMeansMaxK = 64;

// doubles of the statistics of a pass: [k * d sums (centre-major), k counts, cost, live rows]
constexpr int kmeans_stats_size(int k, int d) { return k * d + k + 2; }
// doubles of the device centre buffer: [k * d centres (centre-major), k half squared norms]
constexpr int kmeans_centers_size(int k, int d) { return k * d + k; }

// grid of the pass for (d, k, n, feature dtype, mode): occupancy-sized, >= ~4 supersteps per wave
int kmeans_blocks(int d, int k, int64_t n, int xdt, int mode);
// One pass over feature-major f32 / f64 X (a.X, a.ld, a.d, a.n, a.xdt, a.sel; 16-byte aligned
// feature rows, ld >= n), d in [1, 64], k in [2, 64], against centers = [kmeans_centers_size].
// KM_STEP: a.partials = [blocks][kmeans_stats_size] slabs for kmeans_reduce; state = [kKMeansState],
// and a pass whose state says done returns at once and leaves the slabs as they are.
// KM_ASSIGN: assign = [n] int32, cost = [n] f64 or null.
void kmeans_pass(GramArgs a, const double* centers, int k, const double* state, int mode, int32_t* assign,
                 double* cost, int blocks, hipStream_t st);
// stats[i] = sum of partials[b][i] over the blocks in block order
void kmeans_reduce(const double* partials, int blocks, int k, int d, double* stats, hipStream_t st);
// Not done: centre = sum / count (a centre with count 0 stays), its half squared norm, moved^2 per
// centre against the old position; state = [iterations + 1, every moved^2 <= tol^2, cost of the
// pass, max moved^2].  Done: touches nothing.
void kmeans_update(const double* stats, int k, int d, double tol, double* centers, double* state, hipStream_t st);

}  // namespace dq4ml
