// K5l: one evaluation of the multinomial / binomial logistic loss and its gradient (Spark 2.4
// ml.classification.LogisticRegression's LogisticAggregator) over feature-major X[d, n], or the
// raw / probability / prediction columns of a fitted model (see logreg.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

// LR_GRAD: per-block partial statistics (no per-row output);
// LR_PREDICT: raw[K][n], prob[K][n] (class-major f64) and pred[n] (f64) per row
enum LogregMode : int { LR_GRAD = 0, LR_PREDICT = 1 };

constexpr int kLogregMaxD = 64, kLogregMaxK = 64;

// doubles of the statistics of a GRAD pass over K coefficient rows (multinomial: the classes;
// binomial: 1): [K (d + 1) gradient (row-major, the intercept's in column d), loss, sum w, live
// rows, bad labels]
constexpr int logreg_stats_size(int K, int d) { return K * (d + 1) + 4; }

// grid of the pass for (d, K, n, feature dtype, mode): occupancy-sized, >= ~4 supersteps per wave.
// K = 1 names the binomial kernel, 2 <= K <= 64 the multinomial one.
int logreg_blocks(int d, int K, int64_t n, int xdt, int mode);
// One pass over feature-major f32 / f64 X (a.X, a.ld, a.d, a.n, a.xdt, a.sel; 16-byte aligned
// feature rows, ld >= n), d in [1, 64], against coef = [K][d + 1] f64 (K = 1: binomial).
// LR_GRAD: a.y = class indices (f64 / f32; binomial: 0 / 1), a.w = weights or null, a.partials =
// [blocks][logreg_stats_size(K, d)] slabs for slab_sum.  A live row whose label is no integer in
// [0, classes) adds to the bad-label count and to nothing else.
// LR_PREDICT: raw, prob = [classes][n] (binomial: 2 classes), pred = [n]; dead rows NaN / -1;
// threshold: binomial only (pred = p > threshold).
void logreg_pass(GramArgs a, const double* coef, int K, int mode, double threshold, double* raw, double* prob,
                 double* pred, int blocks, hipStream_t st);

}  // namespace dq4ml
