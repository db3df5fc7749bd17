// K5p: one evaluation of the loss and gradient of a small dense network (Spark 2.4
// ml.classification.MultilayerPerceptronClassifier: FeedForwardModel.computeGradient for
// FeedForwardTopology.multiLayerPerceptron(layers, softmaxOnTop = true)) over feature-major X[d, n],
// or the prediction column of a fitted model (see mlp.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

// MLP_GRAD: per-block partial statistics (no per-row output); MLP_PREDICT: pred[n] (f64) per row
enum MlpMode : int { MLP_GRAD = 0, MLP_PREDICT = 1 };

// The fused range, stated here once (ops/mlp.py mirrors it): `layers` = [d, hidden..., K] with one
// or two hidden layers, d in [1, 64], every hidden width in [1, 32], K in [2, 32].
constexpr int kMlpMinLayers = 3, kMlpMaxLayers = 4;
constexpr int kMlpMaxD = 64, kMlpMaxWidth = 32;

// length P of the flat weight vector in Spark's layout: per affine layer W (numOut x numIn,
// column-major), then b (numOut)
inline int mlp_weight_count(const int* layers, int nlayers) {
  int P = 0;
  for (int l = 0; l + 1 < nlayers; ++l) P += (layers[l] + 1) * layers[l + 1];
  return P;
}
// doubles of the statistics of a GRAD pass: [P gradient (the weight layout), loss sum, live rows,
// bad labels]
inline int mlp_stats_size(const int* layers, int nlayers) { return mlp_weight_count(layers, nlayers) + 3; }

// grid of the pass: occupancy-sized, >= ~4 supersteps per wave
int mlp_blocks(const int* layers, int nlayers, int64_t n, int xdt, int mode);
// One pass over feature-major f32 / f64 X (a.X, a.ld, a.d, a.n, a.xdt, a.sel; 16-byte aligned
// feature rows, ld >= n) with a.d == layers[0], against the flat f64 `weights` [P].
// MLP_GRAD: a.y = class indices (f64 / f32), a.partials = [blocks][mlp_stats_size] slabs for
// slab_sum.  A live row whose label is no integer in [0, K) adds to the bad-label count and to
// nothing else.  MLP_PREDICT: pred = [n], the first maximum of the output layer, dead rows -1.
void mlp_pass(GramArgs a, const double* weights, const int* layers, int nlayers, int mode, double* pred, int blocks,
              hipStream_t st);

}  // namespace dq4ml
