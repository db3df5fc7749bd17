// K5i: one IRLS (iteratively reweighted least squares) pass of a generalized linear model, fused
// into a staged f64 Gram pass (see glm_irls.hip), and the one-block step that closes an iteration.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gram.h"

namespace dq4ml {

// codes shared with the python side (ops/glm.py)
enum GlmFamily : int { GLM_GAUSSIAN = 0, GLM_BINOMIAL = 1, GLM_POISSON = 2, GLM_GAMMA = 3 };
enum GlmLink : int { GLM_IDENTITY = 0, GLM_LOG = 1, GLM_LOGIT = 2, GLM_INVERSE = 3, GLM_SQRT = 4 };
// GLM_INIT: Spark's starting model, z = link(init(y, w)), w' = w (beta is not read);
// GLM_STEP: z and w' from the current beta
enum GlmMode : int { GLM_INIT = 0, GLM_STEP = 1 };

// device state of a fit, f64: [iter, done, status, max |delta|]
constexpr int kGlmState = 4;

bool glm_pair_ok(int family, int link);
// grid of the pass for (d, n, feature dtype): occupancy-sized, >= ~4 supersteps per wave
int glm_irls_blocks(int d, int64_t n, int xdt);
// One pass over feature-major f32 / f64 X (16-byte aligned feature rows, ld >= n), d in [1, 64]:
// a.partials = [blocks][gram_partial_stride(GRAM_F64, d)] slabs of the statistics of (x, z, w'),
// for gram_reduce(GRAM_F64, ...).  beta = [coef(d), intercept] and state = [kGlmState] on the
// device (GLM_STEP only); a pass whose state says done returns at once and leaves the slabs as
// they are.
void glm_irls_pass(GramArgs a, const double* beta, const double* state, int family, int link, int mode, int blocks,
                   hipStream_t st);
// sol = wls_small's output [coef(d), intercept, status, ...].  Not done: max |delta| against beta,
// iter += 1 (not for init = 1, the starting model); a non-zero status sets done with that status,
// else beta = sol and done once max |delta| < tol (never for init).  Done: touches nothing.
void glm_step(const double* sol, int d, double tol, int init, double* beta, double* state, hipStream_t st);

}  // namespace dq4ml
