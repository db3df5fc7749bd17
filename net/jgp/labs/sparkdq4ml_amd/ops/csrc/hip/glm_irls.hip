// K5i: one IRLS pass of a generalized linear model (Spark 2.4 GeneralizedLinearRegression) fused
// into a staged f64 Gram pass: X is read once per iteration.
//
// An IRLS iteration is a weighted least-squares fit of the working response z with the working
// weights w', both functions of eta = x . beta + b of the row.  The staged f64 loop (gram_slab.h
// section 5; this kernel and gram_folds.hip's keep it) stages every 16-feature x 64-row tile of a
// superstep in LDS before the MFMAs, so eta is formed right there: lane = row reads
// xs[f * kStageLd + lane] of the 16 staged features (one bank per lane) against beta in LDS.
// After the last tile the lane derives mu, z, w' of its row in registers (plain f64 exp / log /
// sqrt / divide), writes w' and w'z to the row-scalar area, and the pass goes on as a plain
// weighted statistics pass: column sums, X'z and the MFMA Gram with x . w'.  The per-block slabs are gram_slab.h's, so gram_reduce and wls_small take them
// unchanged.  Dead rows (selection) and rows >= n are selected to zero, never multiplied: their
// features and label may be NaN.  The ragged last superstep is staged through LDS too (guarded,
// zero-filled), so one eta path serves both.  Plain launches, no atomics: bit-identical run to run.
#include "glm_irls.h"

#include <cfloat>

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

struct GlmArgs {
  const double* beta;   // [coef(d), intercept]
  const double* state;  // [kGlmState]
  int mode;
};

constexpr double kGlmEps = 1e-16;

// ---- links -------------------------------------------------------------------------------------
template <int LINK>
__device__ __forceinline__ double glm_link(double mu) {
  if constexpr (LINK == GLM_IDENTITY) return mu;
  else if constexpr (LINK == GLM_LOG) return log(mu);
  else if constexpr (LINK == GLM_LOGIT) return log(mu / (1.0 - mu));
  else if constexpr (LINK == GLM_INVERSE) return 1.0 / mu;
  else return sqrt(mu);
}

template <int LINK>
__device__ __forceinline__ double glm_unlink(double eta) {
  if constexpr (LINK == GLM_IDENTITY) return eta;
  else if constexpr (LINK == GLM_LOG) return exp(eta);
  else if constexpr (LINK == GLM_LOGIT) return 1.0 / (1.0 + exp(-eta));
  else if constexpr (LINK == GLM_INVERSE) return 1.0 / eta;
  else return eta * eta;
}

template <int LINK>
__device__ __forceinline__ double glm_dlink(double mu) {
  if constexpr (LINK == GLM_IDENTITY) return 1.0;
  else if constexpr (LINK == GLM_LOG) return 1.0 / mu;
  else if constexpr (LINK == GLM_LOGIT) return 1.0 / (mu * (1.0 - mu));
  else if constexpr (LINK == GLM_INVERSE) return -1.0 / (mu * mu);
  else return 1.0 / (2.0 * sqrt(mu));
}

// ---- families ----------------------------------------------------------------------------------
template <int FAM>
__device__ __forceinline__ double glm_variance(double mu) {
  if constexpr (FAM == GLM_GAUSSIAN) return 1.0;
  else if constexpr (FAM == GLM_BINOMIAL) return mu * (1.0 - mu);
  else if constexpr (FAM == GLM_POISSON) return mu;
  else return mu * mu;
}

template <int FAM>
__device__ __forceinline__ double glm_init(double y, double w) {
  if constexpr (FAM == GLM_BINOMIAL) return (w * y + 0.5) / (w + 1.0);
  else if constexpr (FAM == GLM_POISSON) return y > 0.1 ? y : 0.1;
  else return y;
}

template <int FAM>
__device__ __forceinline__ double glm_project(double mu) {
  if constexpr (FAM == GLM_GAUSSIAN) {
    return mu == HUGE_VAL ? DBL_MAX : (mu == -HUGE_VAL ? -DBL_MAX : mu);
  } else if constexpr (FAM == GLM_BINOMIAL) {
    return mu < kGlmEps ? kGlmEps : (mu > 1.0 - kGlmEps ? 1.0 - kGlmEps : mu);
  } else {
    return mu < kGlmEps ? kGlmEps : (mu == HUGE_VAL ? DBL_MAX : mu);
  }
}

__device__ __forceinline__ double load_f32_f64(const void* p, int dt, int64_t r) {
  return dt == DT_F64 ? reinterpret_cast<const double*>(p)[r] : (double)reinterpret_cast<const float*>(p)[r];
}

// The ragged superstep's tile: features [f0, f0 + 16) x rows [r0, r0 + 64) into xs[f][row] like
// stage_tile (gram_slab.h), lane = row, zeros for features >= d and rows >= n.
template <typename TX>
__device__ __forceinline__ void stage_tile_guarded(const TX* __restrict__ X, int64_t ld, int d, int f0, int64_t r0,
                                                   int64_t n, int lane, double* xs) {
  const bool in = r0 + lane < n;
#pragma unroll
  for (int fl = 0; fl < 16; ++fl) {
    const int feat = f0 + fl;
    double v = 0.0;
    if (in && feat < d) v = (double)X[(int64_t)feat * ld + r0 + lane];
    xs[fl * kStageLd + lane] = v;
  }
}

// a.nsuper = supersteps (ceil(n / 64)), a.spw = supersteps per wave; a.partials = [gridDim.x][P].
// LDS: the tall f64 loop's (row scalars + one staged tile per wave), then beta[65].
template <typename TX, int NT, int FAM, int LINK>
__global__ __launch_bounds__(kBlock) void glm_irls_f64_kernel(GramArgs a, GlmArgs g) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  const bool step = g.mode == GLM_STEP;
  if (step && g.state[1] != 0.0) return;  // the fit is done: the slabs stay as they are
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  double* lw = reinterpret_cast<double*>(smem) + wave * 128;  // [w'(64), w'z(64)]
  double* xs = reinterpret_cast<double*>(smem) + kWavesPerBlock * 128 + wave * (16 * kStageLd);
  double* bl = reinterpret_cast<double*>(smem) + kTallF64LoopBytes / sizeof(double);  // coef (64, zero padded), intercept
  double* red = reinterpret_cast<double*>(smem);  // block reduction: aliases the loop's area
  // accumulators per tile pair.  The MFMAs are issued row by row (below), so consecutive ones go
  // to different pairs: from 6 pairs on those are the independent chains that cover the f64 MFMA
  // latency, and one accumulator per pair leaves <*, 4> the registers it otherwise spills
  constexpr int kChains = NT >= 3 ? 1 : (NT == 2 ? 2 : 4);

  const int d = a.d;
  const int P = a.P;
  if (threadIdx.x < 65) {
    double v = 0.0;
    if (step && (threadIdx.x < d || threadIdx.x == 64)) v = g.beta[threadIdx.x < d ? threadIdx.x : d];
    bl[threadIdx.x] = v;
  }
  __syncthreads();

  f64x4 acc[NPAIR][kChains];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p)
#pragma unroll
    for (int c = 0; c < kChains; ++c) acc[p][c] = f64x4{};
  double cs[NT], ab[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) cs[t] = ab[t] = 0.0;
  RowAcc ra;

  const TX* X = reinterpret_cast<const TX*>(a.X);
  const int64_t nfull = a.n / 64;  // supersteps below are whole; superstep nfull is the n % 64 tail
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  int64_t s0 = gw * a.spw;
  int64_t s1 = s0 + a.spw;
  if (s0 > a.nsuper) s0 = a.nsuper;
  if (s1 > a.nsuper) s1 = a.nsuper;

  for (int64_t s = s0; s < s1; ++s) {
    const int64_t r0 = s * 64;
    const int64_t r = r0 + lane;
    bool live = false;
    double y = 0.0, w = 1.0;
    if (r < a.n) {
      live = a.sel ? (a.sel[r] != 0) : true;
      if (live) {
        y = load_f32_f64(a.y, a.ydt, r);
        if (a.w) w = load_f32_f64(a.w, a.wdt, r);
      }
    }
    double eta = bl[64];
    double x[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (s < nfull) stage_tile<TX>(X, a.ld, d, t * 16, r0, lane, xs);
      else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
      __builtin_amdgcn_wave_barrier();
      if (step) {  // lane = row: one bank per lane, beta broadcast
#pragma unroll
        for (int k = 0; k < 16; ++k) eta += xs[k * kStageLd + lane] * bl[t * 16 + k];
      }
      const f64x2* src = reinterpret_cast<const f64x2*>(xs + f * kStageLd + 16 * q);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f64x2 v = src[i];
        x[t][2 * i] = v[0];
        x[t][2 * i + 1] = v[1];
      }
      __builtin_amdgcn_wave_barrier();
    }
    // the row's working response and weight (dead rows: eta, y and so all of this may be NaN)
    double z, wp;
    if (step) {
      const double mu = glm_project<FAM>(glm_unlink<LINK>(eta));
      const double gp = glm_dlink<LINK>(mu);
      z = eta + (y - mu) * gp;
      wp = w / (gp * gp * glm_variance<FAM>(mu));
    } else {
      z = glm_link<LINK>(glm_init<FAM>(y, w));
      wp = w;
    }
    RowVals rv{live, 0.0, 0.0, 0.0};
    rv.w = live ? wp : 0.0;
    rv.y = live ? z : 0.0;
    rv.wy = live ? wp * z : 0.0;
    ra.add(rv);
    lw[lane] = rv.w;
    lw[64 + lane] = rv.wy;
    const unsigned long long livemask = __ballot(live);
    __builtin_amdgcn_wave_barrier();
    // dead rows: select, never multiply -- their stored features may be NaN
    const unsigned m16 = (unsigned)(livemask >> (16 * q)) & 0xffffu;
    // row e of the lane's 16 at a time, its two scalars read when they are used: the row scalars of
    // all 16 rows held beside x[NT][16] is what the <double, 4> registers do not have room for
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const double we = lw[16 * q + e], wye = lw[64 + 16 * q + e];
      const bool on = (m16 >> e) & 1u;
      double xw[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        x[t][e] = on ? x[t][e] : 0.0;
        xw[t] = x[t][e] * we;
        cs[t] += xw[t];
        ab[t] += x[t][e] * wye;
      }
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++p)
          acc[p][e % kChains] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[I][e], xw[J], acc[p][e % kChains], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }

  // block reduction over the waves in order + slab store (the tall f64 kernel's)
  __syncthreads();
  for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
  double sc[kSlabScalars];
  wave_scalars(ra, sc);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    cs[t] += __shfl_xor(cs[t], 16, 64);
    cs[t] += __shfl_xor(cs[t], 32, 64);
    ab[t] += __shfl_xor(ab[t], 16, 64);
    ab[t] += __shfl_xor(ab[t], 32, 64);
  }
  __syncthreads();
  for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
    if (wave == wvi) {
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSlabScalars; ++k) red[k] += sc[k];
      }
      if (q == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int feat = t * 16 + f;
          if (feat < d) {
            red[kSlabScalars + feat] += cs[t];
            red[kSlabScalars + d + feat] += ab[t];
          }
        }
      }
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++p) {
          double* tile = slab_tile<16>(red, d, p);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < kChains; ++c) v += acc[p][c][r];
            tile[mfma16d_row(lane, r) * 16 + mfma16d_col(lane)] += v;
          }
        }
    }
    __syncthreads();
  }
  double* out = a.partials + (int64_t)blockIdx.x * P;
  for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
}

// One wave.  sol: wls_small's [coef(d), intercept, status, ...]; state: [iter, done, status, max |delta|].
__global__ __launch_bounds__(kWave) void glm_step_kernel(const double* __restrict__ sol, int d, double tol, int init,
                                                         double* beta, double* state) {
  if (state[1] != 0.0) return;
  const int lane = threadIdx.x;
  const double status = sol[d + 1];
  double dl = 0.0;
  for (int j = lane; j <= d; j += kWave) dl = fmax(dl, fabs(beta[j] - sol[j]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dl = fmax(dl, __shfl_xor(dl, o, 64));
  const bool ok = status == 0.0;
  if (ok)
    for (int j = lane; j <= d; j += kWave) beta[j] = sol[j];
  if (lane == 0) {
    if (!init) {
      state[0] += 1.0;
      state[3] = dl;
    }
    if (!ok) {
      state[1] = 1.0;
      state[2] = status;
    } else if (!init && dl < tol) {
      state[1] = 1.0;
    }
  }
}

size_t glm_lds(int d) { return staged_f64_lds(d, 65 * sizeof(double)); }  // (+ beta[65])

template <typename TX, int FAM, int LINK, typename F>
void with_glm_nt(int NT, F&& f) {
  switch (NT) {
    case 1: return f(glm_irls_f64_kernel<TX, 1, FAM, LINK>);
    case 2: return f(glm_irls_f64_kernel<TX, 2, FAM, LINK>);
    case 3: return f(glm_irls_f64_kernel<TX, 3, FAM, LINK>);
    default: return f(glm_irls_f64_kernel<TX, 4, FAM, LINK>);
  }
}

template <typename TX, typename F>
void with_glm_pair(int family, int link, int NT, F&& f) {
#define DQ_GLM_CASE(FAM, LINK) \
  if (family == FAM && link == LINK) return with_glm_nt<TX, FAM, LINK>(NT, f);
  DQ_GLM_CASE(GLM_GAUSSIAN, GLM_IDENTITY)
  DQ_GLM_CASE(GLM_GAUSSIAN, GLM_LOG)
  DQ_GLM_CASE(GLM_GAUSSIAN, GLM_INVERSE)
  DQ_GLM_CASE(GLM_BINOMIAL, GLM_LOGIT)
  DQ_GLM_CASE(GLM_POISSON, GLM_LOG)
  DQ_GLM_CASE(GLM_POISSON, GLM_IDENTITY)
  DQ_GLM_CASE(GLM_POISSON, GLM_SQRT)
  DQ_GLM_CASE(GLM_GAMMA, GLM_INVERSE)
  DQ_GLM_CASE(GLM_GAMMA, GLM_IDENTITY)
  DQ_GLM_CASE(GLM_GAMMA, GLM_LOG)
#undef DQ_GLM_CASE
  throw std::invalid_argument("glm_irls: unsupported (family, link) pair");
}

template <typename F>
void with_glm_kernel(int xdt, int d, int family, int link, F&& f) {
  const int NT = (d + 15) / 16;
  if (xdt == DT_F64) return with_glm_pair<double>(family, link, NT, f);
  if (xdt == DT_F32) return with_glm_pair<float>(family, link, NT, f);
  throw std::invalid_argument("glm_irls: features must be f32 or f64");
}

}  // namespace

bool glm_pair_ok(int family, int link) {
  switch (family) {
    case GLM_GAUSSIAN: return link == GLM_IDENTITY || link == GLM_LOG || link == GLM_INVERSE;
    case GLM_BINOMIAL: return link == GLM_LOGIT;
    case GLM_POISSON: return link == GLM_LOG || link == GLM_IDENTITY || link == GLM_SQRT;
    case GLM_GAMMA: return link == GLM_INVERSE || link == GLM_IDENTITY || link == GLM_LOG;
    default: return false;
  }
}

int glm_irls_blocks(int d, int64_t n, int xdt) {
  if (d < 1 || d > 64) throw std::invalid_argument("glm_irls: d must be in [1, 64]");
  int nb = 1;
  // (the register count, and so the occupancy, is the Gram loop's: one pair stands for all)
  with_glm_kernel(xdt, d, GLM_BINOMIAL, GLM_LOGIT, [&](auto kern) { nb = staged_f64_blocks(kern, glm_lds(d), n); });
  return nb;
}

void glm_irls_pass(GramArgs a, const double* beta, const double* state, int family, int link, int mode, int blocks,
                   hipStream_t st) {
  staged_f64_plan(a, blocks, "glm_irls");
  if (!glm_pair_ok(family, link)) throw std::invalid_argument("glm_irls: unsupported (family, link) pair");
  if (mode != GLM_INIT && mode != GLM_STEP) throw std::invalid_argument("glm_irls: mode must be INIT (0) or STEP (1)");
  if (mode == GLM_STEP && (beta == nullptr || state == nullptr))
    throw std::invalid_argument("glm_irls: a STEP pass needs beta and state");
  if (a.w != nullptr && a.wdt != DT_F64 && a.wdt != DT_F32)
    throw std::invalid_argument("glm_irls: weights must be f32 or f64");
  if (a.partials == nullptr || a.X == nullptr || a.y == nullptr) throw std::invalid_argument("glm_irls: null operand");
  const GlmArgs g{beta, state, mode};
  const size_t lds = glm_lds(a.d);
  with_glm_kernel(a.xdt, a.d, family, link,
                  [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), lds, st, a, g); });
  DQ_HIP_CHECK(hipGetLastError());
}

void glm_step(const double* sol, int d, double tol, int init, double* beta, double* state, hipStream_t st) {
  if (d < 1 || d > 64) throw std::invalid_argument("glm_step: d must be in [1, 64]");
  if (sol == nullptr || beta == nullptr || state == nullptr) throw std::invalid_argument("glm_step: null operand");
  hipLaunchKernelGGL(glm_step_kernel, dim3(1), dim3(kWave), 0, st, sol, d, tol, init, beta, state);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
