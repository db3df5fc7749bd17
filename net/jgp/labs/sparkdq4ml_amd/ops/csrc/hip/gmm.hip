// K5m: one EM pass of a Gaussian mixture as ONE kernel over feature-major X[d, n]: nothing of size
// n x k is written in a STEP pass, and X comes from HBM once.
//
// Work split: the staged f64 plan of gram_slab.h section 5 (kBlock = 256, a wave keeps one
// contiguous range of 64-row supersteps, a cooperative stage for the full ones, a guarded
// zero-filling stage for the ragged last one).  Rows that are dead or >= n are selected to zero,
// never multiplied.  NT = ceil(d / 16) is 1 or 2; at NT = 2 both 16-feature tiles of a superstep
// are staged side by side (the second one in LDS of its own behind the loop's area), because
// both phases below walk the components in their outer loop and need every feature each time.
//
// Parameters: per component j the pseudo-inverse root W_j (zero padded to dp x dp, dp = 16 NT, row
// stride dp + 1 so the 16 rows of an A operand fall into different banks), c_j = W_j mu_j, the
// weight w_j and the constant u_j = -0.5 (d log 2 pi + logdet_j) sit in LDS for the whole kernel,
// loaded once per block from the buffer the host builds after its M-step.
//
// Density phase, one component at a time (a real loop, so only one component's accumulators are
// live): z = W_j x by v_mfma_f64_16x16x4f64 with A = 16 rows of W_j x 4 features (LDS) and B = 4
// features x 16 rows (the staged tile, lane = row): NT x 4 accumulators.  A lane holds z of W rows
// 16 mt + q + 4 reg for row 16 rt + f; it sums (z - c_j)^2 over its registers in a fixed order, the
// four lane groups combine with __shfl_xor 16 / 32, and lane 16 q + f keeps row tile q's result,
// which is row `lane` of the superstep.  p_j = EPS + w_j exp(u_j - 0.5 |z - c_j|^2) (Spark's form:
// no log-sum-exp), P = sum_j p_j in component order, and the 64 x k values p_j go to the wave's LDS,
// where a second sweep turns them into r_j = p_j / P (0 for dead rows).
//
// Moment phase (GMM_STEP): S_j += (X diag(r_j)) X^T as a second MFMA over the same staged tiles:
// A = r_j(row 16 q + e) x(feature 16 ti + f, row 16 q + e), B = x(feature 16 tj + f, row 16 q + e),
// into the upper tile pairs of every component, K x NT (NT + 1) / 2 accumulators that live across
// the supersteps.  That product needs the component count at compile time (K = k exactly: a padded
// count would spend MFMAs on components that do not exist).  sm_j rides on one more MFMA per tile
// with A = r_f (component f of the lane), as kmeans.hip's one-hot sums do, and sw_j is the sum of
// that same A operand per lane, closed over the lane groups at the end.  No ones row: it would
// need a free pad feature, which d = 16 and d = 32 lack.
//
// Slabs: one partial per block, [k sw, k d sm, k d (d + 1) / 2 S packed upper, loglik, live rows],
// folded over the waves in order in LDS (the loop's area, dead by then), reduced over the blocks in
// block order by slab_sum.  Plain launches, no atomics: bit-identical run to run.
#include "gmm.h"

#include <cmath>

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

struct GmmArgs {
  const double* par;  // [gmm_params_size]
  int k;
  int32_t* assign;    // GMM_ASSIGN: [n]
  double* prob;       // GMM_ASSIGN: [k][n]
  double* logp;       // GMM_ASSIGN: [n] or null
};

constexpr double kGmmEps = 2.220446049250313e-16;  // 2^-52, Spark's EPSILON
constexpr int kTileD = 16 * kStageLd;              // doubles of a staged tile
constexpr int kLoopD = (int)(kTallF64LoopBytes / sizeof(double));
// doubles per LDS row of W
constexpr int gmm_ldw(int NT) { return 16 * NT + 1; }
// LDS doubles behind the loop's area: the second tile (NT = 2), W, c, (w, u), the responsibilities
constexpr int gmm_extra(int NT, int k) {
  return (NT - 1) * kWavesPerBlock * kTileD + k * 16 * NT * gmm_ldw(NT) + k * 16 * NT + 2 * k + kWavesPerBlock * 64 * k;
}
constexpr size_t gmm_lds_bytes(int NT, int k) { return kTallF64LoopBytes + (size_t)gmm_extra(NT, k) * sizeof(double); }
static_assert(gmm_lds_bytes(1, 16) <= 160 * 1024 && gmm_lds_bytes(2, 8) <= 160 * 1024, "the pass must fit 160 KiB of LDS");
// the block reduction's slab aliases the loop's area
static_assert((size_t)gmm_stats_size(16, 16) * sizeof(double) <= kTallF64LoopBytes &&
                  (size_t)gmm_stats_size(8, 32) * sizeof(double) <= kTallF64LoopBytes,
              "the mixture slab must fit the staged loop's LDS");

// a.nsuper = supersteps (ceil(n / 64)), a.spw = supersteps per wave; a.partials = [gridDim.x][P].
// K: the component count of a STEP pass (== g.k); 0 for ASSIGN, which needs it at run time only.
template <typename TX, int NT, int K, int MODE>
__global__ __launch_bounds__(kBlock) void gmm_em_f64_kernel(GramArgs a, GmmArgs g) {
  constexpr bool kStep = MODE == GMM_STEP;
  constexpr int kDp = 16 * NT, kLdw = gmm_ldw(NT), kNP = NT * (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  const int d = a.d, k = g.k;
  double* sm = reinterpret_cast<double*>(smem);
  int* lv = reinterpret_cast<int*>(sm + wave * 128);           // the superstep's live flags
  double* xt[NT];                                              // the staged tiles
  xt[0] = sm + kWavesPerBlock * 128 + wave * kTileD;
  constexpr int kTile1 = kLoopD - kWavesPerBlock * 128;       // from a wave's first tile to its second
  if constexpr (NT == 2) xt[1] = xt[0] + kTile1;
  double* wl = sm + kLoopD + (NT - 1) * kWavesPerBlock * kTileD;  // [k][kDp][kLdw]
  double* cl = wl + k * kDp * kLdw;                               // [k][kDp]
  double* wu = cl + k * kDp;                                      // [k] w, [k] u
  double* rl = wu + 2 * k + wave * 64 * k;                        // [k][64]: p_j, then r_j, of the wave's superstep
  double* red = sm;  // block reduction: aliases the loop's area

  for (int i = threadIdx.x; i < k * kDp * kDp; i += kBlock) wl[(i / kDp) * kLdw + i % kDp] = g.par[i];
  for (int i = threadIdx.x; i < k * kDp + 2 * k; i += kBlock) cl[i] = g.par[k * kDp * kDp + i];
  __syncthreads();

  f64x4 S[kStep ? K : 1][kNP], mean[NT];
  double sw_acc = 0.0, ll_acc = 0.0, live_acc = 0.0;
  if constexpr (kStep) {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int p = 0; p < kNP; ++p) S[j][p] = f64x4{};
#pragma unroll
    for (int t = 0; t < NT; ++t) mean[t] = f64x4{};
  }

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
    const bool live = r < a.n && (a.sel ? a.sel[r] != 0 : true);
    __builtin_amdgcn_wave_barrier();
    // (a real loop: unrolled, both tiles' loads are in flight at once, registers <float, 2, 8> lacks)
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      double* xs = xt[0] + t * kTile1;
      if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
      else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
    }
    __builtin_amdgcn_wave_barrier();

    // ---- densities: one component at a time (a real loop: unrolled, the compiler keeps several
    // components' accumulators and W operands live, registers the second moments need)
    double P = 0.0, best = -1.0;
    int bidx = 0;
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
      const double* wj = wl + j * kDp * kLdw;
      f64x4 z[NT][4];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) z[mt][rt] = f64x4{};
      // z[mt][rt] += W_j(16 mt + i, 16 t + 4 ks + kk) * x(16 t + 4 ks + kk, row 16 rt + j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          double b[4];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) b[rt] = xt[t][(4 * ks + q) * kStageLd + 16 * rt + f];
#pragma unroll
          for (int mt = 0; mt < NT; ++mt) {
            const double av = wj[(16 * mt + f) * kLdw + 16 * t + 4 * ks + q];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) z[mt][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[rt], z[mt][rt], 0, 0, 0);
          }
        }
      // |z - c_j|^2 of row 16 rt + f over the lane's W rows 16 mt + q + 4 reg, then over the lane
      // groups (dead rows: the sum may be NaN and is not used)
      double cj[NT][4];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cj[mt][reg] = cl[j * kDp + 16 * mt + mfma16d_row(lane, reg)];
      double qq = 0.0;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        double sq = 0.0;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const double dz = z[mt][rt][reg] - cj[mt][reg];
            sq += dz * dz;
          }
        sq += __shfl_xor(sq, 16, 64);
        sq += __shfl_xor(sq, 32, 64);
        if (q == rt) qq = sq;  // row 16 q + f = lane
      }
      const double p = live ? kGmmEps + wu[j] * exp(wu[k + j] - 0.5 * qq) : 0.0;
      rl[j * 64 + lane] = p;
      P += p;
      if (p > best) {  // the first maximum
        best = p;
        bidx = j;
      }
    }
    const double lp = live ? log(P) : 0.0;
    if constexpr (!kStep) {
      if (r < a.n) {
        g.assign[r] = live ? bidx : -1;
        if (g.logp != nullptr) g.logp[r] = lp;
        for (int j = 0; j < k; ++j) g.prob[(int64_t)j * a.n + r] = live ? rl[j * 64 + lane] / P : 0.0;
      }
    } else {
      for (int j = 0; j < k; ++j) rl[j * 64 + lane] = live ? rl[j * 64 + lane] / P : 0.0;
      ll_acc += lp;
      live_acc += live ? 1.0 : 0.0;
      lv[lane] = live ? 1 : 0;
      __builtin_amdgcn_wave_barrier();
      // ---- moments: k-step e of the MFMAs covers rows 16 q + e of the four lane groups
      const double* rq = rl + 16 * q;                               // r_j(row 16 q + e) = rq[64 j + e]
      const double* rf = rl + (f < k ? f : k - 1) * 64 + 16 * q;    // component f's (clamped: never read past k)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        // dead rows: select, never multiply -- their features may be NaN
        const bool on = lv[16 * q + e] != 0;
        double xv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f64x2* src = reinterpret_cast<const f64x2*>(xt[t] + f * kStageLd + 16 * q);
          xv[t] = on ? src[e >> 1][e & 1] : 0.0;
        }
        const double am = f < k ? rf[e] : 0.0;
        sw_acc += am;
#pragma unroll
        for (int t = 0; t < NT; ++t) mean[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, xv[t], mean[t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const double rj = rq[64 * j + e];
          int p = 0;
#pragma unroll
          for (int ti = 0; ti < NT; ++ti) {
            const double av = rj * xv[ti];
#pragma unroll
            for (int tj = ti; tj < NT; ++tj, ++p) S[j][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xv[tj], S[j][p], 0, 0, 0);
          }
        }
      }
    }
  }

  if constexpr (kStep) {
    // block reduction over the waves in order + slab store
    const int P = gmm_stats_size(k, d), tri = d * (d + 1) / 2;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
    ll_acc = wave_sum_f64(ll_acc);
    live_acc = wave_sum_f64(live_acc);
    sw_acc += __shfl_xor(sw_acc, 16, 64);
    sw_acc += __shfl_xor(sw_acc, 32, 64);
    __syncthreads();
    for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
      if (wave == wvi) {
        if (lane == 0) {
          red[P - 2] += ll_acc;
          red[P - 1] += live_acc;
        }
        if (q == 0 && f < k) red[f] += sw_acc;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int c = mfma16d_row(lane, reg), j = t * 16 + mfma16d_col(lane);
            if (c < k && j < d) red[k + c * d + j] += mean[t][reg];
          }
#pragma unroll
        for (int j = 0; j < K; ++j) {
          int p = 0;
#pragma unroll
          for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = ti; tj < NT; ++tj, ++p)
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int fa = ti * 16 + mfma16d_row(lane, reg), fb = tj * 16 + mfma16d_col(lane);
                if (fa <= fb && fb < d) red[k + k * d + j * tri + fa * d - fa * (fa - 1) / 2 + (fb - fa)] += S[j][p][reg];
              }
        }
      }
      __syncthreads();
    }
    double* out = a.partials + (int64_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
  }
}

// f(kernel) for the instantiation of (TX, NT, k): K = k in a STEP pass
template <typename TX, int NT, int K = 2, typename F>
void with_gmm_k(int k, F&& f) {
  if constexpr (gmm_in_range(16 * NT, K)) {
    if (k == K) return f(gmm_em_f64_kernel<TX, NT, K, GMM_STEP>);
    return with_gmm_k<TX, NT, K + 1>(k, f);
  }
}

template <typename TX, typename F>
void with_gmm_tx(int NT, int k, int mode, F&& f) {
  if (mode == GMM_ASSIGN) return NT == 1 ? f(gmm_em_f64_kernel<TX, 1, 0, GMM_ASSIGN>) : f(gmm_em_f64_kernel<TX, 2, 0, GMM_ASSIGN>);
  return NT == 1 ? with_gmm_k<TX, 1>(k, f) : with_gmm_k<TX, 2>(k, f);
}

template <typename F>
void with_gmm_kernel(int xdt, int d, int k, int mode, F&& f) {
  if (d < 1 || d > kGmmMaxD) throw std::invalid_argument("gmm: d must be in [1, 32]");
  if (!gmm_in_range(d, k)) throw std::invalid_argument("gmm: k must be in [2, 16] at d <= 16 and in [2, 8] at d <= 32");
  if (mode != GMM_STEP && mode != GMM_ASSIGN) throw std::invalid_argument("gmm: mode must be STEP (0) or ASSIGN (1)");
  if (xdt == DT_F64) return with_gmm_tx<double>((d + 15) / 16, k, mode, f);
  if (xdt == DT_F32) return with_gmm_tx<float>((d + 15) / 16, k, mode, f);
  throw std::invalid_argument("gmm: features must be f32 or f64");
}

// the kernel may use more dynamic LDS than the default limit of a launch
template <typename Kern>
size_t gmm_lds(Kern kern, int d, int k) {
  const size_t lds = gmm_lds_bytes((d + 15) / 16, k);
  DQ_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return lds;
}

}  // namespace

int gmm_blocks(int d, int k, int64_t n, int xdt, int mode) {
  int nb = 1;
  with_gmm_kernel(xdt, d, k, mode, [&](auto kern) { nb = staged_f64_blocks(kern, gmm_lds(kern, d, k), n); });
  return nb;
}

void gmm_pass(GramArgs a, const double* params, int k, int mode, int32_t* assign, double* prob, double* logp,
              int blocks, hipStream_t st) {
  a.ydt = DT_F64;  // (no label: the shared plan checks the code only)
  staged_f64_plan(a, blocks, "gmm");
  if (a.X == nullptr || params == nullptr) throw std::invalid_argument("gmm: null operand");
  if (mode == GMM_STEP && a.partials == nullptr) throw std::invalid_argument("gmm: a STEP pass needs partials");
  if (mode == GMM_ASSIGN && (assign == nullptr || prob == nullptr))
    throw std::invalid_argument("gmm: an ASSIGN pass needs assign and prob");
  const GmmArgs g{params, k, assign, prob, logp};
  with_gmm_kernel(a.xdt, a.d, k, mode, [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), gmm_lds(kern, a.d, k), st, a, g);
  });
  DQ_HIP_CHECK(hipGetLastError());
}

void gmm_reduce(const double* partials, int blocks, int k, int d, double* stats, hipStream_t st) {
  slab_sum(partials, blocks, gmm_stats_size(k, d), stats, st);
}

}  // namespace dq4ml
