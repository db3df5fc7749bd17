// K5l: one evaluation of the logistic loss and its gradient as ONE kernel over feature-major
// X[d, n]: nothing of size n x K is written, and X comes from HBM once (tiles of d > 16 are staged a
// second time, see Gradient).  The same kernels, in LR_PREDICT mode, write a fitted model's raw /
// probability / prediction columns.
//
// Work split: the staged f64 plan of gram_slab.h section 5 (kBlock = 256, a wave keeps one
// contiguous range of 64-row supersteps, stage_tile_batched for the full ones, stage_tile_guarded
// for the ragged last one).  Rows that are dead, >= n or carry a bad label are selected to zero,
// never multiplied: their features, labels and weights may be NaN.
//
// ---- multinomial, 2 <= K <= 64: <TX, NT, KT, MODE>, KT = ceil(K / 16) -------------------------
// Coefficients: the K x d coefficients (zero padded to 16 KT x 16 NT, row stride 16 NT + 1) and
// the intercepts sit in LDS behind the loop's area for the whole kernel.  The pad classes carry the
// intercept -inf (a bias, not a mask): their margin is -inf for every live row, so they never win
// the max and add exp(-inf) = 0 to the sum, and their multiplier is exactly 0.
//
// Margins: D[row][class] by v_mfma_f64_16x16x4f64 with A = the staged tile (16 rows x 4 features,
// xs[(4 ks + q) * kStageLd + 16 rt + f]) and B = the LDS coefficients (4 features x 16 classes),
// the accumulators starting at the class's intercept.  Lane (f, q) then holds class 16 ct + f of
// rows 16 rt + q + 4 reg -- the transpose of kmeans.hip's scores.
//
// Softmax: a row's classes lie in the lane's own KT accumulators and across the 16 lanes of its
// lane group: max and sum of exp are in-lane over ct, then __shfl_xor 1, 2, 4, 8.  The max is
// subtracted before exp.  The row's weight and class come from the wave's row-scalar area (staged
// once per superstep by lane = row, which also counts live rows, bad labels and sum w).  The
// multiplier w (p_c - [y == c]) overwrites the margin in place; the lane that owns class y takes
// the row loss -w (m_y - max - log sum).
//
// Gradient: G[class][feature] += mult[class][row] x[feature][row] by a second MFMA whose A operand
// is the lane's own accumulator register: k-step (rt, reg) covers rows 16 rt + q + 4 reg, and lane
// (f, q) supplies A[class f][k = q] from m[ct][rt][reg] with no move; B = xs[f * kStageLd + 16 rt
// + q + 4 reg] (selected to zero for rows that do not count).  KT x NT accumulators live across the
// supersteps.  As in kmeans.hip the last tile of the margin phase is still staged and tiles
// NT-2 .. 0 are staged again.  The intercept gradient is the in-lane sum of the multipliers; the
// four lane groups are combined once at the end.
//
// LR_PREDICT: the margins go through the wave's staged-tile area (dead after the margin phase) one
// class tile at a time, so that lane = row writes raw[c][row] in 512-byte runs and keeps the first
// maximum; the probabilities of the shared softmax follow the same way.
//
// ---- binomial: <TX, NT, MODE> ----------------------------------------------------------------
// The margin is a per-lane dot product (lane = row) of the staged tile against the coefficients
// read as LDS broadcasts, as glm_irls.hip forms eta.  One exp per row: t = exp(-|m|) gives p =
// 1 / (1 + t) or t / (1 + t) and log(1 + exp(m)) = max(m, 0) + log1p(t), both overflow-safe.  The
// gradient X^T mult is an MFMA with A = the staged tile (16 features x 4 rows) and B = the
// multipliers from the row-scalar area, broadcast over the 16 columns; column 0 is kept.
//
// Slabs (LR_GRAD): one partial per block, [K (d + 1) gradient, loss, sum w, live rows, bad labels]
// (binomial: K = 1), folded over the waves in order in LDS (the loop's area, dead by then), summed
// over the blocks in block order by slab_sum.  Plain launches, no atomics: bit-identical run to run.
//
// Registers, and what deviates from the first plan: as in kmeans.hip the margin loops over the
// tiles and k-steps are real loops (#pragma unroll 1), or the compiler hoists the loop-invariant
// coefficient operands out of the superstep loop, and f64 tiles are staged in two batches.  That was
// not enough: with all 4 row tiles of a superstep in flight (16 KT margin registers of f64x4 beside
// the 4 KT NT gradient accumulators) every GRAD instantiation with KT = 4 and most with KT NT >= 9
// spilled, up to 708 bytes of scratch per lane at <float, 4, 4>.  Those instantiations take the
// superstep in parts of RT row tiles -- margins, softmax and gradient of rows [16 RT h, 16 RT (h +
// 1)) before the next part -- with RT = 2 for KT = 4 or KT NT = 9 and RT = 1 for KT NT >= 12.  A part
// stages every tile again (from L2: the superstep's rows were just read), so such a pass stages
// 4 / RT times as often; the sums and their order per accumulator are the same.  Scratch is 0 in
// all 80 instantiations, but not every spill: 14 GRAD instantiations move 4 to 14 VGPRs through
// AGPRs, and SGPRs are parked in VGPR lanes (up to 477 at <float, 4, 4>); profiles/logreg.md lists
// registers and spills of each.  Scheduling barriers between
// the softmax rows or the gradient tiles did not help and are not in the code.
#include "logreg.h"

#include <cmath>

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

struct LrArgs {
  const double* coef;  // [K][d + 1]
  int K;
  double threshold;    // binomial LR_PREDICT
  double* raw;         // LR_PREDICT: [classes][n]
  double* prob;        // LR_PREDICT: [classes][n]
  double* pred;        // LR_PREDICT: [n]
};

// doubles per LDS coefficient row
constexpr int lr_ldc(int NT) { return 16 * NT + 1; }
// LDS behind the loop's area: coefficients + intercepts
constexpr size_t lr_extra(int NT, int KT) { return (size_t)(16 * KT * lr_ldc(NT) + 16 * KT) * sizeof(double); }
// the block reduction's slab aliases the loop's area
static_assert((size_t)logreg_stats_size(kLogregMaxK, kLogregMaxD) * sizeof(double) <= kTallF64LoopBytes,
              "the logistic slab must fit the staged loop's LDS");

// What row r adds to a GRAD pass, by lane = row: y = -1 and w = 0 unless the row counts.
struct LrRow {
  double w;
  int y;
  bool live, bad;
};

__device__ __forceinline__ LrRow lr_row(const GramArgs& a, int64_t r, int classes) {
  LrRow o{0.0, -1, false, false};
  if (r < a.n && (a.sel ? a.sel[r] != 0 : true)) {
    o.live = true;
    const double y = load_f32_f64(a.y, a.ydt, r);
    if (y >= 0.0 && y < (double)classes && y == floor(y)) {  // (NaN fails the first compare)
      o.y = (int)y;
      o.w = a.w ? load_f32_f64(a.w, a.wdt, r) : 1.0;
    } else {
      o.bad = true;
    }
  }
  return o;
}

// The lane's accumulators of class tile ct (class 16 ct + f of rows 16 rt + q + 4 reg) to
// dst[class][row] through the wave's tile area: lane = row stores 16 classes in 512-byte runs.
// best / bidx: the first maximum so far (raw only).
template <bool ARGMAX>
__device__ __forceinline__ void lr_put_tile(const f64x4 (&m)[4], int ct, int K, int64_t n, int64_t r, bool live,
                                            int lane, double* xs, double* dst, double& best, int& bidx) {
  const int f = lane & 15, q = lane >> 4;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) xs[f * kStageLd + 16 * rt + q + 4 * reg] = m[rt][reg];
  __builtin_amdgcn_wave_barrier();
  if (r < n) {
    for (int cc = 0; cc < 16 && 16 * ct + cc < K; ++cc) {
      const double v = xs[cc * kStageLd + lane];
      if (ARGMAX && v > best) {
        best = v;
        bidx = 16 * ct + cc;
      }
      dst[(int64_t)(16 * ct + cc) * n + r] = live ? v : NAN;
    }
  }
}

// a.nsuper = supersteps (ceil(n / 64)), a.spw = supersteps per wave; a.partials = [gridDim.x][P].
// LDS: the tall f64 loop's (row scalars + one staged tile per wave), then coefficients and intercepts.
template <typename TX, int NT, int KT, int MODE>
__global__ __launch_bounds__(kBlock) void logreg_multi_f64_kernel(GramArgs a, LrArgs g) {
  constexpr bool kGrad = MODE == LR_GRAD;
  constexpr int kLdc = lr_ldc(NT);
  constexpr int RT = !kGrad ? 4 : (KT * NT >= 12 ? 1 : (KT == 4 || KT * NT == 9 ? 2 : 4));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  double* rs = reinterpret_cast<double*>(smem) + wave * 128;  // the superstep's [w(64), class(64)]
  double* xs = reinterpret_cast<double*>(smem) + kWavesPerBlock * 128 + wave * (16 * kStageLd);
  double* cl = reinterpret_cast<double*>(smem) + kTallF64LoopBytes / sizeof(double);  // [16 KT][kLdc]
  double* cb = cl + 16 * KT * kLdc;                                                   // [16 KT]
  double* red = reinterpret_cast<double*>(smem);  // block reduction: aliases the loop's area

  const int d = a.d, K = g.K;
  for (int i = threadIdx.x; i < 16 * KT * 16 * NT; i += kBlock) {
    const int c = i / (16 * NT), j = i % (16 * NT);
    cl[c * kLdc + j] = (c < K && j < d) ? g.coef[c * (d + 1) + j] : 0.0;
  }
  for (int c = threadIdx.x; c < 16 * KT; c += kBlock) cb[c] = c < K ? g.coef[c * (d + 1) + d] : -HUGE_VAL;
  __syncthreads();

  f64x4 G[kGrad ? KT : 1][kGrad ? NT : 1];
  double gi[kGrad ? KT : 1];
  if constexpr (kGrad) {
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      gi[ct] = 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) G[ct][t] = f64x4{};
    }
  }
  double loss_acc = 0.0, w_acc = 0.0, live_acc = 0.0, bad_acc = 0.0;

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
    [[maybe_unused]] bool live;
    if constexpr (kGrad) {
      const LrRow row = lr_row(a, r, K);
      live = row.live;
      w_acc += row.w;
      live_acc += row.live ? 1.0 : 0.0;
      bad_acc += row.bad ? 1.0 : 0.0;
      rs[lane] = row.w;
      rs[64 + lane] = (double)row.y;
    } else {
      live = r < a.n && (a.sel ? a.sel[r] != 0 : true);
    }
    // RT row tiles at a time: all 4, or 2 and 2 where 4 KT margin accumulators beside the KT NT
    // gradient accumulators spill (see Registers); rb = the first row of the part
#pragma unroll 1
    for (int h = 0; h < 4 / RT; ++h) {
      const int rb = 16 * RT * h;
      f64x4 m[KT][RT];
#pragma unroll
      for (int ct = 0; ct < KT; ++ct) {
        const double b = cb[ct * 16 + f];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) m[ct][rt] = f64x4{b, b, b, b};
      }
      // (real loops over the tiles and k-steps: unrolled, the compiler hoists the loop-invariant
      // coefficient operands out of the superstep loop, 8 KT NT registers that the accumulators need)
#pragma unroll 1
      for (int t = 0; t < NT; ++t) {
        if (NT > 1 || h == 0) {  // (one tile: the second half finds it staged)
          __builtin_amdgcn_wave_barrier();
          if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
          else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
          __builtin_amdgcn_wave_barrier();
        }
        // m[ct][rt] += x(row 16 rt + i, 16 t + 4 ks + kk) * coef(16 ct + j, 16 t + 4 ks + kk)
#pragma unroll 1
        for (int ks = 0; ks < 4; ++ks) {
          double av[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) av[rt] = xs[(4 * ks + q) * kStageLd + rb + 16 * rt + f];
#pragma unroll
          for (int ct = 0; ct < KT; ++ct) {
            const double bv = cl[(ct * 16 + f) * kLdc + 16 * t + 4 * ks + q];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
              m[ct][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt], bv, m[ct][rt], 0, 0, 0);
          }
        }
      }
      if constexpr (!kGrad) {
        double best = -HUGE_VAL;
        int bidx = 0;
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) lr_put_tile<true>(m[ct], ct, K, a.n, r, live, lane, xs, g.raw, best, bidx);
        if (r < a.n) g.pred[r] = live ? (double)bidx : -1.0;
      }
      // softmax of row 16 rt + q + 4 reg over the lane's KT classes and the lane group's 16 lanes
      // (rows that do not count: their margins may be NaN and are not used)
      unsigned cnt = 0;  // bit 4 rt + reg: the row counts
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          double mx = m[0][rt][reg];
#pragma unroll
          for (int ct = 1; ct < KT; ++ct) mx = fmax(mx, m[ct][rt][reg]);
#pragma unroll
          for (int o = 1; o <= 8; o <<= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
          double e[KT], sm = 0.0;
#pragma unroll
          for (int ct = 0; ct < KT; ++ct) {
            e[ct] = exp(m[ct][rt][reg] - mx);
            sm += e[ct];
          }
#pragma unroll
          for (int o = 1; o <= 8; o <<= 1) sm += __shfl_xor(sm, o, 64);
          const double inv = 1.0 / sm;
          if constexpr (kGrad) {
            const int R = rb + 16 * rt + q + 4 * reg;
            const double w = rs[R];
            const int y = (int)rs[64 + R];
            const bool on = y >= 0;
            cnt |= (on ? 1u : 0u) << (4 * rt + reg);
#pragma unroll
            for (int ct = 0; ct < KT; ++ct) {
              const bool mine = y == ct * 16 + f;
              if (mine) loss_acc -= w * (m[ct][rt][reg] - mx - log(sm));
              const double mult = on ? w * (e[ct] * inv - (mine ? 1.0 : 0.0)) : 0.0;
              m[ct][rt][reg] = mult;
              gi[ct] += mult;
            }
          } else {
#pragma unroll
            for (int ct = 0; ct < KT; ++ct) m[ct][rt][reg] = e[ct] * inv;
          }
        }
      if constexpr (!kGrad) {
        double best = 0.0;
        int bidx = 0;
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) lr_put_tile<false>(m[ct], ct, K, a.n, r, live, lane, xs, g.prob, best, bidx);
      } else {
        // tiles in reverse: the last one is still staged, the others are staged again
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          const int t = NT - 1 - tt;
          if (tt > 0) {
            __builtin_amdgcn_wave_barrier();
            if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
            else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
            __builtin_amdgcn_wave_barrier();
          }
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              // rows that do not count: select, never multiply -- their features may be NaN
              const double xv = (cnt >> (4 * rt + reg)) & 1u ? xs[f * kStageLd + rb + 16 * rt + q + 4 * reg] : 0.0;
#pragma unroll
              for (int ct = 0; ct < KT; ++ct)
                G[ct][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[ct][rt][reg], xv, G[ct][t], 0, 0, 0);
            }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (kGrad) {
    // block reduction over the waves in order + slab store
    const int P = logreg_stats_size(K, d);
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
    loss_acc = wave_sum_f64(loss_acc);
    w_acc = wave_sum_f64(w_acc);
    live_acc = wave_sum_f64(live_acc);
    bad_acc = wave_sum_f64(bad_acc);
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      gi[ct] += __shfl_xor(gi[ct], 16, 64);
      gi[ct] += __shfl_xor(gi[ct], 32, 64);
    }
    __syncthreads();
    for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
      if (wave == wvi) {
        if (lane == 0) {
          red[K * (d + 1)] += loss_acc;
          red[K * (d + 1) + 1] += w_acc;
          red[K * (d + 1) + 2] += live_acc;
          red[K * (d + 1) + 3] += bad_acc;
        }
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) {
          if (q == 0 && ct * 16 + f < K) red[(ct * 16 + f) * (d + 1) + d] += gi[ct];
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int c = ct * 16 + mfma16d_row(lane, reg), j = t * 16 + mfma16d_col(lane);
              if (c < K && j < d) red[c * (d + 1) + j] += G[ct][t][reg];
            }
        }
      }
      __syncthreads();
    }
    double* out = a.partials + (int64_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
  }
}

// LDS: the tall f64 loop's, then coef[64] (zero padded) and the intercept.
template <typename TX, int NT, int MODE>
__global__ __launch_bounds__(kBlock) void logreg_binom_f64_kernel(GramArgs a, LrArgs g) {
  constexpr bool kGrad = MODE == LR_GRAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  double* rs = reinterpret_cast<double*>(smem) + wave * 128;  // the superstep's [mult(64), counts(64)]
  double* xs = reinterpret_cast<double*>(smem) + kWavesPerBlock * 128 + wave * (16 * kStageLd);
  double* bl = reinterpret_cast<double*>(smem) + kTallF64LoopBytes / sizeof(double);
  double* red = reinterpret_cast<double*>(smem);

  const int d = a.d;
  if (threadIdx.x < 65) {
    double v = 0.0;
    if (threadIdx.x < d || threadIdx.x == 64) v = g.coef[threadIdx.x < d ? threadIdx.x : d];
    bl[threadIdx.x] = v;
  }
  __syncthreads();

  f64x4 G[kGrad ? NT : 1];
#pragma unroll
  for (int t = 0; t < (kGrad ? NT : 1); ++t) G[t] = f64x4{};
  double gi = 0.0, loss_acc = 0.0, w_acc = 0.0, live_acc = 0.0, bad_acc = 0.0;

  const TX* X = reinterpret_cast<const TX*>(a.X);
  const int64_t nfull = a.n / 64;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  int64_t s0 = gw * a.spw;
  int64_t s1 = s0 + a.spw;
  if (s0 > a.nsuper) s0 = a.nsuper;
  if (s1 > a.nsuper) s1 = a.nsuper;

  for (int64_t s = s0; s < s1; ++s) {
    const int64_t r0 = s * 64;
    const int64_t r = r0 + lane;
    LrRow row{0.0, -1, false, false};
    if constexpr (kGrad) row = lr_row(a, r, 2);
    else row.live = r < a.n && (a.sel ? a.sel[r] != 0 : true);
    double eta = bl[64];
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      __builtin_amdgcn_wave_barrier();
      if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
      else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < 16; ++k) eta += xs[k * kStageLd + lane] * bl[t * 16 + k];  // lane = row: one bank per lane
    }
    // (rows that do not count: eta may be NaN and is not used)
    const double tn = exp(-fabs(eta));
    const double hi = 1.0 / (1.0 + tn), lo = tn / (1.0 + tn);
    const double p = eta >= 0.0 ? hi : lo;
    if constexpr (!kGrad) {
      if (r < a.n) {
        const bool lv = row.live;
        g.raw[r] = lv ? -eta : NAN;
        g.raw[a.n + r] = lv ? eta : NAN;
        g.prob[r] = lv ? (eta >= 0.0 ? lo : hi) : NAN;
        g.prob[a.n + r] = lv ? p : NAN;
        g.pred[r] = lv ? (p > g.threshold ? 1.0 : 0.0) : -1.0;
      }
    } else {
      const bool on = row.y >= 0;
      const double yv = (double)row.y;
      const double mult = on ? row.w * (p - yv) : 0.0;
      loss_acc += on ? row.w * (fmax(eta, 0.0) + log1p(tn) - yv * eta) : 0.0;
      gi += mult;
      w_acc += row.w;
      live_acc += row.live ? 1.0 : 0.0;
      bad_acc += row.bad ? 1.0 : 0.0;
      rs[lane] = mult;
      rs[64 + lane] = on ? 1.0 : 0.0;
      __builtin_amdgcn_wave_barrier();
      // tiles in reverse: the last one is still staged, the others are staged again
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int t = NT - 1 - tt;
        if (tt > 0) {
          __builtin_amdgcn_wave_barrier();
          if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
          else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
          __builtin_amdgcn_wave_barrier();
        }
        // G[feature 16 t + i][*] += x(16 t + i, row 16 q + e) * mult(row 16 q + e), k = q
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const double xv = rs[64 + 16 * q + e] != 0.0 ? xs[f * kStageLd + 16 * q + e] : 0.0;
          G[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, rs[16 * q + e], G[t], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (kGrad) {
    const int P = logreg_stats_size(1, d);
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
    gi = wave_sum_f64(gi);
    loss_acc = wave_sum_f64(loss_acc);
    w_acc = wave_sum_f64(w_acc);
    live_acc = wave_sum_f64(live_acc);
    bad_acc = wave_sum_f64(bad_acc);
    __syncthreads();
    for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
      if (wave == wvi) {
        if (lane == 0) {
          red[d] += gi;
          red[d + 1] += loss_acc;
          red[d + 2] += w_acc;
          red[d + 3] += live_acc;
          red[d + 4] += bad_acc;
        }
        if (mfma16d_col(lane) == 0) {  // (every column holds the same sums)
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int j = t * 16 + mfma16d_row(lane, reg);
              if (j < d) red[j] += G[t][reg];
            }
        }
      }
      __syncthreads();
    }
    double* out = a.partials + (int64_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
  }
}

template <typename TX, int NT, int MODE, typename F>
void with_lr_kt(int KT, F&& f) {
  switch (KT) {
    case 0: return f(logreg_binom_f64_kernel<TX, NT, MODE>);
    case 1: return f(logreg_multi_f64_kernel<TX, NT, 1, MODE>);
    case 2: return f(logreg_multi_f64_kernel<TX, NT, 2, MODE>);
    case 3: return f(logreg_multi_f64_kernel<TX, NT, 3, MODE>);
    default: return f(logreg_multi_f64_kernel<TX, NT, 4, MODE>);
  }
}

template <typename TX, int MODE, typename F>
void with_lr_nt(int NT, int KT, F&& f) {
  switch (NT) {
    case 1: return with_lr_kt<TX, 1, MODE>(KT, f);
    case 2: return with_lr_kt<TX, 2, MODE>(KT, f);
    case 3: return with_lr_kt<TX, 3, MODE>(KT, f);
    default: return with_lr_kt<TX, 4, MODE>(KT, f);
  }
}

// KT = 0 names the binomial kernel (K = 1)
template <typename F>
void with_lr_kernel(int xdt, int d, int K, int mode, F&& f) {
  if (d < 1 || d > kLogregMaxD) throw std::invalid_argument("logreg: d must be in [1, 64]");
  if (K < 1 || K > kLogregMaxK) throw std::invalid_argument("logreg: K must be 1 (binomial) or in [2, 64]");
  if (mode != LR_GRAD && mode != LR_PREDICT) throw std::invalid_argument("logreg: mode must be GRAD (0) or PREDICT (1)");
  const int NT = (d + 15) / 16, KT = K == 1 ? 0 : (K + 15) / 16;
  if (xdt == DT_F64)
    return mode == LR_GRAD ? with_lr_nt<double, LR_GRAD>(NT, KT, f) : with_lr_nt<double, LR_PREDICT>(NT, KT, f);
  if (xdt == DT_F32)
    return mode == LR_GRAD ? with_lr_nt<float, LR_GRAD>(NT, KT, f) : with_lr_nt<float, LR_PREDICT>(NT, KT, f);
  throw std::invalid_argument("logreg: features must be f32 or f64");
}

size_t lr_lds(int d, int K) {
  if (K == 1) return kTallF64LoopBytes + 65 * sizeof(double);
  return kTallF64LoopBytes + lr_extra((d + 15) / 16, (K + 15) / 16);
}

}  // namespace

int logreg_blocks(int d, int K, int64_t n, int xdt, int mode) {
  int nb = 1;
  with_lr_kernel(xdt, d, K, mode, [&](auto kern) { nb = staged_f64_blocks(kern, lr_lds(d, K), n); });
  return nb;
}

void logreg_pass(GramArgs a, const double* coef, int K, int mode, double threshold, double* raw, double* prob,
                 double* pred, int blocks, hipStream_t st) {
  if (mode == LR_PREDICT) a.ydt = DT_F64;  // (no label: the shared plan checks the code only)
  staged_f64_plan(a, blocks, "logreg");
  if (a.X == nullptr || coef == nullptr) throw std::invalid_argument("logreg: null operand");
  if (mode == LR_GRAD && (a.partials == nullptr || a.y == nullptr))
    throw std::invalid_argument("logreg: a GRAD pass needs partials and the label");
  if (mode == LR_GRAD && a.w != nullptr && a.wdt != DT_F64 && a.wdt != DT_F32)
    throw std::invalid_argument("logreg: weights must be f32 or f64");
  if (mode == LR_PREDICT && (raw == nullptr || prob == nullptr || pred == nullptr))
    throw std::invalid_argument("logreg: a PREDICT pass needs raw, prob and pred");
  const LrArgs g{coef, K, threshold, raw, prob, pred};
  with_lr_kernel(a.xdt, a.d, K, mode, [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), lr_lds(a.d, K), st, a, g);
  });
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
