// K5k: one Lloyd iteration of k-means as ONE kernel over feature-major X[d, n]: nothing of size
// n x k is written, and X comes from HBM once (tiles of d > 16 are staged a second time, see Sums).
//
// Work split: the staged f64 plan of gram_slab.h section 5 (kBlock = 256, a wave keeps one
// contiguous range of 64-row supersteps, a cooperative stage for the full ones, a guarded
// zero-filling stage for the ragged last one).  Rows that are dead or >= n are selected to zero,
// never multiplied.
//
// Centres: the k x d centres (padded with zero features to 16 KT x 16 NT, row stride 16 NT + 1 so
// the 16 centres of an A operand fall into different banks) and the bias 0.5 |c|^2 per centre
// (+inf for the pad centres, which therefore never win) sit in LDS behind the loop's area for the
// whole kernel, loaded once per block from the buffer that kmeans_update_kernel writes.
//
// Distances: score(row, centre) = 0.5 |c|^2 - x . c.  Per staged 16-feature tile and k-step of 4
// features, v_mfma_f64_16x16x4f64 with A = 16 centres x 4 features (LDS centres) and B = 4 features
// x 16 rows (the staged tile, lane = row) accumulates the 16 x 16 dot products of every (centre
// tile, row tile): KT x 4 accumulators per superstep.  The feature tile is the outer loop because
// a wave stages one tile at a time, so all KT x 4 accumulators are live until the last tile.  Each
// lane then reduces the (score, index) pairs of its 4 KT accumulator rows, and the four lane groups
// combine with __shfl_xor 16 / 32.  Pairs compare as (score, index), so ties go to the lowest
// centre index whatever the order of the reduction.  Every lane group ends with the result of all
// four row tiles; lane 16 q + f keeps row tile q's, which is row `lane` of the superstep -- the
// same lane that summed |x|^2 from the staged tile (lane = row, as glm_irls.hip forms eta).
// Row cost = max(0, |x|^2 + 2 score).
//
// Sums (KM_STEP): the 64 assignments go to the wave's LDS, and the centre sums are a second MFMA:
// A = one-hot (assign[row 16 q + e] == centre 16 ct + f), B = x(feature 16 t + f, row 16 q + e) read
// from the staged tile, into KT x NT accumulators that live across the supersteps.  The one-hot
// products are exact and the order is fixed.  Counts are integer compares beside the one-hot (a
// lane counts its 16 rows for its centre; the lane groups are summed at the end), the cost a
// per-lane f64 sum closed by the fixed-order wave reduction.
//
// What deviates from the first plan, and why:
// * The Gram loops' x[NT][16] registers are not kept through the distance phase.  With them,
//   KT x 4 distance accumulators, KT x NT sums and the compiler's hoisting of the loop-invariant
//   centre operands, every <*, NT >= 3, KT >= 3> instantiation spilled (up to 1232 bytes of scratch
//   per lane at <4, 4>).  Instead the sums read their B operand from the staged tile: the last tile
//   of the distance phase is still in LDS, and tiles NT-2 .. 0 are staged again (d <= 16: no second
//   stage; d = 64: three of four tiles, re-read right after their first use).  The distance loops
//   over the tiles and k-steps are real loops (#pragma unroll 1) to keep the centre operands from
//   being hoisted, and f64 tiles are staged in two batches of 8 features.  Scratch is 0 in all 64
//   instantiations; profiles/kmeans.md lists their registers.
// * Counts are integer adds, not a ones column: no extra MFMA and no pad feature needed at d = 64.
//
// Slabs: one partial per block, [k d sums (centre-major), k counts, cost, live rows], folded over
// the waves in order in LDS (the loop's area, dead by then), reduced over the blocks in block order
// by slab_sum (gram.h; sum_slabs_kernel of rowops.hip walks the columns serially in one block,
// which suits 8 columns, not 4162).  Plain launches, no atomics: bit-identical run to run.
#include "kmeans.h"

#include <climits>
#include <cmath>

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

struct KmArgs {
  const double* cen;    // [k * d centres, k half squared norms]
  const double* state;  // [kKMeansState] (KM_STEP) or null
  int k;
  int32_t* assign;      // KM_ASSIGN: [n]
  double* cost;         // KM_ASSIGN: [n] or null
};

// doubles per LDS centre row
constexpr int km_ldc(int NT) { return 16 * NT + 1; }
// LDS behind the loop's area: centres + bias
constexpr size_t km_extra(int NT, int KT) { return (size_t)(16 * KT * km_ldc(NT) + 16 * KT) * sizeof(double); }
// the block reduction's slab aliases the loop's area
static_assert((size_t)kmeans_stats_size(kKMeansMaxK, kKMeansMaxD) * sizeof(double) <= kTallF64LoopBytes,
              "the k-means slab must fit the staged loop's LDS");

// (score, index) pairs: the smaller score, then the smaller index
__device__ __forceinline__ void km_take(double& b, int& bi, double s, int c) {
  if (s < b || (s == b && c < bi)) {
    b = s;
    bi = c;
  }
}

// a.nsuper = supersteps (ceil(n / 64)), a.spw = supersteps per wave; a.partials = [gridDim.x][P].
// LDS: the tall f64 loop's (row scalars + one staged tile per wave), then centres and bias.
template <typename TX, int NT, int KT, int MODE>
__global__ __launch_bounds__(kBlock) void kmeans_lloyd_f64_kernel(GramArgs a, KmArgs g) {
  constexpr bool kStep = MODE == KM_STEP;
  constexpr int kLdc = km_ldc(NT);
  if (kStep && g.state[1] != 0.0) return;  // the fit is done: the slabs stay as they are
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  int* ai = reinterpret_cast<int*>(reinterpret_cast<double*>(smem) + wave * 128);  // the superstep's assignments
  double* xs = reinterpret_cast<double*>(smem) + kWavesPerBlock * 128 + wave * (16 * kStageLd);
  double* cl = reinterpret_cast<double*>(smem) + kTallF64LoopBytes / sizeof(double);  // [16 KT][kLdc]
  double* cb = cl + 16 * KT * kLdc;                                                   // [16 KT]
  double* red = reinterpret_cast<double*>(smem);  // block reduction: aliases the loop's area

  const int d = a.d, k = g.k;
  for (int i = threadIdx.x; i < 16 * KT * 16 * NT; i += kBlock) {
    const int c = i / (16 * NT), j = i % (16 * NT);
    cl[c * kLdc + j] = (c < k && j < d) ? g.cen[c * d + j] : 0.0;
  }
  for (int c = threadIdx.x; c < 16 * KT; c += kBlock) cb[c] = c < k ? g.cen[k * d + c] : HUGE_VAL;
  __syncthreads();

  f64x4 sums[kStep ? KT : 1][kStep ? NT : 1];
  int cnt[kStep ? KT : 1];
  if constexpr (kStep) {
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      cnt[ct] = 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) sums[ct][t] = f64x4{};
    }
  }
  double cost_acc = 0.0, live_acc = 0.0;

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
    f64x4 dot[KT][4];
#pragma unroll
    for (int ct = 0; ct < KT; ++ct)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) dot[ct][rt] = f64x4{};
    double xx = 0.0;
    // (a real loop over the tiles: unrolled, the compiler hoists the loop-invariant centre operands
    // of every tile out of the superstep loop, 8 KT NT registers that the accumulators need)
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      __builtin_amdgcn_wave_barrier();
      if (s < nfull) stage_tile_batched<TX>(X, a.ld, d, t * 16, r0, lane, xs);
      else stage_tile_guarded<TX>(X, a.ld, d, t * 16, r0, a.n, lane, xs);
      __builtin_amdgcn_wave_barrier();
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {  // lane = row: one bank per lane
        const double v = xs[j * kStageLd + lane];
        xx += v * v;
      }
      // dot[ct][rt] += centres(16 ct + i, 16 t + 4 ks + kk) * x(16 t + 4 ks + kk, row 16 rt + j)
#pragma unroll 1
      for (int ks = 0; ks < 4; ++ks) {
        double b[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) b[rt] = xs[(4 * ks + q) * kStageLd + 16 * rt + f];
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) {
          const double av = cl[(ct * 16 + f) * kLdc + 16 * t + 4 * ks + q];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
            dot[ct][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[rt], dot[ct][rt], 0, 0, 0);
        }
      }
    }
    // nearest centre of row 16 rt + f among the lane's centres 16 ct + q + 4 reg, then over the
    // lane groups (dead rows: their scores may be NaN and are not used)
    double best = HUGE_VAL;
    int bidx = INT_MAX;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      double b = HUGE_VAL;
      int bi = INT_MAX;
#pragma unroll
      for (int ct = 0; ct < KT; ++ct)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int c = ct * 16 + mfma16d_row(lane, reg);
          km_take(b, bi, cb[c] - dot[ct][rt][reg], c);
        }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const double ob = __shfl_xor(b, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        km_take(b, bi, ob, oi);
      }
      if (q == rt) {  // row 16 q + f = lane
        best = b;
        bidx = bi;
      }
    }
    const double cost = live ? fmax(0.0, xx + 2.0 * best) : 0.0;
    const int asg = live ? bidx : -1;
    if constexpr (!kStep) {
      if (r < a.n) {
        g.assign[r] = asg;
        if (g.cost != nullptr) g.cost[r] = cost;
      }
    } else {
      cost_acc += cost;
      live_acc += live ? 1.0 : 0.0;
      ai[lane] = asg;
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
        const f64x2* src = reinterpret_cast<const f64x2*>(xs + f * kStageLd + 16 * q);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          // dead rows: select, never multiply -- their features may be NaN
          const int as = ai[16 * q + e];  // (read where it is used: 16 registers <double, 4, 4> lacks)
          const double xv = as >= 0 ? src[e >> 1][e & 1] : 0.0;
#pragma unroll
          for (int ct = 0; ct < KT; ++ct) {
            const bool hit = as == ct * 16 + f;
            if (tt == 0) cnt[ct] += hit ? 1 : 0;
            sums[ct][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(hit ? 1.0 : 0.0, xv, sums[ct][t], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  if constexpr (kStep) {
    // block reduction over the waves in order + slab store
    const int P = kmeans_stats_size(k, d);
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
    cost_acc = wave_sum_f64(cost_acc);
    live_acc = wave_sum_f64(live_acc);
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      cnt[ct] += __shfl_xor(cnt[ct], 16, 64);
      cnt[ct] += __shfl_xor(cnt[ct], 32, 64);
    }
    __syncthreads();
    for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
      if (wave == wvi) {
        if (lane == 0) {
          red[k * d + k] += cost_acc;
          red[k * d + k + 1] += live_acc;
        }
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) {
          if (q == 0 && ct * 16 + f < k) red[k * d + ct * 16 + f] += (double)cnt[ct];
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int c = ct * 16 + mfma16d_row(lane, reg), j = t * 16 + mfma16d_col(lane);
              if (c < k && j < d) red[c * d + j] += sums[ct][t][reg];
            }
        }
      }
      __syncthreads();
    }
    double* out = a.partials + (int64_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
  }
}

// One block, one thread per centre.
__global__ __launch_bounds__(kKMeansMaxK) void kmeans_update_kernel(const double* __restrict__ stats, int k, int d,
                                                                    double tol2, double* cen, double* state) {
  if (state[1] != 0.0) return;
  __shared__ double mv[kKMeansMaxK];
  const int c = threadIdx.x;
  if (c < k) {
    const double n = stats[k * d + c];
    double moved = 0.0, hn = 0.0;
    for (int j = 0; j < d; ++j) {
      const double old = cen[c * d + j];
      const double nw = n > 0.0 ? stats[c * d + j] / n : old;
      moved += (nw - old) * (nw - old);
      hn += nw * nw;
      cen[c * d + j] = nw;
    }
    cen[k * d + c] = 0.5 * hn;
    mv[c] = moved;
  }
  __syncthreads();
  if (c == 0) {
    double mx = 0.0;
    for (int i = 0; i < k; ++i) mx = fmax(mx, mv[i]);
    state[0] += 1.0;
    state[1] = mx <= tol2 ? 1.0 : 0.0;
    state[2] = stats[k * d + k];
    state[3] = mx;
  }
}

template <typename TX, int NT, int MODE, typename F>
void with_km_kt(int KT, F&& f) {
  switch (KT) {
    case 1: return f(kmeans_lloyd_f64_kernel<TX, NT, 1, MODE>);
    case 2: return f(kmeans_lloyd_f64_kernel<TX, NT, 2, MODE>);
    case 3: return f(kmeans_lloyd_f64_kernel<TX, NT, 3, MODE>);
    default: return f(kmeans_lloyd_f64_kernel<TX, NT, 4, MODE>);
  }
}

template <typename TX, int MODE, typename F>
void with_km_nt(int NT, int KT, F&& f) {
  switch (NT) {
    case 1: return with_km_kt<TX, 1, MODE>(KT, f);
    case 2: return with_km_kt<TX, 2, MODE>(KT, f);
    case 3: return with_km_kt<TX, 3, MODE>(KT, f);
    default: return with_km_kt<TX, 4, MODE>(KT, f);
  }
}

template <typename F>
void with_km_kernel(int xdt, int d, int k, int mode, F&& f) {
  if (d < 1 || d > kKMeansMaxD) throw std::invalid_argument("kmeans: d must be in [1, 64]");
  if (k < 2 || k > kKMeansMaxK) throw std::invalid_argument("kmeans: k must be in [2, 64]");
  if (mode != KM_STEP && mode != KM_ASSIGN) throw std::invalid_argument("kmeans: mode must be STEP (0) or ASSIGN (1)");
  const int NT = (d + 15) / 16, KT = (k + 15) / 16;
  if (xdt == DT_F64)
    return mode == KM_STEP ? with_km_nt<double, KM_STEP>(NT, KT, f) : with_km_nt<double, KM_ASSIGN>(NT, KT, f);
  if (xdt == DT_F32)
    return mode == KM_STEP ? with_km_nt<float, KM_STEP>(NT, KT, f) : with_km_nt<float, KM_ASSIGN>(NT, KT, f);
  throw std::invalid_argument("kmeans: features must be f32 or f64");
}

size_t km_lds(int d, int k) { return kTallF64LoopBytes + km_extra((d + 15) / 16, (k + 15) / 16); }

}  // namespace

int kmeans_blocks(int d, int k, int64_t n, int xdt, int mode) {
  int nb = 1;
  with_km_kernel(xdt, d, k, mode, [&](auto kern) { nb = staged_f64_blocks(kern, km_lds(d, k), n); });
  return nb;
}

void kmeans_pass(GramArgs a, const double* centers, int k, const double* state, int mode, int32_t* assign,
                 double* cost, int blocks, hipStream_t st) {
  a.ydt = DT_F64;  // (no label: the shared plan checks the code only)
  staged_f64_plan(a, blocks, "kmeans");
  if (a.X == nullptr || centers == nullptr) throw std::invalid_argument("kmeans: null operand");
  if (mode == KM_STEP && (a.partials == nullptr || state == nullptr))
    throw std::invalid_argument("kmeans: a STEP pass needs partials and state");
  if (mode == KM_ASSIGN && assign == nullptr) throw std::invalid_argument("kmeans: an ASSIGN pass needs assign");
  const KmArgs g{centers, state, k, assign, cost};
  with_km_kernel(a.xdt, a.d, k, mode, [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), km_lds(a.d, k), st, a, g);
  });
  DQ_HIP_CHECK(hipGetLastError());
}

namespace {
__global__ __launch_bounds__(256) void slab_sum_kernel(const double* __restrict__ partials, int nslab, int P,
                                                       double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  double s = 0.0;
  for (int b = 0; b < nslab; ++b) s += partials[(int64_t)b * P + i];
  out[i] = s;
}
}  // namespace

void slab_sum(const double* partials, int nslab, int P, double* out, hipStream_t st) {
  if (partials == nullptr || out == nullptr || nslab < 1 || P < 1) throw std::invalid_argument("slab_sum: bad operand");
  hipLaunchKernelGGL(slab_sum_kernel, dim3((P + 255) / 256), dim3(256), 0, st, partials, nslab, P, out);
  DQ_HIP_CHECK(hipGetLastError());
}

void kmeans_reduce(const double* partials, int blocks, int k, int d, double* stats, hipStream_t st) {
  slab_sum(partials, blocks, kmeans_stats_size(k, d), stats, st);
}

void kmeans_update(const double* stats, int k, int d, double tol, double* centers, double* state, hipStream_t st) {
  if (d < 1 || d > kKMeansMaxD || k < 2 || k > kKMeansMaxK)
    throw std::invalid_argument("kmeans_update: d must be in [1, 64] and k in [2, 64]");
  if (stats == nullptr || centers == nullptr || state == nullptr) throw std::invalid_argument("kmeans_update: null operand");
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(kKMeansMaxK), 0, st, stats, k, d, tol * tol, centers, state);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
