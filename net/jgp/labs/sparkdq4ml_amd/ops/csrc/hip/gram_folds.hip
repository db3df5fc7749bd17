// Fold-partitioned WLS statistics: one pass over X -> one flat f64 statistics vector per
// cross-validation fold (models/tuning.py).
//
// The statistics are additive over rows, so k-fold cross-validation needs only the k per-fold
// vectors: train(f) = total - fold(f), and every validation metric is a closed form of fold(f).
//
// Fold rule (gram_folds.h): rows are grouped in granules of G rows, granule g hashes to a uint32,
// thresholds cut the uint32 range into k classes.  The one-pass kernel fixes G = 64 = one
// superstep of the staged f64 loop (gram_slab.h section 5; this kernel and glm_irls.hip's keep
// it), so a superstep's fold is wave-uniform: a wave keeps its contiguous superstep range and ONE
// accumulator set, and sweeps the range once per fold, loading only that fold's supersteps.
// Every row is read once; MFMA work, VGPRs and LDS are those of one plain pass of that loop; the
// extras are the hash (scalar values) and k block reductions + slab stores per block.  Slabs:
// partials[fold][block][P] in the f64 slab layout (gram_slab.h), so gram_reduce folds each fold's
// slabs unchanged, in fixed order (no atomics: bit-identical run to run).
#include "gram_folds.h"

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

// per-row scalars of row r (lane = row): liveness and label; a dead row's label is never loaded
struct RowVals {
  bool live;
  double y;
};

__device__ __forceinline__ RowVals row_vals(const GramArgs& a, int64_t r) {
  RowVals v{false, 0.0};
  if (r < a.n) {
    const bool live = a.sel ? (a.sel[r] != 0) : true;
    if (live) {
      v.live = true;
      v.y = a.ydt == DT_F64 ? reinterpret_cast<const double*>(a.y)[r] : (double)reinterpret_cast<const float*>(a.y)[r];
    }
  }
  return v;
}

// a.nsuper = granules (ceil(n / 64)), a.spw = granules per wave; a.partials = [k][gridDim.x][P]
template <typename TX, int NT>
__global__ __launch_bounds__(kBlock) void gram_folds_f64_kernel(GramArgs a, FoldRule fr) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  double* lw = reinterpret_cast<double*>(smem) + wave * 128;  // [live(64), y(64)]
  double* xs = reinterpret_cast<double*>(smem) + kWavesPerBlock * 128 + wave * (16 * kStageLd);
  double* red = reinterpret_cast<double*>(smem);  // block reduction: aliases the staging area
  constexpr int kChains = NT >= 2 ? 2 : 4;

  const TX* X = reinterpret_cast<const TX*>(a.X);
  const TX* fp[NT];
  bool fvalid[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int feat = t * 16 + f;
    fvalid[t] = feat < a.d;
    fp[t] = X + (int64_t)(fvalid[t] ? feat : 0) * a.ld + 16 * q;
  }
  const bool masked = a.sel != nullptr;
  const int64_t nfull = a.n / 64;  // granules below are whole supersteps; granule nfull is the n % 64 tail
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  int64_t s0 = gw * a.spw;
  int64_t s1 = s0 + a.spw;
  if (s0 > a.nsuper) s0 = a.nsuper;
  if (s1 > a.nsuper) s1 = a.nsuper;
  const int d = a.d;
  const int P = a.P;

  for (int fold = 0; fold < fr.k; ++fold) {
    f64x4 acc[NPAIR][kChains];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
#pragma unroll
      for (int c = 0; c < kChains; ++c) acc[p][c] = f64x4{};
    double cs[NT], ab[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cs[t] = ab[t] = 0.0;
    double cnt = 0.0, bs = 0.0, bbs = 0.0;

    for (int64_t s = s0; s < s1; ++s) {
      if (fold_of(fr, (uint64_t)s) != fold) continue;  // wave-uniform: s and the rule are scalar
      const int64_t r0 = s * 64;
      const RowVals rv = row_vals(a, r0 + lane);
      if (rv.live) {
        cnt += 1.0;
        bs += rv.y;
        bbs += rv.y * rv.y;
      }
      lw[lane] = rv.live ? 1.0 : 0.0;
      lw[64 + lane] = rv.y;  // 0 on dead rows
      __builtin_amdgcn_wave_barrier();
      const int64_t rows_left = a.n - (r0 + 16 * q);
      double lv[16], yv[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        lv[e] = lw[16 * q + e];
        yv[e] = lw[64 + 16 * q + e];
      }
      double x[NT][16];
      load_superstep_f64<TX, NT>(X, a.ld, d, s < nfull, r0, rows_left, fp, fvalid, lane, xs, x);
      if (masked) {
        // dead rows: select, never multiply -- their stored features may be NaN
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) x[t][e] = lv[e] != 0.0 ? x[t][e] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          cs[t] += x[t][e];
          ab[t] += x[t][e] * yv[e];
        }
      int p = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            acc[p][e % kChains] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[I][e], x[J][e], acc[p][e % kChains], 0, 0, 0);
      __builtin_amdgcn_wave_barrier();
    }

    // block reduction of this fold's sweep (the tall f64 kernel's, once per fold)
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) red[i] = 0.0;
    double sc[3] = {cnt, bs, bbs};
#pragma unroll
    for (int i = 0; i < 3; ++i) sc[i] = wave_sum_f64(sc[i]);
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
        if (lane == 0) {  // unit weights: count = wSum = wwSum
          red[0] += sc[0];
          red[1] += sc[0];
          red[2] += sc[0];
          red[3] += sc[1];
          red[4] += sc[2];
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
    // every (fold, block) slab is written, zeros included: partials is uninitialised memory
    double* out = a.partials + ((int64_t)fold * gridDim.x + blockIdx.x) * P;
    for (int i = threadIdx.x; i < P; i += kBlock) out[i] = red[i];
    __syncthreads();  // red is the next sweep's staging area
  }
}

__global__ __launch_bounds__(256) void fold_ids_kernel(int64_t n, int64_t granule, FoldRule fr, uint8_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride)
    out[r] = (uint8_t)fold_of(fr, (uint64_t)(r / granule));
}

template <typename F>
void with_folds_kernel(int xdt, int d, F&& f) {
  const int NT = (d + 15) / 16;
#define DQ_FOLDS_CASE(TX)                                     \
  switch (NT) {                                               \
    case 1: return f(gram_folds_f64_kernel<TX, 1>);           \
    case 2: return f(gram_folds_f64_kernel<TX, 2>);           \
    case 3: return f(gram_folds_f64_kernel<TX, 3>);           \
    default: return f(gram_folds_f64_kernel<TX, 4>);          \
  }
  if (xdt == DT_F64) { DQ_FOLDS_CASE(double) }
  if (xdt == DT_F32) { DQ_FOLDS_CASE(float) }
#undef DQ_FOLDS_CASE
  throw std::invalid_argument("gram_folds: features must be f32 or f64");
}

void check_rule(const FoldRule& fr) {
  if (fr.k < 1 || fr.k > kMaxFolds) throw std::invalid_argument("fold rule: 1 <= k <= 16");
  for (int j = 1; j < fr.k - 1; ++j)
    if (fr.thr[j] < fr.thr[j - 1]) throw std::invalid_argument("fold rule: thresholds must not decrease");
}

}  // namespace

int gram_folds_blocks(int d, int64_t n, int xdt) {
  if (d < 1 || d > 64) throw std::invalid_argument("gram_folds: d must be in [1, 64]");
  int nb = 1;
  with_folds_kernel(xdt, d, [&](auto kern) { nb = staged_f64_blocks(kern, staged_f64_lds(d), n); });
  return nb;
}

void gram_folds(GramArgs a, const FoldRule& fr, int blocks, double* out, hipStream_t st) {
  staged_f64_plan(a, blocks, "gram_folds");  // (granules = supersteps: a.nsuper, a.spw)
  if (a.w != nullptr) throw std::invalid_argument("gram_folds: instance weights are not supported");
  check_rule(fr);
  const size_t lds = staged_f64_lds(a.d);
  with_folds_kernel(a.xdt, a.d,
                    [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), lds, st, a, fr); });
  DQ_HIP_CHECK(hipGetLastError());
  const int64_t pout = 5 + 2 * (int64_t)a.d + (int64_t)a.d * (a.d + 1) / 2;
  for (int fold = 0; fold < fr.k; ++fold)
    gram_reduce(GRAM_F64, a.partials + (int64_t)fold * blocks * a.P, blocks, a.d, out + fold * pout, st);
}

void fold_ids(int64_t n, int64_t granule, const FoldRule& fr, uint8_t* out, hipStream_t st) {
  if (granule < 1) throw std::invalid_argument("fold_ids: granule must be >= 1");
  check_rule(fr);
  if (n <= 0) return;
  int64_t blocks = (n + 256 * 8 - 1) / (256 * 8);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(fold_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, granule, fr, out);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
