// The level passes of a decision tree on integer words.
//
// tree_bin reads feature-major X once and writes the row-major u8 bins B[n, dpad]: every later pass
// reads d bytes per row, and one row's bins are contiguous.  The thresholds of as many features as
// fit 64 KiB sit in LDS (at 255 splits: 32 features, so d = 64 takes two rounds over the block's
// rows); a bin is a lower-bound binary search in f64.
//
// tree_hist is the hot pass.  A block owns a contiguous range of 256-row tiles and, in LDS, the
// histogram [G nodes][d][nb bins][W words] of one node group.  A lane owns a row: it reads the
// row's slot first (a row outside the group costs 4 bytes), computes the row's words once --
// classification: its class; regression: 1 and the four fixed-point limbs of y and of y * y
// (fixed_point.h, exponents e and 2e, y * y rounded once to f64) -- and adds them to the cell of
// each of its d bins, read four at a time as one dword of B.  The lanes of a wave start at
// different features (lane mod dpad / 4) so that, at the root, 64 lanes do not all land in the
// <= nb cells of one feature.  All accumulators are integers (u32 class counts / i64 limbs in
// LDS, i64 in HBM), so the words do not depend on the grid, the schedule or a shard split.  The
// block flushes its non-zero words with 64-bit integer atomics.
//
// LDS per block: 64 KiB.  That is the static limit a launch needs no opt-in for, and it leaves two
// blocks (8 waves) per CU on the 160 KiB of a gfx950 CU, which is what hides the latency of the
// per-lane dword reads of B.  G = 64 KiB / (d nb W cell bytes) nodes; a level with more open
// nodes takes ceil(open / G) launches (Spark's node groups).  A shape whose single node does not
// fit (regression at d = 64 beyond 14 bins) is outside the fused range.
//
// Measured (profiles/tree.md, 32 bins): the root level of 1e7 rows takes 0.14 ms (classification,
// d = 8) to 0.36 ms (d = 32) and 0.23 ms for regression at d = 8, 1000x and more under the torch
// bincount composite.  The plan's same-cell combine within the wave ahead of the LDS atomic was
// not built (the lane rotation above stands in for it), so what it would add is not measured.
// What measurement did move: the node groups.  Each launch re-reads
// every row's slot, so 22 groups (regression, d = 8, 64 open nodes) cost 4.6 ms against 0.23 ms
// for one; a deep level is bound by ceil(open / G), not by the atomics.  Still fused is 3.5x
// ahead of the composite there.  Not done: the 160 KiB budget (2.5x the nodes per group at one
// block per CU, and regression beyond 910 cells), rows sorted by node, and matrix instructions
// (a one-hot product over bins has density 1 / nb).
//
// tree_split: one block per open node, one wave per feature at a time, lanes over bins.  The bin
// prefix is an integer wave scan, so left / right words are exact; a fixed-point sum becomes a
// double by limbs_to_f64 below, the one statement of that conversion (ops/tree.py has its twin).
// A forest (forest.hip) hands it each node's feature subset: the search then walks the node's m
// positions, looks the split count up by the real feature and reports that feature.
// All f64 arithmetic of this file is compiled without contraction, so each operation rounds as
// the twin's does.
#include "tree.h"

#include <stdexcept>
#include <type_traits>

#include "common.h"
#include "fixed_point.h"

#pragma clang fp contract(off)

namespace dq4ml {
namespace {

typedef unsigned long long u64;
typedef long long i64;

template <typename T>
__global__ __launch_bounds__(kTreeThreads) void tree_bin_kernel(const T* X, int64_t ld, int d, int64_t n,
                                                                const uint8_t* sel, const double* thr,
                                                                const int* nsplit, int S, int fchunk, int dpad,
                                                                uint8_t* B, int* flag) {
  extern __shared__ double lthr[];  // [fchunk][S]
  bool bad = false;
  for (int f0 = 0; f0 < dpad; f0 += fchunk) {  // (fchunk and dpad are multiples of 4: f0 < d)
    const int nf = min(fchunk, d - f0), quads = min(fchunk, dpad - f0) / 4;
    __syncthreads();
    for (int i = threadIdx.x; i < nf * S; i += kTreeThreads) lthr[i] = gptr<double>(thr)[(int64_t)f0 * S + i];
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
      const bool live = sel == nullptr || gptr<uint8_t>(sel)[r] != 0;
      for (int q = 0; q < quads; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = f0 + 4 * q + j;
          if (!live || f >= d) continue;
          const double x = (double)gptr<T>(X)[(int64_t)f * ld + r];
          bad = bad || x != x;
          int lo = 0, hi = gptr<int>(nsplit)[f];
          const double* t = lthr + (f - f0) * S;
          while (lo < hi) {  // the number of thresholds below x
            const int mid = (lo + hi) >> 1;
            if (t[mid] < x) lo = mid + 1;
            else hi = mid;
          }
          word |= (uint32_t)lo << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(B + r * dpad + f0 + 4 * q) = word;
      }
    }
  }
  if (bad) atomicOr(flag, 1);
}

template <int KIND>
__global__ __launch_bounds__(kTreeThreads) void tree_hist_kernel(TreeHistArgs a, u64* H) {
  using Cell = typename std::conditional<KIND == TREE_CLS, uint32_t, u64>::type;
  extern __shared__ u64 lds_raw[];
  Cell* lds = reinterpret_cast<Cell*>(lds_raw);
  const int W = KIND == TREE_CLS ? a.classes : kTreeRegWords;
  const int cells = a.d * a.nb;      // of one node
  const int total = a.G * cells * W;  // words; at most kTreeLdsBytes of them (the launcher checks)
  for (int i = threadIdx.x; i < total; i += kTreeThreads) lds[i] = 0;
  __syncthreads();
  const int64_t tiles = (a.n + kTreeThreads - 1) / kTreeThreads;
  const int64_t t_lo = tiles * blockIdx.x / gridDim.x, t_hi = tiles * (blockIdx.x + 1) / gridDim.x;
  const int quads = a.dpad / 4, q0 = (threadIdx.x & (kWave - 1)) % quads;
  for (int64_t t = t_lo; t < t_hi; ++t) {
    const int64_t r = t * kTreeThreads + threadIdx.x;
    if (r >= a.n) continue;
    const int s = gptr<int>(a.node)[r] - a.g0;
    if (s < 0 || s >= a.G) continue;  // dead, in a leaf, or another group's row
    const double y = a.ydt == DT_F32 ? (double)gptr<float>(a.y)[r] : gptr<double>(a.y)[r];
    int cls = 0;
    i64 w[kTreeRegWords];
    if constexpr (KIND == TREE_CLS) {
      cls = (int)y;
      if (!(y >= 0.0) || cls >= a.classes) continue;  // (the fit's label flag reports these rows)
    } else {
      if (!(fabs(y) < __longlong_as_double(0x7ff0000000000000ll))) continue;
      w[0] = 1;
      cut_limbs(y, a.e, w + 1);
      cut_limbs(y * y, 2 * a.e, w + 1 + kSumLimbs);
    }
    const uint8_t* row = a.B + r * a.dpad;
    for (int qi = 0; qi < quads; ++qi) {
      const int q = q0 + qi < quads ? q0 + qi : q0 + qi - quads;
      const uint32_t bins = *gptr<uint32_t>(row + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * q + j, bin = (bins >> (8 * j)) & 255;
        if (f >= a.d || bin >= a.nb) continue;  // pad bytes; never index past the node's cells
        Cell* cell = lds + ((int64_t)s * cells + f * a.nb + bin) * W;
        if constexpr (KIND == TREE_CLS) {
          atomicAdd(cell + cls, 1u);
        } else {
#pragma unroll
          for (int k = 0; k < kTreeRegWords; ++k)
            if (w[k] != 0) atomicAdd(cell + k, (u64)w[k]);
        }
      }
    }
  }
  __syncthreads();
  u64* out = H + (int64_t)a.g0 * cells * W;
  for (int i = threadIdx.x; i < total; i += kTreeThreads) {
    const Cell v = lds[i];
    if (v != 0) atomicAdd(out + i, (u64)v);
  }
}

// A fixed-point sum as a double: carry-normalise the limbs in integers from the bottom (the three
// low limbs end in [0, 2^32), the top one keeps the sign), then Horner from the top limb down in
// f64 -- the conversion of the top limb and each of the three adds round once, the multiplications
// by 2^32 are exact -- and scale by 2^(e - 128).
__device__ __forceinline__ double limbs_to_f64(const i64* L, int e) {
  constexpr i64 kMask = 0xffffffffll;
  i64 l[kSumLimbs];
  i64 carry = 0;
#pragma unroll
  for (int k = kSumLimbs - 1; k > 0; --k) {
    const i64 v = L[k] + carry;
    carry = v >> 32;
    l[k] = v & kMask;
  }
  l[0] = L[0] + carry;
  double v = (double)l[0];
#pragma unroll
  for (int k = 1; k < kSumLimbs; ++k) v = v * 4294967296.0 + (double)l[k];
  return ldexp(v, e - 32 * kSumLimbs);
}

struct NodeStats {
  double n, imp, pred;
};

// count, impurity and prediction of the words of a set of rows (n >= 1)
__device__ __forceinline__ NodeStats node_stats(const i64* w, const TreeSplitArgs& a) {
  NodeStats s;
  if (a.kind == TREE_REG) {
    s.n = (double)w[0];
    const double s1 = limbs_to_f64(w + 1, a.e), s2 = limbs_to_f64(w + 1 + kSumLimbs, 2 * a.e);
    s.pred = s1 / s.n;
    s.imp = (s2 - s1 * s1 / s.n) / s.n;
    return s;
  }
  i64 n = 0, top = -1;
  int arg = 0;
  for (int k = 0; k < a.classes; ++k) {
    n += w[k];
    if (w[k] > top) top = w[k], arg = k;
  }
  s.n = (double)n;
  s.pred = (double)arg;
  double acc = a.impurity == TREE_GINI ? 1.0 : 0.0;
  for (int k = 0; k < a.classes; ++k) {
    if (w[k] <= 0) continue;
    const double f = (double)w[k] / s.n;
    if (a.impurity == TREE_GINI) acc -= f * f;
    else acc -= f * log2(f);
  }
  s.imp = acc;
  return s;
}

struct Best {
  double gain;
  int f, b;
};

__device__ __forceinline__ bool better(double g, int f, int b, const Best& o) {
  return f >= 0 && (o.f < 0 || g > o.gain || (g == o.gain && (f < o.f || (f == o.f && b < o.b))));
}

__global__ __launch_bounds__(kTreeThreads) void tree_split_kernel(TreeSplitArgs a, double* rec) {
  constexpr int kMaxW = kTreeMaxClasses;
  constexpr int kWaves = kTreeThreads / kWave;
  __shared__ Best wbest[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int W = tree_words(a.kind, a.classes);
  // positions of the node's cells: every feature, or the m features of its subset (ascending, so
  // the (position, split) order of the search below is the (feature, split) order either way)
  const int np = a.feats ? a.m : a.d;
  const int* fs = a.feats ? a.feats + (int64_t)blockIdx.x * a.m : nullptr;
  const i64* Hn = a.H + (int64_t)blockIdx.x * np * a.nb * W;
  // the node's words: the sum over the bins of feature 0 (every wave, for itself)
  i64 tot[kMaxW];
#pragma unroll
  for (int k = 0; k < kMaxW; ++k) {
    i64 v = 0;
    if (k < W)
      for (int b = lane; b < a.nb; b += kWave) v += gptr<i64>(Hn)[(int64_t)b * W + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    tot[k] = v;
  }
  i64 rows = tot[0];
  if (a.kind == TREE_CLS)
    for (int k = 1; k < W; ++k) rows += tot[k];
  double* out = rec + (int64_t)blockIdx.x * kTreeRecord;
  if (rows <= 0) {  // (no row reached this slot: an all-zero leaf)
    for (int i = threadIdx.x; i < kTreeRecord; i += kTreeThreads) out[i] = i == 0 ? -1.0 : (i == 10 ? 1.0 : 0.0);
    return;
  }
  const NodeStats P = node_stats(tot, a);
  Best best{0.0, -1, 0};
  for (int f = wave; f < np; f += kWaves) {  // f: the position; best.f keeps it until the record is written
    const int feat = fs ? gptr<int>(fs)[f] : f;
    if (feat < 0 || feat >= a.d) continue;  // (wave-uniform; never index past nsplit)
    const int ns = min(gptr<int>(a.nsplit)[feat], a.nb - 1);
    i64 carry[kMaxW];
#pragma unroll
    for (int k = 0; k < kMaxW; ++k) carry[k] = 0;
    for (int b0 = 0; b0 < ns; b0 += kWave) {  // wave-uniform
      const int b = b0 + lane;
      i64 left[kMaxW], right[kMaxW];
#pragma unroll
      for (int k = 0; k < kMaxW; ++k) {
        i64 v = (k < W && b < ns) ? gptr<i64>(Hn)[((int64_t)f * a.nb + b) * W + k] : 0;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {  // inclusive scan over the lanes
          const i64 u = __shfl_up(v, o, kWave);
          if (lane >= o) v += u;
        }
        left[k] = carry[k] + v;
        right[k] = tot[k] - left[k];
        carry[k] += __shfl(v, kWave - 1, kWave);
      }
      if (b >= ns) continue;
      i64 nl = left[0];
      if (a.kind == TREE_CLS)
        for (int k = 1; k < W; ++k) nl += left[k];
      if (nl < a.min_rows || rows - nl < a.min_rows) continue;
      const NodeStats L = node_stats(left, a), R = node_stats(right, a);
      const double gain = (P.imp - (L.n / P.n) * L.imp) - (R.n / P.n) * R.imp;
      if (!(gain >= a.min_gain)) continue;
      if (better(gain, f, b, best)) best = Best{gain, f, b};
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best u;
    u.gain = __shfl_xor(best.gain, o, kWave);
    u.f = __shfl_xor(best.f, o, kWave);
    u.b = __shfl_xor(best.b, o, kWave);
    if (better(u.gain, u.f, u.b, best)) best = u;
  }
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 1; i < kWaves; ++i)
    if (better(wbest[i].gain, wbest[i].f, wbest[i].b, best)) best = wbest[i];
  for (int i = 0; i < kTreeRecord; ++i) out[i] = 0.0;
  const bool found = best.f >= 0;
  out[0] = found ? (double)(fs ? gptr<int>(fs)[best.f] : best.f) : -1.0;
  out[3] = P.imp, out[4] = P.n, out[5] = P.pred;
  out[10] = (a.force_leaf || !found || !(best.gain > 0.0)) ? 1.0 : 0.0;
  if (a.kind == TREE_CLS)
    for (int k = 0; k < W; ++k) out[16 + k] = (double)tot[k];
  if (!found) return;
  i64 left[kMaxW], right[kMaxW];
  for (int k = 0; k < W; ++k) {  // the winner's words again (integers: the same as the scan's)
    i64 v = 0;
    for (int b = 0; b <= best.b; ++b) v += gptr<i64>(Hn)[((int64_t)best.f * a.nb + b) * W + k];
    left[k] = v, right[k] = tot[k] - v;
  }
  const NodeStats L = node_stats(left, a), R = node_stats(right, a);
  out[1] = (double)best.b, out[2] = best.gain;
  out[6] = L.n, out[7] = R.n, out[8] = L.imp, out[9] = R.imp;
  out[11] = (a.child_leaf || L.imp == 0.0) ? 1.0 : 0.0;
  out[12] = (a.child_leaf || R.imp == 0.0) ? 1.0 : 0.0;
  out[13] = L.pred, out[14] = R.pred;
  if (a.kind == TREE_CLS)
    for (int k = 0; k < W; ++k) out[32 + k] = (double)left[k], out[48 + k] = (double)right[k];
}

__global__ __launch_bounds__(kTreeThreads) void tree_route_kernel(const uint8_t* B, int dpad, int64_t n, const int* tab,
                                                                  int open, int* node) {
  for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
    const int s = node[r];
    if (s < 0) continue;
    int next = -1;
    if (s < open) {
      const int f = gptr<int>(tab)[4 * s];
      if (f >= 0 && f < dpad)
        next = gptr<uint8_t>(B)[r * dpad + f] <= gptr<int>(tab)[4 * s + 1] ? gptr<int>(tab)[4 * s + 2] : gptr<int>(tab)[4 * s + 3];
    }
    node[r] = next;
  }
}

template <typename T>
__global__ __launch_bounds__(kTreeThreads) void tree_predict_kernel(const T* X, int64_t ld, int d, int64_t n,
                                                                    const uint8_t* sel, const int* feat,
                                                                    const double* thr, const int* left,
                                                                    const int* right, int m, int* leaf) {
  for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
    int i = -1;
    if (sel == nullptr || gptr<uint8_t>(sel)[r] != 0) {
      i = 0;
      for (int step = 0; step < 64; ++step) {  // (a tree is at most 30 deep)
        const int f = gptr<int>(feat)[i];
        if (f < 0 || f >= d) break;
        const double x = (double)gptr<T>(X)[(int64_t)f * ld + r];
        const int c = x <= gptr<double>(thr)[i] ? gptr<int>(left)[i] : gptr<int>(right)[i];
        if (c < 0 || c >= m) break;  // never index past the tree
        i = c;
      }
    }
    leaf[r] = i;
  }
}

void check_rows(int64_t n, int blocks, const char* who) {
  if (n < 1 || n >= ((int64_t)1 << 31)) throw std::invalid_argument(std::string(who) + ": needs 1 <= n < 2^31");
  if (blocks < 1) throw std::invalid_argument(std::string(who) + ": blocks must be >= 1");
}

void check_features(int d, int dpad, const char* who) {
  if (d < 1 || d > kTreeMaxD || dpad != (d + 3) / 4 * 4)
    throw std::invalid_argument(std::string(who) + ": needs 1 <= d <= 64 and dpad = d rounded up to 4");
}

}  // namespace

// two 64 KiB blocks per CU (the histogram pass's residency; the lighter passes take the same grid)
int tree_blocks(int64_t n) { return grid_for(2, (n + kTreeThreads - 1) / kTreeThreads); }

void tree_bin(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const double* thr,
              const int* nsplit, int S, int dpad, uint8_t* B, int* flag, int blocks, hipStream_t st) {
  check_rows(n, blocks, "tree_bin");
  check_features(d, dpad, "tree_bin");
  if (ld < n || S < 1 || S > kTreeMaxBins - 1) throw std::invalid_argument("tree_bin: needs ld >= n and 1 <= S <= 255");
  if (xdt != DT_F32 && xdt != DT_F64) throw std::invalid_argument("tree_bin: f32 / f64 features only");
  if (!X || !thr || !nsplit || !B || !flag) throw std::invalid_argument("tree_bin: null operand");
  int fchunk = kTreeLdsBytes / (S * (int)sizeof(double)) / 4 * 4;  // >= 32 features
  if (fchunk > dpad) fchunk = dpad;
  const size_t lds = (size_t)fchunk * S * sizeof(double);
  if (xdt == DT_F32)
    hipLaunchKernelGGL(tree_bin_kernel<float>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, (const float*)X, ld, d,
                       n, sel, thr, nsplit, S, fchunk, dpad, B, flag);
  else
    hipLaunchKernelGGL(tree_bin_kernel<double>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, (const double*)X, ld,
                       d, n, sel, thr, nsplit, S, fchunk, dpad, B, flag);
  DQ_HIP_CHECK(hipGetLastError());
}

void tree_hist(const TreeHistArgs& a, int kind, long long* H, int blocks, hipStream_t st) {
  check_rows(a.n, blocks, "tree_hist");
  check_features(a.d, a.dpad, "tree_hist");
  if (kind != TREE_REG && kind != TREE_CLS) throw std::invalid_argument("tree_hist: unknown kind");
  if (a.nb < 1 || a.nb > kTreeMaxBins) throw std::invalid_argument("tree_hist: needs 1 <= bins <= 256");
  if (kind == TREE_CLS && (a.classes < 1 || a.classes > kTreeMaxClasses))
    throw std::invalid_argument("tree_hist: needs 1 <= classes <= 16");
  if (a.ydt != DT_F32 && a.ydt != DT_F64) throw std::invalid_argument("tree_hist: f32 / f64 labels only");
  if (kind == TREE_REG && (a.e < -400 || a.e > 400)) throw std::invalid_argument("tree_hist: label exponent out of range");
  if (a.g0 < 0 || a.G < 1 || a.G > tree_group(kind, a.d, a.nb, a.classes))
    throw std::invalid_argument("tree_hist: the node group does not fit the block's LDS");
  if (!a.B || !a.node || !a.y || !H) throw std::invalid_argument("tree_hist: null operand");
  const size_t lds = (size_t)a.G * a.d * a.nb * tree_words(kind, a.classes) * (kind == TREE_CLS ? 4 : 8);
  if (kind == TREE_CLS)
    hipLaunchKernelGGL(tree_hist_kernel<TREE_CLS>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, a, (u64*)H);
  else
    hipLaunchKernelGGL(tree_hist_kernel<TREE_REG>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, a, (u64*)H);
  DQ_HIP_CHECK(hipGetLastError());
}

void tree_split(const TreeSplitArgs& a, double* rec, hipStream_t st) {
  if (a.open < 1) throw std::invalid_argument("tree_split: at least one open node");
  if (a.d < 1 || a.d > kTreeMaxD || a.nb < 1 || a.nb > kTreeMaxBins)
    throw std::invalid_argument("tree_split: needs 1 <= d <= 64 and 1 <= bins <= 256");
  if (a.kind == TREE_CLS ? (a.classes < 1 || a.classes > kTreeMaxClasses ||
                            (a.impurity != TREE_GINI && a.impurity != TREE_ENTROPY))
                         : (a.kind != TREE_REG || a.impurity != TREE_VARIANCE))
    throw std::invalid_argument("tree_split: variance for regression; gini / entropy and 1 <= classes <= 16 otherwise");
  if (a.min_rows < 1) throw std::invalid_argument("tree_split: minInstancesPerNode must be >= 1");
  if (!a.H || !a.nsplit || !rec) throw std::invalid_argument("tree_split: null operand");
  if (a.feats && (a.m < 1 || a.m > a.d)) throw std::invalid_argument("tree_split: a feature subset needs 1 <= m <= d");
  hipLaunchKernelGGL(tree_split_kernel, dim3((unsigned)a.open), dim3(kTreeThreads), 0, st, a, rec);
  DQ_HIP_CHECK(hipGetLastError());
}

void tree_route(const uint8_t* B, int dpad, int64_t n, const int* tab, int open, int* node, int blocks, hipStream_t st) {
  check_rows(n, blocks, "tree_route");
  if (dpad < 4 || dpad > kTreeMaxD || dpad % 4 || open < 1 || !B || !tab || !node)
    throw std::invalid_argument("tree_route: bad operands");
  hipLaunchKernelGGL(tree_route_kernel, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, B, dpad, n, tab, open, node);
  DQ_HIP_CHECK(hipGetLastError());
}

void tree_predict(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const int* feat,
                  const double* thr, const int* left, const int* right, int m, int* leaf, int blocks, hipStream_t st) {
  check_rows(n, blocks, "tree_predict");
  if (d < 1 || ld < n || m < 1) throw std::invalid_argument("tree_predict: needs d >= 1, ld >= n and a tree");
  if (xdt != DT_F32 && xdt != DT_F64) throw std::invalid_argument("tree_predict: f32 / f64 features only");
  if (!X || !feat || !thr || !left || !right || !leaf) throw std::invalid_argument("tree_predict: null operand");
  if (xdt == DT_F32)
    hipLaunchKernelGGL(tree_predict_kernel<float>, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, (const float*)X, ld,
                       d, n, sel, feat, thr, left, right, m, leaf);
  else
    hipLaunchKernelGGL(tree_predict_kernel<double>, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, (const double*)X,
                       ld, d, n, sel, feat, thr, left, right, m, leaf);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
