// The level passes of a random forest on integer words: tree.hip's passes, for all trees at once.
//
// What a forest has that one tree has not, and what this file is built on:
//  * a row's bins B[r, :] are the same for every tree, so one launch that covers open nodes of
//    several trees reads the row's dpad bytes once, where a forest grown tree by tree reads them
//    once per tree per level (and pays tree_hist's launches-per-level bound once per tree);
//  * a node looks at m <= d features only (Spark: ceil(sqrt d) for classification, ceil(d / 3) for
//    regression), so a slot needs m nb W cells, not d nb W: 64 KiB of LDS holds d / m times the
//    slots, and a level takes that many fewer launches.  With d <= 64 a slot's subset is one
//    64-bit mask, and the position of feature f among the slot's cells is popcount(mask below f).
//
// forest_bag writes node[T, n], tree-major so that each tree's reads are coalesced: the bag count c
// of (tree t, global row g) is the number of the rule's thresholds that fold_hash(seed_t, g)
// reaches (Poisson / Bernoulli / constant 1: ops/forest.py builds the table), and a live row with
// c >= 1 starts at (c << 24) | t, the root slot of tree t.  The count rides in the word from then
// on, so the hot pass gets slot and weight from one 4-byte read and a row outside the bag costs
// no more than that.
//
// forest_hist is the hot pass.  Slots of a level are numbered tree-major; a launch covers the
// slots [g0, g0 + G) and the trees [t0, t1] that own them.  A block owns a contiguous range of
// 256-row tiles and, in LDS, the G masks and the cells [G][m][nb][W] of the group.  A lane owns a
// row: it reads node[t, r] for the launch's trees, and only at the first word that falls into the
// group computes the row's label words (exactly tree_hist's: the class, or 1 and the limbs of y
// and y * y).  For each such word it walks the row's bins a dword at a time, as tree_hist does
// and from the same rotated starting quad, and adds c x the words to the cell of every feature in
// the slot's mask.  The dwords are read again for each hit rather than held in registers: the
// rotation makes their index dynamic, and after the first hit they come from the cache line the
// row occupies.  Measured (profiles/forest.md) against the dwords held in registers without the
// rotation and against a loop over the mask's set bits with byte reads, neither choice wins
// everywhere: registers halve the root level at d = 32 and lose up to 35 % on deep regression
// levels; the set-bit loop gains 16 % on deep regression levels at d = 32 and loses at d = 8.
// Accumulators are integers (u32 class counts / i64 limbs in LDS, i64 in HBM), so the words depend
// on neither the grid, the schedule, the group split nor a shard split; m = d with full masks
// gives tree_hist's words.  The block flushes its non-zero words with 64-bit integer atomics.
// LDS per block stays within the 64 KiB static limit, and with it two blocks per CU, for the
// reasons tree.hip gives.  Matrix instructions do not fit here either: a one-hot product over
// bins has density 1 / nb (tree.hip), and the mask thins it by another m / d.
//
// forest_route moves the word of every tree through the level's table and keeps the count bits;
// forest_predict walks all trees per row and adds their leaf values in tree order in f64 (compiled
// without contraction), so its sums are those of the twin in ops/forest.py bit for bit.
#include "forest.h"

#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "fixed_point.h"
#include "gram_folds.h"

#pragma clang fp contract(off)

namespace dq4ml {
namespace {

typedef unsigned long long u64;
typedef long long i64;

__global__ __launch_bounds__(kTreeThreads) void forest_bag_kernel(int64_t n, int64_t row_offset, const uint8_t* sel,
                                                                  const uint64_t* seeds, int trees, BagRule rule,
                                                                  int* node) {
  for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
    const bool live = sel == nullptr || gptr<uint8_t>(sel)[r] != 0;
    for (int t = 0; t < trees; ++t) {
      const uint32_t u = fold_hash(gptr<uint64_t>(seeds)[t], (uint64_t)(row_offset + r));
      int c = 0;
#pragma unroll
      for (int j = 0; j < kForestMaxCount; ++j) c += (j < rule.k && u >= rule.thr[j]) ? 1 : 0;
      node[(int64_t)t * n + r] = (live && c >= 1) ? ((c << kForestCountShift) | t) : -1;
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kTreeThreads) void forest_hist_kernel(ForestHistArgs a, u64* H) {
  using Cell = typename std::conditional<KIND == TREE_CLS, uint32_t, u64>::type;
  extern __shared__ u64 lds_raw[];
  u64* lmask = lds_raw;                                   // [G]
  Cell* lds = reinterpret_cast<Cell*>(lds_raw + a.G);     // [G][m][nb][W]
  const int W = KIND == TREE_CLS ? a.classes : kTreeRegWords;
  const int cells = a.m * a.nb;       // of one slot
  const int total = a.G * cells * W;  // words; with the masks at most kTreeLdsBytes (the launcher checks)
  for (int i = threadIdx.x; i < total; i += kTreeThreads) lds[i] = 0;
  for (int i = threadIdx.x; i < a.G; i += kTreeThreads) lmask[i] = gptr<u64>(a.mask)[a.g0 + i];
  __syncthreads();
  const int64_t tiles = (a.n + kTreeThreads - 1) / kTreeThreads;
  const int64_t t_lo = tiles * blockIdx.x / gridDim.x, t_hi = tiles * (blockIdx.x + 1) / gridDim.x;
  const int quads = a.dpad / 4, q0 = (threadIdx.x & (kWave - 1)) % quads;
  for (int64_t tile = t_lo; tile < t_hi; ++tile) {
    const int64_t r = tile * kTreeThreads + threadIdx.x;
    if (r >= a.n) continue;
    const uint8_t* row = a.B + r * a.dpad;
    bool ready = false;
    int cls = 0;
    i64 w[kTreeRegWords];
    for (int t = a.t0; t <= a.t1; ++t) {
      const int word = gptr<int>(a.node)[(int64_t)t * a.n + r];
      if (word < 0) continue;  // dead, outside tree t's bag, or in a leaf of it
      const int s = (word & kForestSlotMask) - a.g0;
      if (s < 0 || s >= a.G) continue;  // another group's slot
      const int c = word >> kForestCountShift;
      if (!ready) {  // the row's label words, once, and only for a row of this group
        const double y = a.ydt == DT_F32 ? (double)gptr<float>(a.y)[r] : gptr<double>(a.y)[r];
        if constexpr (KIND == TREE_CLS) {
          cls = (int)y;
          if (!(y >= 0.0) || cls >= a.classes) break;  // (the fit's label flag reports these rows)
        } else {
          if (!(fabs(y) < __longlong_as_double(0x7ff0000000000000ll))) break;
          w[0] = 1;
          cut_limbs(y, a.e, w + 1);
          cut_limbs(y * y, 2 * a.e, w + 1 + kSumLimbs);
        }
        ready = true;
      }
      const u64 mk = lmask[s];
      Cell* slot = lds + (int64_t)s * cells * W;
      for (int qi = 0; qi < quads; ++qi) {
        const int q = q0 + qi < quads ? q0 + qi : q0 + qi - quads;
        if (((mk >> (4 * q)) & 15) == 0) continue;  // none of the quad's features is in the subset
        const uint32_t bins = *gptr<uint32_t>(row + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * q + j, bin = (bins >> (8 * j)) & 255;
          if (f >= a.d || bin >= a.nb || ((mk >> f) & 1) == 0) continue;  // pad bytes, features outside the subset
          const int pos = __popcll(mk & ((1ull << f) - 1));
          if (pos >= a.m) continue;  // never index past the slot's cells
          Cell* cell = slot + (pos * a.nb + bin) * W;
          if constexpr (KIND == TREE_CLS) {
            atomicAdd(cell + cls, (uint32_t)c);
          } else {
#pragma unroll
            for (int k = 0; k < kTreeRegWords; ++k)
              if (w[k] != 0) atomicAdd(cell + k, (u64)(w[k] * c));
          }
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

__global__ __launch_bounds__(kTreeThreads) void forest_route_kernel(const uint8_t* B, int dpad, int64_t n, const int* tab,
                                                                    int open, int* node, int trees) {
  for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
    const uint8_t* row = B + r * dpad;  // one line of at most 64 bytes: fetched once, whatever the trees ask of it
    for (int t = 0; t < trees; ++t) {
      int* p = node + (int64_t)t * n + r;
      const int word = *p;
      if (word < 0) continue;
      const int s = word & kForestSlotMask;
      int next = -1;
      if (s < open) {
        const int f = gptr<int>(tab)[4 * s];
        if (f >= 0 && f < dpad) {
          const int child = gptr<uint8_t>(row)[f] <= gptr<int>(tab)[4 * s + 1] ? gptr<int>(tab)[4 * s + 2] : gptr<int>(tab)[4 * s + 3];
          if (child >= 0 && child <= kForestSlotMask) next = (word & ~kForestSlotMask) | child;
        }
      }
      *p = next;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kTreeThreads) void forest_predict_kernel(const T* X, int64_t ld, int d, int64_t n,
                                                                      const uint8_t* sel, const int* feat,
                                                                      const double* thr, const int* left,
                                                                      const int* right, int nodes, const int* root,
                                                                      int trees, const double* val, int C, double* out) {
  for (int64_t r = (int64_t)blockIdx.x * kTreeThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTreeThreads) {
    const bool live = sel == nullptr || gptr<uint8_t>(sel)[r] != 0;
    double acc[kTreeMaxClasses];
#pragma unroll
    for (int k = 0; k < kTreeMaxClasses; ++k) acc[k] = 0.0;
    for (int t = 0; live && t < trees; ++t) {
      int i = gptr<int>(root)[t];
      if (i < 0 || i >= nodes) continue;  // never index past the forest
      for (int step = 0; step < 64; ++step) {  // (a tree is at most 30 deep)
        const int f = gptr<int>(feat)[i];
        if (f < 0 || f >= d) break;
        const double x = (double)gptr<T>(X)[(int64_t)f * ld + r];
        const int c = x <= gptr<double>(thr)[i] ? gptr<int>(left)[i] : gptr<int>(right)[i];
        if (c < 0 || c >= nodes) break;
        i = c;
      }
#pragma unroll
      for (int k = 0; k < kTreeMaxClasses; ++k)
        if (k < C) acc[k] = acc[k] + gptr<double>(val)[(int64_t)i * C + k];  // tree order, one rounding each
    }
#pragma unroll
    for (int k = 0; k < kTreeMaxClasses; ++k)
      if (k < C) out[(int64_t)k * n + r] = live ? acc[k] : __longlong_as_double(0x7ff8000000000000ll);
  }
}

void check_rows(int64_t n, int blocks, const char* who) {
  if (n < 1 || n >= ((int64_t)1 << 31)) throw std::invalid_argument(std::string(who) + ": needs 1 <= n < 2^31");
  if (blocks < 1) throw std::invalid_argument(std::string(who) + ": blocks must be >= 1");
}

void check_trees(int trees, const char* who) {
  if (trees < 1 || trees > kForestSlotMask) throw std::invalid_argument(std::string(who) + ": needs 1 <= trees < 2^24");
}

}  // namespace

void forest_bag(int64_t n, int64_t row_offset, const uint8_t* sel, const uint64_t* seeds, int trees, const BagRule& rule,
                int* node, int blocks, hipStream_t st) {
  check_rows(n, blocks, "forest_bag");
  check_trees(trees, "forest_bag");
  if (row_offset < 0 || rule.k < 0 || rule.k > kForestMaxCount)
    throw std::invalid_argument("forest_bag: needs row_offset >= 0 and at most 15 thresholds");
  if (!seeds || !node) throw std::invalid_argument("forest_bag: null operand");
  hipLaunchKernelGGL(forest_bag_kernel, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, n, row_offset, sel, seeds, trees,
                     rule, node);
  DQ_HIP_CHECK(hipGetLastError());
}

void forest_hist(const ForestHistArgs& a, int kind, long long* H, int blocks, hipStream_t st) {
  check_rows(a.n, blocks, "forest_hist");
  if (a.d < 1 || a.d > kTreeMaxD || a.dpad != (a.d + 3) / 4 * 4 || a.m < 1 || a.m > a.d)
    throw std::invalid_argument("forest_hist: needs 1 <= m <= d <= 64 and dpad = d rounded up to 4");
  if (kind != TREE_REG && kind != TREE_CLS) throw std::invalid_argument("forest_hist: unknown kind");
  if (a.nb < 1 || a.nb > kTreeMaxBins) throw std::invalid_argument("forest_hist: needs 1 <= bins <= 256");
  if (kind == TREE_CLS && (a.classes < 1 || a.classes > kTreeMaxClasses))
    throw std::invalid_argument("forest_hist: needs 1 <= classes <= 16");
  if (a.ydt != DT_F32 && a.ydt != DT_F64) throw std::invalid_argument("forest_hist: f32 / f64 labels only");
  if (kind == TREE_REG && (a.e < -400 || a.e > 400)) throw std::invalid_argument("forest_hist: label exponent out of range");
  if (a.g0 < 0 || a.G < 1 || a.G > forest_group(kind, a.m, a.nb, a.classes) || a.g0 > kForestSlotMask - a.G)
    throw std::invalid_argument("forest_hist: the slot group does not fit the block's LDS");
  if (a.t0 < 0 || a.t1 < a.t0 || a.t1 >= kForestSlotMask) throw std::invalid_argument("forest_hist: needs 0 <= t0 <= t1");
  // a block's u32 class counts hold its rows times the largest bag count
  if (kind == TREE_CLS && (a.n / kTreeThreads / blocks + 2) * kTreeThreads * kForestMaxCount >= ((int64_t)1 << 32))
    throw std::invalid_argument("forest_hist: too few blocks for this many rows");
  if (!a.B || !a.node || !a.y || !a.mask || !H) throw std::invalid_argument("forest_hist: null operand");
  const size_t lds = (size_t)a.G * forest_slot_bytes(kind, a.m, a.nb, a.classes);
  if (kind == TREE_CLS)
    hipLaunchKernelGGL(forest_hist_kernel<TREE_CLS>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, a, (u64*)H);
  else
    hipLaunchKernelGGL(forest_hist_kernel<TREE_REG>, dim3((unsigned)blocks), dim3(kTreeThreads), lds, st, a, (u64*)H);
  DQ_HIP_CHECK(hipGetLastError());
}

void forest_route(const uint8_t* B, int dpad, int64_t n, const int* tab, int open, int* node, int trees, int blocks,
                  hipStream_t st) {
  check_rows(n, blocks, "forest_route");
  check_trees(trees, "forest_route");
  if (dpad < 4 || dpad > kTreeMaxD || dpad % 4 || open < 1 || open > kForestSlotMask || !B || !tab || !node)
    throw std::invalid_argument("forest_route: bad operands");
  hipLaunchKernelGGL(forest_route_kernel, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, B, dpad, n, tab, open, node,
                     trees);
  DQ_HIP_CHECK(hipGetLastError());
}

void forest_predict(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const int* feat,
                    const double* thr, const int* left, const int* right, int nodes, const int* root, int trees,
                    const double* val, int C, double* out, int blocks, hipStream_t st) {
  check_rows(n, blocks, "forest_predict");
  check_trees(trees, "forest_predict");
  if (d < 1 || ld < n || nodes < 1) throw std::invalid_argument("forest_predict: needs d >= 1, ld >= n and a forest");
  if (C < 1 || C > kTreeMaxClasses) throw std::invalid_argument("forest_predict: needs 1 <= values per leaf <= 16");
  if (xdt != DT_F32 && xdt != DT_F64) throw std::invalid_argument("forest_predict: f32 / f64 features only");
  if (!X || !feat || !thr || !left || !right || !root || !val || !out)
    throw std::invalid_argument("forest_predict: null operand");
  if (xdt == DT_F32)
    hipLaunchKernelGGL(forest_predict_kernel<float>, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, (const float*)X, ld,
                       d, n, sel, feat, thr, left, right, nodes, root, trees, val, C, out);
  else
    hipLaunchKernelGGL(forest_predict_kernel<double>, dim3((unsigned)blocks), dim3(kTreeThreads), 0, st, (const double*)X,
                       ld, d, n, sel, feat, thr, left, right, nodes, root, trees, val, C, out);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
