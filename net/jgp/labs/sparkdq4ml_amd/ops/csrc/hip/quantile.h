// Exact order statistics by MSD radix select (see quantile.hip): C typed columns x Q
// probabilities, kQuantPasses histogram passes over order-preserving 64-bit keys with a one-block
// pick kernel between them.  No host read: ranks, prefixes and counts live in HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

constexpr int kMaxQuantiles = 16;   // probabilities per call (summary() needs 3)
constexpr int kMaxQuantCols = 32;   // columns per launch (the python launcher chunks above it)
constexpr int kQuantBits = 8;       // digit width
constexpr int kQuantBins = 1 << kQuantBits;
constexpr int kQuantPasses = 64 / kQuantBits;
constexpr int kQuantRun = 4;        // consecutive rows per thread and trip
constexpr int kQuantThreads = 256;
constexpr int kQuantTrip = kQuantRun * kQuantThreads;  // rows per block and grid-stride trip

// The columns of one call, by value in the kernarg.  valid[c] / sel: 0/1 bytes or null.
struct QuantCols {
  const void* col[kMaxQuantCols];
  const uint8_t* valid[kMaxQuantCols];
  int dt[kMaxQuantCols];
  const uint8_t* sel;
  int64_t n;
  int C, Q;
};

// int64 words of control state per column: [0] live histogram slots U, [1] live count n_c,
// [2, 2+Q) prefix of slot u, [2+Q, 2+2Q) slot of target q, [2+2Q, 2+3Q) remaining 1-based rank
// of target q.  Targets whose prefixes are equal share one slot (one histogram, one atomic per row).
__host__ __device__ constexpr int quant_state_stride(int Q) { return 2 + 3 * Q; }

// occupancy-sized grid (x dimension; y is the column) for n rows
int quantile_blocks(int64_t n);
// pass `pass` (0 .. kQuantPasses-1): hist is [C][Q][kQuantBins] u64 counters (zero on entry),
// state the control words the previous pick left (unread in pass 0)
void quantile_hist(const QuantCols& a, int pass, const int64_t* state, unsigned long long* hist, int blocks,
                   hipStream_t st);
// scan the bins of every target, extend prefix and rank, re-zero hist; after the last pass
// values[C][Q] (NaN where n_c = 0) and counts[C] are written
void quantile_pick(int C, int Q, int pass, const double* probs, int64_t* state, unsigned long long* hist,
                   double* values, int64_t* counts, hipStream_t st);

}  // namespace dq4ml
