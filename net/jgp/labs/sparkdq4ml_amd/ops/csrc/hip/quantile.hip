// Exact quantiles by most-significant-digit-first radix select.
//
// A value becomes a 64-bit key whose unsigned order is the numeric order of the value cast to
// double: the folded float key of keys.h (-0.0 folded into +0.0) of that double, read with the
// run loaders of keys.h.  Pass k of kQuantPasses histograms digit k (kQuantBits wide, most significant first) of the
// keys whose higher digits equal a target's prefix; the one-block pick kernel then finds the bin
// that holds the target's rank, appends it to the prefix and reduces the rank by the count below
// it.  After the last pass the prefix is the key of the order statistic.
//
// Counting is integer only (LDS u32 atomics per block, flushed with u64 global atomics), so the
// result does not depend on the grid, the schedule or a shard split.  Targets whose prefixes are
// equal (every target in pass 0, duplicated probabilities, quantiles inside one run of ties) share
// one histogram slot, so a row costs one LDS atomic per distinct prefix it matches.
//
// Contention: the lanes of a wave that agree with the first live lane on the digit are counted by
// one add of their number, twice in a row; whatever is left takes per-lane atomics.  A constant or
// sorted column, and the high digits of any real column (sign + exponent), therefore cost one or
// two LDS adds per wave instead of a 64-way serialised atomic.
#include "quantile.h"

#include <cmath>
#include <stdexcept>

#include "common.h"
#include "keys.h"
#include "scan.h"

namespace dq4ml {
namespace {

static_assert(kQuantRun == kRawRun, "the run loaders of keys.h read kQuantRun rows");

// One count of bin d for every lane with m set.  Two rounds of "the lanes that agree with the
// first live lane are one add of their number", then plain atomics for the rest.  Every lane of
// the wave calls this (the ballots need them all).
__device__ __forceinline__ void count_digit(uint32_t* h, bool m, unsigned d, int lane) {
  uint64_t rem = __ballot(m);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (rem == 0) return;  // wave-uniform
    const int leader = __ffsll((long long)rem) - 1;
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, leader);
    const bool same = m && d == d0;
    const uint64_t grp = __ballot(same);
    if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(grp));
    m = m && !same;
    rem &= ~grp;
  }
  if (m) atomicAdd(&h[d], 1u);
}

template <int DT>
__device__ __forceinline__ void hist_column(const void* col, const uint8_t* valid, const uint8_t* sel, int64_t n,
                                            int pass, int U, const uint64_t* upref, uint32_t* h) {
  const int lane = threadIdx.x & (kWave - 1);
  const int dshift = 64 - kQuantBits * (pass + 1);
  const int64_t trips = (n + kQuantTrip - 1) / kQuantTrip;
  // the trip loop is block-uniform: rows past n are dead lanes, never absent ones
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    const int64_t r0 = t * kQuantTrip + (int64_t)threadIdx.x * kQuantRun;
    u64 raw[kQuantRun];
    load_run_raw<DT>(col, r0, n, raw);
    unsigned live = mask_run(sel, r0, n);
    if (valid != nullptr) live &= mask_run(valid, r0, n);
#pragma unroll
    for (int j = 0; j < kQuantRun; ++j) {
      // nothing is narrowed: f64 stays f64, i64 rounds to nearest as a cast does
      const double x = raw_as_f64(raw[j], DT == DT_F64 || DT == DT_F32);
      const bool ok = ((live >> j) & 1u) && x == x;  // NaN is never counted ...
      const uint64_t key = float_key((u64)__double_as_longlong(x), true);  // ... so its key is never read
      const unsigned d = (unsigned)(key >> dshift) & (kQuantBins - 1);
      const uint64_t hi = pass == 0 ? 0ull : key >> (dshift + kQuantBits);
      for (int u = 0; u < U; ++u) count_digit(h + u * kQuantBins, ok && hi == upref[u], d, lane);
    }
  }
}

__global__ __launch_bounds__(kQuantThreads) void quantile_hist_kernel(QuantCols a, int pass, const int64_t* state,
                                                                      unsigned long long* hist) {
  __shared__ uint32_t h[kMaxQuantiles * kQuantBins];
  __shared__ uint64_t upref[kMaxQuantiles];
  const int c = blockIdx.y;
  const int64_t* s = state + (int64_t)c * quant_state_stride(a.Q);
  int U = 1;
  if (pass > 0) {
    U = (int)s[0];
    U = U < 1 ? 1 : (U > a.Q ? a.Q : U);
  }
  if (threadIdx.x < kMaxQuantiles) upref[threadIdx.x] = (pass > 0 && (int)threadIdx.x < U) ? (uint64_t)s[2 + threadIdx.x] : 0;
  for (int i = threadIdx.x; i < U * kQuantBins; i += kQuantThreads) h[i] = 0;
  __syncthreads();
  switch (a.dt[c]) {
    case DT_F64: hist_column<DT_F64>(a.col[c], a.valid[c], a.sel, a.n, pass, U, upref, h); break;
    case DT_F32: hist_column<DT_F32>(a.col[c], a.valid[c], a.sel, a.n, pass, U, upref, h); break;
    case DT_I32: hist_column<DT_I32>(a.col[c], a.valid[c], a.sel, a.n, pass, U, upref, h); break;
    default: hist_column<DT_I64>(a.col[c], a.valid[c], a.sel, a.n, pass, U, upref, h); break;
  }
  __syncthreads();
  unsigned long long* H = hist + (int64_t)c * a.Q * kQuantBins;
  for (int i = threadIdx.x; i < U * kQuantBins; i += kQuantThreads) {
    const uint32_t v = h[i];
    if (v != 0) atomicAdd(&H[i], (unsigned long long)v);
  }
}

// One block per column.  Thread t owns bin t of the target's slot; the counts below a bin come
// from scan.h's block scan, once per target.
__global__ __launch_bounds__(kQuantBins) void quantile_pick_kernel(int Q, int pass, const double* probs, int64_t* state,
                                                                   unsigned long long* hist, double* values,
                                                                   int64_t* counts) {
  __shared__ unsigned long long red[kQuantBins / kWave];
  __shared__ uint64_t npref[kMaxQuantiles];
  __shared__ int64_t nrank[kMaxQuantiles];
  __shared__ int64_t ntot;
  const int c = blockIdx.x, t = threadIdx.x;
  int64_t* s = state + (int64_t)c * quant_state_stride(Q);
  unsigned long long* H = hist + (int64_t)c * Q * kQuantBins;
  if (t < kMaxQuantiles) npref[t] = 0, nrank[t] = 0;
  if (t == 0) ntot = pass == 0 ? 0 : s[1];
  __syncthreads();
  for (int q = 0; q < Q; ++q) {
    const int slot = pass == 0 ? 0 : (int)s[2 + Q + q];
    const unsigned long long cnt = H[slot * kQuantBins + t];
    unsigned long long total;
    const int64_t excl = (int64_t)block_exclusive<AddU64, kQuantBins / kWave>(cnt, total, red);
    const int64_t inc = excl + (int64_t)cnt;
    int64_t rank;
    uint64_t pref = 0;
    if (pass == 0) {
      // QuantileSummaries.query on an exact summary: p = 0 the minimum, p = 1 the maximum, else
      // the 1-based rank ceil(p * n) of one double multiply
      const int64_t n = (int64_t)total;
      const double p = probs[q];
      if (p <= 0.0) rank = 1;
      else if (p >= 1.0) rank = n;
      else rank = (int64_t)ceil(p * (double)n);
      rank = rank < 1 ? 1 : (rank > n ? n : rank);  // (n = 0: rank 0, no bin matches)
      if (t == 0) ntot = n;
    } else {
      rank = s[2 + 2 * Q + q];
      pref = (uint64_t)s[2 + slot];
    }
    if (cnt > 0 && excl < rank && rank <= inc) {
      npref[q] = (pref << kQuantBits) | (uint64_t)t;
      nrank[q] = rank - excl;
    }
  }
  __syncthreads();
  // every read of state and hist is done: thread 0 regroups the targets by prefix, all re-zero
  if (t == 0) {
    int U = 0;
    for (int q = 0; q < Q; ++q) {
      int slot = -1;
      for (int p = 0; p < q && slot < 0; ++p)
        if (npref[p] == npref[q]) slot = (int)s[2 + Q + p];
      if (slot < 0) {
        slot = U++;
        s[2 + slot] = (int64_t)npref[q];
      }
      s[2 + Q + q] = slot;
      s[2 + 2 * Q + q] = nrank[q];
    }
    s[0] = U;
    s[1] = ntot;
    if (pass == kQuantPasses - 1) {
      counts[c] = ntot;
      for (int q = 0; q < Q; ++q)
        values[c * Q + q] = ntot > 0 ? __longlong_as_double((long long)unkey(npref[q])) : __longlong_as_double(0x7ff8000000000000ll);
    }
  }
  for (int i = t; i < Q * kQuantBins; i += kQuantBins) H[i] = 0ull;
}

void check_shape(int C, int Q) {
  if (Q < 1 || Q > kMaxQuantiles)
    throw std::invalid_argument("quantiles: between 1 and " + std::to_string(kMaxQuantiles) + " probabilities per call");
  if (C < 1 || C > kMaxQuantCols)
    throw std::invalid_argument("quantiles: between 1 and " + std::to_string(kMaxQuantCols) + " columns per launch");
}

}  // namespace

// x dimension: 4 blocks of 4 waves per CU and column (the grid is blocks x C, so C >= 2 columns
// already ask for more than the 8 wave slots per SIMD hold and the dispatcher queues the rest);
// 32 bytes in flight per thread cover the HBM latency, and the 16.1 KiB of static LDS per block
// would allow 9 blocks per CU, so the wave slots, not LDS, bound the residency
int quantile_blocks(int64_t n) { return grid_for(4, (n + kQuantTrip - 1) / kQuantTrip); }

void quantile_hist(const QuantCols& a, int pass, const int64_t* state, unsigned long long* hist, int blocks,
                   hipStream_t st) {
  check_shape(a.C, a.Q);
  if (pass < 0 || pass >= kQuantPasses) throw std::invalid_argument("quantiles: pass out of range");
  if (blocks < 1) throw std::invalid_argument("quantiles: blocks must be >= 1");
  if (a.n < 0) throw std::invalid_argument("quantiles: negative row count");
  for (int c = 0; c < a.C; ++c) {
    if (!is_key_dt(a.dt[c]) || a.dt[c] == DT_U8)  // (order statistics of a boolean: not offered)
      throw std::invalid_argument("quantiles: columns must be f64, f32, i32 or i64");
    if (a.col[c] == nullptr && a.n > 0) throw std::invalid_argument("quantiles: null column");
  }
  // the per-block LDS bins are u32: keep a block's rows below 2^32
  const int64_t need = a.n / ((int64_t)1 << 31) + 1;
  if (blocks < need) blocks = (int)need;
  if (a.n == 0) return;  // nothing to count; the counters stay zero
  hipLaunchKernelGGL(quantile_hist_kernel, dim3((unsigned)blocks, (unsigned)a.C), dim3(kQuantThreads), 0, st, a, pass,
                     state, hist);
  DQ_HIP_CHECK(hipGetLastError());
}

void quantile_pick(int C, int Q, int pass, const double* probs, int64_t* state, unsigned long long* hist,
                   double* values, int64_t* counts, hipStream_t st) {
  check_shape(C, Q);
  if (pass < 0 || pass >= kQuantPasses) throw std::invalid_argument("quantiles: pass out of range");
  hipLaunchKernelGGL(quantile_pick_kernel, dim3((unsigned)C), dim3(kQuantBins), 0, st, Q, pass, probs, state, hist,
                     values, counts);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
