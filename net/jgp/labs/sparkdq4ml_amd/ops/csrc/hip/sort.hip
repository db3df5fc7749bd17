// Stable LSD radix sort of (u64 order key, u32 row index) pairs.
//
// sort_keys builds the keys of one sort column through the current permutation: the folded order
// key of keys.h (-0.0 == +0.0, one canonical NaN above +inf, integers biased by the sign bit),
// complemented for a descending order; a null row gets key 0 and carries its null flag in the top
// bit of its stored row index (row indices are below 2^31).  The same launch histograms the eight
// key bytes and the null digit, so the launcher knows which digits are constant over the live rows
// (their passes are skipped) and where each bin of a live digit starts.
//
// A pass sorts stably by one 8-bit digit in three ordinary launches over fixed tiles of kSortTile
// consecutive positions (the tiling depends on m alone; the grid only deals the tiles):
//   count    counts[digit value][tile]
//   scan     per digit value, the exclusive scan over the tiles added to the bin's global base
//   scatter  re-reads the tile and ranks it: a wave owns kSortRun rounds of 64 consecutive keys; in
//            a round the lanes that share a digit find each other with one __ballot per digit bit
//            and rank by the population count of the peers below; per-wave digit counters in LDS
//            carry the rounds, an exclusive scan over the block's waves carries the waves.  The
//            tile is written to LDS in digit order and stored from there, so that consecutive
//            lanes store consecutive positions of a digit value's run.
// No kernel waits on another block; only integer LDS / global atomics and plain stores are used.
// Both scans (the tiles of a digit value, the digit values of a tile) are scan.h's.
#include "sort.h"

#include <stdexcept>

#include "common.h"
#include "keys.h"
#include "scan.h"

namespace dq4ml {
namespace {

constexpr int kSortWaves = kSortThreads / kWave;
static_assert(kSortThreads == kSortBins, "thread d owns digit value d in the count and scatter kernels");

// the digit of a pair: a key byte, or the null flag for digit kSortDigits (block-uniform choice)
__device__ __forceinline__ unsigned digit_of(u64 key, unsigned idx, int digit) {
  return digit < kSortDigits ? (unsigned)(key >> (kSortBits * digit)) & (kSortBins - 1) : idx >> 31;
}

// +1 in bin b of h for every lane with `on` set.  When the live lanes of the wave agree (a constant
// byte, the common case of the high bytes) one lane adds their number.  Every lane calls this.
__device__ __forceinline__ void hist_add(unsigned* h, bool on, unsigned b, int lane) {
  const uint64_t act = __ballot(on);
  if (act == 0) return;  // wave-uniform
  const int leader = __ffsll((long long)act) - 1;
  const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)b, leader);
  if (__ballot(on && b != b0) == 0) {
    if (lane == leader) atomicAdd(h + b0, (unsigned)__popcll(act));
  } else if (on) {
    atomicAdd(h + b, 1u);
  }
}

__global__ __launch_bounds__(kSortThreads) void sort_keys_kernel(SortKeyCol a, u64* keys, unsigned* idx, u64* hist) {
  __shared__ unsigned h[kSortHists * kSortBins];
  for (int i = threadIdx.x; i < kSortHists * kSortBins; i += kSortThreads) h[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const bool isf = is_float_dt(a.dt);
  const int64_t tiles = (a.m + kSortTile - 1) / kSortTile;
  // the tile loop is block-uniform: positions past m are dead lanes, never absent ones
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      const int64_t i = t * kSortTile + j * kSortThreads + threadIdx.x;
      const bool on = i < a.m;
      u64 key = 0;
      unsigned out = 0;
      if (on) {
        const int64_t r = a.perm != nullptr ? (int64_t)(gptr<unsigned>(a.perm)[i] & ~kSortNullBit) : i;
        bool null = r >= a.n;  // (never, for a permutation of the column's rows: no read past the column)
        if (!null && a.valid != nullptr) null = gptr<uint8_t>(a.valid)[r] == 0;
        if (!null) {
          key = order_key(load_raw(a.col, a.dt, r), isf, true);
          if (a.descending) key = ~key;
        }
        out = (unsigned)r | (null ? kSortNullBit : 0u);
        keys[i] = key;
        idx[i] = out;
      }
#pragma unroll
      for (int d = 0; d < kSortHists; ++d) hist_add(h + d * kSortBins, on, digit_of(key, out, d), lane);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSortHists * kSortBins; i += kSortThreads)
    if (h[i] != 0) atomicAdd(hist + i, (u64)h[i]);
}

__global__ __launch_bounds__(kSortThreads) void sort_count_kernel(const u64* keys, const unsigned* idx, int64_t m, int digit,
                                                                  unsigned* counts, int64_t stride) {
  __shared__ unsigned h[kSortWaves][kSortBins];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t tiles = (m + kSortTile - 1) / kSortTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) h[w][threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      const int64_t i = t * kSortTile + j * kSortThreads + threadIdx.x;
      const bool on = i < m;
      unsigned b = 0;
      if (on) b = digit < kSortDigits ? digit_of(gptr<u64>(keys)[i], 0u, digit) : gptr<unsigned>(idx)[i] >> 31;
      hist_add(h[wave], on, b, lane);
    }
    __syncthreads();
    unsigned c = 0;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) c += h[w][threadIdx.x];
    counts[(int64_t)threadIdx.x * stride + t] = c;
    __syncthreads();
  }
}

// block d: counts[d][0 .. tiles) -> base[d] + its exclusive scan, in place
__global__ __launch_bounds__(kSortThreads) void sort_scan_kernel(unsigned* counts, int64_t stride, int64_t tiles,
                                                                 const u64* hist_row, const unsigned* base) {
  __shared__ unsigned red[kSortWaves];
  const int d = blockIdx.x;
  if (gptr<u64>(hist_row)[d] == 0) return;  // (block-uniform) no pair carries this digit value: its row is never read
  // a thread owns a quad (stride is a multiple of 4: the whole quad is inside the row, and its
  // padding, which the count kernel never wrote, reads as 0)
  scan_row<AddU32, kSortWaves, 4>(counts + (int64_t)d * stride, tiles, gptr<unsigned>(base)[d], red);
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const u64* keys_in, const unsigned* idx_in, u64* keys_out,
                                                                    unsigned* idx_out, int64_t m, int digit,
                                                                    const unsigned* counts, int64_t stride) {
  // per wave and digit value: the pairs ranked so far, then the wave's first slot in the staged tile
  __shared__ unsigned cnt[kSortWaves][kSortBins];
  __shared__ unsigned dbase[kSortBins], red[kSortWaves];
  __shared__ u64 skey[kSortTile];  // the tile staged in digit order (24 KiB with the indices)
  __shared__ unsigned sidx[kSortTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint64_t below = (1ull << lane) - 1ull;
  const int bits = digit < kSortDigits ? kSortBits : 1;  // block-uniform
  volatile unsigned* mine = cnt[wave];
  const int64_t tiles = (m + kSortTile - 1) / kSortTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    // the wave owns kSortRun rounds of 64 consecutive positions
    const int64_t p0 = t * kSortTile + (int64_t)wave * (kWave * kSortRun) + lane;
    u64 key[kSortRun];
    unsigned ix[kSortRun], where[kSortRun];  // where: digit value (low 8 bits) | rank inside the wave << 8
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      const int64_t i = p0 + j * kWave;
      key[j] = i < m ? gptr<u64>(keys_in)[i] : 0ull;
      ix[j] = i < m ? gptr<unsigned>(idx_in)[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      const bool on = p0 + j * kWave < m;
      const unsigned d = digit_of(key[j], ix[j], digit);
      uint64_t peers = __ballot(on);  // lanes past m take no part
      for (int b = 0; b < bits; ++b) {
        const bool set = (d >> b) & 1u;
        const uint64_t mb = __ballot(set);
        peers &= set ? mb : ~mb;
      }
      const unsigned rank = (unsigned)__popcll(peers & below), c = (unsigned)__popcll(peers);
      unsigned old = 0;
      if (on) {
        old = mine[d];
        if (rank == c - 1) mine[d] = old + c;  // the last peer closes the round for its digit value
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next round reads what this one wrote
      where[j] = d | ((old + rank) << kSortBits);
    }
    __syncthreads();
    {
      // thread d: digit value d over the block's waves, then over the digit values of the tile
      unsigned tot = 0, pre[kSortWaves];
#pragma unroll
      for (int w = 0; w < kSortWaves; ++w) pre[w] = tot, tot += cnt[w][threadIdx.x];
      unsigned all;  // (the pairs of the tile)
      const unsigned start = block_exclusive<AddU32, kSortWaves>(tot, all, red);  // first slot of digit value d in the staged tile
#pragma unroll
      for (int w = 0; w < kSortWaves; ++w) cnt[w][threadIdx.x] = start + pre[w];
      // slot p of the staged tile goes to position dbase[d] + p (unsigned wrap-around is intended)
      dbase[threadIdx.x] = gptr<unsigned>(counts)[(int64_t)threadIdx.x * stride + t] - start;
    }
    __syncthreads();
    // stage the tile in digit order ...
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      if (p0 + j * kWave < m) {
        const unsigned p = cnt[wave][where[j] & (kSortBins - 1)] + (where[j] >> kSortBits);
        if (p < (unsigned)kSortTile) skey[p] = key[j], sidx[p] = ix[j];  // (always: p counts pairs of this tile)
      }
    }
    __syncthreads();
    // ... so that consecutive lanes store consecutive positions of a digit value's run
    const int64_t left = m - t * kSortTile;
    const unsigned held = left < kSortTile ? (unsigned)left : (unsigned)kSortTile;
#pragma unroll
    for (int j = 0; j < kSortRun; ++j) {
      const unsigned p = j * kSortThreads + threadIdx.x;
      if (p < held) {
        const u64 k = skey[p];
        const unsigned x = sidx[p];
        const int64_t dst = (int64_t)(unsigned)(dbase[digit_of(k, x, digit)] + p);
        if (dst < m) {  // (always, for counts of these very pairs: no store past the buffers)
          keys_out[dst] = k;
          idx_out[dst] = x;
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

// up to 8 blocks of 4 waves per CU (the scatter's 29 KiB of LDS allow 5); the rest of the tiles are grid-strided
int sort_blocks(int64_t m) { return grid_for(8, sort_tiles(m)); }

void sort_keys(const SortKeyCol& a, unsigned long long* keys, unsigned* idx, unsigned long long* hist, int blocks,
               hipStream_t st) {
  if (a.m < 0 || a.n < 0) throw std::invalid_argument("sort: negative row count");
  if (a.m >= ((int64_t)1 << 31) || a.n >= ((int64_t)1 << 31)) throw std::invalid_argument("sort: fewer than 2^31 rows per call");
  if (blocks < 1) throw std::invalid_argument("sort: blocks must be >= 1");
  if (!is_key_dt(a.dt)) throw std::invalid_argument("sort: columns must be f64, f32, i32, i64 or u8");
  if (a.perm == nullptr && a.m > a.n) throw std::invalid_argument("sort: more positions than rows");
  if (a.m == 0) return;
  if (a.col == nullptr || keys == nullptr || idx == nullptr || hist == nullptr) throw std::invalid_argument("sort: null buffer");
  hipLaunchKernelGGL(sort_keys_kernel, dim3((unsigned)blocks), dim3(kSortThreads), 0, st, a, keys, idx, hist);
  DQ_HIP_CHECK(hipGetLastError());
}

void sort_pass(const unsigned long long* keys_in, const unsigned* idx_in, unsigned long long* keys_out, unsigned* idx_out,
               int64_t m, int digit, unsigned* counts, int64_t stride, const unsigned long long* hist_row,
               const unsigned* base, int blocks, hipStream_t st) {
  if (m < 0) throw std::invalid_argument("sort: negative row count");
  if (m >= ((int64_t)1 << 31)) throw std::invalid_argument("sort: fewer than 2^31 rows per call");
  if (blocks < 1) throw std::invalid_argument("sort: blocks must be >= 1");
  if (digit < 0 || digit > kSortDigits) throw std::invalid_argument("sort: digit out of range");
  const int64_t tiles = sort_tiles(m);
  if (stride < tiles || (stride & 3) != 0 || (reinterpret_cast<uintptr_t>(counts) & 15) != 0)
    throw std::invalid_argument("sort: the counts rows must hold the tiles, padded to 4 entries and 16-byte aligned");
  if (m == 0) return;
  if (keys_in == nullptr || idx_in == nullptr || keys_out == nullptr || idx_out == nullptr || counts == nullptr ||
      hist_row == nullptr || base == nullptr)
    throw std::invalid_argument("sort: null buffer");
  if (keys_in == keys_out || idx_in == idx_out) throw std::invalid_argument("sort: a pass needs distinct in and out buffers");
  hipLaunchKernelGGL(sort_count_kernel, dim3((unsigned)blocks), dim3(kSortThreads), 0, st, keys_in, idx_in, m, digit, counts,
                     stride);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(kSortBins), dim3(kSortThreads), 0, st, counts, stride, tiles, hist_row, base);
  hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)blocks), dim3(kSortThreads), 0, st, keys_in, idx_in, keys_out, idx_out,
                     m, digit, counts, stride);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
