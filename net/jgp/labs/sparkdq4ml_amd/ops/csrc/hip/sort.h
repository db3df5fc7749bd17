// Stable LSD radix sort of (u64 order key, u32 row index) pairs (see sort.hip): 8-bit digits,
// ping-pong buffers, reduce-then-scan.  Every pass is three ordinary launches (count, scan,
// scatter) over fixed tiles of kSortTile consecutive positions; nothing waits on another block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

constexpr int kSortThreads = 256;                    // 4 waves per block
constexpr int kSortRun = 8;                          // keys per thread and tile (rounds of 64 per wave)
constexpr int kSortTile = kSortThreads * kSortRun;   // positions per tile
constexpr int kSortBits = 8;                         // digit width
constexpr int kSortBins = 1 << kSortBits;
constexpr int kSortDigits = 64 / kSortBits;          // key digits; digit kSortDigits is the null digit
constexpr int kSortHists = kSortDigits + 1;
constexpr unsigned kSortNullBit = 0x80000000u;       // carried in the top bit of the stored row index

// one sort column read through a permutation
struct SortKeyCol {
  const void* col;
  const uint8_t* valid;  // 0/1 per row, or null
  const unsigned* perm;  // row of position i (top bit ignored), or null: the identity
  int64_t n;             // rows of the column
  int64_t m;             // positions
  int dt;
  int descending;
};

// tiles of m positions
inline int64_t sort_tiles(int64_t m) { return (m + kSortTile - 1) / kSortTile; }
// occupancy-sized grid for m positions
int sort_blocks(int64_t m);
// keys[i], idx[i] (row | kSortNullBit when the row is null) for i < m; hist [kSortHists][kSortBins]
// u64, zeroed by the caller, receives the digit counts
void sort_keys(const SortKeyCol& a, unsigned long long* keys, unsigned* idx, unsigned long long* hist, int blocks,
               hipStream_t st);
// One pass on digit `digit` (kSortDigits: the null digit).  counts: [kSortBins][stride] u32 with
// stride >= sort_tiles(m) a multiple of 4; hist_row: the digit's kSortBins global counts; base: the
// first output position of each bin.  Stable: equal digits keep their order.
void sort_pass(const unsigned long long* keys_in, const unsigned* idx_in, unsigned long long* keys_out,
               unsigned* idx_out, int64_t m, int digit, unsigned* counts, int64_t stride,
               const unsigned long long* hist_row, const unsigned* base, int blocks, hipStream_t st);

}  // namespace dq4ml
