// Window functions over the sorted positions of one window specification (see window.hip): rows
// are read through the sort permutation, every scan is reduce-then-scan in three ordinary launches
// over fixed tiles of kWinTile consecutive positions; nothing waits on another block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

constexpr int kWinThreads = 256;                  // 4 waves per block
constexpr int kWinRun = 8;                        // consecutive positions per thread and tile
constexpr int kWinTile = kWinThreads * kWinRun;   // positions per tile
constexpr int kWinMaxKeys = 8;                    // key columns per heads launch (the launcher chunks above it)
constexpr int kWinMaxWords = 8;                   // prefix words per pass, output words per finish launch
constexpr int kWinSumWords = 7;                   // SUM_F: 4 limbs + the counts of NaN, +inf, -inf
constexpr unsigned kWinRowMask = 0x7fffffffu;     // the sort carries a null flag in the top bit of a row index

// the word kinds of a prefix pass (the codes of the GroupOp they accumulate like)
enum WinWord : int { WW_ROWS = 0, WW_COUNT = 1, WW_SUM_I = 2, WW_SUM_F = 3 };

// what window_finish writes into one output word
enum WinOut : int {
  WO_DIFF = 0,      // src: one prefix word [m]; P[hi] - P[lo - 1], 0 over an empty frame
  WO_PICK_HI = 1,   // src: a min / max scan [m]; its value at hi (0 over an empty frame)
  WO_PICK_LO = 2,   // ... at lo
  WO_ROW_NUMBER = 3,
  WO_RANK = 4,
  WO_DENSE_RANK = 5,
  WO_PART_SIZE = 6,
  WO_PEER_END = 7,  // peer_end - part_start + 1: the rows at or before the current row's peers
  WO_SHIFT = 8,     // arg: signed distance d; the row at position i + d, -1 outside the partition
};

__host__ __device__ constexpr int win_word_count(int op) { return op == WW_SUM_F ? kWinSumWords : 1; }

// the key columns of one heads launch, by value in the kernarg; part[c] != 0: a partition column
struct WinKeyArgs {
  const void* col[kWinMaxKeys];
  const uint8_t* valid[kWinMaxKeys];
  int dt[kWinMaxKeys];
  int part[kWinMaxKeys];
  const unsigned* perm;
  int64_t n, m;
  int K;
  int accumulate;  // OR into heads (a later chunk of the columns)
};

// the slots of one prefix pass; slot s owns the words [woff[s], woff[s] + win_word_count(op[s]))
struct WinPrefixArgs {
  const void* col[kWinMaxWords];
  const uint8_t* valid[kWinMaxWords];
  int op[kWinMaxWords];
  int dt[kWinMaxWords];
  int e[kWinMaxWords];
  int woff[kWinMaxWords];
  const unsigned* perm;
  int64_t n, m;
  int S, words;
};

struct WinBounds {
  const unsigned *part_start, *peer_start, *part_end, *peer_end, *dense;
};

struct WinFinishArgs {
  WinBounds b;
  const unsigned* perm;
  const void* src[kWinMaxWords];
  int kind[kWinMaxWords];
  long long arg[kWinMaxWords];
  int64_t n, m;
  int words;
  int is_range, lo_unbounded, hi_unbounded;
  long long lo_off, hi_off;  // rows frame: offsets from the current position
};

inline int64_t win_tiles(int64_t m) { return (m + kWinTile - 1) / kWinTile; }
// occupancy-sized grid for m positions
int window_blocks(int64_t m);
// heads[i]: bit 0 first position of its partition, bit 1 first position of its peer group
void window_heads(const WinKeyArgs& a, uint8_t* heads, int blocks, hipStream_t st);
// part_start / peer_start / part_end / peer_end / dense, [m] u32 each; totals: 2 * win_tiles(m) * 16 bytes
void window_bounds(const uint8_t* heads, int64_t m, unsigned* part_start, unsigned* peer_start, unsigned* part_end,
                   unsigned* peer_end, unsigned* dense, void* totals, int blocks, hipStream_t st);
// prefix: [words][m] i64 inclusive sums; totals: [words][win_tiles(m)] i64
void window_prefix(const WinPrefixArgs& a, long long* prefix, long long* totals, int blocks, hipStream_t st);
// out[i]: min (max) of the unfolded order keys of the non-null rows from the partition's first
// (backward: last) position to i, all ones (0) when there is none; totals: win_tiles(m) * 16 bytes
void window_minmax(const void* col, int dt, const uint8_t* valid, const unsigned* perm, int64_t n, int64_t m,
                   const uint8_t* heads, bool is_max, bool backward, unsigned long long* out, void* totals, int blocks,
                   hipStream_t st);
// Self-test of the row walker of scan.h under the operators it runs with: the exclusive scan of
// every row of a [rows][len] array, in place.  kind 0: i64 add; 1: u32 add, four entries per thread
// (the rows pitched at len rounded up to 4); 2 / 3: the forward / backward bounds triples of
// window_bounds, 16 bytes (a, b, c, -) each; 4: the segmented min of window_minmax, 16 bytes (u64
// key, u32 flag, -) each.
void scan_rows(int kind, void* a, int64_t rows, int64_t len, hipStream_t st);
// out: [n][words] i64, row perm[i] receives position i's words
void window_finish(const WinFinishArgs& a, long long* out, int blocks, hipStream_t st);

}  // namespace dq4ml
