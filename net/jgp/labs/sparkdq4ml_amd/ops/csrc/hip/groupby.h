// Grouped aggregation (see groupby.hip): one key column -> dense-or-direct group ids, then up to
// kGroupMaxSlots integer-only aggregate slots per pass over the rows.  Every accumulator is a
// 64-bit integer word updated with integer atomics, so the raw accumulators do not depend on the
// grid, the schedule or a shard split.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "keys.h"

namespace dq4ml {

constexpr int kGroupRun = 4;  // consecutive rows per thread and trip
constexpr int kGroupThreads = 256;
constexpr int kGroupTrip = kGroupRun * kGroupThreads;  // rows per block and grid-stride trip
constexpr int kGroupMaxSlots = 8;                      // aggregate slots per call (the launcher chunks above it)
constexpr int kGroupSumWords = 5;                      // SUM_F: 4 limbs + 1 flag word
constexpr int kGroupMaxWords = kGroupMaxSlots * kGroupSumWords;
constexpr int kGroupLdsWords = 4096;  // G * words at or below this accumulates in LDS (32 KiB of u64)
constexpr int64_t kGroupDefaultCapacity = 1 << 16;  // first hash table (u64 slots), grown 8x on overflow
constexpr int64_t kGroupDirectCap = 1 << 20;        // integer keys whose live range is at most this skip the table

enum GroupOp : int {
  GOP_ROWS = 0,    // +1 per live row
  GOP_COUNT = 1,   // +1 per live non-null row
  GOP_SUM_I = 2,   // i64 add (wraps)
  GOP_SUM_F = 3,   // 4 fixed-point limbs (i64 adds) + flag word (OR: 1 NaN, 2 +inf, 4 -inf)
  GOP_MIN = 4,     // u64 min of the order key
  GOP_MAX = 5,     // u64 max of the order key
  GOP_FIRST = 6,   // min of row_offset + row index
  GOP_ABSMAX = 7,  // u64 max of the bits of |x| over finite x
};

// how one accumulator word is updated; its identity is 0 except for GK_MIN (all ones)
enum GroupWordKind : int { GK_ADD = 0, GK_OR = 1, GK_MAX = 2, GK_MIN = 3 };

// One call, by value in the kernarg.  Slot s owns the words [woff[s], woff[s] + words of op[s]) of
// every group's row of the [G, words] accumulator.  gid null: every live row is group 0.
struct GroupAggArgs {
  const void* col[kGroupMaxSlots];
  const uint8_t* valid[kGroupMaxSlots];
  int op[kGroupMaxSlots];
  int dt[kGroupMaxSlots];
  int e[kGroupMaxSlots];  // SUM_F: frexp exponent of the largest finite |x|
  int woff[kGroupMaxSlots];
  const int* gid;
  const uint8_t* sel;
  int64_t n;
  int64_t row_offset;
  int G, S, words;
};

__host__ __device__ constexpr int group_op_words(int op) { return op == GOP_SUM_F ? kGroupSumWords : 1; }

// occupancy-sized grid for n rows
int group_blocks(int64_t n);
// acc is [G, words] u64, initialised by the caller to each word's identity
void group_agg(const GroupAggArgs& a, unsigned long long* acc, int blocks, hipStream_t st);
// gid[r] = -1 (dead), 0 (null key) or key - base + 1; values outside [base, base + span) are dead
void group_encode_direct(const KeyCol& a, int64_t base, int64_t span, int* gid, int blocks, hipStream_t st);
// table: capacity u64 slots, all ones on entry; state: [occupied, overflow, has_null, has_top] zeroed
void group_hash_insert(const KeyCol& a, unsigned long long* table, int64_t capacity, unsigned long long* state,
                       int blocks, hipStream_t st);
// row -> slot -> slot_gid[slot]; null keys get 0, the all-ones key (out of band) gets top_gid
void group_hash_lookup(const KeyCol& a, const unsigned long long* table, int64_t capacity, const int* slot_gid,
                       int top_gid, int* gid, int blocks, hipStream_t st);

}  // namespace dq4ml
