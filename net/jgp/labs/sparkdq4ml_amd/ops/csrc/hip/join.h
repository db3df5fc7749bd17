// Equi-join of two 64-bit key columns (see join.hip): the right side builds an open-addressing
// table of its keys (slot -> count, first row), the left side probes it, and an expansion pass
// writes the (left row, right row) pairs in a defined order: left rows in row order, the matches
// of one left row in right row order.  Every loop in these kernels is bounded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "keys.h"

namespace dq4ml {

constexpr int kJoinRun = 4;  // consecutive rows per thread and trip
constexpr int kJoinThreads = 256;
constexpr int kJoinTrip = kJoinRun * kJoinThreads;     // rows per block and grid-stride trip
constexpr int kJoinOutRun = 8;                         // output positions per thread and tile
constexpr int kJoinTile = kJoinOutRun * kJoinThreads;  // output positions per expansion tile
constexpr int kJoinLdsRows = 4096;                     // left rows of a tile whose offsets are staged in LDS (16 KiB)
constexpr int64_t kJoinMaxCapacity = (int64_t)1 << 30; // slot ids (and the extra slot `capacity`) fit an i32

// probe modes
enum JoinMode : int {
  JOIN_INNER = 0,  // a row without a match gives no pair
  JOIN_OUTER = 1,  // a live row without a match gives one pair (l, -1)
  JOIN_FULL = 2,   // JOIN_OUTER, and matched[slot] = 1 for every slot a left row met
  JOIN_SEMI = 3,   // only mask[l] = 1 when the row has a match (nothing is counted)
};

// occupancy-sized grid for n rows / for `total` output positions
int join_blocks(int64_t n);
int join_expand_blocks(int64_t total);
// table: capacity u64 slots, all ones on entry; cnt [capacity + 1] u32 zeroed; first [capacity + 1]
// i32 set to INT32_MAX; bslot [n] i32; state: [distinct keys in the table, rows inserted, overflow,
// the all-ones key was seen] zeroed.  The all-ones key owns the extra slot `capacity`.
void join_build(const KeyCol& right, unsigned long long* table, int64_t capacity, unsigned* cnt, int* first, int* bslot,
                unsigned long long* state, int blocks, hipStream_t st);
// pslot [n] i32 (-1: no match), pcnt [n] i32 (output pairs of the row), matched [capacity + 1] u8
// (JOIN_FULL), mask [n] u8 (JOIN_SEMI; pslot and pcnt are not written then)
void join_probe(const KeyCol& left, const unsigned long long* table, int64_t capacity, const unsigned* cnt, int mode,
                int* pslot, int* pcnt, uint8_t* matched, uint8_t* mask, int blocks, hipStream_t st);
// offsets [n_left + 1] i64: the exclusive prefix sum of pcnt and the total.  li / ri [total] i64.
// start [capacity + 1] i32 and brow [nbrow] i32 (the right rows grouped by slot, in row order), or
// both null when every right key is unique: then first[slot] is the slot's only row.
void join_expand(const int64_t* offsets, int64_t n_left, int64_t total, const int* pslot, const int* start, const int* brow,
                 int64_t nbrow, const int* first, int64_t capacity, int64_t* li, int64_t* ri, int blocks, hipStream_t st);

}  // namespace dq4ml
