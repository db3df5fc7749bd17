// Equi-join of two key columns on the open-addressing table of hashtable.h.
//
// The key of a row is the folded order key of keys.h (-0.0 == 0.0, every NaN one value, integers
// as i64), so equal keys are equal u64 words.  A null key matches nothing; a row outside its
// side's selection does not exist.  The right side builds, the left side probes.
//
//   build   one pass over the right rows: the key's slot is found or claimed, cnt[slot] counts the
//           slot's rows, first[slot] keeps its smallest row (integer atomicMin), bslot[r] is the
//           row's slot (-1: dead or null key).  The all-ones key (INT64_MAX) cannot enter the table
//           and owns the extra slot `capacity`.
//   probe   one pass over the left rows: pslot[l] is the slot of the row's key (-1: no match) and
//           pcnt[l] the pairs the row gives: cnt[slot], 1 for an unmatched live row of an outer
//           join, else 0.  A full outer join marks matched[slot] (a plain store of 1 from every
//           lane that meets the slot).  A semi join writes only the mask pcnt > 0.
//   expand  over fixed tiles of kJoinTile output positions (the tiling depends on the total alone;
//           the grid only deals the tiles): two waves find the left rows of the tile's first and
//           last position by a 64-ary search of the offsets, the block stages the offsets of that
//           row range in LDS when it holds at most kJoinLdsRows rows, and every lane finds the row
//           of its positions by a binary search there (else in the global array).  The work of a
//           lane is kJoinOutRun positions whatever the multiplicity of a key.
//
// Every loop is bounded: a probe sequence by the capacity, a search by its round count.  An insert
// that finds no free slot sets the overflow word, and the blocks stop inserting once it is set.
// Only integer atomics and plain stores are used; nothing waits on another block.
#include "join.h"

#include <stdexcept>

#include "common.h"
#include "hashtable.h"
#include "keys.h"

namespace dq4ml {
namespace {

static_assert(kJoinRun == kRawRun, "the run loaders of keys.h read kJoinRun rows");
static_assert(kJoinThreads >= 2 * kWave, "the expansion's two boundary searches take a wave each");

// state: [0] distinct keys in the table, [1] rows inserted, [2] overflow, [3] the all-ones key was seen
__global__ __launch_bounds__(kJoinThreads) void join_build_kernel(KeyCol a, u64* table, u64 mask, unsigned* cnt, int* first,
                                                                  int* bslot, u64* state) {
  const int lane = threadIdx.x & (kWave - 1);
  const int top = (int)(mask + 1);  // the slot of the all-ones key
  const int64_t trips = (a.n + kJoinTrip - 1) / kJoinTrip;
  unsigned inserted = 0;
  bool saw_top = false, full = false;
  // the trip loop is block-uniform: rows past n are dead lanes, never absent ones
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    // a full table: stop inserting, the launcher raises (wave-uniform read)
    if (__builtin_amdgcn_readfirstlane((int)load_slot(state + 2)) != 0) break;
    const int64_t r0 = t * kJoinTrip + (int64_t)threadIdx.x * kJoinRun;
    const KeyRun k = load_keys(a, r0);
    int s[kJoinRun];
#pragma unroll
    for (int j = 0; j < kJoinRun; ++j) {
      const int row = (int)(r0 + j);
      bool ins = (k.valid >> j) & 1u;
      int slot = -1;
      if (ins && k.key[j] == kEmpty) {
        slot = top, saw_top = true, ins = false;
        atomicAdd(cnt + top, 1u);
        atomicMin(first + top, row);
        ++inserted;
      }
      // the lanes that hold the first live lane's key claim once: the leader adds their number, and
      // its row is their smallest (rows ascend with the lane)
      const uint64_t rem = __ballot(ins);
      if (rem != 0) {
        const int leader = __ffsll((long long)rem) - 1;
        const u64 k0 = __shfl(k.key[j], leader, kWave);
        const bool same = ins && k.key[j] == k0;
        const uint64_t grp = __ballot(same);
        int s0 = -1;
        if (lane == leader) {
          s0 = (int)table_claim(table, mask, state, k0);
          if (s0 >= 0) {
            atomicAdd(cnt + s0, (unsigned)__popcll(grp));
            atomicMin(first + s0, row);
          }
        }
        s0 = __builtin_amdgcn_readlane(s0, leader);
        if (same) {
          slot = s0, ins = false;
          if (s0 >= 0) ++inserted;
          else full = true;
        }
      }
      if (ins) {
        slot = (int)table_claim(table, mask, state, k.key[j]);
        if (slot >= 0) {
          atomicAdd(cnt + slot, 1u);
          atomicMin(first + slot, row);
          ++inserted;
        } else {
          full = true;
        }
      }
      s[j] = slot;
    }
    store_run(bslot, r0, a.n, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) inserted += __shfl_xor(inserted, o, kWave);
  if (lane == 0 && inserted != 0) atomicAdd(state + 1, (u64)inserted);
  if (full) atomicOr(state + 2, 1ull);
  if (saw_top) atomicOr(state + 3, 1ull);
}

__global__ __launch_bounds__(kJoinThreads) void join_probe_kernel(KeyCol a, const u64* table, u64 mask, const unsigned* cnt,
                                                                  int mode, int* pslot, int* pcnt, uint8_t* matched,
                                                                  uint8_t* out_mask) {
  const int64_t top = (int64_t)(mask + 1);
  const int64_t trips = (a.n + kJoinTrip - 1) / kJoinTrip;
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    const int64_t r0 = t * kJoinTrip + (int64_t)threadIdx.x * kJoinRun;
    const KeyRun k = load_keys(a, r0);
    int ps[kJoinRun], pc[kJoinRun];
#pragma unroll
    for (int j = 0; j < kJoinRun; ++j) {
      const bool live = (k.live >> j) & 1u, valid = (k.valid >> j) & 1u;
      int slot = -1;
      unsigned c = 0;
      if (valid) {
        const int64_t s = k.key[j] == kEmpty ? top : table_slot(table, mask, k.key[j]);
        if (s >= 0) c = gptr<unsigned>(cnt)[s];
        if (c > 0) slot = (int)s;
      }
      if (mode == JOIN_FULL && slot >= 0) matched[slot] = 1;
      ps[j] = slot;
      pc[j] = c > 0 ? (int)c : ((mode == JOIN_OUTER || mode == JOIN_FULL) && live ? 1 : 0);
    }
    if (mode == JOIN_SEMI) {  // block-uniform
#pragma unroll
      for (int j = 0; j < kJoinRun; ++j)
        if (r0 + j < a.n) out_mask[r0 + j] = pc[j] > 0 ? 1 : 0;
    } else {
      store_run(pslot, r0, a.n, ps);
      store_run(pcnt, r0, a.n, pc);
    }
  }
}

// the largest row l of [0, n) with off[l] <= o, for off ascending, off[0] <= o: a 64-ary search by
// the whole wave (six rounds reach one row from 2^31); the result is wave-uniform
__device__ __forceinline__ int64_t wave_row_of(const int64_t* off, int64_t n, int64_t o, int lane) {
  int64_t lo = 0, hi = n;  // the answer lies in [lo, hi)
  for (int round = 0; round < 8; ++round) {
    const int64_t len = hi - lo;
    if (len <= 1) break;  // wave-uniform
    const int64_t step = (len + kWave - 1) / kWave;
    const int64_t i = lo + (int64_t)lane * step;
    const bool ok = i < hi && gptr<int64_t>(off)[i] <= o;  // a prefix of the lanes (lane 0 always)
    const int c = __popcll(__ballot(ok));
    lo += (int64_t)(c > 0 ? c - 1 : 0) * step;
    hi = hi < lo + step ? hi : lo + step;
  }
  return lo;
}

__global__ __launch_bounds__(kJoinThreads) void join_expand_kernel(const int64_t* off, int64_t n_left, int64_t total,
                                                                   const int* pslot, const int* start, const int* brow,
                                                                   int64_t nbrow, const int* first, int64_t capacity, int64_t* li,
                                                                   int64_t* ri) {
  __shared__ int soff[kJoinLdsRows];  // offsets of the tile's left rows, relative to the tile's first position
  __shared__ int64_t srow[2];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t tiles = (total + kJoinTile - 1) / kJoinTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t o0 = t * kJoinTile;
    const int64_t o1 = o0 + kJoinTile < total ? o0 + kJoinTile : total;
    if (wave < 2) {  // the left rows of the tile's first and last position
      const int64_t r = wave_row_of(off, n_left, wave == 0 ? o0 : o1 - 1, lane);
      if (lane == 0) srow[wave] = r;
    }
    __syncthreads();
    const int64_t l0 = srow[0];
    const int64_t rows = srow[1] - l0 + 1;  // at least 1, at most n_left - l0
    const bool staged = rows <= kJoinLdsRows;  // block-uniform
    if (staged)
      for (int i = threadIdx.x; i < (int)rows; i += kJoinThreads) soff[i] = (int)(gptr<int64_t>(off)[l0 + i] - o0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kJoinOutRun; ++j) {
      const int64_t o = o0 + j * kJoinThreads + threadIdx.x;
      if (o >= o1) continue;
      int64_t l, k;
      if (staged) {
        const int p = (int)(o - o0);
        int lo = 0, len = (int)rows;  // the largest i with soff[i] <= p lies in [lo, lo + len)
        for (int it = 0; it < 13; ++it) {  // 2^12 = kJoinLdsRows
          if (len <= 1) break;
          const int half = len >> 1;
          if (soff[lo + half] <= p) lo += half, len -= half;
          else len = half;
        }
        l = l0 + lo, k = p - soff[lo];
      } else {
        int64_t lo = 0, len = rows;
        for (int it = 0; it < 32; ++it) {  // rows < 2^31
          if (len <= 1) break;
          const int64_t half = len >> 1;
          if (gptr<int64_t>(off)[l0 + lo + half] <= o) lo += half, len -= half;
          else len = half;
        }
        l = l0 + lo, k = o - gptr<int64_t>(off)[l];
      }
      const int slot = gptr<int>(pslot)[l];
      int64_t r = -1;
      if (slot >= 0 && slot <= capacity) {  // (always at most capacity: no read past the slot arrays)
        if (brow == nullptr) {
          r = gptr<int>(first)[slot];
        } else {
          const int64_t b = (int64_t)gptr<int>(start)[slot] + k;
          if (b >= 0 && b < nbrow) r = gptr<int>(brow)[b];  // (always, for the counts of these very rows)
        }
      }
      li[o] = l;
      ri[o] = r;
    }
    __syncthreads();  // the next tile rewrites srow and soff
  }
}

void check_side(const KeyCol& a, int blocks) {
  check_key_col(a, blocks, "join");
  if (a.n >= ((int64_t)1 << 31)) throw std::invalid_argument("join: fewer than 2^31 rows per side");
}

void check_join_table(int64_t capacity) {
  check_table(capacity, kJoinMaxCapacity, "join: the table capacity must be a power of two in [2, 2^30]");
}

}  // namespace

// 8 blocks of 4 waves per CU: a probe is a chain of dependent random reads, which only more waves
// in flight hide; the rest of the trips are grid-strided
int join_blocks(int64_t n) { return grid_for(8, (n + kJoinTrip - 1) / kJoinTrip); }

int join_expand_blocks(int64_t total) { return grid_for(8, (total + kJoinTile - 1) / kJoinTile); }

void join_build(const KeyCol& right, unsigned long long* table, int64_t capacity, unsigned* cnt, int* first, int* bslot,
                unsigned long long* state, int blocks, hipStream_t st) {
  check_side(right, blocks);
  check_join_table(capacity);
  if (right.n == 0) return;
  if (table == nullptr || cnt == nullptr || first == nullptr || bslot == nullptr || state == nullptr)
    throw std::invalid_argument("join: null buffer");
  hipLaunchKernelGGL(join_build_kernel, dim3((unsigned)blocks), dim3(kJoinThreads), 0, st, right, table, (u64)(capacity - 1), cnt,
                     first, bslot, state);
  DQ_HIP_CHECK(hipGetLastError());
}

void join_probe(const KeyCol& left, const unsigned long long* table, int64_t capacity, const unsigned* cnt, int mode,
                int* pslot, int* pcnt, uint8_t* matched, uint8_t* mask, int blocks, hipStream_t st) {
  check_side(left, blocks);
  check_join_table(capacity);
  if (mode < JOIN_INNER || mode > JOIN_SEMI) throw std::invalid_argument("join: unknown probe mode");
  if (left.n == 0) return;
  if (table == nullptr || cnt == nullptr) throw std::invalid_argument("join: null buffer");
  if (mode == JOIN_SEMI ? mask == nullptr : (pslot == nullptr || pcnt == nullptr))
    throw std::invalid_argument("join: null buffer");
  if (mode == JOIN_FULL && matched == nullptr) throw std::invalid_argument("join: null buffer");
  hipLaunchKernelGGL(join_probe_kernel, dim3((unsigned)blocks), dim3(kJoinThreads), 0, st, left, table, (u64)(capacity - 1), cnt,
                     mode, pslot, pcnt, matched, mask);
  DQ_HIP_CHECK(hipGetLastError());
}

void join_expand(const int64_t* offsets, int64_t n_left, int64_t total, const int* pslot, const int* start, const int* brow,
                 int64_t nbrow, const int* first, int64_t capacity, int64_t* li, int64_t* ri, int blocks, hipStream_t st) {
  if (n_left < 0 || total < 0 || nbrow < 0) throw std::invalid_argument("join: negative row count");
  if (n_left >= ((int64_t)1 << 31)) throw std::invalid_argument("join: fewer than 2^31 rows per side");
  if (total >= ((int64_t)1 << 31)) throw std::invalid_argument("join: fewer than 2^31 pairs per call");
  if (blocks < 1) throw std::invalid_argument("join: blocks must be >= 1");
  check_join_table(capacity);
  if ((start == nullptr) != (brow == nullptr))
    throw std::invalid_argument("join: the slot starts and the grouped right rows come together or not at all");
  if (total == 0) return;
  if (n_left == 0) throw std::invalid_argument("join: pairs without a left row");
  if (offsets == nullptr || pslot == nullptr || first == nullptr || li == nullptr || ri == nullptr)
    throw std::invalid_argument("join: null buffer");
  hipLaunchKernelGGL(join_expand_kernel, dim3((unsigned)blocks), dim3(kJoinThreads), 0, st, offsets, n_left, total, pslot, start,
                     brow, nbrow, first, capacity, li, ri);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
