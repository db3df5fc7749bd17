// Open-addressing table of u64 order keys in HBM: the one home of the probe for the grouping
// kernels (groupby.hip) and the join kernels (join.hip).  Power-of-two capacity, multiplicative
// hash, linear probing, 64-bit atomicCAS; one probe loop for writers (table_acquire) and one
// for readers (table_slot).  The empty slot is all ones, which is the order key of INT64_MAX: that
// one key never enters the table (the callers keep it out of band).  Every probe sequence is
// bounded by the capacity.  ops.keys.hash_home is the Python statement of the hash.  Device code
// only.
#pragma once
#include "common.h"
#include "keys.h"

namespace dq4ml {

constexpr u64 kEmpty = ~0ull;

__device__ __forceinline__ u64 home_slot(u64 key, u64 mask) { return ((key * 0x9E3779B97F4A7C15ull) >> 20) & mask; }

__device__ __forceinline__ u64 load_slot(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The slot of `key`, claimed when the key is new (`fresh` then says so); -1 when the probe met
// neither the key nor a free slot in mask + 1 steps (the table is full).
__device__ __forceinline__ int64_t table_acquire(u64* table, u64 mask, u64 key, bool& fresh) {
  fresh = false;
  u64 slot = home_slot(key, mask);
  // a slot only ever changes from empty to a key, so a stale read costs one failed CAS at most;
  // the bound ends the probe of a table that other waves filled after the overflow check
  for (u64 i = 0; i <= mask; ++i) {
    const u64 cur = load_slot(table + slot);
    if (cur == key) return (int64_t)slot;
    if (cur == kEmpty) {
      const u64 old = atomicCAS(table + slot, kEmpty, key);
      if (old == key) return (int64_t)slot;
      if (old == kEmpty) {
        fresh = true;
        return (int64_t)slot;
      }
    }
    slot = (slot + 1) & mask;
  }
  return -1;
}

// state: [0] occupied slots, [1] overflow (past half full, or no free slot), [2] a null key was
// seen, [3] the all-ones key was seen
__device__ __forceinline__ void table_insert(u64* table, u64 mask, u64* state, u64 key) {
  bool fresh;
  if (table_acquire(table, mask, key, fresh) < 0) {
    atomicOr(state + 1, 1ull);
  } else if (fresh) {
    const u64 c = atomicAdd(state, 1ull) + 1;
    if (c > (mask + 1) / 2) atomicOr(state + 1, 1ull);
  }
}

// The slot of `key`, claimed when the key is new (`occupied` then counts it), -1 when the table is
// full (the caller flags it).  For callers that need the slot itself and size the table beforehand
// (no half-full rule).
__device__ __forceinline__ int64_t table_claim(u64* table, u64 mask, u64* occupied, u64 key) {
  bool fresh;
  const int64_t slot = table_acquire(table, mask, key, fresh);
  if (fresh) atomicAdd(occupied, 1ull);
  return slot;
}

// the slot of `key` in a finished table, -1 when it is absent (no insert)
__device__ __forceinline__ int64_t table_slot(const u64* table, u64 mask, u64 key) {
  u64 slot = home_slot(key, mask);
  for (u64 i = 0; i <= mask; ++i) {
    const u64 cur = gptr<u64>(table)[slot];
    if (cur == key) return (int64_t)slot;
    if (cur == kEmpty) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

}  // namespace dq4ml
