// Grouped aggregation on integer words.
//
// group_encode turns one key column into group ids.  A key value becomes an order-preserving u64
// (floats: IEEE bits of the value as a double, -0.0 folded into +0.0, every NaN one canonical NaN
// above +inf; integers and booleans: biased by the sign bit).  Integer keys of a small live range
// index a slot directly (gid = key - base + 1, null = 0); everything else goes through an
// open-addressing table of u64 slots in HBM (linear probing, 64-bit atomicCAS, power-of-two
// capacity).  The empty slot is all ones, which is the key of INT64_MAX: that one key never enters
// the table, a flag records that it was seen and the launcher gives it the last group id.
//
// group_agg makes one pass over the rows for up to kGroupMaxSlots aggregate slots.  Every
// accumulator word is a u64 updated by an integer atomic (add / or / max / min), so any order of
// the updates gives the same bits.  Doubles are summed in fixed point: with e the frexp exponent
// of the largest finite |x| of the column, x is split into four signed 32-bit limbs of
// x * 2^(128 - e) (each step exact in f64) and limb k is an i64 add.
//
// Contention: before any atomic the lanes of a wave that share the first live lane's group reduce
// their contributions in the wave and the leader issues one atomic, twice in a row; whatever is
// left takes per-lane atomics.  When G * words fits kGroupLdsWords a block accumulates in LDS and
// flushes its non-identity words once.
#include "groupby.h"

#include <stdexcept>

#include "common.h"
#include "hashtable.h"
#include "keys.h"

namespace dq4ml {
namespace {

static_assert(kGroupRun == kRawRun, "the run loaders of keys.h read kGroupRun rows");

__device__ __forceinline__ int word_kind(int op, int w) {
  switch (op) {
    case GOP_SUM_F: return w == kGroupSumWords - 1 ? GK_OR : GK_ADD;
    case GOP_MIN:
    case GOP_FIRST: return GK_MIN;
    case GOP_MAX:
    case GOP_ABSMAX: return GK_MAX;
    default: return GK_ADD;
  }
}

__device__ __forceinline__ u64 kind_identity(int kind) { return kind == GK_MIN ? ~0ull : 0ull; }

__device__ __forceinline__ void word_update(u64* p, int kind, u64 v) {
  switch (kind) {
    case GK_ADD: atomicAdd(p, v); break;
    case GK_OR: atomicOr(p, v); break;
    case GK_MAX: atomicMax(p, v); break;
    default: atomicMin(p, v); break;
  }
}

__device__ __forceinline__ u64 wave_reduce(int kind, u64 v) {
  switch (kind) {  // wave-uniform
    case GK_ADD:
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
      break;
    case GK_OR:
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, kWave);
      break;
    case GK_MAX:
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 u = __shfl_xor(v, o, kWave);
        v = u > v ? u : v;
      }
      break;
    default:
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 u = __shfl_xor(v, o, kWave);
        v = u < v ? u : v;
      }
      break;
  }
  return v;
}

// Word w of group g takes v from every lane with `on` set.  Two rounds of "the lanes that share
// the first live lane's group reduce in the wave, the leader issues one atomic", then per-lane
// atomics.  Identity contributions are dropped.  Every lane of the wave calls this.
__device__ __forceinline__ void emit(u64* acc, int words, bool on, int g, int w, int kind, u64 v, int lane) {
  const u64 ident = kind_identity(kind);
  on = on && v != ident;
  uint64_t rem = __ballot(on);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (rem == 0) return;  // wave-uniform
    const int leader = __ffsll((long long)rem) - 1;
    const int g0 = __builtin_amdgcn_readlane(g, leader);
    const bool same = on && g == g0;
    const uint64_t grp = __ballot(same);
    u64 red = v;  // (a group of one lane: the leader's own value)
    if (__popcll(grp) > 1) red = wave_reduce(kind, same ? v : ident);
    if (lane == leader && red != ident) word_update(acc + (int64_t)g0 * words + w, kind, red);
    on = on && !same;
    rem &= ~grp;
  }
  if (on) word_update(acc + (int64_t)g * words + w, kind, v);
}

template <bool LDS>
__global__ __launch_bounds__(kGroupThreads) void group_agg_kernel(GroupAggArgs a, u64* out) {
  __shared__ u64 lds[LDS ? kGroupLdsWords : 1];
  __shared__ int wkind[kGroupMaxWords];
  const int lane = threadIdx.x & (kWave - 1);
  const int total = LDS ? a.G * a.words : 0;  // at most kGroupLdsWords (the launcher picks the kernel)
  if constexpr (LDS) {
    if ((int)threadIdx.x < a.words) {
      int kind = GK_ADD;
      for (int s = 0; s < a.S; ++s) {
        const int w = (int)threadIdx.x - a.woff[s];
        if (w >= 0 && w < group_op_words(a.op[s])) kind = word_kind(a.op[s], w);
      }
      wkind[threadIdx.x] = kind;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += kGroupThreads) lds[i] = kind_identity(wkind[i % a.words]);
    __syncthreads();
  }
  u64* acc = LDS ? lds : out;
  const bool galigned = (reinterpret_cast<uintptr_t>(a.gid) & 15) == 0;
  const int64_t trips = (a.n + kGroupTrip - 1) / kGroupTrip;
  // the trip loop is block-uniform: rows past n are dead lanes, never absent ones
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    const int64_t r0 = t * kGroupTrip + (int64_t)threadIdx.x * kGroupRun;
    unsigned live = mask_run(a.sel, r0, a.n);
    int g[kGroupRun] = {0, 0, 0, 0};
    if (a.gid != nullptr) {
      if (galigned && r0 + kGroupRun <= a.n) {
        const i32x4 v = *gptr<i32x4>(a.gid + r0);
#pragma unroll
        for (int j = 0; j < kGroupRun; ++j) g[j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < kGroupRun; ++j) g[j] = r0 + j < a.n ? gptr<int>(a.gid)[r0 + j] : -1;
      }
#pragma unroll
      for (int j = 0; j < kGroupRun; ++j)
        if (g[j] < 0 || g[j] >= a.G) live &= ~(1u << j), g[j] = 0;  // -1: dead row; never index past G
    }
    for (int s = 0; s < a.S; ++s) {  // block-uniform
      const int op = a.op[s], w0 = a.woff[s], dt = a.dt[s];
      const bool isf = is_float_dt(dt);
      const bool reads = op != GOP_ROWS && op != GOP_FIRST && op != GOP_COUNT;
      u64 raw[kGroupRun] = {0, 0, 0, 0};
      if (reads) load_run(a.col[s], dt, r0, a.n, raw);
      unsigned ok = live;
      if (op != GOP_ROWS && op != GOP_FIRST && a.valid[s] != nullptr) ok &= mask_run(a.valid[s], r0, a.n);
#pragma unroll
      for (int j = 0; j < kGroupRun; ++j) {
        const bool on = (ok >> j) & 1u;
        switch (op) {  // block-uniform
          case GOP_ROWS:
          case GOP_COUNT: emit(acc, a.words, on, g[j], w0, GK_ADD, 1ull, lane); break;
          case GOP_SUM_I: emit(acc, a.words, on, g[j], w0, GK_ADD, raw[j], lane); break;
          case GOP_MIN: emit(acc, a.words, on, g[j], w0, GK_MIN, order_key(raw[j], isf, false), lane); break;
          case GOP_MAX: emit(acc, a.words, on, g[j], w0, GK_MAX, order_key(raw[j], isf, false), lane); break;
          case GOP_FIRST: emit(acc, a.words, on, g[j], w0, GK_MIN, (u64)(a.row_offset + r0 + j), lane); break;
          case GOP_ABSMAX: {
            const u64 b = (u64)__double_as_longlong(raw_as_f64(raw[j], isf)) & ~kSign;
            emit(acc, a.words, on && b < kInfBits, g[j], w0, GK_MAX, b, lane);
            break;
          }
          default: {  // GOP_SUM_F
            const double x = raw_as_f64(raw[j], isf);
            const u64 b = (u64)__double_as_longlong(x);
            const bool finite = (b & ~kSign) < kInfBits;
            const u64 flag = finite ? 0ull : ((b & ~kSign) > kInfBits ? 1ull : ((b & kSign) ? 4ull : 2ull));
            double tt = finite ? ldexp(x, 32 - a.e[s]) : 0.0;
#pragma unroll
            for (int k = 0; k < kGroupSumWords - 1; ++k) {
              const double c = trunc(tt);
              emit(acc, a.words, on, g[j], w0 + k, GK_ADD, (u64)(long long)c, lane);
              tt = ldexp(tt - c, 32);
            }
            emit(acc, a.words, on, g[j], w0 + kGroupSumWords - 1, GK_OR, flag, lane);
            break;
          }
        }
      }
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += kGroupThreads) {
      const int kind = wkind[i % a.words];
      const u64 v = lds[i];
      if (v != kind_identity(kind)) word_update(out + i, kind, v);
    }
  }
}

__global__ __launch_bounds__(kGroupThreads) void group_direct_kernel(KeyCol a, int64_t base, int64_t span, int* gid) {
  const int64_t trips = (a.n + kGroupTrip - 1) / kGroupTrip;
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    const int64_t r0 = t * kGroupTrip + (int64_t)threadIdx.x * kGroupRun;
    u64 raw[kGroupRun];
    load_run(a.col, a.dt, r0, a.n, raw);
    const unsigned live = mask_run(a.sel, r0, a.n);
    unsigned valid = live;
    if (a.valid != nullptr) valid &= mask_run(a.valid, r0, a.n);
    int g[kGroupRun];
#pragma unroll
    for (int j = 0; j < kGroupRun; ++j) {
      const u64 off = raw[j] - (u64)base;  // (unsigned: a value below base wraps far past span)
      g[j] = !((live >> j) & 1u) ? -1 : (!((valid >> j) & 1u) ? 0 : (off < (u64)span ? (int)off + 1 : -1));
    }
    store_run(gid, r0, a.n, g);
  }
}

__global__ __launch_bounds__(kGroupThreads) void group_hash_insert_kernel(KeyCol a, u64* table, u64 mask, u64* state) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t trips = (a.n + kGroupTrip - 1) / kGroupTrip;
  bool saw_null = false, saw_top = false;
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    // past half full: stop inserting, the launcher retries with a larger table (wave-uniform read)
    if (__builtin_amdgcn_readfirstlane((int)load_slot(state + 1)) != 0) break;
    const int64_t r0 = t * kGroupTrip + (int64_t)threadIdx.x * kGroupRun;
    const KeyRun k = load_keys(a, r0);
#pragma unroll
    for (int j = 0; j < kGroupRun; ++j) {
      const bool live = (k.live >> j) & 1u, valid = (k.valid >> j) & 1u;
      saw_null = saw_null || (live && !valid);
      saw_top = saw_top || (valid && k.key[j] == kEmpty);
      bool ins = valid && k.key[j] != kEmpty;
      // the lanes that hold the first live lane's key insert once
      const uint64_t rem = __ballot(ins);
      if (rem != 0) {
        const int leader = __ffsll((long long)rem) - 1;
        const u64 k0 = __shfl(k.key[j], leader, kWave);
        if (ins && k.key[j] == k0 && lane != leader) ins = false;
      }
      if (ins) table_insert(table, mask, state, k.key[j]);
    }
  }
  if (saw_null) atomicOr(state + 2, 1ull);
  if (saw_top) atomicOr(state + 3, 1ull);
}

// the group id of a key of a finished table, -1 when the key is absent
__device__ __forceinline__ int gid_of(const u64* table, u64 mask, const int* slot_gid, u64 key) {
  const int64_t slot = table_slot(table, mask, key);
  return slot < 0 ? -1 : gptr<int>(slot_gid)[slot];
}

__global__ __launch_bounds__(kGroupThreads) void group_hash_lookup_kernel(KeyCol a, const u64* table, u64 mask,
                                                                         const int* slot_gid, int top_gid, int* gid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t trips = (a.n + kGroupTrip - 1) / kGroupTrip;
  for (int64_t t = blockIdx.x; t < trips; t += gridDim.x) {
    const int64_t r0 = t * kGroupTrip + (int64_t)threadIdx.x * kGroupRun;
    const KeyRun k = load_keys(a, r0);
    int g[kGroupRun];
#pragma unroll
    for (int j = 0; j < kGroupRun; ++j) {
      const bool live = (k.live >> j) & 1u, valid = (k.valid >> j) & 1u;
      int res = !live ? -1 : (!valid ? 0 : top_gid);
      bool need = valid && k.key[j] != kEmpty;
      // the lanes that hold the first live lane's key look it up once
      const uint64_t rem = __ballot(need);
      if (rem != 0) {
        const int leader = __ffsll((long long)rem) - 1;
        const u64 k0 = __shfl(k.key[j], leader, kWave);
        int g0 = -1;
        if (lane == leader) g0 = gid_of(table, mask, slot_gid, k0);
        g0 = __builtin_amdgcn_readlane(g0, leader);
        if (need && k.key[j] == k0) res = g0, need = false;
      }
      if (need) res = gid_of(table, mask, slot_gid, k.key[j]);
      g[j] = res;
    }
    store_run(gid, r0, a.n, g);
  }
}

void check_group_table(int64_t capacity) {
  check_table(capacity, (int64_t)1 << 40, "group_encode: the table capacity must be a power of two >= 2");
}

}  // namespace

// 4 blocks of 4 waves per CU: the 32 KiB of LDS accumulators allow that many, and 16 to 48 bytes
// in flight per thread and slot cover the HBM latency
int group_blocks(int64_t n) { return grid_for(4, (n + kGroupTrip - 1) / kGroupTrip); }

void group_agg(const GroupAggArgs& a, unsigned long long* acc, int blocks, hipStream_t st) {
  if (a.n < 0) throw std::invalid_argument("group_agg: negative row count");
  if (blocks < 1) throw std::invalid_argument("group_agg: blocks must be >= 1");
  if (a.G < 1) throw std::invalid_argument("group_agg: at least one group");
  if (a.S < 1 || a.S > kGroupMaxSlots)
    throw std::invalid_argument("group_agg: between 1 and " + std::to_string(kGroupMaxSlots) + " slots per call");
  if (acc == nullptr) throw std::invalid_argument("group_agg: null accumulator");
  int words = 0;
  for (int s = 0; s < a.S; ++s) {
    const int op = a.op[s];
    if (op < GOP_ROWS || op > GOP_ABSMAX) throw std::invalid_argument("group_agg: unknown op");
    if (a.woff[s] != words) throw std::invalid_argument("group_agg: slot words must be packed in slot order");
    words += group_op_words(op);
    const bool reads = op != GOP_ROWS && op != GOP_FIRST && op != GOP_COUNT;
    if (reads) {
      const int dt = a.dt[s];
      if (!is_key_dt(dt)) throw std::invalid_argument("group_agg: columns must be f64, f32, i32, i64 or u8");
      if (a.col[s] == nullptr && a.n > 0) throw std::invalid_argument("group_agg: null column");
      if (op == GOP_SUM_I && (dt == DT_F64 || dt == DT_F32)) throw std::invalid_argument("group_agg: SUM_I of a float column");
    }
    if (op == GOP_SUM_F && a.n >= ((int64_t)1 << 31))
      throw std::invalid_argument("group_agg: a fixed-point sum takes fewer than 2^31 rows per call");
  }
  if (words != a.words) throw std::invalid_argument("group_agg: words does not match the slots");
  if (a.n == 0) return;  // the accumulators keep their identities
  const bool lds = (int64_t)a.G * a.words <= kGroupLdsWords;
  if (lds)
    hipLaunchKernelGGL(group_agg_kernel<true>, dim3((unsigned)blocks), dim3(kGroupThreads), 0, st, a, acc);
  else
    hipLaunchKernelGGL(group_agg_kernel<false>, dim3((unsigned)blocks), dim3(kGroupThreads), 0, st, a, acc);
  DQ_HIP_CHECK(hipGetLastError());
}

void group_encode_direct(const KeyCol& a, int64_t base, int64_t span, int* gid, int blocks, hipStream_t st) {
  check_key_col(a, blocks, "group_encode");
  if (a.dt == DT_F64 || a.dt == DT_F32) throw std::invalid_argument("group_encode: direct mode takes integer keys");
  if (span < 0 || span > kGroupDirectCap) throw std::invalid_argument("group_encode: direct range above the cap");
  if (a.n == 0) return;
  hipLaunchKernelGGL(group_direct_kernel, dim3((unsigned)blocks), dim3(kGroupThreads), 0, st, a, base, span, gid);
  DQ_HIP_CHECK(hipGetLastError());
}

void group_hash_insert(const KeyCol& a, unsigned long long* table, int64_t capacity, unsigned long long* state,
                       int blocks, hipStream_t st) {
  check_key_col(a, blocks, "group_encode");
  check_group_table(capacity);
  if (a.n == 0) return;
  hipLaunchKernelGGL(group_hash_insert_kernel, dim3((unsigned)blocks), dim3(kGroupThreads), 0, st, a, table,
                     (u64)(capacity - 1), state);
  DQ_HIP_CHECK(hipGetLastError());
}

void group_hash_lookup(const KeyCol& a, const unsigned long long* table, int64_t capacity, const int* slot_gid,
                       int top_gid, int* gid, int blocks, hipStream_t st) {
  check_key_col(a, blocks, "group_encode");
  check_group_table(capacity);
  if (a.n == 0) return;
  hipLaunchKernelGGL(group_hash_lookup_kernel, dim3((unsigned)blocks), dim3(kGroupThreads), 0, st, a, table,
                     (u64)(capacity - 1), slot_gid, top_gid, gid);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
