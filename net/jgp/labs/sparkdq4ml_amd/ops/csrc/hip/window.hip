// Window functions over the m sorted positions of one window specification.
//
// The sort (sort.hip) leaves a permutation: position i holds row perm[i], partitions are runs of
// positions, and inside a partition the positions follow the order columns.  Every kernel here
// works on positions and reads rows through perm, so the rows outside the selection are never read.
//
//   window_heads    one byte per position: bit 0 first of its partition, bit 1 first of its peer
//                   group (the folded keys of keys.h compared with the position before; two nulls
//                   are equal)
//   window_bounds   forward max-scans of the head positions (part_start, peer_start), backward
//                   min-scans of the end positions (part_end, peer_end), add-scan of the peer heads
//                   (dense)
//   window_prefix   UNSEGMENTED inclusive i64 prefix sums of the value words: ROWS, COUNT, SUM_I
//                   and the four fixed-point limbs of SUM_F (groupby.hip's split, same exponent)
//                   plus the counts of NaN / +inf / -inf.  A limb is a signed 32-bit value and a
//                   call has fewer than 2^31 positions, so no prefix overflows, and the sum over a
//                   frame [lo, hi] is P[hi] - P[lo - 1] word by word: the very words group_agg
//                   accumulates over those rows.
//   window_minmax   segmented inclusive min-scan of (flag, key) pairs, forward or backward,
//                   restarting at the partition heads; max runs on the complemented keys
//   window_finish   per position: the frame [lo, hi] from the bounds, prefix differences or scan
//                   picks, the ranking integers and the lag / lead source rows, scattered to row
//                   perm[i] of an [n, words] table
//
// A scan is reduce-then-scan in three ordinary launches over fixed tiles of kWinTile positions (a
// thread owns kWinRun consecutive ones): tile totals, one block scanning the totals (kWinThreads
// per trip), then the tile scan with its carry-in.  A backward scan counts its positions from the
// end, so it is the same three launches.  No block waits on another, there is no atomic, every
// loop is bounded, and every store is an ordinary vector store.  The scans themselves (the block
// scan of the tile kernels, the row walker over the totals) are scan.h's; the operators Bnd and
// Seg below are the window semantics they run with.
#include "window.h"

#include <stdexcept>

#include "common.h"
#include "keys.h"
#include "scan.h"

namespace dq4ml {
namespace {

constexpr int kWinWaves = kWinThreads / kWave;

// block r: the exclusive scan of row r of a [rows][pitch] array, in place (scan.h's row walker, E
// entries per thread): the step between the tile totals and the tile scan
template <class S, int E>
__global__ __launch_bounds__(kWinThreads) void scan_rows_kernel(typename S::T* a, int64_t pitch, int64_t len) {
  __shared__ typename S::T red[kWinWaves];
  scan_row<S, kWinWaves, E>(a + (int64_t)blockIdx.x * pitch, len, S::id(), red);
}

template <class S, int E>
void launch_scan_rows(typename S::T* a, int64_t rows, int64_t pitch, int64_t len, hipStream_t st) {
  hipLaunchKernelGGL((scan_rows_kernel<S, E>), dim3((unsigned)rows), dim3(kWinThreads), 0, st, a, pitch, len);
}

// forward: (max, max, add) over (partition head position, peer head position, peer head);
// backward: (min, min, -) over (partition end position, peer end position, -)
template <bool BWD>
struct Bnd {
  struct T {
    unsigned a, b, c, pad;
  };
  static __device__ __forceinline__ T id() { return BWD ? T{~0u, ~0u, 0u, 0u} : T{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ T op(T x, T y) {
    if (BWD) return T{x.a < y.a ? x.a : y.a, x.b < y.b ? x.b : y.b, 0u, 0u};
    return T{x.a > y.a ? x.a : y.a, x.b > y.b ? x.b : y.b, x.c + y.c, 0u};
  }
};

// segmented min: a set flag starts a new segment
struct Seg {
  struct T {
    u64 key;
    unsigned flag, pad;
  };
  static __device__ __forceinline__ T id() { return T{~0ull, 0u, 0u}; }
  static __device__ __forceinline__ T op(T x, T y) {
    if (y.flag) return y;
    return T{x.key < y.key ? x.key : y.key, x.flag, 0u};
  }
};

__global__ __launch_bounds__(kWinThreads) void win_heads_kernel(WinKeyArgs a, uint8_t* heads) {
  const int64_t tiles = (a.m + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kWinRun; ++j) {
      const int64_t i = t * kWinTile + j * kWinThreads + threadIdx.x;
      if (i >= a.m) continue;
      unsigned bits = 0;
      if (i == 0) {
        bits = 3;
      } else {
        const int64_t r = gptr<unsigned>(a.perm)[i] & kWinRowMask, p = gptr<unsigned>(a.perm)[i - 1] & kWinRowMask;
        for (int c = 0; c < a.K; ++c) {  // block-uniform
          const bool isf = is_float_dt(a.dt[c]);
          // (a row index past the column never comes out of the sort: it reads as a null)
          bool nr = r >= a.n, np = p >= a.n;
          if (!nr && a.valid[c] != nullptr) nr = gptr<uint8_t>(a.valid[c])[r] == 0;
          if (!np && a.valid[c] != nullptr) np = gptr<uint8_t>(a.valid[c])[p] == 0;
          bool diff = nr != np;
          if (!nr && !np)
            diff = order_key(load_raw(a.col[c], a.dt[c], r), isf, true) != order_key(load_raw(a.col[c], a.dt[c], p), isf, true);
          if (diff) bits |= a.part[c] ? 3u : 2u;
        }
      }
      heads[i] = a.accumulate ? (uint8_t)(heads[i] | bits) : (uint8_t)bits;
    }
  }
}

template <bool BWD, bool SCAN>
__global__ __launch_bounds__(kWinThreads) void win_bounds_kernel(const uint8_t* heads, int64_t m, unsigned* o0, unsigned* o1,
                                                                 unsigned* o2, typename Bnd<BWD>::T* totals) {
  typedef Bnd<BWD> S;
  typedef typename S::T T;
  __shared__ T red[kWinWaves];
  const int64_t tiles = (m + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // block-uniform
    const int64_t q0 = t * kWinTile + (int64_t)threadIdx.x * kWinRun;
    T v[kWinRun];
    T agg = S::id();
#pragma unroll
    for (int k = 0; k < kWinRun; ++k) {
      const int64_t q = q0 + k;
      T x = S::id();
      if (q < m) {
        if (BWD) {
          const int64_t i = m - 1 - q;
          const unsigned h = i + 1 < m ? gptr<uint8_t>(heads)[i + 1] : 3u;  // the position after starts a partition / peer group
          x = T{(h & 1u) ? (unsigned)i : ~0u, (h & 2u) ? (unsigned)i : ~0u, 0u, 0u};
        } else {
          const unsigned h = gptr<uint8_t>(heads)[q];
          x = T{(h & 1u) ? (unsigned)q : 0u, (h & 2u) ? (unsigned)q : 0u, (h >> 1) & 1u, 0u};
        }
      }
      agg = S::op(agg, x);
      v[k] = agg;
    }
    T total;
    const T ex = block_exclusive<S, kWinWaves>(agg, total, red);
    if (!SCAN) {
      if (threadIdx.x == 0) totals[t] = total;
    } else {
      const T carry = S::op(totals[t], ex);
#pragma unroll
      for (int k = 0; k < kWinRun; ++k) {
        const int64_t q = q0 + k;
        if (q < m) {
          const int64_t i = BWD ? m - 1 - q : q;
          const T r = S::op(carry, v[k]);
          o0[i] = r.a;
          o1[i] = r.b;
          if (!BWD) o2[i] = r.c;
        }
      }
    }
  }
}

// word w of a slot for one row (group_agg_kernel's contributions; SUM_F: limbs 0..3, then the
// NaN / +inf / -inf counts)
__device__ __forceinline__ long long word_value(int op, u64 raw, bool isf, int e, int w) {
  if (op == WW_ROWS || op == WW_COUNT) return 1;
  if (op == WW_SUM_I) return (long long)raw;
  const double x = raw_as_f64(raw, isf);
  const u64 b = (u64)__double_as_longlong(x);
  const bool finite = (b & ~kSign) < kInfBits;
  if (w >= 4) {
    if (w == 4) return (b & ~kSign) > kInfBits ? 1 : 0;
    return b == (w == 5 ? kInfBits : (kInfBits | kSign)) ? 1 : 0;
  }
  double tt = finite ? ldexp(x, 32 - e) : 0.0;
  for (int k = 0; k < w; ++k) tt = ldexp(tt - trunc(tt), 32);  // (w < 4)
  return (long long)trunc(tt);
}

template <bool SCAN>
__global__ __launch_bounds__(kWinThreads) void win_prefix_kernel(WinPrefixArgs a, long long* prefix, long long* totals,
                                                                 int64_t tiles) {
  __shared__ long long red[kWinWaves];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // block-uniform
    const int64_t q0 = t * kWinTile + (int64_t)threadIdx.x * kWinRun;
    int64_t rows[kWinRun];
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < kWinRun; ++k) {
      rows[k] = 0;
      if (q0 + k < a.m) {
        rows[k] = gptr<unsigned>(a.perm)[q0 + k] & kWinRowMask;
        if (rows[k] < a.n) live |= 1u << k;  // (always, for a permutation of the column's rows)
      }
    }
    for (int s = 0; s < a.S; ++s) {  // block-uniform
      const int op = a.op[s], dt = a.dt[s], nw = win_word_count(op);
      const bool isf = is_float_dt(dt);
      unsigned ok = live;
      u64 raw[kWinRun];
#pragma unroll
      for (int k = 0; k < kWinRun; ++k) {
        raw[k] = 0;
        if (!((ok >> k) & 1u)) continue;
        if (op != WW_ROWS && a.valid[s] != nullptr && gptr<uint8_t>(a.valid[s])[rows[k]] == 0) ok &= ~(1u << k);
        else if (op >= WW_SUM_I) raw[k] = load_raw(a.col[s], dt, rows[k]);
      }
      for (int w = 0; w < nw; ++w) {  // block-uniform
        long long v[kWinRun];
        long long agg = 0;
#pragma unroll
        for (int k = 0; k < kWinRun; ++k) {
          if ((ok >> k) & 1u) agg += word_value(op, raw[k], isf, a.e[s], w);
          v[k] = agg;
        }
        long long total;
        const long long ex = block_exclusive<AddI64, kWinWaves>(agg, total, red);
        const int64_t W = a.woff[s] + w;
        if (!SCAN) {
          if (threadIdx.x == 0) totals[W * tiles + t] = total;
        } else {
          const long long carry = totals[W * tiles + t] + ex;
#pragma unroll
          for (int k = 0; k < kWinRun; ++k)
            if (q0 + k < a.m) prefix[W * a.m + q0 + k] = carry + v[k];
        }
      }
    }
  }
}

template <bool SCAN>
__global__ __launch_bounds__(kWinThreads) void win_minmax_kernel(const void* col, int dt, const uint8_t* valid,
                                                                 const unsigned* perm, int64_t n, int64_t m,
                                                                 const uint8_t* heads, int is_max, int bwd, u64* out,
                                                                 Seg::T* totals) {
  typedef Seg::T T;
  __shared__ T red[kWinWaves];
  const bool isf = is_float_dt(dt);
  const int64_t tiles = (m + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // block-uniform
    const int64_t q0 = t * kWinTile + (int64_t)threadIdx.x * kWinRun;
    T v[kWinRun];
    T agg = Seg::id();
#pragma unroll
    for (int k = 0; k < kWinRun; ++k) {
      const int64_t q = q0 + k;
      T x = Seg::id();
      if (q < m) {
        const int64_t i = bwd ? m - 1 - q : q;
        // the scan restarts where its partition starts: at a head, or (backward) before one
        const unsigned flag = bwd ? (i + 1 < m ? gptr<uint8_t>(heads)[i + 1] & 1u : 1u) : gptr<uint8_t>(heads)[i] & 1u;
        const int64_t r = gptr<unsigned>(perm)[i] & kWinRowMask;
        u64 key = ~0ull;  // a null row contributes the identity
        if (r < n && (valid == nullptr || gptr<uint8_t>(valid)[r] != 0)) {
          key = order_key(load_raw(col, dt, r), isf, false);
          if (is_max) key = ~key;
        }
        x = T{key, flag, 0u};
      }
      agg = Seg::op(agg, x);
      v[k] = agg;
    }
    T total;
    const T ex = block_exclusive<Seg, kWinWaves>(agg, total, red);
    if (!SCAN) {
      if (threadIdx.x == 0) totals[t] = total;
    } else {
      const T carry = Seg::op(totals[t], ex);
#pragma unroll
      for (int k = 0; k < kWinRun; ++k) {
        const int64_t q = q0 + k;
        if (q < m) {
          const u64 key = Seg::op(carry, v[k]).key;
          out[bwd ? m - 1 - q : q] = is_max ? ~key : key;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kWinThreads) void win_finish_kernel(WinFinishArgs a, long long* out) {
  const int64_t tiles = (a.m + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll 2
    for (int j = 0; j < kWinRun; ++j) {
      const int64_t i = t * kWinTile + j * kWinThreads + threadIdx.x;
      if (i >= a.m) continue;
      const int64_t row = gptr<unsigned>(a.perm)[i] & kWinRowMask;
      if (row >= a.n) continue;  // (never, for a permutation of the table's rows: no store past the table)
      const int64_t ps = gptr<unsigned>(a.b.part_start)[i], pe = gptr<unsigned>(a.b.part_end)[i];
      const int64_t qs = gptr<unsigned>(a.b.peer_start)[i], qe = gptr<unsigned>(a.b.peer_end)[i];
      if (ps > i || pe < i || pe >= a.m) continue;  // (never, for the bounds of window_bounds: no read past the positions)
      int64_t lo, hi;
      if (a.is_range) {
        lo = a.lo_unbounded ? ps : qs;
        hi = a.hi_unbounded ? pe : qe;
      } else {
        lo = a.lo_unbounded ? ps : (i + a.lo_off > ps ? i + a.lo_off : ps);
        hi = a.hi_unbounded ? pe : (i + a.hi_off < pe ? i + a.hi_off : pe);
      }
      // inside [0, m) whenever the frame is not empty; an empty frame reads nothing
      const bool some = lo <= hi && lo >= 0 && hi < a.m;
      long long* o = out + row * a.words;
      for (int w = 0; w < a.words; ++w) {  // block-uniform
        long long v = 0;
        switch (a.kind[w]) {  // block-uniform
          case WO_DIFF:
            if (some) v = gptr<long long>(a.src[w])[hi] - (lo > 0 ? gptr<long long>(a.src[w])[lo - 1] : 0ll);
            break;
          case WO_PICK_HI:
            if (some) v = gptr<long long>(a.src[w])[hi];
            break;
          case WO_PICK_LO:
            if (some) v = gptr<long long>(a.src[w])[lo];
            break;
          case WO_ROW_NUMBER: v = i - ps + 1; break;
          case WO_RANK: v = qs - ps + 1; break;
          case WO_DENSE_RANK: v = (long long)gptr<unsigned>(a.b.dense)[i] - (long long)gptr<unsigned>(a.b.dense)[ps] + 1; break;
          case WO_PART_SIZE: v = pe - ps + 1; break;
          case WO_PEER_END: v = qe - ps + 1; break;
          default: {  // WO_SHIFT
            const int64_t p = i + a.arg[w];
            v = p >= ps && p <= pe ? (long long)(gptr<unsigned>(a.perm)[p] & kWinRowMask) : -1ll;
            break;
          }
        }
        o[w] = v;
      }
    }
  }
}

void check_positions(int64_t n, int64_t m, int blocks) {
  if (n < 0 || m < 0) throw std::invalid_argument("window: negative row count");
  if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31)) throw std::invalid_argument("window: fewer than 2^31 rows per call");
  if (m > n) throw std::invalid_argument("window: more positions than rows");
  if (blocks < 1) throw std::invalid_argument("window: blocks must be >= 1");
}

}  // namespace

// the scans hold a tile's run in registers and 64 bytes of LDS: 8 blocks of 4 waves per CU
int window_blocks(int64_t m) { return grid_for(8, win_tiles(m)); }

void window_heads(const WinKeyArgs& a, uint8_t* heads, int blocks, hipStream_t st) {
  check_positions(a.n, a.m, blocks);
  if (a.K < 0 || a.K > kWinMaxKeys)
    throw std::invalid_argument("window_heads: at most " + std::to_string(kWinMaxKeys) + " key columns per launch");
  for (int c = 0; c < a.K; ++c) {
    if (!is_key_dt(a.dt[c])) throw std::invalid_argument("window_heads: keys must be f64, f32, i32, i64 or u8");
    if (a.col[c] == nullptr && a.m > 0) throw std::invalid_argument("window_heads: null column");
  }
  if (a.m == 0) return;
  if (a.perm == nullptr || heads == nullptr) throw std::invalid_argument("window_heads: null buffer");
  hipLaunchKernelGGL(win_heads_kernel, dim3((unsigned)blocks), dim3(kWinThreads), 0, st, a, heads);
  DQ_HIP_CHECK(hipGetLastError());
}

void window_bounds(const uint8_t* heads, int64_t m, unsigned* part_start, unsigned* peer_start, unsigned* part_end,
                   unsigned* peer_end, unsigned* dense, void* totals, int blocks, hipStream_t st) {
  check_positions(m, m, blocks);
  if (m == 0) return;
  if (heads == nullptr || part_start == nullptr || peer_start == nullptr || part_end == nullptr || peer_end == nullptr ||
      dense == nullptr || totals == nullptr)
    throw std::invalid_argument("window_bounds: null buffer");
  if ((reinterpret_cast<uintptr_t>(totals) & 15) != 0) throw std::invalid_argument("window_bounds: totals must be 16-byte aligned");
  const int64_t tiles = win_tiles(m);
  const dim3 grid((unsigned)blocks), block(kWinThreads);
  Bnd<false>::T* tf = reinterpret_cast<Bnd<false>::T*>(totals);
  Bnd<true>::T* tb = reinterpret_cast<Bnd<true>::T*>(totals) + tiles;
  hipLaunchKernelGGL((win_bounds_kernel<false, false>), grid, block, 0, st, heads, m, part_start, peer_start, dense, tf);
  launch_scan_rows<Bnd<false>, 1>(tf, 1, tiles, tiles, st);
  hipLaunchKernelGGL((win_bounds_kernel<false, true>), grid, block, 0, st, heads, m, part_start, peer_start, dense, tf);
  hipLaunchKernelGGL((win_bounds_kernel<true, false>), grid, block, 0, st, heads, m, part_end, peer_end, dense, tb);
  launch_scan_rows<Bnd<true>, 1>(tb, 1, tiles, tiles, st);
  hipLaunchKernelGGL((win_bounds_kernel<true, true>), grid, block, 0, st, heads, m, part_end, peer_end, dense, tb);
  DQ_HIP_CHECK(hipGetLastError());
}

void window_prefix(const WinPrefixArgs& a, long long* prefix, long long* totals, int blocks, hipStream_t st) {
  check_positions(a.n, a.m, blocks);
  if (a.S < 1 || a.S > kWinMaxWords) throw std::invalid_argument("window_prefix: between 1 and 8 slots per pass");
  int words = 0;
  for (int s = 0; s < a.S; ++s) {
    const int op = a.op[s];
    if (op < WW_ROWS || op > WW_SUM_F) throw std::invalid_argument("window_prefix: unknown word kind");
    if (a.woff[s] != words) throw std::invalid_argument("window_prefix: slot words must be packed in slot order");
    words += win_word_count(op);
    if (op >= WW_SUM_I) {
      if (!is_key_dt(a.dt[s])) throw std::invalid_argument("window_prefix: columns must be f64, f32, i32, i64 or u8");
      if (a.col[s] == nullptr && a.m > 0) throw std::invalid_argument("window_prefix: null column");
      if (op == WW_SUM_I && (a.dt[s] == DT_F64 || a.dt[s] == DT_F32))
        throw std::invalid_argument("window_prefix: SUM_I of a float column");
    }
  }
  if (words != a.words || words > kWinMaxWords)
    throw std::invalid_argument("window_prefix: at most " + std::to_string(kWinMaxWords) + " words per pass, matching the slots");
  if (a.m == 0) return;
  if (a.perm == nullptr || prefix == nullptr || totals == nullptr) throw std::invalid_argument("window_prefix: null buffer");
  const int64_t tiles = win_tiles(a.m);
  const dim3 grid((unsigned)blocks), block(kWinThreads);
  hipLaunchKernelGGL(win_prefix_kernel<false>, grid, block, 0, st, a, prefix, totals, tiles);
  launch_scan_rows<AddI64, 1>(totals, words, tiles, tiles, st);
  hipLaunchKernelGGL(win_prefix_kernel<true>, grid, block, 0, st, a, prefix, totals, tiles);
  DQ_HIP_CHECK(hipGetLastError());
}

void window_minmax(const void* col, int dt, const uint8_t* valid, const unsigned* perm, int64_t n, int64_t m,
                   const uint8_t* heads, bool is_max, bool backward, unsigned long long* out, void* totals, int blocks,
                   hipStream_t st) {
  check_positions(n, m, blocks);
  if (!is_key_dt(dt)) throw std::invalid_argument("window_minmax: columns must be f64, f32, i32, i64 or u8");
  if (m == 0) return;
  if (col == nullptr || perm == nullptr || heads == nullptr || out == nullptr || totals == nullptr)
    throw std::invalid_argument("window_minmax: null buffer");
  if ((reinterpret_cast<uintptr_t>(totals) & 15) != 0) throw std::invalid_argument("window_minmax: totals must be 16-byte aligned");
  const int64_t tiles = win_tiles(m);
  const dim3 grid((unsigned)blocks), block(kWinThreads);
  Seg::T* tt = reinterpret_cast<Seg::T*>(totals);
  const int mx = is_max ? 1 : 0, bw = backward ? 1 : 0;
  hipLaunchKernelGGL(win_minmax_kernel<false>, grid, block, 0, st, col, dt, valid, perm, n, m, heads, mx, bw, out, tt);
  launch_scan_rows<Seg, 1>(tt, 1, tiles, tiles, st);
  hipLaunchKernelGGL(win_minmax_kernel<true>, grid, block, 0, st, col, dt, valid, perm, n, m, heads, mx, bw, out, tt);
  DQ_HIP_CHECK(hipGetLastError());
}

void scan_rows(int kind, void* a, int64_t rows, int64_t len, hipStream_t st) {
  if (rows < 0 || len < 0) throw std::invalid_argument("scan_rows: negative shape");
  if (rows == 0 || len == 0) return;
  if (a == nullptr || (reinterpret_cast<uintptr_t>(a) & 15) != 0) throw std::invalid_argument("scan_rows: a 16-byte aligned buffer");
  switch (kind) {
    case 0: launch_scan_rows<AddI64, 1>(static_cast<long long*>(a), rows, len, len, st); break;
    case 1: launch_scan_rows<AddU32, 4>(static_cast<unsigned*>(a), rows, (len + 3) & ~(int64_t)3, len, st); break;
    case 2: launch_scan_rows<Bnd<false>, 1>(static_cast<Bnd<false>::T*>(a), rows, len, len, st); break;
    case 3: launch_scan_rows<Bnd<true>, 1>(static_cast<Bnd<true>::T*>(a), rows, len, len, st); break;
    case 4: launch_scan_rows<Seg, 1>(static_cast<Seg::T*>(a), rows, len, len, st); break;
    default: throw std::invalid_argument("scan_rows: unknown kind");
  }
  DQ_HIP_CHECK(hipGetLastError());
}

void window_finish(const WinFinishArgs& a, long long* out, int blocks, hipStream_t st) {
  check_positions(a.n, a.m, blocks);
  if (a.words < 1 || a.words > kWinMaxWords)
    throw std::invalid_argument("window_finish: between 1 and " + std::to_string(kWinMaxWords) + " words per launch");
  for (int w = 0; w < a.words; ++w) {
    if (a.kind[w] < WO_DIFF || a.kind[w] > WO_SHIFT) throw std::invalid_argument("window_finish: unknown output kind");
    if (a.kind[w] <= WO_PICK_LO && a.src[w] == nullptr && a.m > 0) throw std::invalid_argument("window_finish: null source");
    if (a.arg[w] <= -((long long)1 << 32) || a.arg[w] >= ((long long)1 << 32))
      throw std::invalid_argument("window_finish: shift distance out of range");
  }
  if (a.lo_off <= -((long long)1 << 32) || a.lo_off >= ((long long)1 << 32) || a.hi_off <= -((long long)1 << 32) ||
      a.hi_off >= ((long long)1 << 32))
    throw std::invalid_argument("window_finish: frame offset out of range");
  if (a.m == 0) return;
  if (a.perm == nullptr || out == nullptr || a.b.part_start == nullptr || a.b.peer_start == nullptr || a.b.part_end == nullptr ||
      a.b.peer_end == nullptr || a.b.dense == nullptr)
    throw std::invalid_argument("window_finish: null buffer");
  hipLaunchKernelGGL(win_finish_kernel, dim3((unsigned)blocks), dim3(kWinThreads), 0, st, a, out);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
