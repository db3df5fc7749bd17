// K5a: one ALS half-step -- gather the factor rows a destination rated, form its normal equations,
// solve them -- as ONE kernel over a segment table, plus a small second one for long segments.
//
// Work split.  Segment lengths follow a power law, so the unit of work is a chunk: at most
// `chunk` ratings of one destination, owned by one wave (four independent waves per block, a
// grid-stride loop over the chunk table).  A destination of one chunk -- the common case -- is
// accumulated, solved and stored by its wave with no global intermediate.  A destination of
// several chunks has each wave write its partial system to a slab row; als_long_kernel sums the
// rows in chunk order and solves.  What a wave computes for a chunk does not depend on the grid and
// there are no floating-point atomics, so two runs are bit-identical.
//
// Accumulate.  One v_mfma_f64_16x16x4f64 step contracts 4 ratings.  In its fragment layout
// (tile_layout.h: f = f64_col(lane), q = f64_k(lane)) lane (f, q) holds element 16 t + f of rating
// q's row for every 16-wide tile t of the band, so 16 adjacent lanes read 16 adjacent elements of
// one gathered factor row straight from global memory -- no trip through LDS -- and the register
// is the A operand of tile row t and the B operand of tile column t of Y^T Y.  The band is the
// factor row, then the rating, then a 1: [y (rank) | r | 1], NT = ceil((rank + 2) / 16) tiles.  The
// upper tiles of the product then hold the matrix, the right-hand side (column rank) and the rating
// count m (entry (rank + 1, rank + 1)) together; only tiles I <= J are computed.
//
// Loads in flight.  The pass is latency bound on dependent loads (index, then row).  A wave reads
// the indices and ratings of 64 ratings with one coalesced load each and hands them to the lanes
// by shuffles; the next 64 are requested before the current 64 are used.  Rows are gathered in
// groups of 4 steps (16 ratings) into one of two register buffers: the gathers of group g + 1
// (across the 64-rating boundary too) are issued before the MFMAs of group g.
//
// Solve.  The owning wave writes the accumulators to its LDS area as one packed system
// (als_system_size: upper triangle column-major, right-hand side, m), adds reg m to the diagonal
// and factors A = U^T U in place, right-looking, lane j owning column j; the forward substitution
// rides in the same loop (the right-hand side stays in registers, lane j holding component j), the
// backward substitution follows, and lane j stores component j, rounded once.  m = 0 stores zeros.
// A non-positive pivot (possible only with reg = 0) adds one to status[0] and stores NaN.
#include "als.h"

#include <cmath>
#include <stdexcept>

#include "common.h"
#include "tile_layout.h"

namespace dq4ml {

namespace {

constexpr int kAlsBlock = 256;
constexpr int kAlsWaves = kAlsBlock / kWave;
constexpr int kIdxBlock = kWave;                            // ratings indexed by one load of the wave
constexpr int kGroupSteps = 4;                              // MFMA steps per gather group
constexpr int kGroupRatings = kGroupSteps * tile::kF64K;    // 16
constexpr int kGroups = kIdxBlock / kGroupRatings;          // 4: even, so the buffer parity is static
static_assert(kGroups % 2 == 0 && kAlsChunk % kIdxBlock == 0, "the gather ring's plan");

struct AlsArgs {
  AlsTable t;
  const void* Y;  // [S, rank] source factors
  void* X;        // [D, rank] destination factors
  int64_t S;
  int rank;
  double reg;
  double* slab;
  unsigned* status;
  double* presolve;
};

// doubles of a wave's LDS area: one system, padded to an even count
__host__ __device__ constexpr int als_area(int rank) { return (rank * (rank + 1) / 2 + rank + 1 + 1) & ~1; }

// Solve the system in `sys` (LDS, this wave's) and store row `out`; every lane of the wave calls.
template <typename TF>
__device__ __forceinline__ void als_solve(double* sys, int rank, double reg, int lane, TF* out, unsigned* status) {
  double* A = sys;
  const double* b = sys + rank * (rank + 1) / 2;
  const int j = lane;
  const bool has = j < rank;
  double* col = A + j * (j + 1) / 2;  // column j: rows 0..j
  const double m = b[rank];
  if (m == 0.0) {  // no rating: zeros, not a failure
    if (has) out[j] = (TF)0.0;
    return;
  }
  double bj = has ? b[j] : 0.0;
  if (has) col[j] += reg * m;
  bool fail = false;
  for (int k = 0; k < rank; ++k) {
    __builtin_amdgcn_wave_barrier();
    const double piv = A[k * (k + 1) / 2 + k];
    if (!(piv > 0.0)) {  // (NaN too)
      fail = true;
      break;
    }
    const double ukk = sqrt(piv);
    double ukj = 0.0;
    if (has && j >= k) {
      ukj = j == k ? ukk : col[k] / ukk;
      col[k] = ukj;
    }
    const double yk = __shfl(bj, k, kWave) / ukk;  // forward substitution: y_k, then b_j -= U[k][j] y_k
    if (j == k) bj = yk;
    else if (j > k) bj -= ukj * yk;
    __builtin_amdgcn_wave_barrier();
    if (has && j > k)
      for (int i = k + 1; i <= j; ++i) col[i] -= A[i * (i + 1) / 2 + k] * ukj;  // A[i][j] -= U[k][i] U[k][j]
  }
  __builtin_amdgcn_wave_barrier();
  if (fail) {
    if (lane == 0) atomicAdd(status, 1u);
    if (has) out[j] = (TF)NAN;
    return;
  }
  for (int k = rank - 1; k >= 0; --k) {  // U x = y: lane i < k holds y_i - sum over solved columns
    const double* ck = A + k * (k + 1) / 2;
    const double xk = __shfl(bj, k, kWave) / ck[k];
    if (j == k) bj = xk;
    else if (j < k) bj -= ck[j] * xk;
  }
  if (has) out[j] = (TF)bj;
}

// The gathers of one group: lane (f, q) takes element 16 t + f of the row of rating 16 g + 4 s + q
// of the indexed 64, s = 0..3; ex[s] is the lane's extra column of that rating (the rating, the 1,
// or nothing).  A rating past the segment's end has index -1: zeros everywhere.
template <typename TF, int NT>
__device__ __forceinline__ void als_gather(const TF* __restrict__ Y, int64_t S, int rank, int idx, double rat, int g,
                                           int f, int q, int xkind, TF (&v)[kGroupSteps][NT], double (&ex)[kGroupSteps],
                                           unsigned& bad) {
#pragma unroll
  for (int s = 0; s < kGroupSteps; ++s) {
    const int from = kGroupRatings * g + tile::kF64K * s + q;
    const int src = __shfl(idx, from, kWave);
    const double r = __shfl(rat, from, kWave);
    const bool live = src >= 0;
    const bool ok = (unsigned long long)(long long)src < (unsigned long long)S;  // (false for -1)
    if (live && !ok && f == 0) ++bad;
    const TF* row = Y + (int64_t)(ok ? src : 0) * rank;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = tile::kF64Tile * t + f;
      v[s][t] = ok && c < rank ? row[c] : (TF)0;
    }
    ex[s] = !ok ? 0.0 : xkind == 1 ? r : xkind == 2 ? 1.0 : 0.0;
  }
}

template <typename TF, int NT>
__device__ __forceinline__ void als_mfma(const TF (&v)[kGroupSteps][NT], const double (&ex)[kGroupSteps], int xt,
                                         int64_t left, f64x4 (&acc)[NT][NT]) {
#pragma unroll
  for (int s = 0; s < kGroupSteps; ++s) {
    if (tile::kF64K * s >= left) break;  // wave-uniform: the rest of the group is past the end
    double x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) x[t] = t >= NT - 2 && t == xt ? ex[s] : (double)v[s][t];
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J) acc[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[I], x[J], acc[I][J], 0, 0, 0);
  }
}

template <typename TF, int NT>
__global__ __launch_bounds__(kAlsBlock) void als_accum_kernel(AlsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int f = tile::f64_col(lane), q = tile::f64_k(lane);
  const int rank = a.rank;
  const int P = als_system_size(rank);
  double* sys = reinterpret_cast<double*>(smem) + wave * als_area(rank);
  const TF* Y = reinterpret_cast<const TF*>(a.Y);
  TF* X = reinterpret_cast<TF*>(a.X);

  // the lane's extra column: band column rank is the rating (kind 1), rank + 1 the 1 (kind 2)
  int xt = -1, xkind = 0;
  if (rank % tile::kF64Tile == f) xt = rank / tile::kF64Tile, xkind = 1;
  if ((rank + 1) % tile::kF64Tile == f) xt = (rank + 1) / tile::kF64Tile, xkind = 2;
  unsigned bad = 0;

  for (int64_t c = (int64_t)blockIdx.x * kAlsWaves + wave; c < a.t.nchunks; c += (int64_t)gridDim.x * kAlsWaves) {
    const int d = a.t.chunk_dst[c];
    const int64_t k = c - a.t.cstart[d];
    const int64_t seg0 = a.t.offsets[d] + k * a.t.chunk;
    int64_t seg1 = a.t.offsets[d + 1];
    if (seg1 > seg0 + a.t.chunk) seg1 = seg0 + a.t.chunk;

    f64x4 acc[NT][NT];
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J) acc[I][J] = f64x4{};

    TF v[2][kGroupSteps][NT];
    double ex[2][kGroupSteps];
    int idx = -1;
    double rat = 0.0;
    if (seg0 + lane < seg1) {
      idx = a.t.src[seg0 + lane];
      rat = a.t.rating[seg0 + lane];
    }
    if (seg0 < seg1) als_gather<TF, NT>(Y, a.S, rank, idx, rat, 0, f, q, xkind, v[0], ex[0], bad);
    for (int64_t b0 = seg0; b0 < seg1; b0 += kIdxBlock) {
      const int64_t nb0 = b0 + kIdxBlock;
      int nidx = -1;
      double nrat = 0.0;
      if (nb0 + lane < seg1) {  // the next 64: in flight for the whole of this 64
        nidx = a.t.src[nb0 + lane];
        nrat = a.t.rating[nb0 + lane];
      }
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        const int64_t gnext = b0 + kGroupRatings * (g + 1);
        if (gnext < seg1) {  // the next group's rows, before this group's products
          if (g + 1 < kGroups) als_gather<TF, NT>(Y, a.S, rank, idx, rat, g + 1, f, q, xkind, v[(g + 1) & 1], ex[(g + 1) & 1], bad);
          else als_gather<TF, NT>(Y, a.S, rank, nidx, nrat, 0, f, q, xkind, v[0], ex[0], bad);
        }
        als_mfma<TF, NT>(v[g & 1], ex[g & 1], xt, seg1 - (b0 + kGroupRatings * g), acc);
        if (gnext >= seg1) break;
      }
      idx = nidx;
      rat = nrat;
    }

    // accumulators -> the packed system: D[i = f64_acc_row(reg, lane)][j = f] of tile (I, J)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = tile::kF64Tile * I + tile::f64_acc_row(reg, lane), j = tile::kF64Tile * J + f;
          const double val = acc[I][J][reg];
          if (j < rank && i <= j) sys[j * (j + 1) / 2 + i] = val;
          else if (j == rank && i < rank) sys[rank * (rank + 1) / 2 + i] = val;
          else if (j == rank + 1 && i == rank + 1) sys[P - 1] = val;
        }
    __builtin_amdgcn_wave_barrier();

    const int64_t row = a.t.slab_of[d];
    if (row >= 0) {  // one of several chunks: the partial system to its slab row
      double* out = a.slab + (row + k) * P;
      for (int p = lane; p < P; p += kWave) out[p] = sys[p];
    } else {
      if (a.presolve != nullptr)
        for (int p = lane; p < P; p += kWave) a.presolve[(int64_t)d * P + p] = sys[p];
      als_solve<TF>(sys, rank, a.reg, lane, X + (int64_t)d * rank, a.status);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (bad != 0) atomicAdd(a.status + 1, bad);
}

// one wave per long destination: the slab rows of its chunks summed in chunk order, then the solve
template <typename TF>
__global__ __launch_bounds__(kAlsBlock) void als_long_kernel(AlsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int rank = a.rank;
  const int P = als_system_size(rank);
  double* sys = reinterpret_cast<double*>(smem) + wave * als_area(rank);
  for (int64_t l = (int64_t)blockIdx.x * kAlsWaves + wave; l < a.t.nlong; l += (int64_t)gridDim.x * kAlsWaves) {
    const int d = a.t.long_dst[l];
    const int64_t nch = a.t.cstart[d + 1] - a.t.cstart[d];
    const double* rows = a.slab + a.t.slab_of[d] * P;
    for (int p = lane; p < P; p += kWave) {
      double s = 0.0;
      for (int64_t k = 0; k < nch; ++k) s += rows[k * P + p];
      sys[p] = s;
      if (a.presolve != nullptr) a.presolve[(int64_t)d * P + p] = s;
    }
    __builtin_amdgcn_wave_barrier();
    als_solve<TF>(sys, rank, a.reg, lane, reinterpret_cast<TF*>(a.X) + (int64_t)d * rank, a.status);
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void als_chunk_counts_kernel(const int64_t* offsets, int64_t D, int chunk, long long* cstart) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const int64_t len = offsets[d + 1] - offsets[d];
  cstart[d] = len <= chunk ? 1 : (len + chunk - 1) / chunk;
}

__global__ void als_chunk_fill_kernel(const int64_t* cstart, int64_t D, int* chunk_dst) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  for (int64_t c = cstart[d]; c < cstart[d + 1]; ++c) chunk_dst[c] = (int)d;
}

template <typename TF>
__global__ void als_predict_kernel(const int* u, const int* v, const uint8_t* sel, int64_t n, const TF* U, const TF* V,
                                   int rank, double* out) {
  // 16 lanes per row: lane f takes components f, f + 16, ..., summed over the lanes by a butterfly
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int f = threadIdx.x & 15;
  const bool in = i < n;
  const bool live = in && (sel == nullptr || sel[i] != 0);
  const int ui = live ? u[i] : -1, vi = live ? v[i] : -1;
  const bool ok = ui >= 0 && vi >= 0;
  double s = 0.0;
  if (ok)
    for (int c = f; c < rank; c += 16) s += (double)U[(int64_t)ui * rank + c] * (double)V[(int64_t)vi * rank + c];
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, kWave);
  if (in && f == 0) out[i] = ok ? s : (double)NAN;
}

template <typename TF, typename F>
void with_als_nt(int rank, F&& f) {
  switch ((rank + 2 + 15) / 16) {
    case 1: return f(als_accum_kernel<TF, 1>);
    case 2: return f(als_accum_kernel<TF, 2>);
    case 3: return f(als_accum_kernel<TF, 3>);
    case 4: return f(als_accum_kernel<TF, 4>);
    default: return f(als_accum_kernel<TF, 5>);
  }
}

// f(accumulate kernel, long kernel)
template <typename F>
void with_als_kernel(int rank, int fdt, F&& f) {
  if (rank < kAlsMinRank || rank > kAlsMaxRank) throw std::invalid_argument("als: rank must be in [1, 64]");
  if (fdt == DT_F64) return with_als_nt<double>(rank, [&](auto kern) { f(kern, als_long_kernel<double>); });
  if (fdt == DT_F32) return with_als_nt<float>(rank, [&](auto kern) { f(kern, als_long_kernel<float>); });
  throw std::invalid_argument("als: factors must be f32 or f64");
}

size_t als_lds(int rank) { return (size_t)kAlsWaves * als_area(rank) * sizeof(double); }

}  // namespace

void als_chunk_counts(const int64_t* offsets, int64_t D, int chunk, int64_t* cstart, hipStream_t st) {
  if (offsets == nullptr || cstart == nullptr) throw std::invalid_argument("als: null chunk table operand");
  if (D < 1 || D >= (int64_t)1 << 31) throw std::invalid_argument("als: between 1 and 2^31 - 1 destinations");
  if (chunk < kIdxBlock || chunk % kIdxBlock != 0) throw std::invalid_argument("als: chunk must be a positive multiple of 64");
  hipLaunchKernelGGL(als_chunk_counts_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, offsets, D, chunk,
                     reinterpret_cast<long long*>(cstart));
  DQ_HIP_CHECK(hipGetLastError());
}

void als_chunk_fill(const int64_t* cstart, int64_t D, int* chunk_dst, hipStream_t st) {
  if (cstart == nullptr || chunk_dst == nullptr) throw std::invalid_argument("als: null chunk table operand");
  if (D < 1 || D >= (int64_t)1 << 31) throw std::invalid_argument("als: between 1 and 2^31 - 1 destinations");
  hipLaunchKernelGGL(als_chunk_fill_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, cstart, D, chunk_dst);
  DQ_HIP_CHECK(hipGetLastError());
}

int als_blocks(int rank, int fdt, int64_t nchunks) {
  int nb = 1;
  with_als_kernel(rank, fdt, [&](auto kern, auto) {
    nb = occupancy_grid(kern, kAlsBlock, als_lds(rank), (nchunks + kAlsWaves - 1) / kAlsWaves);
  });
  return nb;
}

void als_half_step(const AlsTable& t, const void* src_f, void* dst_f, int fdt, int64_t S, int rank, double reg,
                   double* slab, unsigned* status, double* presolve, int blocks, hipStream_t st) {
  if (t.offsets == nullptr || t.cstart == nullptr || t.chunk_dst == nullptr || t.slab_of == nullptr || src_f == nullptr ||
      dst_f == nullptr || status == nullptr)
    throw std::invalid_argument("als: null operand");
  if (t.D < 1 || t.D >= (int64_t)1 << 31 || S < 1 || S >= (int64_t)1 << 31)
    throw std::invalid_argument("als: between 1 and 2^31 - 1 destinations and sources");
  if (t.nchunks < t.D || t.nlong < 0 || t.nlong > t.D) throw std::invalid_argument("als: inconsistent chunk table");
  if (t.chunk < kIdxBlock || t.chunk % kIdxBlock != 0) throw std::invalid_argument("als: chunk must be a positive multiple of 64");
  if (t.nchunks > t.D && (t.src == nullptr || t.rating == nullptr)) throw std::invalid_argument("als: null ratings");
  if (t.nlong > 0 && (slab == nullptr || t.long_dst == nullptr)) throw std::invalid_argument("als: long segments need a slab");
  if (!(reg >= 0.0)) throw std::invalid_argument("als: reg must be >= 0");
  if (blocks < 1) throw std::invalid_argument("als: blocks must be >= 1");
  with_als_kernel(rank, fdt, [&](auto kern, auto long_kern) {
    AlsArgs a{t, src_f, dst_f, S, rank, reg, slab, status, presolve};
    const size_t lds = als_lds(rank);
    DQ_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kAlsBlock), lds, st, a);
    if (t.nlong > 0) {
      DQ_HIP_CHECK(hipFuncSetAttribute((const void*)long_kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const int64_t want = (t.nlong + kAlsWaves - 1) / kAlsWaves;
      hipLaunchKernelGGL(long_kern, dim3((unsigned)(want < blocks ? want : blocks)), dim3(kAlsBlock), lds, st, a);
    }
  });
  DQ_HIP_CHECK(hipGetLastError());
}

void als_predict(const int* u, const int* v, const uint8_t* sel, int64_t n, const void* U, const void* V, int fdt, int rank,
                 double* out, hipStream_t st) {
  if (n < 0 || n >= (int64_t)1 << 31) throw std::invalid_argument("als_predict: fewer than 2^31 rows per call");
  if (rank < kAlsMinRank || rank > kAlsMaxRank) throw std::invalid_argument("als_predict: rank must be in [1, 64]");
  if (n == 0) return;
  if (u == nullptr || v == nullptr || U == nullptr || V == nullptr || out == nullptr)
    throw std::invalid_argument("als_predict: null operand");
  const dim3 grid((unsigned)((n * 16 + 255) / 256));
  if (fdt == DT_F64)
    hipLaunchKernelGGL(als_predict_kernel<double>, grid, dim3(256), 0, st, u, v, sel, n, reinterpret_cast<const double*>(U),
                       reinterpret_cast<const double*>(V), rank, out);
  else if (fdt == DT_F32)
    hipLaunchKernelGGL(als_predict_kernel<float>, grid, dim3(256), 0, st, u, v, sel, n, reinterpret_cast<const float*>(U),
                       reinterpret_cast<const float*>(V), rank, out);
  else
    throw std::invalid_argument("als_predict: factors must be f32 or f64");
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
