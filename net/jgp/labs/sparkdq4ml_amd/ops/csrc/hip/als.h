// K5a: one half-step of alternating least squares (Spark 2.4 ml.recommendation.ALS, explicit
// feedback, ALS-WR scaling): for every destination d with ratings r_j of sources y_j, j = 1..m,
// solve (sum y_j y_j^T + reg m I) x = sum r_j y_j by Cholesky and store x as the destination's
// factor row (see als.hip).  Also the prediction pass of a fitted model.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

// The fused range, stated here once (ops/als.py mirrors it).
constexpr int kAlsMinRank = 1, kAlsMaxRank = 64;
// Ratings of one destination that one wave accumulates (a chunk); a multiple of the 64 ratings a
// wave indexes with one load.  profiles/als.md has the alternatives measured.
constexpr int kAlsChunk = 2048;

// doubles of one pre-solve system: the packed upper triangle of Y^T Y (column-major: entry (i, j),
// i <= j, at j (j + 1) / 2 + i), the right-hand side, the rating count m
constexpr int als_system_size(int rank) { return rank * (rank + 1) / 2 + rank + 1; }

// The segment table of one side and its chunk table.  Destination d owns the ratings
// [offsets[d], offsets[d + 1]) of src / rating and the chunks [cstart[d], cstart[d + 1]), at least
// one (an empty segment has one empty chunk); chunk c belongs to destination chunk_dst[c].  A
// destination of several chunks has slab_of[d] >= 0, the slab row of its first chunk, and is
// listed in long_dst; every other destination has slab_of[d] = -1.
struct AlsTable {
  const int64_t* offsets;  // [D + 1]
  const int* src;          // [nnz], each in [0, S)
  const double* rating;    // [nnz]
  const int64_t* cstart;   // [D + 1]
  const int* chunk_dst;    // [nchunks]
  const int64_t* slab_of;  // [D]
  const int* long_dst;     // [nlong]
  int64_t D, nchunks, nlong;
  int chunk;               // ratings per chunk: a positive multiple of 64
};

// cstart[d] = max(1, ceil(len_d / chunk)) for d < D (the caller scans it with scan_counts)
void als_chunk_counts(const int64_t* offsets, int64_t D, int chunk, int64_t* cstart, hipStream_t st);
// chunk_dst of the scanned cstart
void als_chunk_fill(const int64_t* cstart, int64_t D, int* chunk_dst, hipStream_t st);

// grid of the accumulate pass for nchunks chunks: occupancy-sized
int als_blocks(int rank, int fdt, int64_t nchunks);
// One half-step: dst [D, rank] from src_f [S, rank] (both row-major, fdt = DT_F32 or DT_F64).
// slab: [rows of the long destinations' chunks][als_system_size(rank)] doubles (may be null when
// nlong == 0).  status[0] counts the destinations whose factorisation met a non-positive pivot
// (their row is NaN), status[1] the ratings whose source index lies outside [0, S) (skipped).
// presolve (tests; may be null): [D][als_system_size(rank)], every destination's system as it
// enters the solve, before the ridge term.  Two launches; no floating-point atomics.
void als_half_step(const AlsTable& t, const void* src_f, void* dst_f, int fdt, int64_t S, int rank, double reg,
                   double* slab, unsigned* status, double* presolve, int blocks, hipStream_t st);

// out[i] = the f64 dot product of rows u[i] of U and v[i] of V ([*, rank], fdt) for live rows
// (sel null or sel[i] != 0) with both indices >= 0, else NaN
void als_predict(const int* u, const int* v, const uint8_t* sel, int64_t n, const void* U, const void* V, int fdt, int rank,
                 double* out, hipStream_t st);

}  // namespace dq4ml
