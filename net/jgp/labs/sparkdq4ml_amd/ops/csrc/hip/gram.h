// K5 Gram / WLS-statistics kernels (see gram.hip).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"  // PackSrc
#endif

namespace dq4ml {

// GRAM_F32S: f32 statistics from split-bf16 products (each f32 = hi + mid + lo bf16, the six
// leading cross products on the bf16 MFMA; f32 accumulation) — exact-f32-class error at the bf16
// MFMA rate (gram_stream.hip)
enum GramMode : int { GRAM_F64 = 0, GRAM_F32 = 1, GRAM_BF16 = 2, GRAM_FP8 = 3, GRAM_F32S = 4 };

struct GramArgs {
  const void* X;       // feature-major [d, ld]
  int64_t ld;          // elements between consecutive features
  int d;
  int64_t n;
  int xdt;             // DType of X
  const void* y;       // label [n]
  int ydt;
  const void* w;       // weights [n] or null
  int wdt;
  const uint8_t* sel;  // selection [n] (bool) or null
  double* partials;    // [blocks][P]
  int P;
  // Set by each launcher for its kernel.  spw: supersteps (64 rows; gram_cols: per block; the
  // stream kernels: stages of 64 or 32 rows) of a wave's one contiguous range; the tall bf16 kernel
  // interleaves the waves and does not read it.  nsuper: the supersteps the ranges cover -- full
  // ones only, n / 64 (gram_tall) or n / stage rows (gram_stream), the ragged rest handled apart;
  // the ragged one included, ceil(n / 64), for gram_cols, gram_folds and glm_irls_pass.
  int64_t spw;
  int64_t nsuper;
  int tiled;           // X is MFMA-fragment-ordered bf16 (tile_bf16 layout)
  // columnar skinny f64 mode (cols = d <= 8, X unused): feature f is the source column colp[f]
  // of DType coldt[f] — a VectorAssembler output read straight from its inputs, never packed
  const void* colp[8];
  int coldt[8];
  int cols;
  // stream kernels over source columns (gram_stream_cols): [2 * d] int64 device table of
  // (column pointer, dtype) pairs — feature f is column srcs[2 f] (all of X's dtype xdt)
  const int64_t* srcs;
  // stream kernels only: 1 = wave w takes stages w, w + W, w + 2W, ... (W = total waves) instead of
  // one contiguous range.  gram_stream always sets 0 (the interleaved order lost its A/B there);
  // the tall bf16 kernel takes the interleaved order unconditionally and does not read this
  int interleave;
  // stream kernels compiled with a DQ row predicate (ops/streamfuse.py, hipRTC): per-lane DMA
  // sources of the stage's row-scalar area — [64 lanes][(base, bytes per row) x 2 instructions]
  // int64 pairs, then the region pointers the guarded tail stage copies from
  const int64_t* rawtab;
  // per-feature f32 shift s (null: none): kernels that round the features (bf16 / exact-f32 /
  // split-f32 MFMA) accumulate the statistics of x - s, so a column with |mean| >> std keeps its
  // digits through the cast and the f32 accumulators; stats_unshift restores those of x in f64
  // (SURVEY.md §7e.2).  Dead and padding rows stay exactly zero.
  const float* xshift;
  // tiled storage with a 12-bit packed companion (pack_tiles below; null: none).  xdir[s * NT + t]
  // is the exponent base of superstep-tile (s, t), or 0xFF where that entry is read raw from X;
  // xpack holds one 3 KiB slot per entry at (s * NT + t) * 768 dwords.  The directory is word
  // aligned and allocated in whole 32-bit words (the kernel reads the aligned word around a byte).
  const uint32_t* xpack;
  const uint8_t* xdir;
  // the all-packed ("patched") companion instead (patch_tiles below; null: none): xpack holds a
  // slot for every entry of the full supersteps, xrec one 16-byte directory record per entry
  // (16-byte aligned) and xovf the overflow records of entries with more than three exceptions
  const uint32_t* xrec;
  const uint32_t* xovf;
};

#ifndef __HIPCC_RTC__
// MFMA-fragment-ordered bf16 feature storage ("tiled"): for superstep s (64 rows), 32-feature
// tile t, k-step i: 64 lanes x 16 B contiguous, lane l = 32h + f holding rows s*64+32h+8i..+8 of
// feature 32t+f.  One wave load instruction = 1 KiB contiguous; zero padded to whole supersteps.
int64_t tiled_elems(int d, int64_t n);

// shift: per-feature f32 shift subtracted before the bf16 cast (null: none; rows >= n stay zero)
void tile_bf16(const void* X, int xdt, int64_t ld, int d, int64_t n, void* out, hipStream_t st,
               const float* shift = nullptr);

// Lossless 12-bit companion of the tiled storage (the layout and its torch reference: ops/layout.py
// pack_reference).  Entry (s, t) is packable iff the 8-bit exponent fields of its 2048 stored
// values span <= 15 binades (emax - emin <= 15, emin <= 254); then dir = emin and every value is
// sign + 4-bit exponent offset + 7-bit mantissa.  A lane's fragment of k-step i (8 values = 4
// dwords R0..R3) becomes 3 dwords D0..D2: Dk keeps the sign (bit 15) and the low 11 code bits of
// R_k's two halfwords, and bits 14..11 of D0 / D1 / D2 carry code bits 3..0 / 7..4 / sign:10..8 of
// R3's.  The slot is 3 pieces of 64 lanes x 16 B; piece k holds lane l's D_k of k-steps 0..3.
// Raw entries (dir 0xFF) have a zero-filled slot.  *npacked (one device word, zeroed by the
// caller) counts the packed entries.  One wave per entry.
void pack_tiles(const void* tiles, int d, int64_t n, uint8_t* dir, uint32_t* slots, uint32_t* npacked,
                hipStream_t st);

// The patched companion (torch reference: ops/layout.py patch_reference): EVERY entry of the full
// supersteps is packed (d a multiple of 32; the zero-padded ragged superstep is not covered and is
// read raw).  base = emin where emax - emin <= 15 (the slot is then pack_tiles' bit for bit), else
// emax - 15.  A value whose exponent field is below base is an exception: its slot code is the
// filler 0 (it decodes to +2^(base-127)) and its 16 stored bits travel in a record
//     lane << 21 | dword << 17 | halfword << 16 | bits
// (dword = 4 * k-step + the dword within the lane's fragment, so record >> 16 is the halfword's
// index among the lane-major 2048 of the entry).  The records of an entry are sorted by that
// index: a pure function of the data.  Directory record of entry e, four dwords at rec[4 e]:
//     word 0 = base | count << 8
//     count <= 3: words 1.. = the records themselves (unused words 0)
//     count >  3: word 1 = index into ovf of the entry's first record, all of them there
// The reader decodes the slot like any packed one and then writes each record's bits over the
// named halfword of the owning lane, which restores the raw tile bit for bit.
// patch_tiles_count: counts[e] = exceptions of entry e, stat[0] += their total, stat[1] = max
// (stat zeroed by the caller).  The caller accepts or rejects the table on those, turns counts
// into ovoff (exclusive running sum of the counts above 3) and calls patch_tiles_fill with rec
// zeroed.  One wave per entry in both.
constexpr int kPatchInline = 3;
void patch_tiles_count(const void* tiles, int64_t nent, uint32_t* counts, unsigned long long* stat, hipStream_t st);
void patch_tiles_fill(const void* tiles, int64_t nent, const uint32_t* ovoff, uint32_t* slots, uint32_t* rec,
                      uint32_t* ovf, hipStream_t st);

int64_t gram_partial_stride(int mode, int d);
// grid that exactly fills the chip for the kernel instantiation (occupancy-sized, persistent-style)
int gram_plan_blocks(int mode, int d, int64_t n, int xdt, int xmode);
// xmode: 0 = X already zero on dead rows (or no sel/w), 1 = binary mask from sel, 2 = general weights
// reduce = false: only the per-block partial slabs; gram_reduce (same mode/blocks/d) folds them
// later, possibly on another stream
void gram_tall(int mode, GramArgs a, int xmode, int blocks, double* out, hipStream_t st, bool reduce = true);
void gram_reduce(int mode, const double* partials, int blocks, int d, double* out, hipStream_t st);
// flat statistics of x' = x - s (GramArgs::xshift) -> those of x, in place, in f64:
//   Σw·x = Σw·x' + s·Σw,  Σw·x·y = Σw·x'·y + s·Σw·y,
//   Σw·xᵢ·xⱼ = Σw·x'ᵢ·x'ⱼ + sᵢ·Σw·x'ⱼ + sⱼ·Σw·x'ᵢ + sᵢ·sⱼ·Σw
// (exact algebra for any fixed s: DQ selections and weights are already in the sums)
void stats_unshift(double* flat, const float* shift, int d, hipStream_t st);

// The fused CSV scans' per-window statistics part[rows][gw] (gw = 3 + 2d + d(d+1)/2: live count,
// Σy, Σy², Σx, Σxy, packed-upper Σxx) -> the flat gram_stats layout [n, n, n, Σy, Σy², ...]
// (unit weights), every column summed in one fixed order: one launch instead of a column-sum
// kernel plus a concatenation (ops/scanfuse.py, ops/scancut.py)
void gram_window_fold(const double* part, int64_t rows, int gw, double* flat, hipStream_t st);

// LDS-DMA streamed tall kernels (gram_stream.hip): GRAM_F64 on f64/f32 features, GRAM_F32
// (exact-f32 MFMA) on f32 features.  gram_stream_ok: operand dtypes/alignment the DMA path needs.
bool gram_stream_ok(int mode, const GramArgs& a);
int gram_stream_blocks(int mode, int d, int64_t n, int xdt);
void gram_stream(int mode, GramArgs a, int xmode, int blocks, double* out, hipStream_t st, bool reduce = true);
// GRAM_BF16 on f32 storage rides the same stream kernel (bf16 MFMA on converted LDS tiles); with
// a.srcs set the features are d separate f32 columns (fused VectorAssembler + Gram)

// fused VectorAssembler + bf16 Gram over d <= 64 source columns (a.X unused; a.sel masks rows)
int gram_cols_blocks(int d, int64_t n);
// sdt: the common source dtype (DT_F32 / DT_F64 / DT_BF16, 16-byte aligned columns) or -1 (mixed)
void gram_cols(GramArgs a, const PackSrc* srcs_dev, int sdt, int blocks, double* out, hipStream_t st);

// a stream kernel compiled by hipRTC with a DQ row predicate (ops/streamfuse.py): the same
// argument setup as gram_stream (mode GRAM_F32 / GRAM_BF16, binary row mask), launched through
// the module function ``fn`` with ``lds`` bytes of dynamic LDS
void gram_stream_rtc(void* fn, int mode, GramArgs a, int blocks, size_t lds, double* out, hipStream_t st);
#endif

}  // namespace dq4ml
