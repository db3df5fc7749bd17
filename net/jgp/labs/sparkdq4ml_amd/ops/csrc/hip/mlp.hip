// K5p: one evaluation of the loss and gradient of a small dense network (sigmoid hidden layers,
// softmax + cross-entropy on top) as ONE kernel over feature-major X[d, n]: X comes from HBM once,
// nothing of size n is written, and every activation and delta of a row lives on the chip.  The
// same forward code, in MLP_PREDICT mode, writes a fitted model's prediction column.
//
// Work split: the staged f64 plan of gram_slab.h section 5 (kBlock = 256, a wave keeps one
// contiguous range of 64-row supersteps), but a superstep is taken as four ROW tiles of 16 rows x
// all d features, not as feature tiles of 64 rows: the whole network -- forward, deltas, the three
// weight gradients -- runs for 16 rows before the next 16 are staged, so the first layer's forward
// product and its weight gradient read the same staged tile and no tile is staged twice.  A row
// tile is staged as xs[feature][16 rows] (row stride kLd = 18 doubles) by 16-byte loads, 64-byte
// (f32) or 128-byte (f64) runs per feature.  Rows that are dead, >= n or carry a bad label are
// selected to zero while they are staged, never multiplied: their features and labels may be NaN.
//
// Everything is computed transposed, units x rows, by v_mfma_f64_16x16x4f64 (lane = (f, q), f =
// lane & 15, q = lane >> 4; A[i = f][k = q], B[k = q][j = f], D[i = 4 reg + q][j = f]):
//   forward   Z_l^T[unit][row] = W_l A_{l-1}^T, the accumulators starting at the bias.  A = W_l from
//             LDS (the weights sit there, zero padded, for the whole kernel), B = the staged tile
//             for layer 0 and, for the layers above, the lane's own activation registers: lane
//             (f, q) holds row f of units 16 ut + 4 reg + q, which is the B operand of k-step
//             (ut, reg) of the next layer with no move.
//   softmax   a row's classes lie in the lane's 8 accumulators and across q: max and sum in-lane,
//             then __shfl_xor 16 and 32.  The pad classes carry the bias -inf, so they never win the
//             max, add exp(-inf) = 0 and get the delta 0.  The row loss max + log(sum) - z_y is
//             taken by the lane that owns class y.
//   deltas    Delta_{l-1}^T = (W_l^T Delta_l^T) . a (1 - a): A = the transposed read of W_l from
//             LDS, B = the lane's own delta registers, again with no move.
//   dW_l      Delta_l^T A_{l-1} contracts over rows, which sit on f in the registers: the delta and
//             the activations cross the wave's LDS area (dbuf, abuf: [32 units][kLd]) to put rows
//             on q; for layer 0 the staged tile is already there.
//   db_l      the in-lane sum of the deltas, combined over f once at the end.
//
// Widths: the input tiles NT0 = ceil(d / 16) and the depth are template parameters; the hidden
// and class widths are runtime tile counts (1 or 2) under a compile-time maximum of 2: the loops
// over unit tiles are unrolled and a wave-uniform branch skips the tiles a narrow layer does not
// have.  32 instantiations (2 dtypes x 4 NT0 x 2 depths x 2 modes); profiles/mlp.md lists the
// registers of each.
//
// Slabs (MLP_GRAD): one partial per block, [P gradient in the weight vector's layout, loss, live
// rows, bad labels], folded over the waves in order in LDS (the loop's area, dead by then), summed
// over the blocks in block order by slab_sum.  Plain launches, no atomics: bit-identical run to run.
#include "mlp.h"

#include <cmath>

#include "common.h"
#include "gram_slab.h"

namespace dq4ml {

namespace {

constexpr int kHT = kMlpMaxWidth / 16;  // unit tiles of a hidden / class layer (compile-time maximum)
constexpr int kHW = 16 * kHT;           // padded units
constexpr int kLd = 18;                 // doubles per LDS row of 16 rows: even (16-byte stores), off the banks
constexpr int kLdH = kHW + 1;           // doubles per LDS weight row of a layer above the first

struct MlpArgs {
  const double* w;  // [P]
  double* pred;     // MLP_PREDICT: [n]
  int width[kMlpMaxLayers];
};

// the LDS plan in doubles, per (NT0, DEPTH, GRAD): per wave xs [16 NT0][kLd], then (GRAD) abuf
// [DEPTH][kHW][kLd] and dbuf [kHW][kLd]; behind the four waves W_0 [kHW][16 NT0 + 1], W_l [kHW][kLdH]
// and the biases [DEPTH + 1][kHW]
constexpr int mlp_wave_area(int NT0, int DEPTH, bool grad) { return 16 * NT0 * kLd + (grad ? (DEPTH + 1) * kHW * kLd : 0); }
constexpr int mlp_w_area(int NT0, int DEPTH) { return kHW * (16 * NT0 + 1) + DEPTH * kHW * kLdH + (DEPTH + 1) * kHW; }
constexpr size_t mlp_lds_bytes(int NT0, int DEPTH, bool grad) {
  return (size_t)(kWavesPerBlock * mlp_wave_area(NT0, DEPTH, grad) + mlp_w_area(NT0, DEPTH)) * sizeof(double);
}
// the block reduction's slab aliases the LDS from its start: P + 3 <= the padded weights + 3
static_assert(mlp_lds_bytes(4, 2, true) <= 160 * 1024, "the widest plan must fit the CU's LDS");

// Rows [row0, row0 + 16) x features [0, 16 NT0) into xs[feature][row]; zeros for features >= d,
// rows >= n and rows whose bit in `ok` is clear.  full: all 16 rows exist (16-byte loads).
template <typename TX, int NT0>
__device__ __forceinline__ void mlp_stage(const TX* __restrict__ X, int64_t ld, int d, int64_t row0, int64_t n,
                                          bool full, unsigned ok, int lane, double* xs) {
  if (full) {
    constexpr int kPer = 16 / sizeof(TX);  // elements per 16-byte chunk
    constexpr int kChunks = 16 / kPer;     // chunks per feature
    constexpr int kIters = 16 * NT0 * kChunks / 64;
    typedef __attribute__((ext_vector_type(kPer))) TX vec;
    vec v[kIters];
#pragma unroll
    for (int i = 0; i < kIters; ++i) {  // all loads in flight first
      const int c = i * 64 + lane;
      const int feat = c / kChunks, k = c % kChunks;
      const TX* src = X + (int64_t)(feat < d ? feat : 0) * ld + row0 + k * kPer;
      v[i] = feat < d ? __builtin_nontemporal_load(reinterpret_cast<const vec*>(src)) : vec{};
    }
#pragma unroll
    for (int i = 0; i < kIters; ++i) {
      const int c = i * 64 + lane;
      const int feat = c / kChunks, k = c % kChunks;
      double* dst = xs + feat * kLd + k * kPer;
#pragma unroll
      for (int j = 0; j < kPer; j += 2) {
        const double lo = (ok >> (k * kPer + j)) & 1u ? (double)v[i][j] : 0.0;
        const double hi = (ok >> (k * kPer + j + 1)) & 1u ? (double)v[i][j + 1] : 0.0;
        *reinterpret_cast<f64x2*>(dst + j) = f64x2{lo, hi};
      }
    }
  } else {
    for (int i = lane; i < 16 * NT0 * 16; i += 64) {
      const int feat = i >> 4, rr = i & 15;
      double v = 0.0;
      if (feat < d && row0 + rr < n && ((ok >> rr) & 1u)) v = (double)X[(int64_t)feat * ld + row0 + rr];
      xs[feat * kLd + rr] = v;
    }
  }
}

// a = sigmoid(z), overflow-safe: one exp of a non-positive argument
__device__ __forceinline__ double mlp_sigmoid(double z) {
  const double t = exp(-fabs(z));
  return z >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t);
}

// z = the layer's bias: lane (f, q) holds units 16 ut + 4 reg + q
__device__ __forceinline__ void mlp_bias(const double* b, int q, f64x4 (&z)[kHT]) {
#pragma unroll
  for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) z[ut][reg] = b[16 * ut + 4 * reg + q];
}

// forward of a layer above the first: z += W in, the B operand = the lane's own activations
__device__ __forceinline__ void mlp_forward(const double* W, const f64x4 (&in)[kHT], int IT, int OT, int f, int q,
                                            f64x4 (&z)[kHT]) {
#pragma unroll
  for (int ui = 0; ui < kHT; ++ui)
    if (ui < IT) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int uo = 0; uo < kHT; ++uo)
          if (uo < OT)
            z[uo] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[(16 * uo + f) * kLdH + 16 * ui + 4 * reg + q], in[ui][reg],
                                                         z[uo], 0, 0, 0);
    }
}

// a = sigmoid(z) in place; GRAD: also to abuf[unit][row] for the next layer's weight gradient
template <bool GRAD>
__device__ __forceinline__ void mlp_activate(f64x4 (&z)[kHT], int f, int q, double* abuf) {
#pragma unroll
  for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      z[ut][reg] = mlp_sigmoid(z[ut][reg]);
      if constexpr (GRAD) abuf[(16 * ut + 4 * reg + q) * kLd + f] = z[ut][reg];
    }
}

// the layer's delta: db += delta in-lane, delta to dbuf[unit][row], then
// G[uo][ui] (out 16 uo + 4 reg + q, in 16 ui + f) += delta(out, row) prev(in, row) over the 16 rows
template <int NI>
__device__ __forceinline__ void mlp_dw(const f64x4 (&dl)[kHT], f64x4 (&gb)[kHT], double* dbuf, const double* prev,
                                       int IT, int OT, int f, int q, f64x4 (&G)[kHT][NI]) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ut = 0; ut < kHT; ++ut) {
    gb[ut] += dl[ut];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) dbuf[(16 * ut + 4 * reg + q) * kLd + f] = dl[ut][reg];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    double av[kHT];
#pragma unroll
    for (int uo = 0; uo < kHT; ++uo) av[uo] = dbuf[(16 * uo + f) * kLd + 4 * ks + q];
#pragma unroll
    for (int ui = 0; ui < NI; ++ui)
      if (ui < IT) {
        const double bv = prev[(16 * ui + f) * kLd + 4 * ks + q];
#pragma unroll
        for (int uo = 0; uo < kHT; ++uo)
          if (uo < OT) G[uo][ui] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[uo], bv, G[uo][ui], 0, 0, 0);
      }
  }
  __builtin_amdgcn_wave_barrier();
}

// delta of the layer below: dl = (W^T dl) . a (1 - a), the B operand = the lane's own delta
__device__ __forceinline__ void mlp_backward(const double* W, const f64x4 (&a)[kHT], int IT, int OT, int f, int q,
                                             f64x4 (&dl)[kHT]) {
  f64x4 nd[kHT];
#pragma unroll
  for (int ui = 0; ui < kHT; ++ui) nd[ui] = f64x4{};
#pragma unroll
  for (int uo = 0; uo < kHT; ++uo)
    if (uo < OT) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int ui = 0; ui < kHT; ++ui)
          if (ui < IT)
            nd[ui] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[(16 * uo + 4 * reg + q) * kLdH + 16 * ui + f], dl[uo][reg],
                                                          nd[ui], 0, 0, 0);
    }
#pragma unroll
  for (int ui = 0; ui < kHT; ++ui)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) dl[ui][reg] = nd[ui][reg] * (a[ui][reg] * (1.0 - a[ui][reg]));
}

// one wave's gradient of a layer into the block's slab at `out` (Spark's layout: W column-major
// numOut x numIn, then b); gb is already summed over f
template <int NI>
__device__ __forceinline__ void mlp_fold(double* out, int I, int O, const f64x4 (&G)[kHT][NI], const f64x4 (&gb)[kHT],
                                         int f, int q) {
#pragma unroll
  for (int uo = 0; uo < kHT; ++uo)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = 16 * uo + 4 * reg + q;
      if (o < O) {
        if (f == 0) out[I * O + o] += gb[uo][reg];
#pragma unroll
        for (int ui = 0; ui < NI; ++ui)
          if (16 * ui + f < I) out[(16 * ui + f) * O + o] += G[uo][ui][reg];
      }
    }
}

// a.nsuper = supersteps (ceil(n / 64)), a.spw = supersteps per wave; a.partials = [gridDim.x][P + 3]
template <typename TX, int NT0, int DEPTH, int MODE>
__global__ __launch_bounds__(kBlock) void mlp_f64_kernel(GramArgs a, MlpArgs g) {
  constexpr bool kGrad = MODE == MLP_GRAD;
  constexpr int NL = DEPTH + 1;  // affine layers
  constexpr int kLd0 = 16 * NT0 + 1;
  constexpr int kWave0 = mlp_wave_area(NT0, DEPTH, kGrad);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = lane & 15, q = lane >> 4;
  double* xs = reinterpret_cast<double*>(smem) + wave * kWave0;   // [16 NT0][kLd]
  [[maybe_unused]] double* abuf = xs + 16 * NT0 * kLd;            // [DEPTH][kHW][kLd]
  [[maybe_unused]] double* dbuf = abuf + DEPTH * kHW * kLd;       // [kHW][kLd]
  double* W0 = reinterpret_cast<double*>(smem) + kWavesPerBlock * kWave0;  // [kHW][kLd0]
  double* Wh = W0 + kHW * kLd0;                                   // [DEPTH][kHW][kLdH]
  double* bs = Wh + DEPTH * kHW * kLdH;                           // [NL][kHW]
  double* red = reinterpret_cast<double*>(smem);                  // block reduction: aliases all of it

  const int d = a.d;
  int poff[NL + 1];  // where each layer starts in the weight vector; poff[NL] = P
  poff[0] = 0;
#pragma unroll
  for (int l = 0; l < NL; ++l) poff[l + 1] = poff[l] + (g.width[l] + 1) * g.width[l + 1];
  const int OT1 = (g.width[1] + 15) >> 4;
  [[maybe_unused]] const int OT2 = (g.width[2] + 15) >> 4;
  [[maybe_unused]] const int OT3 = DEPTH == 2 ? (g.width[3] + 15) >> 4 : 0;

  // the weights, zero padded; pad classes get the bias -inf (a bias, not a mask)
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int I = g.width[l], O = g.width[l + 1];
    const int ldw = l == 0 ? kLd0 : kLdH;
    double* W = l == 0 ? W0 : Wh + (l - 1) * kHW * kLdH;
    for (int i = threadIdx.x; i < kHW * ldw; i += kBlock) {
      const int o = i / ldw, j = i % ldw;
      W[i] = (o < O && j < I) ? g.w[poff[l] + j * O + o] : 0.0;
    }
    for (int o = threadIdx.x; o < kHW; o += kBlock)
      bs[l * kHW + o] = o < O ? g.w[poff[l] + I * O + o] : (l == NL - 1 ? -HUGE_VAL : 0.0);
  }
  __syncthreads();

  f64x4 G0[kGrad ? kHT : 1][kGrad ? NT0 : 1];
  f64x4 Gh[kGrad ? DEPTH : 1][kHT][kHT];
  f64x4 gb[kGrad ? NL : 1][kHT];
  if constexpr (kGrad) {
#pragma unroll
    for (int u = 0; u < kHT; ++u) {
#pragma unroll
      for (int t = 0; t < NT0; ++t) G0[u][t] = f64x4{};
#pragma unroll
      for (int l = 0; l < DEPTH; ++l)
#pragma unroll
        for (int v = 0; v < kHT; ++v) Gh[l][u][v] = f64x4{};
#pragma unroll
      for (int l = 0; l < NL; ++l) gb[l][u] = f64x4{};
    }
  }
  double loss_acc = 0.0, live_acc = 0.0, bad_acc = 0.0;

  const TX* X = reinterpret_cast<const TX*>(a.X);
  const int64_t nfull = a.n / 64;  // supersteps below are whole; superstep nfull is the n % 64 tail
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  int64_t s0 = gw * a.spw;
  int64_t s1 = s0 + a.spw;
  if (s0 > a.nsuper) s0 = a.nsuper;
  if (s1 > a.nsuper) s1 = a.nsuper;

  for (int64_t s = s0; s < s1; ++s) {
    const int64_t r0 = s * 64;
    const int64_t r = r0 + lane;
    const bool live = r < a.n && (a.sel ? a.sel[r] != 0 : true);
    int yl = -1;  // the row's class, -1 unless the row counts
    if constexpr (kGrad) {
      bool bad = false;
      if (live) {
        const double y = load_f32_f64(a.y, a.ydt, r);
        if (y >= 0.0 && y < (double)g.width[NL] && y == floor(y)) yl = (int)y;  // (NaN fails the first compare)
        else bad = true;
      }
      live_acc += live ? 1.0 : 0.0;
      bad_acc += bad ? 1.0 : 0.0;
    }
    const unsigned long long okm = __ballot(kGrad ? yl >= 0 : live);  // bit = row of the superstep: it counts

#pragma unroll 1
    for (int rt = 0; rt < 4; ++rt) {
      const int64_t row0 = r0 + 16 * rt;
      if (row0 >= a.n) break;
      const unsigned ok = (unsigned)(okm >> (16 * rt)) & 0xffffu;
      __builtin_amdgcn_wave_barrier();
      mlp_stage<TX, NT0>(X, a.ld, d, row0, a.n, s < nfull, ok, lane, xs);
      __builtin_amdgcn_wave_barrier();

      // ---- forward: lane (f, q) holds row row0 + f of units 16 ut + 4 reg + q
      f64x4 a1[kHT], z[kHT];
      [[maybe_unused]] f64x4 a2[kHT];
      mlp_bias(bs, q, a1);
      // (a real loop over the k-steps: unrolled, the compiler hoists the loop-invariant weight
      // operands out of the superstep loop)
#pragma unroll 1
      for (int ks = 0; ks < 4 * NT0; ++ks) {
        const double bv = xs[(4 * ks + q) * kLd + f];
#pragma unroll
        for (int ut = 0; ut < kHT; ++ut)
          if (ut < OT1)
            a1[ut] = __builtin_amdgcn_mfma_f64_16x16x4f64(W0[(16 * ut + f) * kLd0 + 4 * ks + q], bv, a1[ut], 0, 0, 0);
      }
      mlp_activate<kGrad>(a1, f, q, abuf);
      if constexpr (DEPTH == 2) {
        mlp_bias(bs + kHW, q, a2);
        mlp_forward(Wh, a1, OT1, OT2, f, q, a2);
        mlp_activate<kGrad>(a2, f, q, abuf + kHW * kLd);
        mlp_bias(bs + 2 * kHW, q, z);
        mlp_forward(Wh + kHW * kLdH, a2, OT2, OT3, f, q, z);
      } else {
        mlp_bias(bs + kHW, q, z);
        mlp_forward(Wh, a1, OT1, OT2, f, q, z);
      }

      if constexpr (!kGrad) {
        // the first maximum: in-lane in index order, then over q (ties: the smaller index)
        double best = -HUGE_VAL;
        int bidx = 0;
#pragma unroll
        for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            if (z[ut][reg] > best) {
              best = z[ut][reg];
              bidx = 16 * ut + 4 * reg + q;
            }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const double ob = __shfl_xor(best, o, 64);
          const int oi = __shfl_xor(bidx, o, 64);
          if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
          }
        }
        if (q == 0 && row0 + f < a.n) g.pred[row0 + f] = (ok >> f) & 1u ? (double)bidx : -1.0;
      } else {
        // ---- softmax + loss of row f over the lane's classes and the four q lanes
        const int yrow = __shfl(yl, 16 * rt + f, 64);
        const bool on = yrow >= 0;
        double mx = z[0][0];
#pragma unroll
        for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) mx = fmax(mx, z[ut][reg]);
        mx = fmax(mx, __shfl_xor(mx, 16, 64));
        mx = fmax(mx, __shfl_xor(mx, 32, 64));
        f64x4 e[kHT];
        double sm = 0.0;
#pragma unroll
        for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            e[ut][reg] = exp(z[ut][reg] - mx);
            sm += e[ut][reg];
          }
        sm += __shfl_xor(sm, 16, 64);
        sm += __shfl_xor(sm, 32, 64);
        const double inv = 1.0 / sm, lse = mx + log(sm);
#pragma unroll
        for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const bool mine = yrow == 16 * ut + 4 * reg + q;
            if (mine) loss_acc += lse - z[ut][reg];
            z[ut][reg] = on ? e[ut][reg] * inv - (mine ? 1.0 : 0.0) : 0.0;  // the delta of the top layer
          }

        // ---- backward: weight gradient of the layer, then the delta of the layer below
        if constexpr (DEPTH == 2) {
          mlp_dw<kHT>(z, gb[2], dbuf, abuf + kHW * kLd, OT2, OT3, f, q, Gh[1]);
          mlp_backward(Wh + kHW * kLdH, a2, OT2, OT3, f, q, z);
          mlp_dw<kHT>(z, gb[1], dbuf, abuf, OT1, OT2, f, q, Gh[0]);
          mlp_backward(Wh, a1, OT1, OT2, f, q, z);
        } else {
          mlp_dw<kHT>(z, gb[1], dbuf, abuf, OT1, OT2, f, q, Gh[0]);
          mlp_backward(Wh, a1, OT1, OT2, f, q, z);
        }
        mlp_dw<NT0>(z, gb[0], dbuf, xs, NT0, OT1, f, q, G0);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (kGrad) {
    // block reduction over the waves in order + slab store
    const int P = poff[NL];
    __syncthreads();
    for (int i = threadIdx.x; i < P + 3; i += kBlock) red[i] = 0.0;
    loss_acc = wave_sum_f64(loss_acc);
    live_acc = wave_sum_f64(live_acc);
    bad_acc = wave_sum_f64(bad_acc);
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int ut = 0; ut < kHT; ++ut)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int o = 1; o <= 8; o <<= 1) gb[l][ut][reg] += __shfl_xor(gb[l][ut][reg], o, 64);
    __syncthreads();
    for (int wvi = 0; wvi < kWavesPerBlock; ++wvi) {
      if (wave == wvi) {
        if (lane == 0) {
          red[P] += loss_acc;
          red[P + 1] += live_acc;
          red[P + 2] += bad_acc;
        }
        mlp_fold<NT0>(red, g.width[0], g.width[1], G0, gb[0], f, q);
#pragma unroll
        for (int l = 1; l < NL; ++l) mlp_fold<kHT>(red + poff[l], g.width[l], g.width[l + 1], Gh[l - 1], gb[l], f, q);
      }
      __syncthreads();
    }
    double* out = a.partials + (int64_t)blockIdx.x * (P + 3);
    for (int i = threadIdx.x; i < P + 3; i += kBlock) out[i] = red[i];
  }
}

template <typename TX, int NT0, int DEPTH, typename F>
void with_mlp_mode(int mode, F&& f) {
  return mode == MLP_GRAD ? f(mlp_f64_kernel<TX, NT0, DEPTH, MLP_GRAD>, mlp_lds_bytes(NT0, DEPTH, true))
                          : f(mlp_f64_kernel<TX, NT0, DEPTH, MLP_PREDICT>, mlp_lds_bytes(NT0, DEPTH, false));
}

template <typename TX, int NT0, typename F>
void with_mlp_depth(int depth, int mode, F&& f) {
  return depth == 1 ? with_mlp_mode<TX, NT0, 1>(mode, f) : with_mlp_mode<TX, NT0, 2>(mode, f);
}

template <typename TX, typename F>
void with_mlp_nt(int NT0, int depth, int mode, F&& f) {
  switch (NT0) {
    case 1: return with_mlp_depth<TX, 1>(depth, mode, f);
    case 2: return with_mlp_depth<TX, 2>(depth, mode, f);
    case 3: return with_mlp_depth<TX, 3>(depth, mode, f);
    default: return with_mlp_depth<TX, 4>(depth, mode, f);
  }
}

// f(kernel, its dynamic LDS bytes)
template <typename F>
void with_mlp_kernel(int xdt, const int* layers, int nlayers, int mode, F&& f) {
  if (layers == nullptr || nlayers < kMlpMinLayers || nlayers > kMlpMaxLayers)
    throw std::invalid_argument("mlp: layers must have 3 or 4 entries (one or two hidden layers)");
  if (layers[0] < 1 || layers[0] > kMlpMaxD) throw std::invalid_argument("mlp: the input width must be in [1, 64]");
  for (int l = 1; l < nlayers; ++l)
    if (layers[l] < (l == nlayers - 1 ? 2 : 1) || layers[l] > kMlpMaxWidth)
      throw std::invalid_argument("mlp: hidden widths must be in [1, 32] and the classes in [2, 32]");
  if (mode != MLP_GRAD && mode != MLP_PREDICT) throw std::invalid_argument("mlp: mode must be GRAD (0) or PREDICT (1)");
  const int NT0 = (layers[0] + 15) / 16, depth = nlayers - 2;
  if (xdt == DT_F64) return with_mlp_nt<double>(NT0, depth, mode, f);
  if (xdt == DT_F32) return with_mlp_nt<float>(NT0, depth, mode, f);
  throw std::invalid_argument("mlp: features must be f32 or f64");
}

// the kernel may use more dynamic LDS than the default limit of a launch
template <typename Kern>
size_t mlp_lds(Kern kern, size_t lds) {
  DQ_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return lds;
}

}  // namespace

int mlp_blocks(const int* layers, int nlayers, int64_t n, int xdt, int mode) {
  int nb = 1;
  with_mlp_kernel(xdt, layers, nlayers, mode,
                  [&](auto kern, size_t lds) { nb = staged_f64_blocks(kern, mlp_lds(kern, lds), n); });
  return nb;
}

void mlp_pass(GramArgs a, const double* weights, const int* layers, int nlayers, int mode, double* pred, int blocks,
              hipStream_t st) {
  if (mode == MLP_PREDICT) a.ydt = DT_F64;  // (no label: the shared plan checks the code only)
  staged_f64_plan(a, blocks, "mlp");
  if (a.X == nullptr || weights == nullptr) throw std::invalid_argument("mlp: null operand");
  if (mode == MLP_GRAD && (a.partials == nullptr || a.y == nullptr))
    throw std::invalid_argument("mlp: a GRAD pass needs partials and the label");
  if (mode == MLP_PREDICT && pred == nullptr) throw std::invalid_argument("mlp: a PREDICT pass needs pred");
  with_mlp_kernel(a.xdt, layers, nlayers, mode, [&](auto kern, size_t lds) {
    if (layers[0] != a.d) throw std::invalid_argument("mlp: the feature width must equal layers[0]");
    MlpArgs g{weights, pred, {0, 0, 0, 0}};
    for (int l = 0; l < nlayers; ++l) g.width[l] = layers[l];
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), mlp_lds(kern, lds), st, a, g);
  });
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
