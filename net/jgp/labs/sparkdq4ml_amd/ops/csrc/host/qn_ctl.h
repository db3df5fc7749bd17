// The Breeze 0.13 quasi-Newton control rules (the optimizer library bundled with Spark 2.4.4), in
// ONE place: the convergence tests, the OWLQN backtracking search, the strong-Wolfe bracket / zoom
// search, the "first failed search resets the history, the second ends the fit" rule, the OWLQN
// pseudo-gradient and orthant projection, and the WeightedLeastSquares standardization of the
// flat statistics.  The four device solvers (wls_small.hip wls_qn_kernel, wls_qn_grid.hip,
// lsq_qn.hip, huber_qn.hip) and the host driver quasi_newton_ctl (solvers.cpp) take every
// decision from here; quasi_newton (solvers.cpp) and models/qn_device.py are written
// independently and are what the tests compare against.
//
// Scalar code only: no thread index, no reduction, no memory but the state structs.  Every
// function compiles for the host (g++) and, under hipcc, for the device; it inherits the
// floating-point contraction setting of the file that includes it, so expressions are written in
// one fixed operand order and must stay that way.  Loops over FvWindow use static indices
// (unrolled, guarded): a kernel that keeps the window in registers gets no scratch.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define DQ_QN_FN __host__ __device__ __forceinline__
#define DQ_QN_UNROLL _Pragma("unroll")
#else
#define DQ_QN_FN inline
#define DQ_QN_UNROLL
#endif

namespace dq4ml {
namespace qn {

constexpr int kFvals = 20;  // FunctionValuesConverged window

// convergence reasons (converged()); -1: go on
enum { kMaxIterations = 0, kFunctionValuesConverged = 1, kGradientConverged = 2, kSearchFailed = 3 };
// what a line search asks for next
enum Step { kEval = 0, kAccept = 1, kFail = 2 };

// ---- FunctionValuesConverged: the last 20 objective values (starts as [+inf]) ----------------
struct FvWindow {
  double fv[kFvals];
  int n;
  DQ_QN_FN void init() {
DQ_QN_UNROLL
    for (int i = 0; i < kFvals; ++i) fv[i] = 0.0;
    fv[kFvals - 1] = __builtin_inf();
    n = 1;
  }
  DQ_QN_FN void push(double v) {
DQ_QN_UNROLL
    for (int i = 0; i < kFvals - 1; ++i) fv[i] = fv[i + 1];
    fv[kFvals - 1] = v;
    n = n < kFvals ? n + 1 : kFvals;
  }
  DQ_QN_FN double max() const {  // a window in registers
    double mx = -__builtin_inf();
DQ_QN_UNROLL
    for (int i = 0; i < kFvals; ++i)
      if (i >= kFvals - n) mx = fmax(mx, fv[i]);
    return mx;
  }
  DQ_QN_FN double max_indexed() const {  // a window in memory: the same fold, one value live at a time
    double mx = -__builtin_inf();
    for (int i = kFvals - n; i < kFvals; ++i) mx = fmax(mx, fv[i]);
    return mx;
  }
};

DQ_QN_FN bool iterations_done(int max_iter, int iter) { return max_iter >= 0 && iter >= max_iter; }
// (wn, wmax): FvWindow's n and max
DQ_QN_FN bool values_converged(int wn, double wmax, double adj, double init_adj, double tol) {
  return wn >= 2 && fabs(adj - wmax) <= tol * fabs(init_adj);
}
DQ_QN_FN bool gradient_converged(double gnorm, double value, double tol) {
  return gnorm <= fmax(tol * fabs(value), 1e-8);
}

// -1, or why the fit ends (adj / init_adj: the regularized objective, value: the smooth part)
DQ_QN_FN int converged(int max_iter, int iter, int wn, double wmax, double adj, double init_adj, double value,
                       double gnorm, double tol, bool search_failed) {
  if (iterations_done(max_iter, iter)) return kMaxIterations;
  if (values_converged(wn, wmax, adj, init_adj, tol)) return kFunctionValuesConverged;
  if (gradient_converged(gnorm, value, tol)) return kGradientConverged;
  if (search_failed) return kSearchFailed;
  return -1;
}

// A FirstOrderException: the first one in a row resets the caller's history (returns true), the
// second ends the fit.  An accepted step clears failed_once.
template <class F>
DQ_QN_FN bool note_failure(F& failed_once, F& search_failed) {
  if (!failed_once) {
    failed_once = 1;
    return true;
  }
  search_failed = 1;
  return false;
}

// The objective history takes one value per loop pass: the slot to store it in, or -1 with the
// overflow flag set once the capacity is used up.
template <class F>
DQ_QN_FN int record(int& H, int hist_cap, F& overflow) {
  if (H >= hist_cap) {
    overflow = 1;
    return -1;
  }
  return H++;
}

// ---- Breeze BacktrackingLineSearch as OWLQN configures it -------------------------------------
struct Backtrack {
  double alpha, initfval, initd, shrink;
  int it, force;
  // gnorm: |g| of the state (seeds the first iteration's step)
  DQ_QN_FN void start(int iter, double adj, double initd_, double gnorm) {
    initfval = adj;
    initd = initd_;
    shrink = iter < 1 ? 0.1 : 0.5;
    alpha = iter < 1 ? 0.5 / gnorm : 1.0;
    it = 0, force = 0;
  }
  // (f, fd): the adjusted value and directional derivative at alpha
  DQ_QN_FN Step next(double f, double fd) {
    const double c1 = 1e-4, c2 = 0.9;
    if (force) return kAccept;
    double mult;
    if (f > initfval + alpha * initd * c1) mult = shrink;
    else if (fd < c2 * initd) mult = 2.1;
    else if (fd > -c2 * initd) mult = shrink;
    else mult = 1.0;
    if (mult == 1.0) return kAccept;
    const double na = alpha * mult;
    if (it >= 20 || na < 1e-10 || na > 1e10) return kFail;
    alpha = na;
    if (it + 1 >= 20) force = 1;  // takeWhile(iter < maxIterations) keeps the last state
    else ++it;
    return kEval;
  }
};

// ---- Breeze StrongWolfeLineSearch: bracketing, then zoom by cubic interpolation ---------------
DQ_QN_FN bool non_descent(double d0) { return d0 > 0.0; }  // "invoked with non-descent direction"
// LBFGS.determineStepSize's first trial
DQ_QN_FN double lbfgs_first_step(int iter, double dnorm) { return iter == 0 ? 1.0 / dnorm : 1.0; }

struct Wolfe {
  double alpha, f0, d0, lo_t, lo_d, lo_f, hi_t, hi_d, hi_f;
  int zooming, bi, zi;
  // false: a FirstOrderException (no trial to evaluate)
  DQ_QN_FN bool start(double value, double d0_, double t0) {
    zooming = 0, bi = 0, zi = 0;
    f0 = value, d0 = d0_;
    if (non_descent(d0_)) return false;
    alpha = t0;
    lo_t = 0.0, lo_d = d0_, lo_f = value;
    return true;
  }
  static DQ_QN_FN double interp(double at, double ad, double af, double bt, double bd, double bf) {
    const double d1 = ad + bd - 3.0 * (af - bf) / (at - bt);
    const double d2 = sqrt(d1 * d1 - ad * bd);
    const double mul = bt - at;
    const double x = bt - mul * (bd + d2 - d1) / (bd - ad + 2.0 * d2);
    const double lb = at + 0.1 * mul, ub = at + 0.9 * mul;
    return x < lb ? lb : (x > ub ? ub : x);
  }
  DQ_QN_FN Step zoom_trial() {  // interp(hi, lo) if lo.t > hi.t
    alpha = lo_t > hi_t ? interp(hi_t, hi_d, hi_f, lo_t, lo_d, lo_f) : interp(lo_t, lo_d, lo_f, hi_t, hi_d, hi_f);
    return kEval;
  }
  // (f, dd): the value and directional derivative at alpha; the caps bound the bracket / zoom steps
  DQ_QN_FN Step next(double f, double dd, int bracket_cap, int zoom_cap) {
    const double c1 = 1e-4, c2 = 0.9, tt = alpha;
    if (!zooming) {
      if (!(f - f == 0.0)) {  // not finite: halve and retry
        alpha = tt / 2.0;
      } else if (f > f0 + c1 * tt * d0 || (f >= lo_f && bi > 0)) {
        hi_t = tt, hi_d = dd, hi_f = f;
        zooming = 1, zi = 0;
        return zoom_trial();
      } else if (fabs(dd) <= c2 * fabs(d0)) {
        return kAccept;
      } else if (dd >= 0.0) {
        hi_t = lo_t, hi_d = lo_d, hi_f = lo_f;
        lo_t = tt, lo_d = dd, lo_f = f;
        zooming = 1, zi = 0;
        return zoom_trial();
      } else {
        lo_t = tt, lo_d = dd, lo_f = f;
        alpha = tt * 1.5;
      }
      return ++bi >= bracket_cap ? kFail : kEval;  // "Line search failed"
    }
    if (f > f0 + c1 * tt * d0 || f >= lo_f) {
      hi_t = tt, hi_d = dd, hi_f = f;
    } else {
      if (fabs(dd) <= c2 * fabs(d0)) return kAccept;
      if (dd * (hi_t - lo_t) >= 0.0) hi_t = lo_t, hi_d = lo_d, hi_f = lo_f;
      lo_t = tt, lo_d = dd, lo_f = f;
    }
    if (++zi >= zoom_cap) return kFail;  // "Line search zoom failed"
    return zoom_trial();
  }
};

// ---- OWLQN, per element ------------------------------------------------------------------------
DQ_QN_FN double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// the pseudo-gradient of f + l1 |x| (l1 == 0: the gradient)
DQ_QN_FN double pseudo_gradient(double x, double g, double l1) {
  if (l1 == 0.0) return g;
  if (x == 0.0) {
    const double dp = g + l1, dm = g - l1;
    return dm > 0.0 ? dm : (dp < 0.0 ? dp : 0.0);
  }
  return g + sgn(x) * l1;
}

// a direction element that does not descend along the pseudo-gradient is dropped
DQ_QN_FN double orthant_direction(double d, double ag) { return d * ag < 0.0 ? d : 0.0; }

// the step nx from x stays in x's orthant (at x == 0: the one the pseudo-gradient points away from)
DQ_QN_FN double orthant_project(double x, double nx, double ag) {
  const double orth = x != 0.0 ? sgn(x) : sgn(-ag);
  return sgn(nx) != orth ? 0.0 : nx;
}

// ---- WeightedLeastSquares from the flat statistics: the standardized system ------------------
struct WlsHead {
  int status;  // 0 ok | 1, 2, 3 label / weight short-circuits (the host owns them) | 9 no L1 term
  double bStd, bBar, bbBar, eff_l1, eff_l2;
};

DQ_QN_FN WlsHead wls_head(double count, double wSum, double bSum, double bbSum, double reg, double enet) {
  WlsHead h = {};
  const double rawBBar = wSum > 0.0 ? bSum / wSum : 0.0;
  const double rawBStd = wSum > 0.0 ? sqrt(fmax(bbSum / wSum - rawBBar * rawBBar, 0.0)) : 0.0;
  if (wSum <= 0.0 || rawBStd == 0.0) {
    h.status = wSum <= 0.0 ? (count > 0 ? 1 : 2) : 3;
    return h;
  }
  h.bStd = rawBStd, h.bBar = rawBBar / h.bStd, h.bbBar = bbSum / wSum / (h.bStd * h.bStd);
  const double eff_reg = reg / h.bStd;
  h.eff_l1 = enet * eff_reg, h.eff_l2 = (1.0 - enet) * eff_reg;
  h.status = h.eff_l1 == 0.0 ? 9 : 0;
  return h;
}

// feature i: population std and standardized mean (aSum_i = Σ w x_i, aa_ii = Σ w x_i²)
DQ_QN_FN void wls_feature(double aSum_i, double aa_ii, double wSum, double& sd, double& bar) {
  const double m = aSum_i / wSum;
  sd = sqrt(fmax(aa_ii / wSum - m * m, 0.0));
  bar = sd == 0.0 ? 0.0 : m / sd;
}
DQ_QN_FN double wls_ab(double abSum_i, double wSum, double sd, double bStd) {
  return sd == 0.0 ? 0.0 : abSum_i / wSum / (sd * bStd);
}
DQ_QN_FN double wls_l1(const WlsHead& h, double sd, bool std_f) {
  return std_f ? h.eff_l1 : (sd != 0.0 ? h.eff_l1 / sd : 0.0);
}
// A(r, j) over the features (aa_rj = Σ w x_r x_j); the diagonal carries the L2 term
DQ_QN_FN double wls_a(const WlsHead& h, double aa_rj, double wSum, double sd_r, double sd_j, bool diagonal,
                      bool std_f, bool std_l) {
  const double den = sd_r * sd_j;
  double v = den == 0.0 ? 0.0 : aa_rj / wSum / den;
  if (diagonal) {
    double lam = h.eff_l2;
    if (!std_f) lam = sd_j != 0.0 ? lam / (sd_j * sd_j) : 0.0;
    if (!std_l) lam *= h.bStd;
    v += lam;
  }
  return v;
}

}  // namespace qn
}  // namespace dq4ml
