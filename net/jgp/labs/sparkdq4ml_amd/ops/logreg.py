"""Logistic regression (Spark 2.4 ``ml.classification.LogisticRegression``): the loss / gradient
pass, its routes and the fit.

One evaluation takes coefficients ``coef`` ``[K, d + 1]`` (class-major, the intercept in column d;
``K = 1`` is the binomial family, whose single row scores class 1) in the ORIGINAL feature space --
the caller has divided by the feature std -- and feature-major ``X[d, n]``.  GRAD gives the flat f64
statistics ``[K (d + 1) gradient, loss, sum w, live rows, bad labels]`` of the weighted log-loss
``-w log p_y`` (multinomial: softmax of the K margins; binomial: ``w (log(1 + e^m) - y m)``);
PREDICT gives ``(raw [C, n], prob [C, n], pred [n])`` as f64, class-major, ``C`` = classes (2 for
binomial: ``raw = [-m, m]``), dead rows NaN / -1.  A live row whose label is no integer in
``[0, C)`` counts as a bad label and adds nothing else; dead rows are selected to zero before any
product, so their features, labels and weights may hold NaN.

Three routes compute a pass:

* the fused device pass (``csrc/hip/logreg.hip`` through ``device.logreg_pass``): dense f32 / f64,
  d <= 64, K <= 64, X read by one kernel per evaluation;
* its fp64 twin :func:`logreg_pass_host`: the CPU engine and the kernel tests' oracle;
* the composite :func:`composite_pass`: torch matmul + ``log_softmax`` + matmul in f64 -- wider d or
  K on the device, and the benchmark's comparator.

:func:`fit` is Spark's ``train``: standardised training space, L2 in the objective and L1 through
OWLQN (``models/qn_device.minimize``), Spark's starting intercepts and post-processing.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

__all__ = ["GRAD", "PREDICT", "FUSED_MAX_D", "FUSED_MAX_K", "stats_size", "logreg_pass_host", "composite_pass",
           "route", "predict", "fit", "LogregResult"]

GRAD, PREDICT = 0, 1  # codes of csrc/hip/logreg.h
FUSED_MAX_D = 64
FUSED_MAX_K = 64


def stats_size(K: int, d: int) -> int:
    return K * (d + 1) + 4


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _coef2(coef, d: int) -> np.ndarray:
    C = np.asarray(_np(coef), dtype=np.float64)
    if C.ndim != 2 or C.shape[1] != d + 1 or C.shape[0] < 1:
        raise ValueError("logreg_pass: coef must be [K, d + 1]")
    return C


def logreg_pass_host(X, y, w, sel, coef, mode: int, threshold: float = 0.5):
    """The fp64 twin of the fused device pass on host data (numpy; torch f64 results)."""
    Xd = _np(X).astype(np.float64)
    d, n = Xd.shape
    C = _coef2(coef, d)
    K = C.shape[0]
    classes = 2 if K == 1 else K
    live = np.ones(n, dtype=bool) if sel is None else _np(sel).astype(bool)
    if live.shape != (n,):
        raise ValueError("logreg_pass: row-count mismatch between features and selection")
    if mode not in (GRAD, PREDICT):
        raise ValueError("logreg_pass: mode must be GRAD (0) or PREDICT (1)")
    with np.errstate(all="ignore"):
        if mode == GRAD:
            yv = _np(y).astype(np.float64)
            ok = live & (yv >= 0) & (yv < classes) & (yv == np.floor(yv))
            wv = np.where(ok, 1.0 if w is None else _np(w).astype(np.float64), 0.0)
            yi = np.where(ok, yv, 0).astype(np.int64)
        else:
            ok = live
        Xz = np.where(ok[None, :], Xd, 0.0)
        M = C[:, :d] @ Xz + C[:, d:]  # [K, n]
        if K == 1:
            eta = M[0]
            t = np.exp(-np.abs(eta))
            hi, lo = 1.0 / (1.0 + t), t / (1.0 + t)
            p = np.where(eta >= 0, hi, lo)
            if mode == PREDICT:
                nan = np.where(live, 0.0, np.nan)
                raw = np.stack([-eta, eta]) + nan
                prob = np.stack([np.where(eta >= 0, lo, hi), p]) + nan
                return (torch.from_numpy(raw), torch.from_numpy(prob),
                        torch.from_numpy(np.where(live, (p > threshold).astype(np.float64), -1.0)))
            mult = (wv * (p - yi))[None, :]
            loss = (wv * (np.maximum(eta, 0.0) + np.log1p(t) - yi * eta)).sum()
        else:
            mx = M.max(axis=0)
            e = np.exp(M - mx)
            sm = e.sum(axis=0)
            p = e / sm
            if mode == PREDICT:
                nan = np.where(live, 0.0, np.nan)
                return (torch.from_numpy(M + nan), torch.from_numpy(p + nan),
                        torch.from_numpy(np.where(live, np.argmax(M, axis=0).astype(np.float64), -1.0)))
            cols = np.arange(n)
            loss = -(wv * (M[yi, cols] - mx - np.log(sm))).sum()
            p[yi, cols] -= 1.0
            mult = wv[None, :] * p
    out = np.empty(stats_size(K, d))
    out[:K * (d + 1)] = np.concatenate([mult @ Xz.T, mult.sum(axis=1)[:, None]], axis=1).reshape(-1)
    out[K * (d + 1):] = loss, wv.sum(), live.sum(), (live & ~ok).sum()
    return torch.from_numpy(out)


def composite_pass(X, y, w, sel, coef, mode: int, threshold: float = 0.5):
    """The same pass from torch ops in f64 (any d and K, host or device): a ``[K, n]`` margin
    matrix, ``log_softmax``, a second matmul."""
    Xd = X.to(torch.float64)
    d, n = Xd.shape
    dev = Xd.device
    C = (coef if torch.is_tensor(coef) else torch.as_tensor(_coef2(coef, d))).to(device=dev, dtype=torch.float64)
    K = C.shape[0]
    classes = 2 if K == 1 else K
    live = torch.ones(n, dtype=torch.bool, device=dev) if sel is None else sel.to(torch.bool)
    if mode == GRAD:
        yv = y.to(torch.float64)
        ok = live & (yv >= 0) & (yv < classes) & (yv == torch.floor(yv))
        wv = torch.where(ok, torch.ones_like(yv) if w is None else w.to(torch.float64), torch.zeros_like(yv))
        yi = torch.where(ok, yv, torch.zeros_like(yv)).to(torch.long)
    else:
        ok = live
    Xz = torch.where(ok[None, :], Xd, torch.zeros_like(Xd))
    M = C[:, :d] @ Xz + C[:, d:]
    raw = torch.cat([-M, M]) if K == 1 else M
    if K == 1:
        M = torch.cat([torch.zeros_like(M), M])  # p = sigmoid(m): the softmax of (0, m)
    lp = torch.log_softmax(M, dim=0)
    if mode == PREDICT:
        nan = torch.where(live, 0.0, float("nan")).to(torch.float64)
        p = lp.exp()
        pred = (p[1] > threshold).to(torch.float64) if K == 1 else torch.argmax(M, dim=0).to(torch.float64)
        return raw + nan, p + nan, torch.where(live, pred, torch.full_like(pred, -1.0))
    cols = torch.arange(n, device=dev)
    loss = -(wv * lp[yi, cols]).sum()
    mult = lp.exp()
    mult[yi, cols] -= 1.0
    mult = (wv[None, :] * mult)[classes - K:]  # (binomial: the row of class 1)
    g = torch.cat([mult @ Xz.t(), mult.sum(dim=1, keepdim=True)], dim=1).reshape(-1)
    tail = torch.stack([loss, wv.sum(), live.sum().to(torch.float64), (live & ~ok).sum().to(torch.float64)])
    return torch.cat([g, tail])


def route(X, K: int) -> str:
    """"fused" (device tensors inside the kernel's range), "composite" (other device tensors) or
    "host" (host tensors: the twin).  ``K``: coefficient rows (1 = binomial).  The fused route is the
    default over its whole range: see profiles/logreg.md for the measurements behind that."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and 1 <= X.shape[0] <= FUSED_MAX_D
          and X.shape[1] >= 1 and 1 <= int(K) <= FUSED_MAX_K)
    return "fused" if ok else "composite"


def _pass(X, y, w, sel, coef, mode: int, how: str, threshold: float = 0.5):
    if how == "composite":
        return composite_pass(X, y, w, sel, coef, mode, threshold)
    if how == "host":
        return logreg_pass_host(X, y, w, sel, coef, mode, threshold)
    from . import device

    return device.logreg_pass(X, y, w, sel, coef, mode, threshold=threshold)


def predict(X, sel, coef, threshold: float = 0.5, how: Optional[str] = None):
    """``(raw, prob, pred)`` on X's device, by the route of (X, K)."""
    return _pass(X, None, None, sel, coef, PREDICT, how or route(X, np.shape(_np(coef))[0]), threshold)


# ---- the fit -----------------------------------------------------------------------------------------
@dataclass
class LogregResult:
    coef: np.ndarray        # [K, d] in the original feature space (K = 1: binomial)
    intercept: np.ndarray   # [K]
    num_classes: int
    objective_history: list
    route: str


def _moments(X, y, w, sel):
    """(feature std [d] with Spark's weighted unbiased variance M2 / (W - sum w^2 / W), class histogram, classes) over the
    ranks: ``gram_stats`` moments and a ``bincount`` of the labels, once per fit."""
    from ..parallel import comm
    from . import kernels

    d, n = int(X.shape[0]), int(X.shape[1])
    live = torch.ones(n, dtype=torch.bool, device=X.device) if sel is None else sel.to(torch.bool)
    yl = y[live].to(torch.float64)
    if yl.numel() and bool(((yl < 0) | (yl != torch.floor(yl)) | torch.isnan(yl)).any()):
        raise ValueError("LogisticRegression: labels must be class indices 0, 1, ... (non-negative integers)")
    wl = None if w is None else w[live].to(torch.float64)
    classes = max(comm.all_gather_object(int(yl.max()) + 1 if yl.numel() else 0))
    hist = torch.bincount(yl.to(torch.long), weights=wl, minlength=classes).to(torch.float64)
    hist = comm.all_reduce_sum(hist).cpu().numpy()
    flat = comm.all_reduce_sum(kernels.gram_stats(X, y, w, sel, "fp64")).cpu().numpy()
    sw, sx = flat[1], flat[5:5 + d]
    diag = np.cumsum(np.arange(1, d + 1)) - 1  # (j, j) of the packed upper triangle, column-major
    sxx = flat[5 + 2 * d:][diag]
    denom = sw - flat[2] / sw  # Spark's MultivariateOnlineSummarizer: W - sum w^2 / W
    var = (sxx - sx * sx / sw) / denom if denom > 0 else np.zeros(d)
    return np.sqrt(np.maximum(var, 0.0)), hist, classes


def fit(X, y, w, sel, family: str = "auto", reg: float = 0.0, alpha: float = 0.0, max_iter: int = 100,
        tol: float = 1e-6, fit_intercept: bool = True, standardization: bool = True, how: str = "auto") -> LogregResult:
    """Fit on feature-major ``X`` ``[d, n]`` with class-index labels ``y``.  ``how``: "auto"
    (:func:`route`) or "fused" / "composite" / "host" to force one (tests, benchmarks)."""
    from ..models.qn_device import minimize
    from ..parallel import comm

    if how not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"logreg fit: unknown route {how!r}")
    if family not in ("auto", "binomial", "multinomial"):
        raise ValueError(f"LogisticRegression: unknown family {family!r}")
    d = int(X.shape[0])
    std, hist, classes = _moments(X, y, w, sel)
    hist = np.pad(hist, (0, max(0, 2 - hist.size)))
    classes = max(classes, 1)
    if hist.sum() <= 0:
        raise ValueError("LogisticRegression: the input has no rows")
    if family == "binomial" and classes > 2:
        raise ValueError(f"LogisticRegression: binomial family supports 1 or 2 outcome classes, found {classes}")
    multi = family == "multinomial" or (family == "auto" and classes > 2)
    K = classes if multi else 1
    if multi and K < 2:
        K = classes = 2  # (Spark trains the multinomial family over at least two classes)
    if how == "auto":
        how = route(X, K)
    if fit_intercept and np.count_nonzero(hist) == 1:  # constant label: Spark's model, no pass
        b = np.zeros(K)
        b[-1] = np.inf if (multi or classes == 2) else -np.inf
        return LogregResult(np.zeros((K, d)), b, classes, [], how)

    dev = X.device
    inv = np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)
    scale = torch.from_numpy(np.concatenate([inv, [1.0 if fit_intercept else 0.0]])).to(dev)  # scaled -> original space
    pen = np.ones(d) if standardization else inv  # Spark: penalise the original-space coefficients
    l2 = torch.from_numpy(np.tile(np.concatenate([reg * (1.0 - alpha) * pen * pen, [0.0]]), K)).to(dev)
    l1 = torch.from_numpy(np.tile(np.concatenate([reg * alpha * pen, [0.0]]), K)).to(dev) if reg * alpha > 0 else None
    x0 = np.zeros((K, d + 1))
    if fit_intercept:
        if multi:
            raw = np.log1p(hist)  # (Spark smooths the starting intercepts by one count)
            x0[:, d] = raw - raw.mean()
        else:
            x0[0, d] = np.log(hist[1] / hist[0])
    plan, first = None, [True]
    if how == "fused":
        from . import device

        plan = device._LogregPlan(X, y, w, sel, K)

    def fg(x):
        coef = (x.view(K, d + 1) * scale).contiguous()
        stats = plan.grad(coef) if plan is not None else _pass(X, y, w, sel, coef, GRAD, how)
        stats = comm.all_reduce_sum(stats.to(dev))
        if first[0]:
            first[0] = False
            if float(stats[-1]) != 0.0:
                raise ValueError(f"LogisticRegression: {int(stats[-1])} labels are no class index in [0, {classes})")
        sw = stats[K * (d + 1) + 1]
        g = (stats[:K * (d + 1)].view(K, d + 1) * scale).reshape(-1) / sw + l2 * x
        return stats[K * (d + 1)] / sw + 0.5 * torch.sum(l2 * x * x), g

    x, hist_f, _ = minimize(fg, torch.from_numpy(x0.reshape(-1)).to(dev), int(max_iter), float(tol), l1=l1)
    B = (x.view(K, d + 1) * scale).cpu().numpy()
    coef, icpt = B[:, :d].copy(), B[:, d].copy()
    if multi:
        if reg == 0.0:
            coef -= coef.mean(axis=0, keepdims=True)
        if fit_intercept:
            icpt -= icpt.mean()
    return LogregResult(coef, icpt, classes, [float(v) for v in hist_f], how)
