"""Gaussian mixtures (Spark 2.4 ``ml.clustering.GaussianMixture``): the EM pass, the start and the loop.

A Gaussian ``(mu, Sigma)`` is evaluated as Spark's ``MultivariateGaussian`` does
(:func:`gaussian_params`, the only statement of that rule): ``Sigma = U diag(lambda) U^T``,
``tol = EPS max(lambda) d``, ``logdet`` and the pseudo-inverse root ``W = diag(lambda^-1/2) U^T`` over
the eigenvalues above ``tol``, ``logpdf(x) = u - 0.5 |W (x - mu)|^2`` with
``u = -0.5 (d log 2 pi + logdet)``.

One E-step over the live rows of feature-major ``X[d, n]``: ``p_j = EPS + w_j exp(logpdf_j(x))``,
``P = sum_j p_j`` in component order, ``r_j = p_j / P``.  This is Spark's form on purpose: no
log-sum-exp, and the second moment is raw, not centred.  The statistics of a pass are the flat f64
``[k sw, k d sm (component-major), k d (d + 1) / 2 S (packed upper), loglik, live rows]`` with
``sw_j = sum r_j``, ``sm_j = sum r_j x``, ``S_j = sum r_j x x^T``, ``loglik = sum log P``.  The
M-step (:func:`m_step_host`) runs on the host in every route.

Three routes compute a pass:

* the fused device pass (``csrc/hip/gmm.hip`` through ``device.gmm_fit``): dense f32 / f64,
  d <= 32, 2 <= k <= 16 and k <= 8 beyond d = 16, X read by one kernel per iteration;
* its fp64 twin :func:`em_pass_host`: the CPU engine and the kernel tests' oracle;
* the composite :func:`composite_pass`: torch f64 ops over ``[k, n]`` densities -- wider d or k on
  the device, and the benchmark's comparator.

The start follows Spark's shape (uniform weights; each Gaussian from 5 sampled rows: their mean and
the diagonal of their population variances) on the project's own seeded rule: the ``5 k`` rows are
the live rows with the smallest (row hash, row) keys of ``ops/kmeans.py``.  Spark samples with
replacement through its own generator, so the start agrees with Spark's in distribution, not bit
for bit; from equal starts the iterations follow Spark 2.4.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

__all__ = ["STEP", "ASSIGN", "FUSED_MAX_D", "FUSED_MAX_K", "EPS", "stats_size", "fused_range", "gaussian_params",
           "params_buffer", "em_pass_host", "composite_pass", "m_step_host", "route", "seed_gaussians", "em", "fit",
           "assign", "GmmResult"]

STEP, ASSIGN = 0, 1  # codes of csrc/hip/gmm.h
FUSED_MAX_D = 32
FUSED_MAX_K = 16
EPS = 2.0 ** -52  # Spark's Utils.EPSILON
_SAMPLES = 5      # rows per starting Gaussian


def stats_size(k: int, d: int) -> int:
    return k + k * d + k * (d * (d + 1) // 2) + 2


def fused_range(d: int, k: int) -> bool:
    """The (d, k) the fused pass serves: k W matrices of dp x dp doubles, dp = 16 ceil(d / 16), in
    64 KiB of LDS."""
    dp = 16 * ((int(d) + 15) // 16)
    return 1 <= d <= FUSED_MAX_D and 2 <= k <= FUSED_MAX_K and k * dp * dp <= 8192


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def gaussian_params(mean, cov):
    """``(W [d, d], u)`` of a Gaussian by the eigen rule above."""
    mu = np.asarray(mean, dtype=np.float64).reshape(-1)
    d = mu.size
    lam, U = np.linalg.eigh(np.asarray(cov, dtype=np.float64).reshape(d, d))
    tol = EPS * lam.max() * d
    keep = lam > tol
    if not keep.any():
        raise ValueError("GaussianMixture: a covariance matrix has no non-zero singular values")
    root = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
    return root[:, None] * U.T, -0.5 * (d * np.log(2.0 * np.pi) + np.log(lam[keep]).sum())


def _check_params(weights, means, covs, d: int):
    w = np.asarray(_np(weights), dtype=np.float64).reshape(-1)
    mu, cov = np.asarray(_np(means), dtype=np.float64), np.asarray(_np(covs), dtype=np.float64)
    k = w.size
    if mu.shape != (k, d) or cov.shape != (k, d, d):
        raise ValueError("gmm_pass: the parameters must be weights [k], means [k, d] and covs [k, d, d]")
    return w, mu, cov


def params_buffer(weights, means, covs) -> np.ndarray:
    """The device parameter buffer of csrc/hip/gmm.h: ``[k dp dp W, k dp c = W mu, k w, k u]``."""
    mu = np.asarray(means, dtype=np.float64)
    k, d = mu.shape
    dp = 16 * ((d + 15) // 16)
    W, c, u = np.zeros((k, dp, dp)), np.zeros((k, dp)), np.zeros(k)
    for j in range(k):
        W[j, :d, :d], u[j] = gaussian_params(mu[j], covs[j])
        c[j, :d] = W[j, :d, :d] @ mu[j]
    return np.concatenate([W.reshape(-1), c.reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1), u])


def _host_rows(X, sel):
    Xd = _np(X).astype(np.float64)
    n = Xd.shape[1]
    live = np.ones(n, dtype=bool) if sel is None else _np(sel).astype(bool)
    if live.shape != (n,):
        raise ValueError("gmm_pass: row-count mismatch between features and selection")
    return np.where(live[None, :], Xd, 0.0), live


def em_pass_host(X, sel, weights, means, covs, mode: int):
    """The fp64 twin of the fused device pass on host data.  STEP: the flat statistics (torch f64);
    ASSIGN: ``(int32 arg-max component, first maximum, -1 for dead rows; probabilities [k, n]; log P
    [n])``, the last two 0 for dead rows.  Dead rows are selected to zero before any product, so
    their features may hold NaN."""
    Xz, live = _host_rows(X, sel)
    d, n = Xz.shape
    w, mu, cov = _check_params(weights, means, covs, d)
    k = w.size
    p = np.empty((k, n))
    for j in range(k):
        W, u = gaussian_params(mu[j], cov[j])
        z = W @ (Xz - mu[j][:, None])
        p[j] = EPS + w[j] * np.exp(u - 0.5 * np.einsum("dn,dn->n", z, z))
    P = np.zeros(n)
    for j in range(k):  # component order
        P += p[j]
    r = np.where(live[None, :], p / P, 0.0)
    logp = np.where(live, np.log(P), 0.0)
    if mode == ASSIGN:
        idx = np.where(live, np.argmax(p, axis=0), -1).astype(np.int32)  # the first maximum
        return torch.from_numpy(idx), torch.from_numpy(r), torch.from_numpy(logp)
    if mode != STEP:
        raise ValueError("gmm_pass: mode must be STEP (0) or ASSIGN (1)")
    iu = np.triu_indices(d)
    S = np.einsum("kn,an,bn->kab", r, Xz, Xz)
    out = np.concatenate([r.sum(axis=1), (r @ Xz.T).reshape(-1), S[:, iu[0], iu[1]].reshape(-1),
                          [logp.sum(), float(live.sum())]])
    return torch.from_numpy(out)


def composite_pass(X, sel, weights, means, covs, mode: int):
    """The same pass from torch ops in f64 (any d and k, host or device): ``[k, n]`` densities, then one
    weighted Gram per component.  X is read k + 2 times."""
    Xd = X.to(torch.float64)
    d, n = Xd.shape
    w, mu, cov = _check_params(weights, means, covs, d)
    k, dev = w.size, Xd.device
    live = torch.ones(n, dtype=torch.bool, device=dev) if sel is None else sel.to(torch.bool)
    Xz = torch.where(live[None, :], Xd, torch.zeros_like(Xd))
    p = torch.empty(k, n, dtype=torch.float64, device=dev)
    for j in range(k):
        W, u = gaussian_params(mu[j], cov[j])
        z = torch.as_tensor(W, device=dev) @ (Xz - torch.as_tensor(mu[j], device=dev)[:, None])
        p[j] = EPS + w[j] * torch.exp(u - 0.5 * (z * z).sum(dim=0))
    P = p.sum(dim=0)
    r = torch.where(live[None, :], p / P, torch.zeros_like(p))
    logp = torch.where(live, torch.log(P), torch.zeros_like(P))
    if mode == ASSIGN:
        best = p.max(dim=0).values  # (torch's argmax may return any of several equal maxima: take the first)
        idx = torch.where(p == best[None, :], torch.arange(k, device=dev)[:, None], k).min(dim=0).values
        return torch.where(live, idx, torch.full_like(idx, -1)).to(torch.int32), r, logp
    iu = torch.triu_indices(d, d, device=dev)
    S = torch.stack([((Xz * r[j][None, :]) @ Xz.t())[iu[0], iu[1]] for j in range(k)])
    return torch.cat([r.sum(dim=1), (r @ Xz.t()).reshape(-1), S.reshape(-1), logp.sum()[None],
                      live.sum().to(torch.float64)[None]])


def m_step_host(stats, k: int, d: int):
    """``(weights [k], means [k, d], covs [k, d, d])`` from reduced statistics, as Spark's
    ``updateWeightsAndGaussians``: ``mu = sm / sw``, ``Sigma = S / sw - mu mu^T``, ``w = sw / sum sw``."""
    s = _np(stats)
    sw, sm = s[:k], s[k:k + k * d].reshape(k, d)
    iu = np.triu_indices(d)
    tri = iu[0].size
    mu = sm / sw[:, None]
    cov = np.empty((k, d, d))
    for j in range(k):
        S = np.zeros((d, d))
        S[iu] = s[k + k * d + j * tri:k + k * d + (j + 1) * tri]
        S = S + np.triu(S, 1).T
        cov[j] = S / sw[j] - np.outer(mu[j], mu[j])
    return sw / sw.sum(), mu, cov


def route(X, k: int) -> str:
    """"fused" (device tensors inside the kernel's range), "composite" (other device tensors) or
    "host" (host tensors: the twin).  The fused route is the default over its whole range: it
    measured faster than the composite at every cell of profiles/gmm.md."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and X.shape[1] >= 1
          and fused_range(int(X.shape[0]), int(k)))
    return "fused" if ok else "composite"


def _pass(X, sel, weights, means, covs, mode: int, how: str):
    from . import kernels

    if how == "composite":
        return composite_pass(X, sel, weights, means, covs, mode)
    return kernels.gmm_pass(X, sel, weights, means, covs, mode)  # fused on device tensors, the twin on host ones


def assign(X, sel, weights, means, covs, how: Optional[str] = None):
    """``(index, probabilities [k, n], log P)`` per row on X's device, by the route of (X, k)."""
    return _pass(X, sel, weights, means, covs, ASSIGN, how or route(X, len(weights)))


def seed_gaussians(X: torch.Tensor, sel, k: int, seed: int):
    """Starting ``(weights, means, covs)``, the same on every rank: uniform weights, and Gaussian j
    from rows 5 j .. 5 j + 4 of the ``5 k`` live rows with the smallest (hash, row) keys."""
    from ..parallel import comm
    from .kmeans import seed_centers

    n = int(X.shape[1])
    nlive = torch.tensor([float(n if sel is None else int(sel.to(torch.bool).sum()))], dtype=torch.float64,
                         device=X.device)
    if float(comm.all_reduce_sum(nlive).cpu()[0]) < _SAMPLES * int(k):
        raise ValueError(f"GaussianMixture: the start samples {_SAMPLES} rows per Gaussian and needs at least "
                         f"{_SAMPLES * int(k)} rows")
    rows = seed_centers(X, sel, _SAMPLES * int(k), "random", 0, seed).reshape(int(k), _SAMPLES, -1)
    means = rows.mean(axis=1)
    var = ((rows - means[:, None, :]) ** 2).mean(axis=1)
    return np.full(int(k), 1.0 / int(k)), means, np.stack([np.diag(v) for v in var])


@dataclass
class GmmResult:
    weights: np.ndarray  # [k]
    means: np.ndarray    # [k, d]
    covs: np.ndarray     # [k, d, d]
    log_likelihood: float  # the last iteration's E-step's
    iterations: int
    route: str


def em(step: Callable, weights, means, covs, max_iter: int, tol: float, how: str) -> GmmResult:
    """Spark's ``while`` over one pass per iteration: ``step(weights, means, covs)`` gives this
    rank's statistics, which are summed over the ranks; the M-step runs on the host."""
    from ..parallel import comm

    w, mu, cov = (np.array(_np(t), dtype=np.float64) for t in (weights, means, covs))
    k, d = mu.shape
    prev, ll, it = 0.0, -sys.float_info.max, 0
    while it < int(max_iter) and abs(ll - prev) > tol:
        stats = _np(comm.all_reduce_sum(step(w, mu, cov)))
        prev, ll = ll, float(stats[-2])
        w, mu, cov = m_step_host(stats, k, d)
        it += 1
    return GmmResult(w, mu, cov, ll, it, how)


def fit(X, sel, k: int, max_iter: int = 100, tol: float = 0.01, seed: int = 0, init=None,
        how: str = "auto") -> GmmResult:
    """Fit on feature-major ``X`` ``[d, n]``.  ``init``: starting ``(weights, means, covs)`` instead
    of :func:`seed_gaussians`.  ``how``: "auto" (:func:`route`) or "fused" / "composite" / "host" to
    force one (tests, benchmarks)."""
    if how not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"gmm fit: unknown route {how!r}")
    if how == "auto":
        how = route(X, k)
    w, mu, cov = _check_params(*(init if init is not None else seed_gaussians(X, sel, k, seed)), int(X.shape[0]))
    if w.size != int(k):
        raise ValueError("gmm fit: init must hold k Gaussians")
    if how == "fused":
        from . import device

        return device.gmm_fit(X, sel, w, mu, cov, max_iter, tol)
    return em(lambda *p: _pass(X, sel, *p, STEP, how), w, mu, cov, max_iter, tol, how)
