"""Generalized linear models: the family / link tables (Spark 2.4 ``GeneralizedLinearRegression``)
and the IRLS (iteratively reweighted least squares) drivers.

One IRLS iteration is a weighted least-squares fit of the working response ``z`` with the working
weights ``w'``; both follow from ``eta = x . beta + b`` of each row:

    mu = project(unlink(eta));  g = link'(mu);  z = eta + (y - mu) g;  w' = w / (g^2 V(mu))

and the starting model fits ``z = link(init(y, w))`` with ``w' = w``.  Three routes compute the
statistics of ``(x, z, w')`` (the ``gram_stats`` layout):

* the fused device pass (``csrc/hip/glm_irls.hip`` through ``device.glm_fit``): d <= 64, X read once
  per iteration, the whole loop enqueued on the device;
* its fp64 twin :func:`glm_pass_host`: the CPU engine and the kernel tests' oracle;
* the composite route :func:`composite_pass`: ``predict``, elementwise torch, weighted ``gram_stats``
  -- d > 64, and the benchmark's comparator.

:func:`fit` picks the route and owns the host loop; a device fit that ends with a non-zero solver
status is re-run on the host route, which owns the warnings, errors and fallbacks.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

__all__ = ["FAMILIES", "LINKS", "SUPPORTED", "DEFAULT_LINK", "INIT", "STEP", "EPS", "MAX_FEATURES", "FUSED_MAX_D",
           "DEVICE_BATCH", "link", "unlink", "dlink", "variance", "project", "init_mu", "working", "glm_pass_host",
           "composite_pass", "irls", "fit", "IrlsResult", "resolve_link", "unit_deviance"]

# codes of csrc/hip/glm_irls.h
FAMILIES = {"gaussian": 0, "binomial": 1, "poisson": 2, "gamma": 3}
LINKS = {"identity": 0, "log": 1, "logit": 2, "inverse": 3, "sqrt": 4}
SUPPORTED = {"gaussian": ("identity", "log", "inverse"), "binomial": ("logit",),
             "poisson": ("log", "identity", "sqrt"), "gamma": ("inverse", "identity", "log")}
DEFAULT_LINK = {f: ls[0] for f, ls in SUPPORTED.items()}
INIT, STEP = 0, 1
EPS = 1e-16
DBL_MAX = sys.float_info.max
MAX_FEATURES = 4096  # Spark's WLS limit, which IRLS inherits
# The fused pass serves d <= FUSED_MAX_D (the kernel's own limit is 64) and the enqueued loop reads
# its state once per DEVICE_BATCH iterations: see profiles/glm.md for both.
FUSED_MAX_D = 64
DEVICE_BATCH = 4


def resolve_link(family: str, link_name: Optional[str]) -> str:
    """The link of a (family, link) request: the family's default for None; ValueError for a pair
    that is not supported."""
    if family not in SUPPORTED:
        raise ValueError(f"GeneralizedLinearRegression: family {family!r} is not supported "
                         f"(supported: {', '.join(SUPPORTED)})")
    if link_name is None:
        return DEFAULT_LINK[family]
    if link_name not in SUPPORTED[family]:
        raise ValueError(f"Generalized Linear Regression with {family} family does not support the {link_name} "
                         f"link function.")
    return link_name


# ---- the tables (torch, f64; any device) ---------------------------------------------------------
def link(name: str, mu: torch.Tensor) -> torch.Tensor:
    if name == "identity":
        return mu
    if name == "log":
        return torch.log(mu)
    if name == "logit":
        return torch.log(mu / (1.0 - mu))
    if name == "inverse":
        return 1.0 / mu
    if name == "sqrt":
        return torch.sqrt(mu)
    raise ValueError(f"unknown link {name!r}")


def unlink(name: str, eta: torch.Tensor) -> torch.Tensor:
    if name == "identity":
        return eta
    if name == "log":
        return torch.exp(eta)
    if name == "logit":
        return 1.0 / (1.0 + torch.exp(-eta))
    if name == "inverse":
        return 1.0 / eta
    if name == "sqrt":
        return eta * eta
    raise ValueError(f"unknown link {name!r}")


def dlink(name: str, mu: torch.Tensor) -> torch.Tensor:
    if name == "identity":
        return torch.ones_like(mu)
    if name == "log":
        return 1.0 / mu
    if name == "logit":
        return 1.0 / (mu * (1.0 - mu))
    if name == "inverse":
        return -1.0 / (mu * mu)
    if name == "sqrt":
        return 1.0 / (2.0 * torch.sqrt(mu))
    raise ValueError(f"unknown link {name!r}")


def variance(family: str, mu: torch.Tensor) -> torch.Tensor:
    if family == "gaussian":
        return torch.ones_like(mu)
    if family == "binomial":
        return mu * (1.0 - mu)
    if family == "poisson":
        return mu
    if family == "gamma":
        return mu * mu
    raise ValueError(f"unknown family {family!r}")


def project(family: str, mu: torch.Tensor) -> torch.Tensor:
    if family == "gaussian":
        return torch.clamp(mu, -DBL_MAX, DBL_MAX)  # +-inf -> +-DBL_MAX (NaN stays)
    if family == "binomial":
        return torch.clamp(mu, EPS, 1.0 - EPS)
    return torch.clamp(mu, EPS, DBL_MAX)  # poisson, gamma


def init_mu(family: str, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if family == "binomial":
        return (w * y + 0.5) / (w + 1.0)
    if family == "poisson":
        return torch.clamp(y, min=0.1)
    return y


def working(family: str, link_name: str, eta: Optional[torch.Tensor], y: torch.Tensor, w: torch.Tensor, mode: int):
    """(z, w') of every row (f64; dead rows are the caller's to select away)."""
    if mode == INIT:
        return link(link_name, init_mu(family, y, w)), w
    mu = project(family, unlink(link_name, eta))
    g = dlink(link_name, mu)
    return eta + (y - mu) * g, w / (g * g * variance(family, mu))


def _ylogy(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a ln(a / b), 0 where a = 0."""
    safe = torch.where(a == 0, torch.ones_like(a), a)
    return torch.where(a == 0, torch.zeros_like(a), a * torch.log(safe / b))


def unit_deviance(family: str, y: torch.Tensor, mu: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if family == "gaussian":
        return w * (y - mu) * (y - mu)
    if family == "binomial":
        return 2.0 * w * (_ylogy(y, mu) + _ylogy(1.0 - y, 1.0 - mu))
    if family == "poisson":
        return 2.0 * w * (_ylogy(y, mu) - (y - mu))
    if family == "gamma":
        return -2.0 * w * (torch.log(y / mu) - (y - mu) / mu)
    raise ValueError(f"unknown family {family!r}")


# ---- the pass: twin and composite ------------------------------------------------------------------
def _beta_parts(beta, d: int):
    b = beta.detach().cpu().numpy() if torch.is_tensor(beta) else np.asarray(beta, dtype=np.float64)
    if b.shape != (d + 1,):
        raise ValueError("glm_pass: beta must hold d coefficients and the intercept")
    return b[:d], float(b[d])


def _check_rows(X, y, w, sel):
    d, n = X.shape
    if int(y.shape[0]) != n or (w is not None and w.shape[0] != n) or (sel is not None and sel.shape[0] != n):
        raise ValueError("glm_pass: row-count mismatch between features, label, weight and selection")
    return int(d), int(n)


def glm_pass_host(X, y, w, sel, beta, family: str, link_name: str, mode: int) -> torch.Tensor:
    """The fp64 twin of the fused device pass on host tensors: the flat statistics (``gram_stats``
    layout) of ``(x, z, w')``.  Dead rows are selected to zero before any product, so their
    features and label may hold NaN."""
    from . import kernels

    resolve_link(family, link_name)
    d, n = _check_rows(X, y, w, sel)
    Xd = X.to(torch.float64)
    yd = y.to(torch.float64)
    wd = torch.ones(n, dtype=torch.float64) if w is None else w.to(torch.float64)
    live = torch.ones(n, dtype=torch.bool) if sel is None else sel.to(torch.bool)
    eta = None
    if mode == STEP:
        coef, icpt = _beta_parts(beta, d)
        eta = torch.as_tensor(coef, dtype=torch.float64) @ torch.where(live, Xd, torch.zeros_like(Xd)) + icpt
    elif mode != INIT:
        raise ValueError("glm_pass: mode must be INIT (0) or STEP (1)")
    z, wp = working(family, link_name, eta, yd, wd, mode)
    zero = torch.zeros(n, dtype=torch.float64)
    z, wp = torch.where(live, z, zero), torch.where(live, wp, zero)
    return kernels.gram_stats(torch.where(live, Xd, torch.zeros_like(Xd)), z, wp, live)


def composite_pass(X, y, w, sel, beta, family: str, link_name: str, mode: int) -> torch.Tensor:
    """The same statistics from the existing ops: ``predict`` (one pass over X), elementwise torch
    on n-vectors, weighted ``gram_stats`` (a second pass over X).  Any d, host or device."""
    from . import kernels

    d, n = _check_rows(X, y, w, sel)
    yd = y.to(torch.float64)
    wd = torch.ones(n, dtype=torch.float64, device=yd.device) if w is None else w.to(torch.float64)
    eta = None
    if mode == STEP:
        coef, icpt = _beta_parts(beta, d)
        eta = kernels.predict(X, coef, icpt)
    z, wp = working(family, link_name, eta, yd, wd, mode)
    if sel is not None:
        zero = torch.zeros_like(z)
        z, wp = torch.where(sel, z, zero), torch.where(sel, wp, zero)
    return kernels.gram_stats(X, z, wp, sel, "fp64")


# ---- the host loop -----------------------------------------------------------------------------
@dataclass
class IrlsResult:
    coefficients: np.ndarray
    intercept: float
    iterations: int
    converged: bool
    wls: object          # the last solve's WLSModel (lazy diagInvAtWA)
    stats: object        # the last solve's GramStats (scalars at least)
    route: str           # "fused" | "host" | "composite" | "fused->host"


def _solve(flat, d, fit_icpt, reg):
    """Spark's inner solver: ``WeightedLeastSquares(fitIntercept, regParam, elasticNetParam = 0,
    standardizeFeatures = false, standardizeLabel = false)`` with its defaults (auto, 100, 1e-6)."""
    from ..models.optim import fit_wls_flat

    return fit_wls_flat(flat, d, fit_icpt, reg, 0.0, False, False, "auto", 100, 1e-6)


def irls(pass_fn: Callable, d: int, family: str, link_name: str, fit_icpt: bool, reg: float, max_iter: int,
         tol: float, route: str = "host") -> IrlsResult:
    """Spark's ``IterativelyReweightedLeastSquares`` over ``pass_fn(beta | None, mode) -> flat``
    (already summed over the ranks).  gaussian / identity is the single starting solve."""
    wls, stats = _solve(pass_fn(None, INIT), d, fit_icpt, reg)
    it, conv = 0, False
    if family == "gaussian" and link_name == "identity":
        return IrlsResult(np.asarray(wls.coefficients, dtype=np.float64), float(wls.intercept), 0, True, wls, stats,
                          route)
    while it < max_iter and not conv:
        beta = np.concatenate([np.asarray(wls.coefficients, dtype=np.float64), [float(wls.intercept)]])
        new, stats = _solve(pass_fn(beta, STEP), d, fit_icpt, reg)
        with np.errstate(invalid="ignore"):  # (a diverged fit: inf - inf; NaN never compares below tol)
            delta = float(np.max(np.abs(beta - np.concatenate([np.asarray(new.coefficients), [float(new.intercept)]]))))
        wls = new
        it += 1
        conv = delta < tol
    return IrlsResult(np.asarray(wls.coefficients, dtype=np.float64), float(wls.intercept), it, conv, wls, stats, route)


def _fused_ok(X) -> bool:
    return (torch.is_tensor(X) and X.is_cuda and X.dim() == 2 and X.dtype in (torch.float32, torch.float64)
            and 1 <= X.shape[0] <= FUSED_MAX_D and X.shape[1] >= 1)


def fit(X, y, w, sel, family: str, link_name: str, fit_icpt: bool, reg: float, max_iter: int, tol: float,
        route: str = "auto") -> IrlsResult:
    """Fit on feature-major ``X`` ``[d, n]``.  ``route``: "auto" (fused where it applies, else the
    host loop over the twin on host tensors / the composite pass on device tensors or d > 64), or
    "fused" / "composite" / "host" to force one (tests, benchmarks)."""
    from ..models.optim import GramStats, WLSModel
    from ..parallel import comm
    from . import kernels

    link_name = resolve_link(family, link_name)
    d = int(X.shape[0])
    if d > MAX_FEATURES:
        raise ValueError(f"requirement failed: Currently, GeneralizedLinearRegression only supports number of "
                         f"features <= {MAX_FEATURES}. Found {d} in the input dataset.")
    if route not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"glm fit: unknown route {route!r}")
    if route == "auto":
        route = "fused" if _fused_ok(X) else ("host" if not X.is_cuda and d <= 64 else "composite")
    handed_back = False
    if route == "fused":
        from . import device

        r = device.glm_fit(X, y, w, sel, family, link_name, fit_icpt, reg, max_iter, tol, DEVICE_BATCH)
        if r["status"] == 0:
            flat = r["flat"]

            def diag_inv():
                return _solve(flat, d, fit_icpt, reg)[0].diagInvAtWA
            head = flat[:5].cpu().numpy()
            wls = WLSModel(r["beta"][:d].copy(), float(r["beta"][d]), diag_inv, np.zeros(1), "cholesky")
            return IrlsResult(wls.coefficients, wls.intercept, r["iterations"], r["done"], wls,
                              GramStats.scalars_only(head, d), "fused")
        handed_back = True  # singular / degenerate solve: the host driver owns it
        route = "composite"
    one = kernels.glm_pass if route == "host" else composite_pass

    def pass_fn(beta, mode):
        return comm.all_reduce_sum(one(X, y, w, sel, beta, family, link_name, mode))
    return irls(pass_fn, d, family, link_name, fit_icpt, reg, max_iter, tol, "fused->host" if handed_back else route)
