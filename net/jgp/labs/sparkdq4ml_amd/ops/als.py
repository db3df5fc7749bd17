"""Alternating least squares (Spark 2.4 ``ml.recommendation.ALS``, explicit feedback): the segment
tables, the half-step, its routes, the start and the fit.

One half-step solves every *destination* (an item, then a user) from the factor rows of the
*sources* it was rated with: for ratings ``r_j`` of sources ``y_j``, ``j = 1..m``,
``(sum y_j y_j^T + regParam m I) x = sum r_j y_j`` -- Spark's ALS-WR scaling by the number of
ratings -- by Cholesky, as Spark's ``CholeskySolver``.  Factors are stored as f32 (Spark's
``Float``), the arithmetic is f64 and a solution is rounded once, at its store.  A destination with
no rating gets zeros.  A non-positive pivot (possible only with ``regParam = 0``) is counted; the
fit reads the count once, at its end, and raises, as Spark does when ``dppsv`` fails.

A side's ratings are a segment table: ``offsets [D + 1]``, and destination-major ``src [nnz]``
(dense source indices, in row order within a destination) and ``rating [nnz]`` (f64).  It is built
once per fit and per side by :func:`build_segments` -- a stable ``sort_permutation`` on the
destination index and a scan of the counts; the iterations then only launch.

Two routes compute a half-step:

* the fused device pass (``csrc/hip/als.hip`` through ``device._AlsPlan``): 1 <= rank <= 64,
  f32 / f64 factors, one launch (and a small second one for long segments);
* its fp64 twin :func:`als_half_step_host`: the CPU engine and the kernel tests' oracle.

There is no composite route: a device rank outside the fused range raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

__all__ = ["RANK_MIN", "RANK_MAX", "CHUNK", "system_size", "Segments", "build_segments", "initial_factors",
           "als_half_step_host", "predict_host", "route", "predict", "fit", "AlsResult"]

# the fused range and the chunk: the constants of csrc/hip/als.h
RANK_MIN, RANK_MAX = 1, 64
CHUNK = 2048


def system_size(rank: int) -> int:
    """Doubles of one pre-solve system: packed upper triangle (column-major), right-hand side, m."""
    return rank * (rank + 1) // 2 + rank + 1


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


@dataclass
class Segments:
    """One side's ratings, destination-major.  ``D`` destinations, ``S`` sources."""
    offsets: torch.Tensor  # int64 [D + 1]
    src: torch.Tensor      # int32 [nnz]
    rating: torch.Tensor   # f64 [nnz]
    D: int
    S: int


def build_segments(dst: torch.Tensor, src: torch.Tensor, rating: torch.Tensor, D: int, S: int) -> Segments:
    """The segment table of the ratings ``(dst[i], src[i], rating[i])`` (dense indices; every row
    counts), on the tensors' device."""
    from .sort import sort_permutation

    n = int(dst.numel())
    if int(src.numel()) != n or int(rating.numel()) != n:
        raise ValueError("als: destination, source and rating must have one entry per row")
    if D < 1 or S < 1:
        raise ValueError("als: at least one destination and one source")
    dst = dst.to(torch.int32).contiguous()
    perm = sort_permutation([dst]).to(dst.device) if n else torch.zeros(0, dtype=torch.int64, device=dst.device)
    counts = torch.zeros(D + 1, dtype=torch.int64, device=dst.device)
    if n:
        counts[:D] = torch.bincount(dst.to(torch.int64), minlength=D)[:D]
    if dst.is_cuda:
        from . import device

        device.scan_counts(counts)
    else:
        counts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts[:D], 0)])
    return Segments(counts, src.to(torch.int32)[perm].contiguous(), rating.to(torch.float64)[perm].contiguous(), int(D),
                    int(S))


def initial_factors(n: int, rank: int, seed: int, side: int) -> np.ndarray:
    """Spark's start: rows of Gaussian vectors scaled to unit norm, as f32 ``[n, rank]``.  The
    normals are Box-Muller transforms of the project's hash of (seed, side, index, component),
    computed on the host so that both engines start from the same bits (Spark's distribution, not
    its bits)."""
    from .kmeans import row_hashes

    cnt = int(n) * int(rank)
    u1 = (row_hashes(int(seed), cnt, draw=2 * int(side)).numpy().astype(np.float64) + 0.5) / 4294967296.0
    u2 = row_hashes(int(seed), cnt, draw=2 * int(side) + 1).numpy().astype(np.float64) / 4294967296.0
    z = (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(int(n), int(rank))
    nrm = np.sqrt((z * z).sum(axis=1, keepdims=True))
    return (z / np.where(nrm > 0.0, nrm, 1.0)).astype(np.float32)


def _solve_spd(A: np.ndarray, b: np.ndarray) -> Optional[np.ndarray]:
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def als_half_step_host(offsets, src, rating, Y, reg: float, dtype=np.float32, presolve: bool = False):
    """The fp64 twin of the fused half-step on host data: ``(X [D, rank] of dtype, failures)``, and
    with ``presolve`` also every destination's ``[system_size]`` sums before the ridge term."""
    off = _np(offsets).astype(np.int64)
    sidx = _np(src).astype(np.int64)
    r = _np(rating).astype(np.float64)
    Yd = _np(Y).astype(np.float64)
    D, rank = off.size - 1, Yd.shape[1]
    X = np.zeros((D, rank), dtype=dtype)
    pre = np.zeros((D, system_size(rank))) if presolve else None
    iu = np.triu_indices(rank)
    order = np.lexsort((iu[0], iu[1]))  # packed upper, column-major
    fails = 0
    for d in range(D):
        o0, o1 = int(off[d]), int(off[d + 1])
        m = o1 - o0
        if m == 0:
            continue
        Ys = Yd[sidx[o0:o1]]
        A, b = Ys.T @ Ys, Ys.T @ r[o0:o1]
        if presolve:
            pre[d] = np.concatenate([A[iu][order], b, [float(m)]])
        A[np.diag_indices(rank)] += float(reg) * m
        x = _solve_spd(A, b)
        if x is None:
            fails += 1
            X[d] = np.nan
        else:
            X[d] = x
    return (X, fails, pre) if presolve else (X, fails)


def predict_host(u, v, sel, U, V) -> torch.Tensor:
    """f64 dot products of rows ``u[i]`` of U and ``v[i]`` of V; NaN for a dead row or an index -1."""
    ui, vi = _np(u).astype(np.int64), _np(v).astype(np.int64)
    ok = (ui >= 0) & (vi >= 0)
    if sel is not None:
        ok &= _np(sel).astype(bool)
    Ud, Vd = _np(U).astype(np.float64), _np(V).astype(np.float64)
    out = np.full(ui.size, np.nan)
    out[ok] = (Ud[ui[ok]] * Vd[vi[ok]]).sum(axis=1)
    return torch.from_numpy(out)


def route(t, rank: int) -> str:
    """"fused" (device tensors) or "host" (host tensors: the twin).  A device rank outside the fused
    range raises: there is no composite route."""
    if not (torch.is_tensor(t) and t.is_cuda):
        return "host"
    if not RANK_MIN <= int(rank) <= RANK_MAX:
        raise ValueError(f"ALS: the device pass takes {RANK_MIN} <= rank <= {RANK_MAX}, got {int(rank)}")
    return "fused"


def predict(u, v, sel, U, V):
    """The prediction column on the indices' device (``kernels.als_predict``)."""
    from . import kernels

    return kernels.als_predict(u, v, sel, U, V)


# ---- the fit -----------------------------------------------------------------------------------------
@dataclass
class AlsResult:
    user_factors: np.ndarray  # [users, rank] of the storage dtype
    item_factors: np.ndarray  # [items, rank]
    route: str


def fit(user: torch.Tensor, item: torch.Tensor, rating: torch.Tensor, n_users: int, n_items: int, rank: int = 10,
        max_iter: int = 10, reg: float = 0.1, seed: int = 0, how: str = "auto", storage=np.float32) -> AlsResult:
    """Fit on the ratings ``(user[i], item[i], rating[i])`` (dense indices, every row counts).
    ``how``: "auto" (:func:`route`) or "fused" / "host" to force one.  ``storage``: the dtype the
    factors are kept in between half-steps, f32 as Spark's; f64 measures what that rounding costs."""
    if how not in ("auto", "fused", "host"):
        raise ValueError(f"als fit: unknown route {how!r}")
    if int(rank) < 1:
        raise ValueError("ALS: rank must be >= 1")
    if how == "auto":
        how = route(user, rank)
    by_item = build_segments(item, user, rating, n_items, n_users)  # items from users
    by_user = build_segments(user, item, rating, n_users, n_items)  # users from items
    storage = np.dtype(storage)
    U = initial_factors(n_users, rank, seed, 0).astype(storage)
    V = initial_factors(n_items, rank, seed, 1).astype(storage)
    if how == "fused":
        from . import device

        plan = device._AlsPlan(by_item, by_user, int(rank), float(reg), torch.from_numpy(U[:0]).dtype)
        U, V, fails = plan.run(U, V, int(max_iter))
    else:
        fails = 0
        for _ in range(int(max_iter)):
            V, f1 = als_half_step_host(by_item.offsets, by_item.src, by_item.rating, U, reg, storage)
            U, f2 = als_half_step_host(by_user.offsets, by_user.src, by_user.rating, V, reg, storage)
            fails += f1 + f2
    if fails:
        raise ArithmeticError(f"ALS: the Cholesky factorisation of {fails} normal-equation systems met a non-positive "
                              "pivot (the matrix is positive definite whenever regParam > 0)")
    return AlsResult(np.asarray(U), np.asarray(V), how)
