"""k-means (Spark 2.4 ``ml.clustering.KMeans``, euclidean): the Lloyd pass, the seeding and the loop.

One Lloyd iteration assigns every live row of feature-major ``X[d, n]`` to its nearest centre --
``score = 0.5 |c|^2 - x . c``, ties to the lowest centre index (Spark's ``findClosest`` keeps the
first strict minimum) -- and sums the rows per centre.  The statistics of a pass are the flat f64
``[k d sums (centre-major), k counts, cost, live rows]`` with row cost ``max(0, |x|^2 + 2 score)``.
A centre that attracts no row keeps its position; the loop ends when every centre moved at most
``tol`` (a centre that did not move counts as converged).

Three routes compute a pass:

* the fused device pass (``csrc/hip/kmeans.hip`` through ``device.kmeans_fit``): dense f32 / f64,
  d <= 64, 2 <= k <= 64, X read by one kernel per iteration, iterations enqueued in batches;
* its fp64 twin :func:`lloyd_pass_host`: the CPU engine and the kernel tests' oracle;
* the composite :func:`composite_pass`: torch matmul + ``argmin`` + ``index_add_`` in f64 -- wider
  d or k on the device, and the benchmark's comparator.

Seeding uses the project's own seeded rule, not Spark's ``XORShiftRandom``: global row ``r`` draws
the uniform ``fold_hash(fold_seed(seed + round, 0), r) / 2^32``, computed on the rows' device.
Starting centres therefore agree with Spark's in distribution, not bit for bit; from equal starting
centres the iterations follow Spark 2.4.  In a data-parallel fit the shards number their rows in
rank order, the cost totals and candidate weights are summed over the ranks and the kept rows are
gathered, so every rank starts from the same centres.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

__all__ = ["STEP", "ASSIGN", "FUSED_MAX_D", "FUSED_MAX_K", "DEVICE_BATCH", "stats_size", "lloyd_pass_host",
           "update_host", "composite_pass", "route", "row_hashes", "row_uniforms", "seed_centers", "lloyd", "fit", "assign",
           "KMeansResult"]

STEP, ASSIGN = 0, 1  # codes of csrc/hip/kmeans.h
FUSED_MAX_D = 64
FUSED_MAX_K = 64
DEVICE_BATCH = 4
_LOCAL_ITERS = 30  # Spark's LocalKMeans


def stats_size(k: int, d: int) -> int:
    return k * d + k + 2


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _host_rows(X, sel, centers):
    Xd = _np(X).astype(np.float64)
    d, n = Xd.shape
    live = np.ones(n, dtype=bool) if sel is None else _np(sel).astype(bool)
    C = np.asarray(_np(centers), dtype=np.float64).reshape(-1, d)
    if live.shape != (n,):
        raise ValueError("kmeans_pass: row-count mismatch between features and selection")
    return np.where(live[None, :], Xd, 0.0), live, C


def lloyd_pass_host(X, sel, centers, mode: int):
    """The fp64 twin of the fused device pass on host data.  STEP: the flat statistics (torch f64);
    ASSIGN: ``(int32 index per row, -1 for dead rows; f64 row cost, 0 for dead rows)``.  Dead rows
    are selected to zero before any product, so their features may hold NaN."""
    Xz, live, C = _host_rows(X, sel, centers)
    k, d = C.shape
    score = 0.5 * np.einsum("kd,kd->k", C, C)[:, None] - C @ Xz  # [k, n]
    a = np.argmin(score, axis=0)  # the first minimum: the lowest index
    cost = np.maximum(0.0, np.einsum("dn,dn->n", Xz, Xz) + 2.0 * score[a, np.arange(a.size)])
    cost = np.where(live, cost, 0.0)
    if mode == ASSIGN:
        return torch.from_numpy(np.where(live, a, -1).astype(np.int32)), torch.from_numpy(cost)
    if mode != STEP:
        raise ValueError("kmeans_pass: mode must be STEP (0) or ASSIGN (1)")
    out = np.zeros(stats_size(k, d))
    for c in range(k):
        m = live & (a == c)
        out[c * d:(c + 1) * d] = Xz[:, m].sum(axis=1)
        out[k * d + c] = m.sum()
    out[k * d + k] = cost.sum()
    out[k * d + k + 1] = live.sum()
    return torch.from_numpy(out)


def update_host(stats, centers, tol: float):
    """New centres ``[k, d]`` and ``(cost, max moved^2, done)`` from reduced statistics."""
    C = np.asarray(_np(centers), dtype=np.float64)
    k, d = C.shape
    s = _np(stats)
    cnt = s[k * d:k * d + k]
    new = np.where(cnt[:, None] > 0, s[:k * d].reshape(k, d) / np.where(cnt > 0, cnt, 1.0)[:, None], C)
    moved = ((new - C) ** 2).sum(axis=1)
    return new, float(s[k * d + k]), float(moved.max()), bool((moved <= tol * tol).all())


def composite_pass(X, sel, centers, mode: int):
    """The same pass from torch ops in f64 (any d and k, host or device): a ``[k, n]`` score matrix,
    ``argmin``, ``index_add_``."""
    Xd = X.to(torch.float64)
    d, n = Xd.shape
    C = torch.as_tensor(_np(centers), dtype=torch.float64).reshape(-1, d).to(Xd.device)
    k = C.shape[0]
    live = torch.ones(n, dtype=torch.bool, device=Xd.device) if sel is None else sel.to(torch.bool)
    Xz = torch.where(live[None, :], Xd, torch.zeros_like(Xd))
    score = 0.5 * (C * C).sum(dim=1)[:, None] - C @ Xz
    best, a = score.min(dim=0)
    # (torch's min may return any of several equal minima: take the lowest index among them)
    a = torch.where(score == best[None, :], torch.arange(k, device=Xd.device)[:, None], k).min(dim=0).values
    cost = torch.clamp((Xz * Xz).sum(dim=0) + 2.0 * best, min=0.0)
    cost = torch.where(live, cost, torch.zeros_like(cost))
    if mode == ASSIGN:
        return torch.where(live, a, torch.full_like(a, -1)).to(torch.int32), cost
    sums = torch.zeros(k + 1, d, dtype=torch.float64, device=Xd.device)
    idx = torch.where(live, a, torch.full_like(a, k))  # dead rows land in a row that is dropped
    sums.index_add_(0, idx, Xz.t())
    cnt = torch.bincount(idx, minlength=k + 1)[:k].to(torch.float64)
    return torch.cat([sums[:k].reshape(-1), cnt, cost.sum()[None], live.sum().to(torch.float64)[None]])


def route(X, k: int) -> str:
    """"fused" (device tensors inside the kernel's range), "composite" (other device tensors) or
    "host" (host tensors: the twin).  The fused route is the default over its whole range: see
    profiles/kmeans.md for the measurements behind that."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and 1 <= X.shape[0] <= FUSED_MAX_D
          and X.shape[1] >= 1 and 2 <= int(k) <= FUSED_MAX_K)
    return "fused" if ok else "composite"


def _pass(X, sel, centers, mode: int, how: str):
    from . import kernels

    if how == "composite":
        return composite_pass(X, sel, centers, mode)
    return kernels.kmeans_pass(X, sel, centers, mode)  # fused on device tensors, the twin on host ones


def assign(X, sel, centers, how: Optional[str] = None):
    """``(index, cost)`` per row on X's device, by the route of (X, k).  More than 64 centres over
    features the fused pass serves (the k-means|| candidates) run it in chunks of at most 64 and keep
    the strictly smaller cost, so the lowest index still wins a tie and nothing of size k x n exists."""
    C = np.asarray(_np(centers), dtype=np.float64)
    k = C.shape[0]
    if how is None and k > FUSED_MAX_K and route(X, 2) == "fused":
        best = bidx = None
        for part in np.array_split(np.arange(k), -(-k // FUSED_MAX_K)):
            idx, cost = _pass(X, sel, C[part], ASSIGN, "fused")
            idx = torch.where(idx >= 0, idx + int(part[0]), idx)
            if best is None:
                best, bidx = cost, idx
            else:
                take = cost < best
                best, bidx = torch.where(take, cost, best), torch.where(take, idx, bidx)
        return bidx, best
    return _pass(X, sel, C, ASSIGN, how or route(X, k))


# ---- seeding ---------------------------------------------------------------------------------------
_KEY_DEAD = (1 << 63) - 1


def _i64(v: int) -> int:
    """A 64-bit pattern as the signed integer torch's wrapping int64 arithmetic takes."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def row_hashes(seed: int, n: int, draw: int = 0, offset: int = 0, device="cpu") -> torch.Tensor:
    """``kernels.fold_hash(fold_seed(seed + draw, 0), offset + r)`` of rows r = 0..n-1 as int64 in
    [0, 2^32), computed on ``device`` (the same bits as the numpy statement: wrapping int64
    multiplies, logical shifts by masking).  ``offset`` is the shard's first global row, so the
    shards of a data-parallel table draw what one process draws for the whole table."""
    from . import kernels

    def lsr(z, sh):
        return (z >> sh) & ((1 << (64 - sh)) - 1)

    g = torch.arange(int(offset) + 1, int(offset) + int(n) + 1, dtype=torch.int64, device=device)
    z = g * _i64(0x9E3779B97F4A7C15) + _i64(kernels.fold_seed(int(seed) + int(draw), 0))
    z = (z ^ lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return lsr(z ^ lsr(z, 31), 32)


def row_uniforms(seed: int, n: int, draw: int = 0, offset: int = 0, device="cpu") -> torch.Tensor:
    """Uniforms in [0, 1) of rows 0..n-1 for draw number ``draw`` of a seed (f64, on ``device``)."""
    return row_hashes(seed, n, draw, offset, device).to(torch.float64) / 4294967296.0


def _rows_of(X: torch.Tensor, idx: torch.Tensor) -> np.ndarray:
    """Rows ``idx`` of feature-major X as a host ``[len(idx), d]`` f64 matrix."""
    return X[:, idx.to(X.device)].to(torch.float64).t().cpu().numpy().reshape(int(idx.numel()), int(X.shape[0]))


def _gather_rows(X: torch.Tensor, idx: torch.Tensor, order_key: torch.Tensor):
    """The rows ``idx`` of every rank's shard, as one host matrix sorted by their (unique) keys."""
    from ..parallel import comm

    parts = comm.all_gather_object((order_key.cpu().numpy(), _rows_of(X, idx)))
    key = np.concatenate([p[0] for p in parts])
    o = np.argsort(key, kind="stable")
    return np.concatenate([p[1] for p in parts])[o], key[o]


def _local_kmeans(P: np.ndarray, w: np.ndarray, k: int, u: np.ndarray) -> np.ndarray:
    """Spark's ``LocalKMeans``: weighted k-means++ over the candidates P ``[m, d]`` (uniforms ``u``,
    one per pick), then at most 30 weighted Lloyd iterations."""
    m = P.shape[0]
    first = min(int(np.searchsorted(np.cumsum(w), u[0] * w.sum(), side="right")), m - 1)
    C = [P[first]]
    cost = ((P - C[0]) ** 2).sum(axis=1)
    for i in range(1, k):
        cw = np.cumsum(w * cost)
        j = min(int(np.searchsorted(cw, u[i] * cw[-1], side="right")), m - 1) if cw[-1] > 0 else 0
        C.append(P[j])
        cost = np.minimum(cost, ((P - P[j]) ** 2).sum(axis=1))
    C = np.array(C)
    prev = None
    for _ in range(_LOCAL_ITERS):
        a = np.argmin(((P[:, None, :] - C[None, :, :]) ** 2).sum(axis=2), axis=1)
        if prev is not None and np.array_equal(a, prev):
            break
        prev = a
        for c in range(k):
            mk = a == c
            if w[mk].sum() > 0:
                C[c] = (P[mk] * w[mk, None]).sum(axis=0) / w[mk].sum()
    return C


def seed_centers(X: torch.Tensor, sel, k: int, mode: str, steps: int, seed: int) -> np.ndarray:
    """Starting centres ``[k, d]`` (host f64), the same on every rank.  The per-row work (hashes,
    thresholds, selection) runs on X's device; only the chosen rows come to the host.  A row's
    identity is its global index (shards in rank order), so contiguous shards draw what one
    process draws.  ``random``: the k live rows with the smallest (hash, row).  ``k-means||``:
    the first of those, ``steps`` rounds that keep row r if ``u_r < 2 k cost_r / sum cost`` against
    the centres so far (cost totals summed over the ranks, kept rows gathered), the candidates
    weighted by one assignment pass, then weighted k-means++ and a short local Lloyd on the host."""
    from ..parallel import comm

    if mode not in ("random", "k-means||"):
        raise ValueError(f"KMeans: unknown initMode {mode!r}")
    n, dev = int(X.shape[1]), X.device
    sizes = comm.all_gather_object(n)
    offset = int(sum(sizes[:comm.rank()]))
    if sum(sizes) >= 1 << 31:
        raise ValueError("KMeans: seeding numbers the rows in 31 bits")
    live = torch.ones(n, dtype=torch.bool, device=dev) if sel is None else sel.to(torch.bool)
    grow = torch.arange(offset, offset + n, dtype=torch.int64, device=dev)
    key = torch.where(live, (row_hashes(seed, n, 0, offset, dev) << 31) | grow, torch.full_like(grow, _KEY_DEAD))
    top = torch.topk(key, min(int(k), n), largest=False, sorted=True) if n else None
    own = top.indices[top.values != _KEY_DEAD] if n else torch.zeros(0, dtype=torch.int64, device=dev)
    first, _ = _gather_rows(X, own, key[own])  # every rank's k smallest, merged: the k smallest are among them
    if first.shape[0] == 0:
        raise ValueError("KMeans: the input has no rows")
    if mode == "random" or first.shape[0] <= 1:
        C = first[:k]
        return C if C.shape[0] == k else np.concatenate([C, np.repeat(C[-1:], k - C.shape[0], axis=0)])
    P, seen = first[:1], set()  # seen: global rows already kept (the first centre may be kept again: np.unique below)
    for s in range(int(steps)):
        _, cost = assign(X, sel, P)
        total = float(comm.all_reduce_sum(cost.sum().reshape(1)).cpu()[0])
        if not total > 0.0:
            break
        keep = torch.nonzero(live & (row_uniforms(seed, n, s + 1, offset, dev) < (2.0 * k / total) * cost)).reshape(-1)
        rows, gid = _gather_rows(X, keep, grow[keep])
        fresh = np.array([int(g) not in seen for g in gid], dtype=bool)
        seen.update(int(g) for g in gid)
        P = np.concatenate([P, rows[fresh]])
    P = np.unique(P, axis=0)
    if P.shape[0] <= k:  # fewer distinct candidates than centres: Spark pads with duplicates
        return np.concatenate([P, np.repeat(P[-1:], k - P.shape[0], axis=0)])
    idx, _ = assign(X, sel, P)
    w = torch.bincount(idx[idx >= 0].to(torch.long), minlength=P.shape[0]).to(torch.float64)
    w = comm.all_reduce_sum(w).cpu().numpy()
    return _local_kmeans(P, w, k, row_uniforms(seed, k, int(steps) + 1).numpy())


# ---- the loop ----------------------------------------------------------------------------------------
@dataclass
class KMeansResult:
    centers: np.ndarray  # [k, d]
    iterations: int
    cost: float          # the last iteration's (Spark's trainingCost)
    converged: bool
    route: str


def lloyd(X, sel, centers, max_iter: int, tol: float, how: str) -> KMeansResult:
    """Spark's ``runAlgorithm`` over one pass per iteration, statistics summed over the ranks."""
    from ..parallel import comm

    C = np.array(_np(centers), dtype=np.float64)
    it, cost, done = 0, 0.0, False
    while it < int(max_iter) and not done:
        stats = comm.all_reduce_sum(_pass(X, sel, C, STEP, how))
        C, cost, _, done = update_host(stats, C, tol)
        it += 1
    return KMeansResult(C, it, cost, done, how)


def fit(X, sel, k: int, init_mode: str = "k-means||", init_steps: int = 2, max_iter: int = 20, tol: float = 1e-4,
        seed: int = 0, init_centers=None, how: str = "auto") -> KMeansResult:
    """Fit on feature-major ``X`` ``[d, n]``.  ``how``: "auto" (:func:`route`) or "fused" /
    "composite" / "host" to force one (tests, benchmarks)."""
    if how not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"kmeans fit: unknown route {how!r}")
    if how == "auto":
        how = route(X, k)
    if init_centers is None:
        init_centers = seed_centers(X, sel, k, init_mode, init_steps, seed)
    C = np.asarray(_np(init_centers), dtype=np.float64)
    if C.shape != (int(k), int(X.shape[0])):
        raise ValueError("kmeans fit: init_centers must be [k, d]")
    if how == "fused":
        from . import device

        r = device.kmeans_fit(X, sel, C, max_iter, tol, DEVICE_BATCH)
        return KMeansResult(r["centers"], r["iterations"], r["cost"], r["done"], "fused")
    return lloyd(X, sel, C, max_iter, tol, how)
