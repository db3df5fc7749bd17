"""Device-op facade.

Every op takes/returns torch tensors.  CUDA (ROCm) tensors go to the gfx950 kernels of
``_dq4ml_hip`` — a missing extension is a hard error on a GPU box, never a silent torch
fallback.  CPU tensors (``local-cpu`` sessions, unit tests) run the host implementations, which
are also the fp64 oracles of the kernel tests.

Ops:
  K3  ``selected_indices``   stream compaction of a selection vector
  K4  ``pack_columns``       columns -> feature-major [d, n] matrix (cast)
  K5  ``gram_stats``         WLS sufficient statistics (MFMA Gram) of [X | 1 | y] with weights/mask
  K5i ``glm_pass``           one IRLS pass of a generalized linear model: statistics of (x, z, w')
  K5q ``quantiles``          exact order statistics of C columns x Q probabilities (radix select)
  K5g ``group_encode`` / ``group_agg``  group ids of key columns, integer-word grouped aggregates
  K5s ``sort_permutation``   stable multi-column radix sort of the live rows (row indices)
  K5w ``window_heads`` / ``window_bounds`` / ``window_prefix`` / ``window_minmax`` / ``window_finish``  scans over sorted positions
  K5j ``join_pairs`` / ``join_mask``  hash equi-join of two key columns: ordered (left, right) row pairs
  K7+K8 ``predict`` / ``regression_metrics``  fused GEMV + metric reductions
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import native
from .layout import gram_layout_size
from .groupby import group_agg, group_encode, group_encode_columns, group_limits, group_scale  # noqa: F401  (K5g)
from .sort import sort_limits, sort_permutation  # noqa: F401  (K5s: dispatches by device itself)
from .window import (window_bounds, window_finish, window_heads, window_limits, window_minmax,  # noqa: F401  (K5w:
                     window_prefix)  # dispatches by device itself)
from .join import join_key_columns, join_limits, join_mask, join_pairs  # noqa: F401  (K5j: dispatches by device itself)

__all__ = ["selected_indices", "pack_columns", "gram_stats", "predict", "regression_metrics",
           "gram_layout_size", "glm_pass", "gram_stats_folds", "fold_ids", "fold_thresholds", "fold_seed", "quantiles", "group_encode", "group_encode_columns",
           "group_agg", "group_scale", "group_limits", "sort_permutation", "sort_limits", "window_heads", "window_bounds",
           "window_prefix", "window_minmax", "window_finish", "window_limits", "join_pairs", "join_mask",
           "join_key_columns", "join_limits"]


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


# ------------------------------------------------------------------------------------------
# K3 — compaction
# ------------------------------------------------------------------------------------------
def selected_indices(sel: torch.Tensor, limit: Optional[int] = None) -> torch.Tensor:
    """Indices (int64) of the true entries of ``sel``, in order; at most ``limit`` of them."""
    if _on_gpu(sel):
        from . import device

        return device.compact_indices(sel, limit)
    idx = torch.nonzero(sel, as_tuple=False).flatten()
    return idx if limit is None else idx[:limit]


# ------------------------------------------------------------------------------------------
# K4 — pack
# ------------------------------------------------------------------------------------------
def pack_columns(parts: Sequence[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """Stack 1-row/k-row pieces (each ``[k_i, n]``) into one feature-major ``[d, n]`` matrix."""
    if parts and _on_gpu(parts[0]):
        from . import device

        return device.pack_columns(list(parts), dtype)
    return torch.cat([p.to(dtype) for p in parts], dim=0)


def pack_tiled(parts: Sequence[torch.Tensor], sel: Optional[torch.Tensor] = None):
    """GPU only: columns -> MFMA-fragment-ordered bf16 (``ops.layout.TiledBF16``); rows outside
    ``sel`` are written as zeros."""
    from . import device

    return device.pack_tiled(list(parts), sel)


def gram_cols(parts: Sequence[torch.Tensor], y: torch.Tensor, sel: Optional[torch.Tensor] = None):
    """GPU only: fused VectorAssembler + bf16 Gram over the source columns (d <= 64)."""
    from . import device

    return device.gram_cols(list(parts), y, sel)


def gram_stream_cols(parts: Sequence[torch.Tensor], y: torch.Tensor, w: Optional[torch.Tensor] = None,
                     sel: Optional[torch.Tensor] = None, compute: str = "fp64"):
    """GPU only: WLS statistics of 9..64 same-dtype source columns through the LDS-DMA stream
    kernels (``gram_stream.hip``); None when the sources do not qualify."""
    from . import device

    return device.gram_stream_cols(list(parts), y, w, sel, compute)


def gram_skinny_cols(parts: Sequence[torch.Tensor], y: torch.Tensor, w: Optional[torch.Tensor] = None,
                     sel: Optional[torch.Tensor] = None):
    """GPU only: f64 statistics of a narrow (d <= 8) assembly read from its source columns."""
    from . import device

    return device.gram_skinny_cols(list(parts), y, w, sel)


def pack_wide(parts: Sequence[torch.Tensor], eb: int, sel: Optional[torch.Tensor] = None):
    """GPU only: columns -> wide (d > 64) fragment layout, bf16 (eb 16) or fp8 e4m3 with
    per-feature scales (eb 8) (``ops.layout.TiledWide``); rows outside ``sel`` become zeros."""
    from . import device

    return device.pack_wide(list(parts), eb, sel)


# ------------------------------------------------------------------------------------------
# K5 — Gram / WLS statistics
# ------------------------------------------------------------------------------------------
_upper_idx = {}


def packed_upper(aa: torch.Tensor) -> torch.Tensor:
    """Packed upper (column-major) entries of a square matrix; index vectors cached per (d, device)."""
    d = aa.shape[0]
    key = (d, aa.device)
    idx = _upper_idx.get(key)
    if idx is None:
        J = torch.repeat_interleave(torch.arange(d, device=aa.device), torch.arange(1, d + 1, device=aa.device))
        I = torch.cat([torch.arange(j + 1, device=aa.device) for j in range(d)]) if d else J
        if len(_upper_idx) > 32:
            _upper_idx.clear()
        idx = _upper_idx[key] = (I, J)
    return aa[idx[0], idx[1]]


def gram_stats(X: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor], sel: Optional[torch.Tensor],
               compute: str = "fp64", x_zero_dead: bool = False, defer: bool = False) -> torch.Tensor:
    """Flat f64 ``[count, wSum, wwSum, bSum, bbSum, aSum[d], abSum[d], aaSum packed-upper]`` over
    live rows (``sel``), with instance weights ``w`` (default 1) — Spark WLS ``Aggregator.add`` over
    every row, in one pass.  ``X`` is feature-major ``[d, n]``."""
    d, n = X.shape
    if int(y.shape[0]) != n or (w is not None and w.shape[0] != n) or (sel is not None and sel.shape[0] != n):
        raise ValueError("gram_stats: row-count mismatch between features, label, weight and selection")
    if _on_gpu(X):
        from . import device

        return device.gram_stats(X, y, w, sel, compute, x_zero_dead=x_zero_dead, defer=defer)
    Xd = (X.to_dense() if hasattr(X, "to_dense") else X).to(torch.float64)
    yd = y.to(torch.float64)
    wv = torch.ones(n, dtype=torch.float64) if w is None else w.to(torch.float64)
    live = torch.ones(n, dtype=torch.bool) if sel is None else sel
    wv = torch.where(live, wv, torch.zeros_like(wv))
    count = float(live.sum())
    Xw = Xd * wv
    aa = Xw @ Xd.t()
    out = torch.empty(gram_layout_size(d), dtype=torch.float64)
    out[0] = count
    out[1] = wv.sum()
    out[2] = (wv * wv).sum()
    out[3] = (wv * yd).sum()
    out[4] = (wv * yd * yd).sum()
    out[5:5 + d] = Xw.sum(1)
    out[5 + d:5 + 2 * d] = Xw @ yd
    out[5 + 2 * d:] = packed_upper(aa)
    return out


# ------------------------------------------------------------------------------------------
# K5i — one IRLS pass of a generalized linear model
# ------------------------------------------------------------------------------------------
def glm_pass(X: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor], sel: Optional[torch.Tensor], beta,
             family: str, link: str, mode: int, blocks: Optional[int] = None) -> torch.Tensor:
    """Flat f64 statistics (the ``gram_stats`` layout) of ``(x, z, w')``: the working response and
    weights of ``ops/glm.py`` from ``beta = [coef(d), intercept]`` (``mode`` 1, STEP) or of the
    starting model (``mode`` 0, INIT).  Device tensors: the fused pass (d <= 64, f32 / f64
    features); host tensors: its fp64 twin."""
    if _on_gpu(X):
        from . import device

        return device.glm_pass(X, y, w, sel, beta, family, link, mode, blocks)
    from . import glm

    return glm.glm_pass_host(X, y, w, sel, beta, family, link, mode)


# ------------------------------------------------------------------------------------------
# K5f — fold-partitioned statistics (k-fold cross-validation in one pass)
# ------------------------------------------------------------------------------------------
MAX_FOLDS = 16
_M64 = (1 << 64) - 1
_RANK_SALT = 0xD1B54A32D192ED03


def fold_seed(seed: int, rank: Optional[int] = None) -> int:
    """Spark's ``long`` seed as the 64-bit hash seed of this rank: ``seed mod 2^64`` XOR
    ``rank * 0xD1B54A32D192ED03 mod 2^64`` (rank 0 / world 1: the seed itself), so the shards of
    a data-parallel table draw different granule hashes."""
    if rank is None:
        from ..parallel import comm

        rank = comm.rank()
    return (int(seed) & _M64) ^ ((int(rank) * _RANK_SALT) & _M64)


def fold_thresholds(k_or_weights) -> np.ndarray:
    """The k - 1 uint32 thresholds of the fold rule: ``(j << 32) // k`` for k equal folds, else
    ``floor(c_j * 2^32)`` with c_j the normalised cumulative weight (f64)."""
    if isinstance(k_or_weights, (int, np.integer)):
        k = int(k_or_weights)
        if not 1 <= k <= MAX_FOLDS:
            raise ValueError(f"number of folds must be in [1, {MAX_FOLDS}], got {k}")
        return np.array([(j << 32) // k for j in range(1, k)], dtype=np.uint32)
    w = np.asarray(list(k_or_weights), dtype=np.float64)
    if not 1 <= w.size <= MAX_FOLDS:
        raise ValueError(f"number of split weights must be in [1, {MAX_FOLDS}], got {w.size}")
    if not np.all(np.isfinite(w)) or np.any(w < 0) or not w.sum() > 0:
        raise ValueError(f"Weights must be nonnegative and their sum positive, but got {w.tolist()}")
    c = np.cumsum(w / w.sum())[:-1]
    return np.minimum(np.floor(c * 4294967296.0), 4294967295.0).astype(np.uint32)


def fold_hash(seed64: int, g: np.ndarray) -> np.ndarray:
    """uint32 hash of granule indices ``g`` (uint64) under the 64-bit seed (splitmix64 finaliser,
    high word); all arithmetic mod 2^64.  The device kernels compute the same bits."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed64) + (g.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def fold_ids_host(n: int, k_or_weights, seed64: int, granule: int) -> np.ndarray:
    """uint8 fold of physical rows 0..n-1 under an already rank-mixed 64-bit seed."""
    thr = fold_thresholds(k_or_weights)
    granule = int(granule)
    if granule < 1:
        raise ValueError("fold granule must be >= 1")
    ng = (int(n) + granule - 1) // granule
    u = fold_hash(seed64, np.arange(ng, dtype=np.uint64))
    f = np.searchsorted(thr, u, side="right").astype(np.uint8)  # = #{j : u >= t_j}
    return np.repeat(f, granule)[:int(n)] if granule > 1 else f


def fold_ids(n: int, k_or_weights, seed: int, granule: int, device=None) -> torch.Tensor:
    """uint8 fold id of every physical row (row r belongs to granule r // granule) under Spark
    seed ``seed`` on this rank; computed on ``device`` when it is a GPU, bit-equal to the host."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type == "cuda":
        from . import device as _device

        return _device.fold_ids(int(n), fold_thresholds(k_or_weights), fold_seed(seed), int(granule), dev)
    return torch.from_numpy(fold_ids_host(n, k_or_weights, fold_seed(seed), granule))


def folds_route(X, granule: int, compute: str = "fp64") -> str:
    """The route ``gram_stats_folds`` takes for these operands: "onepass" (the ``gram_folds``
    kernel) or "masked" (k masked ``gram_stats`` passes; always on the host)."""
    Xt = X if torch.is_tensor(X) else X.buf
    if not _on_gpu(Xt):
        return "masked"
    from . import device

    return "onepass" if device.onepass_ok(X, granule, compute) and int(X.shape[1]) > 0 else "masked"


def gram_stats_folds(X: torch.Tensor, y: torch.Tensor, sel: Optional[torch.Tensor], k_or_weights, seed: int,
                     granule: int, compute: str = "fp64") -> torch.Tensor:
    """``[k, P]`` f64: row f is the ``gram_stats`` vector (unit weights) of the live rows whose
    fold is f.  Device tensors: the one-pass ``gram_folds`` kernel or k masked ``gram_stats``
    passes (``device.gram_stats_folds``); host tensors: fp64 torch (the oracle and CPU engine)."""
    Xt = X if torch.is_tensor(X) else X.buf
    if _on_gpu(Xt):
        from . import device

        return device.gram_stats_folds(X, y, sel, k_or_weights, seed, granule, compute)
    d, n = X.shape
    if int(y.shape[0]) != n or (sel is not None and sel.shape[0] != n):
        raise ValueError("gram_stats_folds: row-count mismatch between features, label and selection")
    thr = fold_thresholds(k_or_weights)
    k = int(thr.size) + 1
    ids = fold_ids(n, k_or_weights, seed, granule)
    live = torch.ones(n, dtype=torch.bool) if sel is None else sel.to(torch.bool)
    Xd = (X.to_dense() if hasattr(X, "to_dense") else X).to(torch.float64)
    Xd = torch.where(live.unsqueeze(0), Xd, torch.zeros_like(Xd))  # dead rows: exact zeros, no NaN
    yd = torch.where(live, y.to(torch.float64), torch.zeros(n, dtype=torch.float64))
    out = torch.empty(k, gram_layout_size(d), dtype=torch.float64)
    for f in range(k):
        m = live & (ids == f)
        out[f] = gram_stats(Xd, yd, None, m, "fp64")
    return out


# ------------------------------------------------------------------------------------------
# K5q — exact quantiles (radix select over order-preserving 64-bit keys)
# ------------------------------------------------------------------------------------------
MAX_QUANTILES = 16
QUANT_BITS = 8  # digit width of the select: 64 / 8 = 8 histogram passes
_QUANT_BINS = 1 << QUANT_BITS
_QUANT_PASSES = 64 // QUANT_BITS
_SIGN = np.uint64(1 << 63)


def quantile_keys(x: np.ndarray) -> np.ndarray:
    """uint64 keys of non-NaN doubles whose unsigned order is the numeric order: -0.0 folded into
    +0.0, IEEE bits, negative values flip every bit, the others the sign bit."""
    b = (np.asarray(x, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where((b & _SIGN) != 0, ~b, b | _SIGN)


def quantile_unkey(k: int) -> float:
    k = int(k)
    b = (k ^ (1 << 63)) if k >> 63 else (~k & _M64)
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def quantile_rank(p: float, n: int) -> int:
    """1-based target rank of probability ``p`` among ``n`` values, as Spark's
    ``QuantileSummaries.query`` ranks an exact summary: the minimum for p = 0, the maximum for
    p = 1, else ``ceil(p * n)`` of one double multiply."""
    if p <= 0.0:
        return min(1, n)
    if p >= 1.0:
        return n
    return min(max(1, int(np.ceil(np.float64(p) * np.float64(n)))), n)


def _quantiles_host(cols, valids, sel, probs: np.ndarray, reduce):
    """The device algorithm in numpy: same keys, digits, slot sharing, rank rule and ``reduce``
    hook (the CPU engine and the gloo path)."""
    C, Q = len(cols), int(probs.size)
    live_sel = None if sel is None else sel.numpy().astype(bool)
    keys = []
    for c, v in zip(cols, valids):
        x = c.numpy().astype(np.float64)
        m = ~np.isnan(x)
        if v is not None:
            m &= v.numpy().astype(bool)
        if live_sel is not None:
            m &= live_sel
        keys.append(quantile_keys(x[m]))
    upref = [[0] for _ in range(C)]  # prefix of slot u
    slot = [[0] * Q for _ in range(C)]  # slot of target q
    rank = [[0] * Q for _ in range(C)]
    counts = [0] * C
    for k in range(_QUANT_PASSES):
        dshift = np.uint64(64 - QUANT_BITS * (k + 1))
        hist = np.zeros((C, Q, _QUANT_BINS), dtype=np.int64)
        for c in range(C):
            hi = keys[c] >> np.uint64(64 - QUANT_BITS * k) if k > 0 else None
            keep = np.zeros(keys[c].size, dtype=bool)
            for u, pref in enumerate(upref[c]):
                m = np.ones(keys[c].size, dtype=bool) if hi is None else hi == np.uint64(pref)
                keep |= m
                d = ((keys[c][m] >> dshift) & np.uint64(_QUANT_BINS - 1)).astype(np.int64)
                hist[c, u] = np.bincount(d, minlength=_QUANT_BINS)
            keys[c] = keys[c][keep]  # a key outside every prefix never matches again
        if reduce is not None:
            hist = reduce(torch.from_numpy(hist)).numpy()
        for c in range(C):
            if k == 0:
                counts[c] = int(hist[c, 0].sum())
                rank[c] = [quantile_rank(float(p), counts[c]) for p in probs]
            npref, nrank = [], []
            for q in range(Q):
                cum = np.cumsum(hist[c, slot[c][q]])
                if counts[c] == 0:
                    npref.append(0), nrank.append(0)
                    continue
                d = int(np.searchsorted(cum, rank[c][q], side="left"))
                npref.append((upref[c][slot[c][q]] << QUANT_BITS) | d)
                nrank.append(rank[c][q] - int(cum[d - 1] if d else 0))
            upref[c] = []
            for q in range(Q):
                if npref[q] not in upref[c]:
                    upref[c].append(npref[q])
                slot[c][q] = upref[c].index(npref[q])
            rank[c] = nrank
    values = np.array([[quantile_unkey(upref[c][slot[c][q]]) if counts[c] else np.nan for q in range(Q)]
                       for c in range(C)], dtype=np.float64).reshape(C, Q)
    return torch.from_numpy(values), torch.tensor(counts, dtype=torch.int64)


def quantiles(cols: Sequence[torch.Tensor], valids, sel: Optional[torch.Tensor], probs, blocks: Optional[int] = None,
              reduce=None):
    """Exact order statistics ``(values [C, Q] f64, counts [C] i64)`` of 1-D f64 / f32 / i32 / i64
    columns at the probabilities ``probs`` (at most ``MAX_QUANTILES``).  A row counts for column c
    when ``sel`` and ``valids[c]`` (each optional) are set and the value, cast to double, is not
    NaN.  The order statistic of p is the minimum for p = 0, the maximum for p = 1, else the
    ``ceil(p * n)``-th smallest; a column with no counted row gives NaN and count 0.  ``reduce``
    sums the per-pass int64 histogram over ranks.  Device tensors: the ``quantile`` kernels; host
    tensors: the same select in numpy."""
    cols = list(cols)
    if cols and _on_gpu(cols[0]):
        from . import device

        return device.quantiles(cols, valids, sel, probs, blocks=blocks, reduce=reduce)
    if not cols:
        raise ValueError("quantiles: no column")
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    if not 1 <= p.size <= MAX_QUANTILES:
        raise ValueError(f"quantiles: between 1 and {MAX_QUANTILES} probabilities per call, got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("quantiles: probabilities must lie in [0, 1]")
    valids = [None] * len(cols) if valids is None else list(valids)
    n = int(cols[0].numel())
    for c in cols:
        if c.dim() != 1 or int(c.numel()) != n:
            raise ValueError("quantiles: columns must be 1-D and of one length")
        if c.dtype not in (torch.float64, torch.float32, torch.int32, torch.int64):
            raise TypeError(f"quantiles: unsupported column dtype {c.dtype}")
    return _quantiles_host(cols, valids, sel, p, reduce)


# ------------------------------------------------------------------------------------------
# K7 / K8 — predict and regression metrics
# ------------------------------------------------------------------------------------------
def predict(X: torch.Tensor, coef: np.ndarray, intercept: float) -> torch.Tensor:
    if _on_gpu(X):
        from . import device

        return device.predict(X, coef, intercept)
    c = torch.as_tensor(np.asarray(coef), dtype=torch.float64)
    return c @ X.to(torch.float64) + intercept


def regression_metrics(X: torch.Tensor, y: torch.Tensor, coef: np.ndarray, intercept: float,
                       sel: Optional[torch.Tensor], shift: float) -> torch.Tensor:
    """f64 sums over live rows: [n, Σ(y-s), Σ(y-s)², Σr, Σr², Σ|r|, Σ(p-s), Σ(p-s)²], r = y - p."""
    if _on_gpu(X):
        from . import device

        return device.regression_metrics(X, y, coef, intercept, sel, shift)
    p = predict(X, coef, intercept)
    yd = y.to(torch.float64)
    live = torch.ones_like(yd, dtype=torch.bool) if sel is None else sel
    yd, p = yd[live], p[live]
    r = yd - p
    ys, ps = yd - shift, p - shift
    return torch.stack([torch.tensor(float(yd.numel()), dtype=torch.float64), ys.sum(), (ys * ys).sum(), r.sum(),
                        (r * r).sum(), r.abs().sum(), ps.sum(), (ps * ps).sum()])


# ------------------------------------------------------------------------------------------
# K9 — huber loss/gradient pass
# ------------------------------------------------------------------------------------------
def huber_pass(X, y, w, sel, ceff: np.ndarray, icpt: float, sigma: float, eps: float) -> torch.Tensor:
    """f64 ``[lossSum, weightSum, g_intercept, g_sigma, Σ_r m_r x_r (d)]`` (Spark HuberAggregator
    sums before division by the weight sum); ``ceff`` = coefficients / feature std."""
    if _on_gpu(X if torch.is_tensor(X) else X.buf):
        from . import device

        return device.huber_pass(X, y, w, sel, ceff, icpt, sigma, eps)
    Xd = (X.to_dense() if hasattr(X, "to_dense") else X).to(torch.float64)
    yd = y.to(torch.float64)
    n = yd.shape[0]
    wt = torch.ones(n, dtype=torch.float64) if w is None else w.to(torch.float64)
    if sel is not None:
        wt = torch.where(sel, wt, torch.zeros_like(wt))
    margin = torch.as_tensor(ceff, dtype=torch.float64) @ Xd + icpt
    lin = yd - margin
    inside = lin.abs() <= sigma * eps
    q = lin / sigma
    loss = torch.where(inside, 0.5 * wt * (sigma + lin * lin / sigma),
                       0.5 * wt * (sigma + 2.0 * eps * lin.abs() - sigma * eps * eps))
    sgn = torch.where(lin >= 0, -1.0, 1.0).to(torch.float64)
    m = torch.where(inside, -wt * q, wt * sgn * eps)
    gs = torch.where(inside, 0.5 * wt * (1.0 - q * q), 0.5 * wt * (1.0 - eps * eps) * torch.ones_like(q))
    live = wt != 0
    out = torch.empty(4 + Xd.shape[0], dtype=torch.float64)
    out[0] = loss[live].sum()
    out[1] = wt.sum()
    out[2] = m[live].sum()
    out[3] = gs[live].sum()
    out[4:] = Xd @ torch.where(live, m, torch.zeros_like(m))
    return out


# ------------------------------------------------------------------------------------------
# K9 — squared-loss l-bfgs evaluation passes
# ------------------------------------------------------------------------------------------
class _HostLsq:
    """fp64 host implementation of :class:`ops.device.LsqPasses` (CPU engine; the kernel tests'
    oracle)."""

    def __init__(self, X, y, w, sel):
        self.X = (X.to_dense() if hasattr(X, "to_dense") else X).to(torch.float64)
        self.d, self.n = int(self.X.shape[0]), int(self.X.shape[1])
        wt = torch.ones(self.n, dtype=torch.float64) if w is None else w.to(torch.float64)
        if sel is not None:
            wt = torch.where(sel.to(torch.bool), wt, torch.zeros_like(wt))
        self.w = wt
        self.y = torch.where(wt != 0, y.to(torch.float64), torch.zeros_like(wt))
        self.device = self.X.device
        self._Xz = torch.where(wt.unsqueeze(0) != 0, self.X, torch.zeros_like(self.X))  # dead rows: no NaN

    def scalars(self):
        w, y = self.w, self.y
        return torch.stack([(w != 0).sum().to(torch.float64), w.sum(), (w * w).sum(), (w * y).sum(),
                            (w * y * y).sum()])

    def moments(self):
        return torch.cat([self._Xz @ self.w, (self._Xz * self._Xz) @ self.w])

    def evaluate(self, cf, offset, inv_ystd):
        cf = cf.to(torch.float64)
        diff = cf @ self._Xz + torch.as_tensor(offset, dtype=torch.float64).reshape(()) - self.y * inv_ystd
        v = torch.where(self.w != 0, self.w * diff, torch.zeros_like(diff))
        out = torch.empty(1 + self.d, dtype=torch.float64)
        out[0] = (0.5 * v * diff).sum()
        out[1:] = self._Xz @ v
        return out

    def wmargins(self, cf):
        return self.w * (cf.to(torch.float64) @ self._Xz)

    def evaluate_u(self, u, cf, offset, inv_ystd):
        live = self.w != 0
        v = torch.where(live, u + self.w * (torch.as_tensor(offset, dtype=torch.float64).reshape(()) - self.y * inv_ystd),
                        torch.zeros_like(u))
        out = torch.empty(1 + self.d, dtype=torch.float64)
        out[0] = torch.where(live, 0.5 * v * v / torch.where(live, self.w, torch.ones_like(self.w)),
                             torch.zeros_like(v)).sum()
        out[1:] = self._Xz @ v
        return out


def lsq_passes(X, y: torch.Tensor, w: Optional[torch.Tensor], sel: Optional[torch.Tensor]):
    """Per-fit state of the squared-loss l-bfgs path: ``.scalars()``,
    ``.moments()`` (summarizer pass) and ``.evaluate(cf, offset, inv_ystd)`` (one
    ``LeastSquaresAggregator`` pass) — device kernels for device data, fp64 torch on the host."""
    if _on_gpu(X if torch.is_tensor(X) else X.buf):
        from . import device

        return device.LsqPasses(X, y, w, sel)
    return _HostLsq(X, y, w, sel)


_ = (List, native)
