"""Window functions over the sorted positions of one window specification: the five contracts of
``csrc/hip/window.hip`` with their numpy twins, and the finalisation both engines share.

The caller sorts once (``sort_permutation`` over the partition columns, then the order columns):
position ``i`` holds row ``perm[i]``.  Device tensors run the kernels through ``ops/device.py``;
host tensors run the numpy forms below.  Every raw output is integer work, so the two engines give
the same bits:

``window_heads``   one byte per position: bit 0 first of its partition, bit 1 first of its peer group.
``window_bounds``  int32 ``[5, m]``: ``part_start``, ``peer_start`` (forward max-scans of the head
                   positions), ``part_end``, ``peer_end`` (backward min-scans of the inclusive last
                   positions), ``dense`` (inclusive add-scan of the peer heads).
``window_prefix``  int64 ``[words, m]``: *unsegmented* inclusive prefix sums of the value words.  A
                   double sum uses the four fixed-point limbs of ``ops/groupby.py`` with the same
                   exponent, plus the counts of NaN, +inf and -inf.  A limb is a signed 32-bit value
                   and a call has fewer than 2^31 positions, so no prefix overflows, and the sum over
                   any frame ``[lo, hi]`` is ``P[hi] - P[lo - 1]`` word by word: the words
                   ``group_agg`` accumulates over those rows.
``window_minmax``  int64 ``[m]``: segmented inclusive min / max scan of the unfolded u64 order key,
                   forward or backward, restarting at the partition heads.
``window_finish``  int64 ``[n, words]``: per position the frame from the bounds, prefix differences
                   or scan picks, the ranking integers, lag / lead source rows; scattered to row
                   ``perm[i]``.  Rows outside the permutation stay 0.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .groupby import finalize_sum
from .keys import I64_MIN, KEY_DTYPES, as_np, column_np, is_cuda, keys_to_values, side_np, skeys_np

__all__ = ["ROWS", "COUNT", "SUM_I", "SUM_F", "O_DIFF", "O_PICK_HI", "O_PICK_LO", "O_ROW_NUMBER", "O_RANK", "O_DENSE_RANK",
           "O_PART_SIZE", "O_PEER_END", "O_SHIFT", "window_limits", "word_count", "window_heads", "window_bounds",
           "window_prefix", "window_minmax", "window_finish", "sum_from_words", "minmax_from_keys", "percent_rank",
           "cume_dist", "ntile"]

ROWS, COUNT, SUM_I, SUM_F = range(4)  # (the codes of the ops/groupby.py ops they accumulate like)
(O_DIFF, O_PICK_HI, O_PICK_LO, O_ROW_NUMBER, O_RANK, O_DENSE_RANK, O_PART_SIZE, O_PEER_END, O_SHIFT) = range(9)

# window.h (checked against the extension's window_limits() on the device path)
WINDOW_THREADS = 256
WINDOW_RUN = 8
WINDOW_TILE = WINDOW_THREADS * WINDOW_RUN
WINDOW_MAX_KEYS = 8
WINDOW_MAX_WORDS = 8
SUM_WORDS = 7
_OFF_LIMIT = 1 << 31  # frame offsets and shift distances are clamped to +-2^31: past any partition


def window_limits():
    """(threads per block, positions per thread, tile in positions, key columns per heads launch,
    words per prefix pass / finish launch)."""
    return WINDOW_THREADS, WINDOW_RUN, WINDOW_TILE, WINDOW_MAX_KEYS, WINDOW_MAX_WORDS


def word_count(op: int) -> int:
    return SUM_WORDS if op == SUM_F else 1


def _clamp(v: int) -> int:
    return max(-_OFF_LIMIT, min(_OFF_LIMIT, int(v)))


def _check_perm(perm: torch.Tensor, n: int):
    if perm.dtype != torch.int64 or perm.dim() != 1:
        raise ValueError("window: the permutation must be a 1-D int64 tensor")
    if n >= 1 << 31:
        raise ValueError("window: fewer than 2^31 rows per call")
    if int(perm.numel()) > n:
        raise ValueError("window: more positions than rows")


def _check_cols(cols, valids, n: int, who: str):
    for c in cols:
        if c is None:
            continue
        if c.dim() != 1 or int(c.numel()) != n:
            raise ValueError(f"{who}: columns must be 1-D and of one length")
        if c.dtype not in KEY_DTYPES:
            raise TypeError(f"{who}: unsupported column dtype {c.dtype}")
    for v in valids:
        if v is not None and (v.dim() != 1 or int(v.numel()) != n):
            raise ValueError(f"{who}: a validity mask must have one entry per row")


# ------------------------------------------------------------------------------------------
# heads
# ------------------------------------------------------------------------------------------
def window_heads(part_cols, part_valids, order_cols, order_valids, perm: torch.Tensor, n: int,
                 blocks: Optional[int] = None) -> torch.Tensor:
    """uint8 ``[m]``: position i is a partition head (bit 0, and bit 1 with it) when ``i == 0`` or
    the folded key or the null flag of any partition column differs between positions i and i - 1;
    a peer head (bit 1) when any order column differs as well.  Two nulls are equal."""
    cols = list(part_cols) + list(order_cols)
    valids = list(part_valids) + list(order_valids)
    part = [True] * len(part_cols) + [False] * len(order_cols)
    if len(valids) != len(cols):
        raise ValueError("window_heads: one validity mask (or None) per column")
    _check_perm(perm, n)
    _check_cols(cols, valids, n, "window_heads")
    if is_cuda(perm, *cols, *valids):
        from . import device

        return device.window_heads(cols, valids, part, perm, n, blocks)
    p = as_np(perm)
    m = int(p.size)
    heads = np.zeros(m, dtype=np.uint8)
    if m:
        heads[0] = 3
    for c, v, isp in zip(cols, valids, part):
        k, _, ok = side_np(c, v, None)
        k, ok = k[p], ok[p]
        diff = (ok[1:] != ok[:-1]) | (ok[1:] & ok[:-1] & (k[1:] != k[:-1]))
        heads[1:] |= np.where(diff, 3 if isp else 2, 0).astype(np.uint8)
    return torch.from_numpy(heads)


# ------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------
def window_bounds(heads: torch.Tensor, blocks: Optional[int] = None) -> torch.Tensor:
    """int32 ``[5, m]``: ``part_start``, ``peer_start``, ``part_end``, ``peer_end`` (inclusive
    positions) and ``dense`` (the peer heads at or before the position)."""
    if heads.dtype != torch.uint8 or heads.dim() != 1:
        raise ValueError("window_bounds: heads must be a 1-D uint8 tensor")
    if heads.is_cuda:
        from . import device

        return device.window_bounds(heads, blocks)
    h = as_np(heads)
    m = int(h.size)
    idx = np.arange(m, dtype=np.int64)
    big = np.int64(0xFFFFFFFF)
    out = np.zeros((5, m), dtype=np.int64)
    if m:
        after = np.concatenate([h[1:], np.array([3], dtype=np.uint8)])  # the position after the last starts a partition
        out[0] = np.maximum.accumulate(np.where(h & 1, idx, 0))
        out[1] = np.maximum.accumulate(np.where(h & 2, idx, 0))
        out[2] = np.minimum.accumulate(np.where(after & 1, idx, big)[::-1])[::-1]
        out[3] = np.minimum.accumulate(np.where(after & 2, idx, big)[::-1])[::-1]
        out[4] = np.cumsum((h >> 1) & 1)
    return torch.from_numpy(out.astype(np.uint32).view(np.int32))


# ------------------------------------------------------------------------------------------
# prefix
# ------------------------------------------------------------------------------------------
def _slot_words(op, col, valid, e, p) -> List[np.ndarray]:
    m = int(p.size)
    ok = np.ones(m, dtype=bool) if (valid is None or op == ROWS) else (as_np(valid) != 0)[p]
    if op in (ROWS, COUNT):
        return [ok.astype(np.int64)]
    x = column_np(col)[p]
    if op == SUM_I:
        return [np.where(ok, x.astype(np.int64), 0)]
    with np.errstate(over="ignore", invalid="ignore"):
        xs = x.astype(np.float64)
        fin = ok & np.isfinite(xs)
        t = np.ldexp(np.where(fin, xs, 0.0), 32 - int(e))
        words = []
        for _ in range(4):
            c = np.trunc(t)
            words.append(c.astype(np.int64))
            t = np.ldexp(t - c, 32)
    words += [(ok & np.isnan(xs)).astype(np.int64), (ok & (xs == np.inf)).astype(np.int64),
              (ok & (xs == -np.inf)).astype(np.int64)]
    return words


def window_prefix(slots, perm: torch.Tensor, n: int, blocks: Optional[int] = None) -> Tuple[torch.Tensor, List[int]]:
    """``(P, offsets)``: ``P`` int64 ``[words, m]``, the inclusive prefix sums over the positions
    of the words of ``slots`` = ``(kind, column, valid, e)`` (``ROWS``: +1 per position; ``COUNT``:
    +1 per non-null row; ``SUM_I``: the value, wrapping; ``SUM_F``: the four limbs of ``x * 2^(128 -
    e)`` and the counts of NaN, +inf, -inf); ``offsets[i]`` is the first word of ``slots[i]``."""
    slots = [tuple(s) + (None,) * (4 - len(s)) for s in slots]
    if not slots:
        raise ValueError("window_prefix: no slot")
    _check_perm(perm, n)
    _check_cols([s[1] for s in slots], [s[2] for s in slots], n, "window_prefix")
    offsets, w = [], 0
    for s in slots:
        if s[0] not in (ROWS, COUNT, SUM_I, SUM_F):
            raise ValueError("window_prefix: unknown word kind")
        if s[0] in (SUM_I, SUM_F) and s[1] is None:
            raise ValueError("window_prefix: a sum needs its column")
        if s[0] == SUM_I and s[1].dtype in (torch.float64, torch.float32):
            raise ValueError("window_prefix: SUM_I of a float column")
        offsets.append(w)
        w += word_count(s[0])
    if is_cuda(perm, *(s[1] for s in slots), *(s[2] for s in slots)):
        from . import device

        return device.window_prefix(slots, perm, n, w, blocks), offsets
    p = as_np(perm)
    rows = []
    for op, col, valid, e in slots:
        rows += _slot_words(op, col, valid, e or 0, p)
    P = np.cumsum(np.stack(rows), axis=1, dtype=np.int64) if p.size else np.zeros((w, 0), dtype=np.int64)
    return torch.from_numpy(P), offsets


# ------------------------------------------------------------------------------------------
# min / max
# ------------------------------------------------------------------------------------------
def _seg_cummin(key: np.ndarray, flag: np.ndarray) -> np.ndarray:
    """Inclusive running minimum of ``key`` (uint64) restarting where ``flag`` is set (position 0
    always restarts): ranks of the keys, offset so that every later segment lies below every
    earlier one, then one running minimum."""
    uniq, r = np.unique(key, return_inverse=True)
    seg = np.cumsum(flag.astype(np.int64))
    seg = seg[-1] - seg  # descending with the position
    U = np.int64(uniq.size)
    run = np.minimum.accumulate(seg * U + r.astype(np.int64))
    return uniq[run - seg * U]


def window_minmax(col: torch.Tensor, valid, perm: torch.Tensor, heads: torch.Tensor, is_max: bool, backward: bool,
                  blocks: Optional[int] = None) -> torch.Tensor:
    """int64 ``[m]`` (the bits of u64 order keys, ``-0.0 < +0.0`` as ``MIN`` / ``MAX`` of
    ``ops/groupby.py``): the min (``is_max``: max) of the keys of the non-null rows from the first
    position of the partition to position i (``backward``: from i to the last position); the
    identity (all ones; max: 0) where there is none."""
    n = int(col.numel())
    _check_perm(perm, n)
    _check_cols([col], [valid], n, "window_minmax")
    if int(heads.numel()) != int(perm.numel()) or heads.dtype != torch.uint8:
        raise ValueError("window_minmax: heads must be uint8 with one entry per position")
    if is_cuda(col, valid, perm, heads):
        from . import device

        return device.window_minmax(col, valid, perm, heads, bool(is_max), bool(backward), blocks)
    p, h = as_np(perm), as_np(heads)
    m = int(p.size)
    if m == 0:
        return torch.zeros(0, dtype=torch.int64)
    key = (skeys_np(column_np(col)[p], False) ^ np.int64(I64_MIN)).view(np.uint64)
    if is_max:
        key = ~key
    if valid is not None:
        key = np.where((as_np(valid) != 0)[p], key, np.uint64(0xFFFFFFFFFFFFFFFF))
    flag = (h & 1) != 0
    if backward:
        flag = np.concatenate([flag[1:], np.array([True])])[::-1]
        out = _seg_cummin(key[::-1], flag)[::-1].copy()
    else:
        out = _seg_cummin(key, flag)
    if is_max:
        out = ~out
    return torch.from_numpy(out.view(np.int64))


# ------------------------------------------------------------------------------------------
# finish
# ------------------------------------------------------------------------------------------
def window_finish(bounds: torch.Tensor, perm: torch.Tensor, n: int, frame, outs, blocks: Optional[int] = None) -> torch.Tensor:
    """int64 ``[n, words]``: row ``perm[i]`` receives the words of position i.

    ``frame`` = ``(is_range, lo, hi)``, ``lo`` / ``hi`` None: unbounded.  A rows frame clamps
    ``i + lo`` and ``i + hi`` to the partition; a range frame takes only 0 (the current row's
    peers).  ``lo > hi`` is an empty frame.  ``outs`` = ``(kind, source, arg)`` per word:
    ``O_DIFF`` (source: one row of ``window_prefix``) ``P[hi] - P[lo - 1]``; ``O_PICK_HI`` /
    ``O_PICK_LO`` (source: a ``window_minmax`` scan) its value at hi / lo; both 0 over an empty
    frame.  ``O_ROW_NUMBER`` ``i - part_start + 1``, ``O_RANK`` ``peer_start - part_start + 1``,
    ``O_DENSE_RANK`` ``dense[i] - dense[part_start] + 1``, ``O_PART_SIZE``, ``O_PEER_END``
    ``peer_end - part_start + 1``; ``O_SHIFT`` (arg: signed distance d) the row at position
    ``i + d``, -1 outside the partition."""
    is_range, lo_off, hi_off = frame
    if is_range and any(v not in (None, 0) for v in (lo_off, hi_off)):
        raise ValueError("window_finish: a range frame is bounded by the partition or the current row's peers")
    outs = [tuple(o) + (None,) * (3 - len(o)) for o in outs]
    if not outs:
        raise ValueError("window_finish: no output word")
    _check_perm(perm, n)
    m = int(perm.numel())
    if bounds.dtype != torch.int32 or tuple(bounds.shape) != (5, m):
        raise ValueError("window_finish: bounds must be int32 [5, m]")
    for kind, src, _ in outs:
        if kind not in range(9):
            raise ValueError("window_finish: unknown output kind")
        if kind <= O_PICK_LO and (src is None or src.dtype != torch.int64 or tuple(src.shape) != (m,)):
            raise ValueError("window_finish: a prefix difference or a pick needs an int64 [m] source")
    lo_c, hi_c = _clamp(lo_off or 0), _clamp(hi_off or 0)
    outs = [(k, s, _clamp(a or 0)) for k, s, a in outs]
    if is_cuda(bounds, perm, *(o[1] for o in outs)):
        from . import device

        return device.window_finish(bounds, perm, n, (bool(is_range), lo_off is None, hi_off is None, lo_c, hi_c), outs, blocks)
    p = as_np(perm)
    b = as_np(bounds).view(np.uint32).astype(np.int64)
    ps, qs, pe, qe, dense = b
    i = np.arange(m, dtype=np.int64)
    if is_range:
        lo = ps if lo_off is None else qs
        hi = pe if hi_off is None else qe
    else:
        lo = ps if lo_off is None else np.maximum(i + lo_c, ps)
        hi = pe if hi_off is None else np.minimum(i + hi_c, pe)
    some = lo <= hi
    out = np.zeros((n, len(outs)), dtype=np.int64)
    if m == 0:
        return torch.from_numpy(out)
    lo_s, hi_s = np.where(some, lo, 0), np.where(some, hi, 0)
    for w, (kind, src, arg) in enumerate(outs):
        if kind == O_DIFF:
            P = as_np(src)
            with np.errstate(over="ignore"):
                v = np.where(some, P[hi_s] - np.where(lo_s > 0, P[np.maximum(lo_s - 1, 0)], 0), 0)
        elif kind == O_PICK_HI:
            v = np.where(some, as_np(src)[hi_s], 0)
        elif kind == O_PICK_LO:
            v = np.where(some, as_np(src)[lo_s], 0)
        elif kind == O_ROW_NUMBER:
            v = i - ps + 1
        elif kind == O_RANK:
            v = qs - ps + 1
        elif kind == O_DENSE_RANK:
            v = dense - dense[ps] + 1
        elif kind == O_PART_SIZE:
            v = pe - ps + 1
        elif kind == O_PEER_END:
            v = qe - ps + 1
        else:
            j = i + arg
            inside = (j >= ps) & (j <= pe)
            v = np.where(inside, p[np.where(inside, j, 0)], -1)
        out[p, w] = v
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------
# finalisation (row-sized torch code, the same for both engines)
# ------------------------------------------------------------------------------------------
def sum_from_words(words: torch.Tensor, e: int) -> torch.Tensor:
    """The double sum behind the seven ``SUM_F`` words of a frame (int64 ``[rows, 7]``): the flag
    word of ``finalize_sum`` is built from the three special-value counts."""
    flags = (words[:, 4] > 0).to(torch.int64) | ((words[:, 5] > 0).to(torch.int64) << 1) | ((words[:, 6] > 0).to(torch.int64) << 2)
    return finalize_sum(words[:, :4], flags, e)


def minmax_from_keys(raw: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The column values behind the u64 order keys of ``window_minmax`` (held as int64 bits)."""
    return keys_to_values(raw ^ I64_MIN, dtype)


def percent_rank(rank: torch.Tensor, size: torch.Tensor) -> torch.Tensor:
    d = (size - 1).to(torch.float64)
    return torch.where(size > 1, (rank - 1).to(torch.float64) / torch.where(size > 1, d, torch.ones_like(d)),
                       torch.zeros_like(d))


def cume_dist(peer_end: torch.Tensor, size: torch.Tensor) -> torch.Tensor:
    return peer_end.to(torch.float64) / torch.clamp(size, min=1).to(torch.float64)


def ntile(row_number: torch.Tensor, size: torch.Tensor, buckets: int) -> torch.Tensor:
    """Spark's NTile: the first ``size % buckets`` buckets hold one row more."""
    nb = int(buckets)
    q = torch.div(size, nb, rounding_mode="floor")
    rem = size - q * nb
    r0 = row_number - 1
    cut = rem * (q + 1)
    small = torch.div(r0, q + 1, rounding_mode="floor") + 1
    large = rem + torch.div(r0 - cut, torch.clamp(q, min=1), rounding_mode="floor") + 1
    return torch.where(r0 < cut, small, large)
