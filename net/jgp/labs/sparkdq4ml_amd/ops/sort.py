"""Stable multi-column sort: ``sort_permutation`` and its numpy twin.

Device tensors run the ``sort.hip`` kernels through ``ops/device.py``; host tensors run the numpy
form below, which is the same algorithm: an LSD radix sort of (order key, row index) pairs with
8-bit digits, over the sort columns from last to first, so that stability makes the earlier columns
dominate.  A stable sort has one right answer, so the two engines return the same permutation.

Keys.  The order key of a value is the folded key of ``ops/keys.py`` (``skeys_np`` with
``fold=True``): ``-0.0`` equals ``0.0`` and every NaN is one value above ``+inf``, which is Spark's
ordering of doubles; integers are biased by the sign bit; booleans (and ``uint8`` columns, read as
0 / non-zero) are 0 / 1.  A descending order complements the key.  A null row has key 0 and a null
digit of 1: the null digit is the most significant one, runs last, and its two bins are ordered
by ``nulls_first``.  A digit that is constant over the live non-null rows is skipped: an ``int32``
column runs at most 4 of the 8 byte passes.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .keys import I64_MIN, KEY_DTYPES, as_np, is_cuda, side_np

__all__ = ["sort_permutation", "sort_limits", "NULL_DIGIT"]

# sort.h (checked against the extension's sort_limits() on the device path)
SORT_THREADS = 256
SORT_RUN = 8
SORT_TILE = SORT_THREADS * SORT_RUN
SORT_BITS = 8
SORT_DIGITS = 64 // SORT_BITS
NULL_DIGIT = SORT_DIGITS  # the pass after the key bytes


def sort_limits():
    """(threads per block, keys per thread, tile in rows, digit width)."""
    return SORT_THREADS, SORT_RUN, SORT_TILE, SORT_BITS


def _flags(v, k: int, what: str) -> List[bool]:
    if v is None:
        return [True] * k
    if isinstance(v, (bool, np.bool_)):
        return [bool(v)] * k
    v = [bool(x) for x in v]
    if len(v) != k:
        raise ValueError(f"sort: {what} must be one flag or one per sort column ({k}), got {len(v)}")
    return v


def _sort_host(cols, valids, sel, ascending, nulls_first, stats) -> torch.Tensor:
    n = int(cols[0].numel())
    perm = np.arange(n, dtype=np.int64) if sel is None else np.nonzero(as_np(sel) != 0)[0].astype(np.int64)
    m = int(perm.size)
    for c, v, asc, nf in reversed(list(zip(cols, valids, ascending, nulls_first))):
        k, _, ok = side_np(c, v, None)
        key = (k[perm] ^ np.int64(I64_MIN)).view(np.uint64)
        if not asc:
            key = ~key
        null = ~ok[perm]
        key[null] = 0
        live = []
        for d in range(SORT_DIGITS):
            digit = ((key >> np.uint64(SORT_BITS * d)) & np.uint64(0xFF)).astype(np.uint8)
            seen = digit[~null]  # (a null's key bytes never decide: the null digit parts it from the rest)
            if seen.size > 1 and seen.min() != seen.max():  # more than one occupied bin
                o = np.argsort(digit, kind="stable")
                key, perm, null = key[o], perm[o], null[o]
                live.append(d)
        if null.any() and not null.all():
            o = np.argsort(~null if nf else null, kind="stable")
            key, perm, null = key[o], perm[o], null[o]
            live.append(NULL_DIGIT)
        if stats is not None:
            stats.append({"live": live})
    return torch.from_numpy(perm)


def sort_permutation(cols: Sequence[torch.Tensor], valids=None, sel: Optional[torch.Tensor] = None, ascending=None,
                     nulls_first=None, blocks: Optional[int] = None, stats: Optional[list] = None) -> torch.Tensor:
    """Row indices (int64 ``[m]``) of the live rows of ``sel`` in the stable sorted order of the
    columns ``cols`` (f64 / f32 / i32 / i64 / bool / u8, first column most significant).
    ``ascending`` / ``nulls_first``: one flag or one per column; the defaults are ascending, and
    nulls first for an ascending column, last for a descending one.  ``blocks`` overrides the grid
    of the device passes.  ``stats`` (a list) receives ``{"live": [digits whose pass ran]}`` per
    column, in the order the columns were processed (last first)."""
    cols = list(cols)
    if not cols:
        raise ValueError("sort: no sort column")
    k = len(cols)
    valids = [None] * k if valids is None else list(valids)
    if len(valids) != k:
        raise ValueError("sort: one validity mask (or None) per column")
    ascending = _flags(ascending, k, "ascending")
    nulls_first = list(ascending) if nulls_first is None else _flags(nulls_first, k, "nulls_first")
    n = int(cols[0].numel())
    for c in cols:
        if c.dim() != 1 or int(c.numel()) != n:
            raise ValueError("sort: columns must be 1-D and of one length")
        if c.dtype not in KEY_DTYPES:
            raise TypeError(f"sort: unsupported column dtype {c.dtype}")
    if n >= 1 << 31:
        raise ValueError("sort: fewer than 2^31 rows per call")
    if is_cuda(*cols, *valids, sel):
        from . import device

        return device.sort_permutation(cols, valids, sel, ascending, nulls_first, blocks, stats)
    for t, what in [(sel, "the selection")] + [(v, "a validity mask") for v in valids]:
        if t is not None and (t.dim() != 1 or int(t.numel()) != n):
            raise ValueError(f"sort: {what} must have one entry per row")
    return _sort_host(cols, valids, sel, ascending, nulls_first, stats)
