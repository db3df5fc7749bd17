"""Equi-join of two key columns: ``join_pairs``, ``join_mask``, ``join_key_columns`` and the numpy twin.

Device tensors run the ``join.hip`` kernels through ``ops/device.py``; host tensors run the numpy
form below.  The pair order is defined, so the two engines return the same pairs:

* left rows come in row order;
* within one left row, its matching right rows come in right row order;
* ``left_outer`` adds ``(l, -1)`` in the left row's place for a live left row without a match (a
  null left key counts as no match);
* ``full_outer`` does the same, then appends ``(-1, r)`` for every live right row that no left row
  matched, in right row order (a null right key counts as unmatched).

Keys.  The key of a row is the folded order key of ``ops/keys.py`` (``skeys_np`` with
``fold=True``): ``-0.0`` joins ``0.0``, every NaN joins every NaN (Spark's ``NaN = NaN`` is true in
join keys), integers compare as int64, booleans / ``uint8`` as 0 / non-zero.  A null key matches
nothing; a row outside its side's selection vector does not exist.

Sides.  The right side is always the build side (a hash table of ``capacity`` slots, by default
the next power of two at or above twice its row count, 12 bytes per slot plus 4 bytes per right
row) and the left side always probes: **the smaller table belongs on the right**.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .groupby import group_encode
from .keys import KEY_DTYPES, is_cuda, mixed_radix, next_pow2, side_np

__all__ = ["join_pairs", "join_mask", "join_key_columns", "join_limits", "join_capacity", "HOWS"]

# join.h (checked against the extension's join_limits() on the device path)
JOIN_TRIP = 1024
JOIN_TILE = 2048
JOIN_LDS_ROWS = 4096
JOIN_MAX_CAPACITY = 1 << 30

HOWS = ("inner", "left_outer", "full_outer")
MAX_PAIRS = 1 << 31


def join_limits():
    """(rows per block trip, output positions per expansion tile, left rows of a tile staged in
    LDS, largest table capacity)."""
    return JOIN_TRIP, JOIN_TILE, JOIN_LDS_ROWS, JOIN_MAX_CAPACITY


def join_capacity(n_right: int) -> int:
    """Default table capacity for ``n_right`` build rows: the next power of two at or above twice
    the row count (known before the launch, so nothing grows or retries), at most 2^30."""
    return min(next_pow2(2 * max(int(n_right), 1)), JOIN_MAX_CAPACITY)


def too_many_pairs(total: int):
    return ValueError(f"join: the result has {total} pairs; a join returns fewer than 2^31 pairs per call")


def _check_side(key, valid, sel, who: str) -> int:
    if key.dim() != 1:
        raise ValueError(f"join: the {who} key must be 1-D")
    if key.dtype not in KEY_DTYPES:
        raise TypeError(f"join: unsupported key dtype {key.dtype}")
    n = int(key.numel())
    if n >= 1 << 31:
        raise ValueError("join: fewer than 2^31 rows per side")
    for t, what in ((valid, "validity mask"), (sel, "selection")):
        if t is not None and (t.dim() != 1 or int(t.numel()) != n):
            raise ValueError(f"join: the {who} {what} must have one entry per row")
    return n


def _check_join(lkey, rkey, lvalid, rvalid, lsel, rsel, capacity, blocks) -> Optional[int]:
    """Checks both sides and the launch overrides (for both engines); returns the capacity."""
    _check_side(lkey, lvalid, lsel, "left")
    _check_side(rkey, rvalid, rsel, "right")
    if blocks is not None and int(blocks) < 1:
        raise ValueError("blocks must be >= 1")
    if capacity is None:
        return None
    cap = int(capacity)
    if cap < 2 or cap & (cap - 1) or cap > JOIN_MAX_CAPACITY:
        raise ValueError("join: capacity must be a power of two in [2, 2^30]")
    return cap


# ------------------------------------------------------------------------------------------
# numpy twin
# ------------------------------------------------------------------------------------------
def _match_host(lkey, rkey, lvalid, rvalid, lsel, rsel):
    """Per left row the run ``[lo, lo + c)`` of its matches in ``srow``, the live non-null right
    rows in the stable order of their keys."""
    lk, llive, lok = side_np(lkey, lvalid, lsel)
    rk, rlive, rok = side_np(rkey, rvalid, rsel)
    rrows = np.nonzero(rok)[0]
    keys = rk[rrows]
    order = np.argsort(keys, kind="stable")
    skeys, srow = keys[order], rrows[order]
    lo = np.searchsorted(skeys, lk, side="left")
    c = np.searchsorted(skeys, lk, side="right") - lo
    c[~lok] = 0
    return lk, llive, lok, rk, rlive, rok, skeys, srow, lo, c


def _stats_host(skeys, pairs: int):
    distinct = int(np.unique(skeys).size)
    return {"distinct": distinct, "unique_build": distinct == int(skeys.size), "pairs": int(pairs)}


def _pairs_host(lkey, rkey, lvalid, rvalid, lsel, rsel, how, stats):
    lk, llive, lok, rk, rlive, rok, skeys, srow, lo, c = _match_host(lkey, rkey, lvalid, rvalid, lsel, rsel)
    pcnt = c.astype(np.int64)
    if how != "inner":
        pcnt = np.where(c > 0, pcnt, llive.astype(np.int64))
    total = int(pcnt.sum())
    extra = np.zeros(0, dtype=np.int64)
    if how == "full_outer":
        hit = np.isin(rk, lk[lok]) & rok
        extra = np.nonzero(rlive & ~hit)[0].astype(np.int64)
    if total + int(extra.size) >= MAX_PAIRS:  # from the counts alone: nothing of that size exists yet
        raise too_many_pairs(total + int(extra.size))
    li = np.repeat(np.arange(lk.size, dtype=np.int64), pcnt)
    off = np.cumsum(pcnt) - pcnt
    k = np.arange(total, dtype=np.int64) - off[li]
    ri = np.full(total, -1, dtype=np.int64)
    m = c[li] > 0
    ri[m] = srow[lo[li][m] + k[m]]
    if extra.size:
        li = np.concatenate([li, np.full(extra.size, -1, dtype=np.int64)])
        ri = np.concatenate([ri, extra])
    if stats is not None:
        stats.append(_stats_host(skeys, li.size))
    return torch.from_numpy(li), torch.from_numpy(ri)


# ------------------------------------------------------------------------------------------
# the API
# ------------------------------------------------------------------------------------------
def join_pairs(lkey: torch.Tensor, rkey: torch.Tensor, lvalid=None, rvalid=None, lsel=None, rsel=None, how: str = "inner",
               capacity: Optional[int] = None, blocks: Optional[int] = None,
               stats: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The pairs ``(li, ri)`` (int64, on the inputs' device, ``-1`` for the missing side) of the
    equi-join of the key columns ``lkey`` and ``rkey`` (f64 / f32 / i32 / i64 / bool / u8; the two
    dtypes may differ inside one class), in the order defined at the top of this module.  ``how``:
    ``inner``, ``left_outer`` or ``full_outer``.  The right side builds the table: put the smaller
    side there.  ``capacity`` overrides the table's slot count (a power of two; it must hold the
    right side's distinct keys plus one empty slot, else ``RuntimeError``), ``blocks`` overrides
    every grid of the device passes.  ``stats`` (a list) receives ``{"distinct", "unique_build",
    "capacity", "pairs"}`` (the numpy twin: no ``capacity``).  Fewer than 2^31 rows per side and
    fewer than 2^31 pairs (``ValueError`` naming the count, before anything of that size exists)."""
    if how not in HOWS:
        raise ValueError(f"join: how must be one of {', '.join(HOWS)}, got {how!r}")
    cap = _check_join(lkey, rkey, lvalid, rvalid, lsel, rsel, capacity, blocks)
    if is_cuda(lkey, rkey, lvalid, rvalid, lsel, rsel):
        from . import device

        return device.join_pairs(lkey, rkey, lvalid, rvalid, lsel, rsel, how, cap, blocks, stats)
    return _pairs_host(lkey, rkey, lvalid, rvalid, lsel, rsel, how, stats)


def join_mask(lkey: torch.Tensor, rkey: torch.Tensor, lvalid=None, rvalid=None, lsel=None, rsel=None,
              capacity: Optional[int] = None, blocks: Optional[int] = None, stats: Optional[list] = None) -> torch.Tensor:
    """bool ``[n_left]``: the live left rows whose key has a match on the right (``left_semi``; the
    caller complements it within the selection for ``left_anti``).  One build pass and one probe
    pass: nothing is expanded and no row is moved."""
    cap = _check_join(lkey, rkey, lvalid, rvalid, lsel, rsel, capacity, blocks)
    if is_cuda(lkey, rkey, lvalid, rvalid, lsel, rsel):
        from . import device

        return device.join_mask(lkey, rkey, lvalid, rvalid, lsel, rsel, cap, blocks, stats)
    *_, skeys, _, _, c = _match_host(lkey, rkey, lvalid, rvalid, lsel, rsel)
    if stats is not None:
        stats.append(_stats_host(skeys, int((c > 0).sum())))
    return torch.from_numpy(c > 0)


def join_key_columns(lcols: Sequence[torch.Tensor], rcols: Sequence[torch.Tensor], lvalids=None, rvalids=None, lsel=None,
                     rsel=None):
    """``(lkey, lvalid, rkey, rvalid)``: a key of several columns (or of columns the kernels cannot
    compare directly) reduced to one int64 key and one validity mask per side.  Each column pair
    (of one dtype) is encoded jointly with ``group_encode`` over the concatenation of the two sides,
    so that equal values get equal codes on both sides; the codes are combined in mixed radix, the
    first column the most significant digit, as ``group_encode_columns`` does.  A row with any null
    component is null.  This is the slower path: a single key column of a kernel dtype needs no
    pre-pass and goes straight to ``join_pairs``."""
    lcols, rcols = list(lcols), list(rcols)
    if not lcols or len(lcols) != len(rcols):
        raise ValueError("join: one right key column per left key column, at least one")
    k = len(lcols)
    lvalids = [None] * k if lvalids is None else list(lvalids)
    rvalids = [None] * k if rvalids is None else list(rvalids)
    nl, nr = int(lcols[0].numel()), int(rcols[0].numel())
    dev = lcols[0].device
    ones = lambda n: torch.ones(n, dtype=torch.bool, device=dev)  # noqa: E731
    sel = None
    if lsel is not None or rsel is not None:
        sel = torch.cat([ones(nl) if lsel is None else lsel.to(torch.bool), ones(nr) if rsel is None else rsel.to(torch.bool)])
    gids: List[torch.Tensor] = []
    cards: List[int] = []
    for lc, rc, lv, rv in zip(lcols, rcols, lvalids, rvalids):
        if lc.dtype != rc.dtype:
            raise TypeError(f"join: the two sides of a key column must share a dtype, got {lc.dtype} and {rc.dtype}")
        valid = None
        if lv is not None or rv is not None:
            valid = torch.cat([ones(nl) if lv is None else lv.to(torch.bool), ones(nr) if rv is None else rv.to(torch.bool)])
        e = group_encode(torch.cat([lc, rc]), valid, sel)
        gids.append(e.gid)
        cards.append(int(e.G))
    code, _ = mixed_radix([g.clamp(min=0) for g in gids], cards, "join")
    ok = None
    for gid in gids:
        present = gid > 0  # 0: a null component, -1: a dead row
        ok = present if ok is None else (ok & present)
    return code[:nl].contiguous(), ok[:nl].contiguous(), code[nl:].contiguous(), ok[nl:].contiguous()
