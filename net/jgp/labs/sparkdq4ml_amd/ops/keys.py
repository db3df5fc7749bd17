"""The numpy / torch statement of ``csrc/hip/keys.h`` and ``csrc/hip/hashtable.h``: the one home
of the key rule and the hash on the Python side, shared by ``ops/groupby.py``, ``ops/sort.py`` and
``ops/join.py``.

A key value becomes an order-preserving 64-bit key.  Doubles and floats use the IEEE bits of the
value as a double with ``-0.0`` folded into ``+0.0`` and every NaN mapped to one canonical NaN that
orders above ``+inf`` (Spark 3's grouping rule; 2.4 kept them apart, SPARK-26021); integers are
biased by the sign bit; booleans, and ``uint8`` columns read as 0 / non-zero, are 0 / 1.  Python
holds a key as the *signed* order key (the u64 key with its top bit flipped, as int64), which for
an integer column is the value itself.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["FLOATS", "INTS", "KEY_DTYPES", "I64_MIN", "I64_MAX", "as_np", "is_cuda", "next_pow2", "hash_home",
           "column_np", "skeys_np", "side_np", "keys_to_values", "mixed_radix"]

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
_NAN_BITS = 0x7FF8000000000000
_INF_BITS = 0x7FF0000000000000
FLOATS = (torch.float64, torch.float32)
INTS = (torch.int32, torch.int64, torch.uint8, torch.bool)
KEY_DTYPES = FLOATS + INTS


def as_np(t) -> Optional[np.ndarray]:
    return None if t is None else t.detach().numpy()


def is_cuda(*ts) -> bool:
    return any(t is not None and t.is_cuda for t in ts)


def next_pow2(v: int) -> int:
    return 1 << max(1, int(v - 1).bit_length())


def hash_home(skey: int, capacity: int) -> int:
    """Home slot of a signed order key in a table of ``capacity`` slots (the kernels' hash)."""
    key = (int(skey) ^ I64_MIN) & ((1 << 64) - 1)
    return ((key * 0x9E3779B97F4A7C15 & ((1 << 64) - 1)) >> 20) & (capacity - 1)


def column_np(t) -> np.ndarray:
    """A host column as the loaders of ``keys.h`` read it: a ``uint8`` column is 0 / non-zero."""
    x = as_np(t)
    return x != 0 if x.dtype == np.uint8 else x


def skeys_np(x: np.ndarray, fold: bool) -> np.ndarray:
    """Signed order keys of a column (int64); ``fold``: the grouping rule (``-0.0 == +0.0``), else
    ``-0.0 < +0.0`` (MIN / MAX)."""
    if x.dtype.kind in "iub":
        return x.astype(np.int64)
    with np.errstate(invalid="ignore"):  # (widening a signalling f32 NaN)
        b = x.astype(np.float64).view(np.int64).copy()
    b[(b & I64_MAX) > _INF_BITS] = _NAN_BITS
    if fold:
        b[b == I64_MIN] = 0
    return np.where(b >= 0, b, ~b ^ np.int64(I64_MIN))


def side_np(col, valid, sel) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(keys, live, ok)`` of one key column, as ``load_keys`` of ``keys.h`` gives them: the folded
    signed order keys, the rows inside the selection, and the live rows whose key is not null."""
    k = skeys_np(column_np(col), True)
    live = np.ones(k.size, dtype=bool) if sel is None else (as_np(sel) != 0)
    ok = live if valid is None else (live & (as_np(valid) != 0))
    return k, live, ok


def keys_to_values(keys: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The column values (of ``dtype``) behind signed order keys."""
    if dtype in FLOATS:
        bits = torch.where(keys >= 0, keys, ~(keys ^ I64_MIN))
        return bits.view(torch.float64).to(dtype)
    return keys.to(dtype) if dtype != torch.bool else keys != 0


def mixed_radix(gids: Sequence[torch.Tensor], cards: Sequence[int], who: str) -> Tuple[torch.Tensor, List[int]]:
    """``(code, strides)``: the per-column codes ``gids`` (each below its cardinality in ``cards``)
    combined into one int64, the first column the most significant digit; ``strides[i]`` is the
    weight of column i's digit."""
    total = 1
    for g in cards:
        total *= int(g)
    if total >= 1 << 63:
        raise ValueError(f"{who}: the product of the key columns' cardinalities does not fit in 63 bits")
    code, stride, strides = None, 1, []
    for gid, g in zip(reversed(gids), reversed(cards)):
        term = gid.to(torch.int64) * stride
        code = term if code is None else code + term
        strides.append(stride)
        stride *= int(g)
    strides.reverse()
    return code, strides
