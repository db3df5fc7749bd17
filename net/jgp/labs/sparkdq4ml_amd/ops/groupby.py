"""Grouped aggregation on integer words: ``group_encode`` / ``group_agg`` and their finalisation.

Device tensors run the ``groupby.hip`` kernels through ``ops/device.py``; host tensors run the
numpy forms below, which do exactly the kernels' arithmetic: the raw accumulators of the two
engines are bit-identical, and so is every result built from them (the finalisation is one piece
of torch integer code for both).

Keys.  A key value becomes the order-preserving 64-bit key of ``ops/keys.py`` (the statement of
``keys.h``), held as the *signed* order key.  Null keys form one group, slot 0; slots ascend with
the key.

Accumulators.  Every word is an int64 updated by an integer add / or / max / min, so the result
does not depend on the grid, the schedule or a shard split.  A double sum is kept in fixed point:
with ``e = frexp(M)[1]`` of the largest finite ``|x|`` of the column, ``x * 2^(128 - e)`` is cut
into four signed 32-bit limbs (every step exact in f64), limb k is an i64 add, and NaN / +inf /
-inf set flag bits instead.  Values at or above ``2^(e - 75)`` in magnitude are represented
exactly, smaller ones are truncated toward zero by less than ``2^(e - 128)`` each.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .keys import (I64_MAX, I64_MIN, INTS, KEY_DTYPES, as_np, column_np, hash_home, is_cuda, keys_to_values,
                   mixed_radix, next_pow2, side_np, skeys_np)

__all__ = ["ROWS", "COUNT", "SUM_I", "SUM_F", "MIN", "MAX", "FIRST", "ABSMAX", "GroupEncoding", "group_limits",
           "group_encode", "group_encode_columns", "group_agg", "group_scale", "op_words", "word_kinds",
           "finalize_sum", "keys_to_values", "hash_home"]

ROWS, COUNT, SUM_I, SUM_F, MIN, MAX, FIRST, ABSMAX = range(8)
K_ADD, K_OR, K_MAX, K_MIN = range(4)

# groupby.h (checked against the extension's group_limits() on the device path)
GROUP_TRIP = 1024
GROUP_LDS_WORDS = 4096
GROUP_MAX_SLOTS = 8
GROUP_DEFAULT_CAPACITY = 1 << 16
GROUP_DIRECT_CAP = 1 << 20

_INF_BITS = 0x7FF0000000000000


def group_limits():
    """(rows per trip, LDS budget in words, aggregate slots per call, default table capacity,
    direct-range cap)."""
    return GROUP_TRIP, GROUP_LDS_WORDS, GROUP_MAX_SLOTS, GROUP_DEFAULT_CAPACITY, GROUP_DIRECT_CAP


def op_words(op: int) -> int:
    return 5 if op == SUM_F else 1


def word_kinds(ops: Sequence[int]) -> List[int]:
    """How each word of a group's accumulator row is combined (add / or / max / min)."""
    out = []
    for op in ops:
        if op == SUM_F:
            out += [K_ADD] * 4 + [K_OR]
        elif op in (MIN, FIRST):
            out.append(K_MIN)
        elif op in (MAX, ABSMAX):
            out.append(K_MAX)
        else:
            out.append(K_ADD)
    return out


def _identity(kinds) -> np.ndarray:
    return np.array([-1 if k == K_MIN else 0 for k in kinds], dtype=np.int64)


# ------------------------------------------------------------------------------------------
# numpy twins (columns are read as the kernels' loaders read them: keys.column_np)
# ------------------------------------------------------------------------------------------
def _agg_host(gid, G, ops, cols, valids, es, sel, n, row_offset, init):
    acc = np.tile(np.asarray(init, dtype=np.int64).reshape(1, -1), (G, 1))
    live = np.ones(n, dtype=bool) if sel is None else (as_np(sel) != 0)
    g = np.zeros(n, dtype=np.int64)
    if gid is not None:
        g = as_np(gid).astype(np.int64)
        live = live & (g >= 0) & (g < G)
    w = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for op, c, v, e in zip(ops, cols, valids, es):
            ok = live if (v is None or op in (ROWS, FIRST)) else live & (as_np(v) != 0)
            x = None if c is None else column_np(c)
            if op in (ROWS, COUNT):
                np.add.at(acc[:, w], g[ok], 1)
            elif op == SUM_I:
                np.add.at(acc[:, w], g[ok], x[ok].astype(np.int64))
            elif op in (MIN, MAX):
                k = skeys_np(x[ok], False)
                m = np.full(G, I64_MAX if op == MIN else I64_MIN, dtype=np.int64)
                (np.minimum if op == MIN else np.maximum).at(m, g[ok], k)
                acc[:, w] = m ^ np.int64(I64_MIN)
            elif op == FIRST:
                m = acc[:, w].view(np.uint64)
                np.minimum.at(m, g[ok], (np.nonzero(ok)[0] + int(row_offset)).astype(np.uint64))
            elif op == ABSMAX:
                b = x[ok].astype(np.float64).view(np.int64) & np.int64(I64_MAX)
                fin = b < _INF_BITS
                np.maximum.at(acc[:, w], g[ok][fin], b[fin])
            else:  # SUM_F
                xs, gs = x[ok].astype(np.float64), g[ok]
                fin = np.isfinite(xs)
                t = np.ldexp(xs[fin], 32 - int(e))
                for k in range(4):
                    c_k = np.trunc(t)
                    np.add.at(acc[:, w + k], gs[fin], c_k.astype(np.int64))
                    t = np.ldexp(t - c_k, 32)
                flag = np.where(np.isnan(xs), 1, np.where(xs > 0, 2, 4))[~fin].astype(np.int64)
                np.bitwise_or.at(acc[:, w + 4], gs[~fin], flag)
            w += op_words(op)
    return torch.from_numpy(acc)


def _direct_host(col, valid, sel, base, span):
    x, live, ok = side_np(col, valid, sel)  # (an integer's key is its value)
    off = x - np.int64(base)  # (wraps like the kernel's unsigned subtraction)
    inside = (off >= 0) & (off < span)
    g = np.where(~live, -1, np.where(~ok, 0, np.where(inside, off + 1, -1)))
    return torch.from_numpy(g.astype(np.int32))


def _hash_host(col, valid, sel, union):
    k, live, ok = side_np(col, valid, sel)
    keys = torch.from_numpy(np.unique(k[ok]))
    if union is not None:
        keys = union(keys)
    g = np.where(~live, -1, np.where(~ok, 0, np.searchsorted(keys.numpy(), k) + 1))
    return torch.from_numpy(g.astype(np.int32)), keys


# ------------------------------------------------------------------------------------------
# group_agg
# ------------------------------------------------------------------------------------------
def _n_rows(gid, sel, slots) -> int:
    for t in (gid, sel):
        if t is not None:
            return int(t.numel())
    for s in slots:
        for t in (s[1], s[2]):
            if t is not None:
                return int(t.numel())
    raise ValueError("group_agg: nothing tells the row count (no gid, selection, column or mask)")


def _agg_call(gid, G, ops, cols, valids, es, sel, n, row_offset, blocks):
    init = _identity(word_kinds(ops))
    if is_cuda(gid, sel, *cols, *valids):
        from . import device

        return device.group_agg_raw(gid, G, ops, cols, valids, es, sel, n, row_offset, init, blocks)
    return _agg_host(gid, G, ops, cols, valids, es, sel, n, row_offset, init)


def group_scale(cols, valids, sel, blocks: Optional[int] = None, reduce=None) -> List[int]:
    """The fixed-point exponent of each column: ``frexp(M)[1]`` of the largest finite ``|x|`` among
    its live non-null rows over all groups (and, through ``reduce``, all ranks); 0 when there is
    none.  One ``ABSMAX`` pass and one host read."""
    if not cols:
        return []
    acc, off = group_agg(None, 1, [(ABSMAX, c, v, 0) for c, v in zip(cols, valids)], sel, blocks=blocks, reduce=reduce)
    bits = acc[0, off].cpu().numpy().astype(np.int64)
    return [int(x) for x in np.frexp(bits.view(np.float64))[1]]  # (frexp(0) = (0, 0))


def group_agg(gid, G: int, slots, sel=None, row_offset: int = 0, blocks: Optional[int] = None, reduce=None, n=None):
    """Raw integer accumulators of the aggregate ``slots`` per group.

    ``gid``: int32 per row from ``group_encode`` (-1: dead row), or None: every live row is group
    0.  ``slots``: ``(op, column, valid, e)`` each -- ``column`` / ``valid`` None where the op reads
    none, ``e`` the fixed-point exponent of a ``SUM_F`` slot (None: measured here by an ``ABSMAX``
    pre-pass, see ``group_scale``).  A ``ROWS`` slot is always put first.  Returns ``(acc, offsets)``:
    ``acc`` int64 ``[G, words]`` with word 0 the live rows of the group, ``offsets[i]`` the first
    word of ``slots[i]``.  ``reduce(acc, kinds)`` combines the ranks' accumulators."""
    slots = [tuple(s) + (None,) * (4 - len(s)) for s in slots]
    n = _n_rows(gid, sel, slots) if n is None else int(n)
    need = [i for i, s in enumerate(slots) if s[0] == SUM_F and s[3] is None]
    if need:
        es = group_scale([slots[i][1] for i in need], [slots[i][2] for i in need], sel, blocks, reduce)
        for i, e in zip(need, es):
            slots[i] = slots[i][:3] + (e,)
    if any(s[0] == SUM_F for s in slots) and n >= 1 << 31:
        raise ValueError("group_agg: a fixed-point sum takes fewer than 2^31 rows per call")
    parts, offsets, w = [], [], 1
    per = GROUP_MAX_SLOTS - 1  # every call carries ROWS in slot 0
    for i in range(0, max(len(slots), 1), per):
        chunk = [(ROWS, None, None, 0)] + slots[i:i + per]
        ops = [s[0] for s in chunk]
        a = _agg_call(gid, int(G), ops, [s[1] for s in chunk], [s[2] for s in chunk], [int(s[3] or 0) for s in chunk],
                      sel, n, row_offset, blocks)
        parts.append(a if i == 0 else a[:, 1:])
        for s in chunk[1:]:
            offsets.append(w)
            w += op_words(s[0])
    acc = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    if reduce is not None:
        acc = reduce(acc, [K_ADD] + word_kinds([s[0] for s in slots]))
    return acc, offsets


# ------------------------------------------------------------------------------------------
# group_encode
# ------------------------------------------------------------------------------------------
@dataclass
class GroupEncoding:
    """``gid``: int32 per row (-1 dead, 0 null key, else the key's slot); ``G`` slots; ``keys``:
    the signed order key of each slot (int64 ``[G]`` on the rows' device, slot 0 unused).  A direct
    encoding has a slot for every value of the live range, so some may receive no row: drop them
    by the ``ROWS`` word after aggregation."""
    gid: torch.Tensor
    G: int
    keys: torch.Tensor
    mode: str
    dtype: torch.dtype
    capacity: Optional[int] = None


def group_encode(col: torch.Tensor, valid=None, sel=None, capacity: Optional[int] = None, blocks: Optional[int] = None,
                 reduce=None, union=None, mode: Optional[str] = None) -> GroupEncoding:
    """Group ids of one key column (f64 / f32 / i32 / i64 / bool / u8).  Integer and boolean keys
    whose live range is at most ``GROUP_DIRECT_CAP`` index their slot directly (``mode`` "hash"
    overrides); the rest go through the hash table, first of ``capacity`` slots.  ``reduce`` /
    ``union`` make the slots global over ranks: the range is all-reduced, the sorted unique keys
    are exchanged."""
    if col.dim() != 1:
        raise ValueError("group_encode: the key column must be 1-D")
    if col.dtype not in KEY_DTYPES:
        raise TypeError(f"group_encode: unsupported key dtype {col.dtype}")
    n = int(col.numel())
    if n >= 1 << 31:
        raise ValueError("group_encode: fewer than 2^31 rows per call")
    dev = col.device
    if col.dtype in INTS and mode != "hash":
        acc, off = group_agg(None, 1, [(MIN, col, valid), (MAX, col, valid), (COUNT, None, valid)], sel, blocks=blocks,
                             reduce=reduce, n=n)
        lo, hi, cnt = (int(v) for v in acc[0, off].tolist())
        lo, hi = lo ^ I64_MIN, hi ^ I64_MIN
        lo, hi = (lo + (1 << 63)) % (1 << 64) - (1 << 63), (hi + (1 << 63)) % (1 << 64) - (1 << 63)
        span = hi - lo + 1 if cnt > 0 else 0
        if span <= GROUP_DIRECT_CAP:
            base = lo if cnt > 0 else 0
            if col.is_cuda:
                from . import device

                gid = device.group_encode_direct(col, valid, sel, base, span, blocks)
            else:
                gid = _direct_host(col, valid, sel, base, span)
            keys = torch.arange(span + 1, dtype=torch.int64, device=dev) - 1 + base  # (slot 0 is unused)
            return GroupEncoding(gid, span + 1, keys, "direct", col.dtype)
    if mode == "direct":
        raise ValueError("group_encode: direct mode takes integer keys of a live range within the cap")
    cap = next_pow2(int(capacity)) if capacity else GROUP_DEFAULT_CAPACITY
    if cap < 2:
        raise ValueError("group_encode: capacity must be at least 2")
    used = None
    if col.is_cuda:
        from . import device

        gid, keys, used = device.group_encode_hash(col, valid, sel, cap, max(cap, next_pow2(2 * max(n, 1))), union, blocks)
    else:
        gid, keys = _hash_host(col, valid, sel, union)
    keys = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), keys.to(dev)])
    return GroupEncoding(gid, int(keys.numel()), keys, "hash", col.dtype, used)


def group_encode_columns(cols, valids=None, sel=None, capacity: Optional[int] = None, blocks: Optional[int] = None,
                         reduce=None, union=None):
    """Group ids of a key of several columns: ``(gid, G, [(values, valid) per column])`` with the
    key values of every slot (``valid`` False where that column's key is null).  Each column is
    encoded on its own, the codes are combined in mixed radix into one int64 (an elementwise op) and
    the combination is encoded once more."""
    cols = list(cols)
    valids = [None] * len(cols) if valids is None else list(valids)
    if not cols:
        raise ValueError("group_encode: no key column")
    encs = [group_encode(c, v, sel, capacity, blocks, reduce, union) for c, v in zip(cols, valids)]
    if len(encs) == 1:
        e = encs[0]
        slot = torch.arange(e.G, device=e.keys.device)
        return e.gid, e.G, [(keys_to_values(e.keys, e.dtype), slot > 0)]
    code, strides = mixed_radix([e.gid for e in encs], [e.G for e in encs], "group_encode")
    c = group_encode(code, None, sel, capacity, blocks, reduce, union)  # (a dead row's code is never read)
    out = []
    for e, s in zip(encs, strides):
        slot = (c.keys // s) % e.G
        slot[0] = 0
        out.append((keys_to_values(e.keys, e.dtype)[slot], slot > 0))
    return c.gid, c.G, out


# ------------------------------------------------------------------------------------------
# finalisation (G-sized torch integer code, the same for both engines)
# ------------------------------------------------------------------------------------------
def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k as a double built from its bits (k int64 in [-1022, 1023]).  ``torch.ldexp`` multiplies
    by ``pow(2.0, k)``, and a device ``pow`` may be an ulp off, which a correctly rounded sum
    cannot afford."""
    return ((k + 1023) << 52).view(torch.float64)


def _ldexp2(m: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """m * 2^s for |s| beyond one power's range (s within +-2044): two exact-or-final steps."""
    h = torch.div(s, 2, rounding_mode="floor")
    return m * _pow2(h) * _pow2(s - h)


def finalize_sum(limbs: torch.Tensor, flags: torch.Tensor, e) -> torch.Tensor:
    """The double nearest (ties to even) to ``T * 2^(e - 128)``, ``T = sum_k limbs[:, k] *
    2^(32 * (3 - k))``, per group; overflow gives +-inf, then the flags override: NaN or both
    infinities give NaN, one infinity gives that infinity.  ``limbs`` int64 ``[G, 4]``."""
    M = 0xFFFFFFFF
    a = [limbs[:, k].clone() for k in range(4)]
    # carry-normalise: a0 keeps the sign, the lower three become digits in [0, 2^32)
    for k in (3, 2, 1):
        a[k - 1] = a[k - 1] + (a[k] >> 32)
        a[k] = a[k] & M
    neg = a[0] < 0
    # magnitude: two's complement of the four-word number where it is negative
    d = [torch.where(neg, ~x & M, x) for x in a[1:]]
    hi = torch.where(neg, ~a[0], a[0])
    carry = neg.to(torch.int64)
    for k in (2, 1, 0):
        v = d[k] + carry
        carry = v >> 32
        d[k] = v & M
    hi = hi + carry
    z = torch.zeros_like(hi)
    D = torch.stack([hi >> 32, hi & M, d[0], d[1], d[2], z, z, z], dim=1)  # 32-bit digits, weight 2^(32 * (4 - i))
    nz = D != 0
    i = torch.argmax(nz.to(torch.int8), dim=1)  # first non-zero digit (0 when there is none)
    idx = i.unsqueeze(1)
    d0, d1, d2 = (torch.gather(D, 1, idx + j).squeeze(1) for j in range(3))
    tail = torch.flip(torch.cumsum(torch.flip(nz.to(torch.int64), [1]), 1), [1])  # non-zero digits at or after i
    sticky = torch.gather(tail, 1, idx + 3).squeeze(1) > 0
    lz = 32 - torch.frexp(d0.to(torch.float64))[1].to(torch.int64)  # leading zeros of d0 in 32 bits
    # W: the top 63 bits of d0:d1:d2 with the leading one at bit 62
    b1 = d1 << 31
    sh1 = 32 - lz
    sh2 = 33 - lz
    W = (d0 << (lz + 31)) + (b1 >> sh1) + (d2 >> sh2)
    one = torch.ones_like(lz)
    sticky = sticky | ((b1 & ((one << sh1) - 1)) != 0) | ((d2 & ((one << sh2) - 1)) != 0)
    mant = W >> 10
    rb = W & 0x3FF
    up = (rb > 0x200) | ((rb == 0x200) & (sticky | ((mant & 1) != 0)))
    mant = mant + up.to(torch.int64)
    e_t = torch.as_tensor(e, dtype=torch.int64, device=limbs.device)
    scale = 43 - lz + 32 * (2 - i) + e_t - 128
    val = _ldexp2(mant.to(torch.float64), scale)
    val = torch.where(neg, -val, val)
    nan = ((flags & 1) != 0) | (((flags & 2) != 0) & ((flags & 4) != 0))
    inf = torch.full_like(val, float("inf"))
    val = torch.where((flags & 2) != 0, inf, val)
    val = torch.where((flags & 4) != 0, -inf, val)
    return torch.where(nan, torch.full_like(val, float("nan")), val)
