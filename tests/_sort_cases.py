"""Shared cases of the sort tests: the frame maker, the key patterns and the oracle.

The oracle is independent of the engines' key function: Python's stable ``sorted`` over the live
row indices with a ``cmp_to_key`` comparator on the raw values that states Spark's rules directly
-- a null by ``nulls_first``; NaN equal to NaN and above everything; ``-0.0 == 0.0``; otherwise
``<``; a descending order negates the comparison of non-null values only; across several orders
the first non-zero comparison decides.  A stable sort has one right answer, so every check is
``torch.equal`` on the permutation."""
from functools import cmp_to_key

import numpy as np
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import kernels

NAN, INF = float("nan"), float("inf")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
THREADS, RUN, TILE, BITS = kernels.sort_limits()

PATTERNS = ("equal", "byte256", "alt", "sorted", "reverse", "random64", "floats", "ties")
DTYPES = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64, "bool": torch.bool,
          "u8": torch.uint8}
# (ascending, nulls_first): the four null placements
PLACEMENTS = ((True, True), (True, False), (False, True), (False, False))


def _specials(np_dt):
    """±0.0, ±inf, denormals, NaNs of different payloads and signs, ordinary values."""
    if np_dt == np.float64:
        nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123,
                         0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
        den = np.array([5e-324, -5e-324, 2.2250738585072009e-308, -1e-310])
    else:
        nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFC00123, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
        den = np.array([1e-45, -1e-45, 1.1754942e-38, -1e-40], dtype=np.float32)
    rest = np.array([0.0, -0.0, INF, -INF, 1.5, -1.5, 1e10, -1e10, 3.0, 0.1, -0.1, 1.0, -1.0], dtype=np_dt)
    return np.concatenate([nans.astype(np_dt), den.astype(np_dt), rest])


def pattern_column(pattern: str, n: int, dtype: str, seed: int = 0) -> torch.Tensor:
    """``n`` values of the pattern in the torch dtype ``DTYPES[dtype]``."""
    rng = np.random.default_rng(1000 * seed + 17 * PATTERNS.index(pattern) + len(dtype))
    td = DTYPES[dtype]
    j = np.arange(n, dtype=np.int64)
    if dtype in ("bool", "u8"):  # 0 / 1 columns
        v = {"equal": np.ones(n, dtype=np.int64), "byte256": j % 2, "alt": j % 2, "sorted": (j >= n // 2).astype(np.int64),
             "reverse": (j < n // 2).astype(np.int64)}.get(pattern)
        if v is None:
            v = rng.integers(0, 2, n)
        return torch.from_numpy(v.astype(np.uint8)).to(td)
    isf = dtype in ("f64", "f32")
    np_dt = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64}[dtype]
    if pattern == "equal":
        v = np.full(n, 7).astype(np_dt)
    elif pattern == "byte256":
        # 256 values that differ in one byte; position j takes value j % 256, so the 64 lanes of a
        # wave (consecutive positions) never share a digit
        if dtype == "f64":
            v = (np.uint64(0x4000000000000000) | ((j % 256).astype(np.uint64) << np.uint64(16))).view(np.float64)
        elif dtype == "f32":
            v = (np.uint32(0x40000000) | ((j % 256).astype(np.uint32) << np.uint32(8))).view(np.float32)
        else:
            v = ((j % 256) << 8).astype(np_dt)
    elif pattern == "alt":
        v = np.where(j % 2 == 0, 3, -5).astype(np_dt)
    elif pattern in ("sorted", "reverse"):
        v = (j - n // 2).astype(np_dt)
        if isf:
            v = v * np_dt(0.25)
        if pattern == "reverse":
            v = v[::-1].copy()
    elif pattern == "random64":
        if dtype == "i64":
            v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
            v[: min(n, 2)] = [I64_MAX, I64_MIN][: min(n, 2)]
        elif dtype == "i32":
            v = rng.integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64, endpoint=True).astype(np.int32)
            v[: min(n, 2)] = [(1 << 31) - 1, -(1 << 31)][: min(n, 2)]
        elif dtype == "f64":  # random bits: every exponent, both signs, some NaN
            v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True).view(np.float64)
        else:
            v = rng.integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64, endpoint=True).astype(np.int32).view(np.float32)
    elif pattern == "floats":
        if isf:
            sp = _specials(np_dt)
            v = sp[rng.integers(0, sp.size, n)]
            some = rng.random(n) < 0.3
            v = np.where(some, (rng.standard_normal(n) * 100).astype(np_dt), v)
        else:
            v = rng.integers(-3, 4, n).astype(np_dt)
    elif pattern == "ties":
        v = np.array([-2, 0, 1, 5, 9])[rng.integers(0, 5, n)].astype(np_dt)
    else:
        raise ValueError(pattern)
    return torch.from_numpy(np.ascontiguousarray(v))


def make_frame(n: int, keys, nulls: bool = False, selection: bool = False, seed: int = 0):
    """``keys``: ``(pattern, dtype)`` per sort column.  Returns ``(cols, valids, sel)`` host
    tensors: a 10% null validity mask per column with ``nulls``, an 80% selection with
    ``selection``."""
    rng = np.random.default_rng(99 + seed)
    cols, valids = [], []
    for i, (p, dt) in enumerate(keys):
        cols.append(pattern_column(p, n, dt, seed + i))
        valids.append(torch.from_numpy(rng.random(n) >= 0.1) if nulls else None)
    sel = torch.from_numpy(rng.random(n) < 0.8) if selection else None
    return cols, valids, sel


def to_device(frame, dev):
    cols, valids, sel = frame
    return ([c.to(dev) for c in cols], [None if v is None else v.to(dev) for v in valids], None if sel is None else sel.to(dev))


def _cmp_values(a, b) -> int:
    an, bn = a != a, b != b
    if an or bn:
        return int(an) - int(bn)  # NaN == NaN, NaN above everything
    return (a > b) - (a < b)  # (-0.0 == 0.0)


def oracle(frame, ascending, nulls_first) -> torch.Tensor:
    """The stable sorted order of the live rows (int64)."""
    cols, valids, sel = frame
    n = int(cols[0].numel())
    k = len(cols)
    asc = [ascending] * k if isinstance(ascending, bool) else list(ascending)
    nf = list(asc) if nulls_first is None else ([nulls_first] * k if isinstance(nulls_first, bool) else list(nulls_first))
    vals = [c.tolist() for c in cols]
    oks = [[True] * n if v is None else v.tolist() for v in valids]
    live = list(range(n)) if sel is None else [i for i, s in enumerate(sel.tolist()) if s]

    def cmp(i, j):
        for v, ok, a, f in zip(vals, oks, asc, nf):
            ni, nj = not ok[i], not ok[j]
            if ni or nj:
                c = 0 if (ni and nj) else ((-1 if ni else 1) if f else (1 if ni else -1))
            else:
                c = _cmp_values(v[i], v[j])
                c = c if a else -c
            if c:
                return c
        return 0

    return torch.tensor(sorted(live, key=cmp_to_key(cmp)), dtype=torch.int64)


_ORACLE = {}


def cached_oracle(tag, frame, ascending, nulls_first) -> torch.Tensor:
    """``oracle`` computed once per ``tag`` (the frame's recipe) and order, shared among tests."""
    key = (tag, repr(ascending), repr(nulls_first))
    if key not in _ORACLE:
        _ORACLE[key] = oracle(frame, ascending, nulls_first)
    return _ORACLE[key]


def run(frame, ascending=True, nulls_first=None, blocks=None, stats=None) -> torch.Tensor:
    cols, valids, sel = frame
    return kernels.sort_permutation(cols, valids, sel, ascending, nulls_first, blocks=blocks, stats=stats)


# the multi-key cases: ties first, so the later keys decide most rows
MULTI = {
    "two": ([("ties", "i32"), ("floats", "f64")], [True, False], None),
    "three": ([("ties", "f64"), ("alt", "i64"), ("random64", "i32")], [False, True, False], [True, True, False]),
}
