"""Shared cases of the join tests: the case maker and the oracle.

The oracle is independent of the engines' key function and of any hashing or sorting: plain
Python, a dict from the canonical key of a value (NaN one key, ``-0.0`` as ``0.0``, integers and
booleans as ``int``) to the list of the right rows that hold it, and nested loops in the order the
contract defines -- left rows in row order, the matches of a left row in right row order, ``(l, -1)``
in place for an unmatched live left row of an outer join, then ``(-1, r)`` for every live right row
no left row matched.  The pair order is defined, so every check is ``torch.equal``."""
import numpy as np
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import kernels

NAN, INF = float("nan"), float("inf")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TRIP, TILE, LDS_ROWS, MAX_CAPACITY = kernels.join_limits()

DTYPES = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64, "bool": torch.bool,
          "u8": torch.uint8}
# the pairs the kernels compare directly: any two dtypes of one class
DTYPE_PAIRS = [("f64", "f64"), ("f64", "f32"), ("f32", "f64"), ("f32", "f32"), ("i32", "i32"), ("i32", "i64"), ("i64", "i32"),
               ("i64", "i64"), ("bool", "bool"), ("u8", "u8"), ("bool", "u8")]
HOWS = ("inner", "left_outer", "full_outer")


def key_column(n: int, dtype: str, span: int, seed: int, specials: bool = True) -> torch.Tensor:
    """``n`` keys drawn from a pool of about ``span`` values of the dtype, so that two columns of
    one ``span`` overlap.  ``specials``: NaN of two payloads, ``-0.0`` / ``0.0``, the infinities
    (floats) and the extreme integers are part of the pool."""
    rng = np.random.default_rng(7919 * seed + 31 * span + len(dtype))
    j = rng.integers(0, max(span, 1), n)
    if dtype in ("bool", "u8"):
        v = (j % 2).astype(np.uint8)
        if dtype == "u8":
            v = v * rng.integers(1, 200, n).astype(np.uint8)  # any non-zero byte is true
        return torch.from_numpy(v).to(DTYPES[dtype])
    if dtype in ("f64", "f32"):
        np_dt = np.float64 if dtype == "f64" else np.float32
        v = (j.astype(np.float64) * 0.5 - span / 8).astype(np_dt)  # (halves: exact in f32, so f32 meets f64)
        if specials and n:
            nan2 = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
            pool = np.array([NAN, nan2, -0.0, 0.0, INF, -INF], dtype=np.float64).astype(np_dt)
            hit = rng.random(n) < 0.25
            v = np.where(hit, pool[rng.integers(0, pool.size, n)], v)
        return torch.from_numpy(np.ascontiguousarray(v))
    np_dt = np.int64 if dtype == "i64" else np.int32
    v = (j - span // 4).astype(np_dt)
    if specials and n:
        top = [I64_MAX, I64_MIN, I64_MAX - 1] if dtype == "i64" else [(1 << 31) - 1, -(1 << 31), 0]
        hit = rng.random(n) < 0.1
        v = np.where(hit, np.array(top, dtype=np_dt)[rng.integers(0, 3, n)], v)
    return torch.from_numpy(np.ascontiguousarray(v))


def make_case(nl: int, nr: int, ldt: str = "i64", rdt: str = "i64", span: int = 50, seed: int = 0, nulls: bool = True,
              selection: bool = True, specials: bool = True):
    """``(lkey, rkey, lvalid, rvalid, lsel, rsel)`` host tensors: 10% nulls per side with ``nulls``,
    an 80% selection per side with ``selection``."""
    rng = np.random.default_rng(4001 + seed)
    lkey = key_column(nl, ldt, span, 2 * seed, specials)
    rkey = key_column(nr, rdt, span, 2 * seed + 1, specials)
    mask = lambda n, p: torch.from_numpy(rng.random(n) < p)  # noqa: E731
    lvalid, rvalid = (mask(nl, 0.9), mask(nr, 0.9)) if nulls else (None, None)
    lsel, rsel = (mask(nl, 0.8), mask(nr, 0.8)) if selection else (None, None)
    return lkey, rkey, lvalid, rvalid, lsel, rsel


def case_of(lkey, rkey, lvalid=None, rvalid=None, lsel=None, rsel=None):
    return lkey, rkey, lvalid, rvalid, lsel, rsel


def to_device(case, dev):
    return tuple(None if t is None else t.to(dev) for t in case)


def canon(v):
    """The canonical join key of a Python value of a key column."""
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, int):
        return v
    if v != v:
        return "nan"
    return float(v) + 0.0  # (-0.0 + 0.0 == 0.0)


def _side(key, valid, sel):
    vals = key.tolist()
    if key.dtype == torch.uint8:
        vals = [int(v != 0) for v in vals]
    n = len(vals)
    live = [True] * n if sel is None else [bool(s) for s in sel.tolist()]
    ok = list(live) if valid is None else [a and bool(b) for a, b in zip(live, valid.tolist())]
    return [canon(v) for v in vals], live, ok


def oracle(case, how: str):
    """``(li, ri)`` int64 tensors of the join in the contract's order."""
    lkey, rkey, lvalid, rvalid, lsel, rsel = case
    lk, llive, lok = _side(lkey, lvalid, lsel)
    rk, rlive, rok = _side(rkey, rvalid, rsel)
    rows = {}
    for r, k in enumerate(rk):
        if rok[r]:
            rows.setdefault(k, []).append(r)
    li, ri, met = [], [], set()
    for l, k in enumerate(lk):
        if not llive[l]:
            continue
        hit = rows.get(k) if lok[l] else None
        if hit:
            met.add(k)
            for r in hit:
                li.append(l)
                ri.append(r)
        elif how != "inner":
            li.append(l)
            ri.append(-1)
    if how == "full_outer":
        for r, k in enumerate(rk):
            if rlive[r] and not (rok[r] and k in met):
                li.append(-1)
                ri.append(r)
    return torch.tensor(li, dtype=torch.int64), torch.tensor(ri, dtype=torch.int64)


def oracle_mask(case) -> torch.Tensor:
    li, _ = oracle(case, "inner")
    m = torch.zeros(int(case[0].numel()), dtype=torch.bool)
    m[li] = True
    return m


def oracle_stats(case, pairs: int) -> dict:
    _, rkey, _, rvalid, _, rsel = case
    rk, _, rok = _side(rkey, rvalid, rsel)
    keys = [k for k, o in zip(rk, rok) if o]
    return {"distinct": len(set(keys)), "unique_build": len(set(keys)) == len(keys), "pairs": pairs}


_ORACLE = {}


def cached_oracle(tag, case, how: str):
    """``oracle`` computed once per ``tag`` (the case's recipe) and ``how``, shared among tests."""
    key = (tag, how)
    if key not in _ORACLE:
        _ORACLE[key] = oracle(case, how) if how != "mask" else oracle_mask(case)
    return _ORACLE[key]


def run(case, how="inner", **kw):
    lkey, rkey, lvalid, rvalid, lsel, rsel = case
    return kernels.join_pairs(lkey, rkey, lvalid, rvalid, lsel, rsel, how=how, **kw)


def run_mask(case, **kw):
    lkey, rkey, lvalid, rvalid, lsel, rsel = case
    return kernels.join_mask(lkey, rkey, lvalid, rvalid, lsel, rsel, **kw)


def core(stats: dict) -> dict:
    """The part of ``stats`` both engines report."""
    return {k: stats[k] for k in ("distinct", "unique_build", "pairs")}
