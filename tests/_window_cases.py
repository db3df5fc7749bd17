"""Shared cases of the window tests: the case maker, the frames, the raw pipeline over
``ops.kernels`` and a plain-Python oracle.

The oracle is independent of the engines: Python's stable ``sorted`` over the live rows with a
comparator that states Spark's rules directly, a walk over the partitions and peer groups with
Python loops, and ``math.fsum`` / ``min`` / ``max`` over the rows of every frame.

Value columns are dyadic: integers below 2^40 in magnitude times 2^-20.  The fixed-point window of
the sum then holds every value exactly and the true sum of any frame is a double, so the engines'
sum must EQUAL ``math.fsum`` of the frame (``assert_dyadic`` checks the premise in integers)."""
import math
from functools import cmp_to_key

import numpy as np
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.ops import window as wn

THREADS, RUN, TILE, MAX_KEYS, MAX_WORDS = kernels.window_limits()
T = TILE
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 77)
LAYOUTS = ("one", "each", "heads", "span3", "peers", "nulls", "sel", "dead")
DTYPES = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64, "bool": torch.bool,
          "u8": torch.uint8}
I64 = 1 << 64

# (is_range, lo, hi); None: unbounded
FRAMES = {
    "default": (True, None, 0),      # RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW
    "whole": (False, None, None),
    "running": (False, None, 0),
    "slide": (False, -3, 3),         # clamped at both partition ends
    "ahead": (False, 1, 2),          # empty at the partition's last row
    "rest": (False, 0, None),
}
# min / max run forward over a frame that starts with its partition, backward over one that ends with it
PICKS = {"default": "hi", "whole": "hi", "running": "hi", "rest": "lo"}
SHIFTS = (-1, 1, -(T + 1), T + 1)  # lag / lead by 1 and across a tile


def dyadic(rng, n):
    v = rng.integers(-(1 << 40) + 1, 1 << 40, n).astype(np.float64) * 2.0 ** -20
    return torch.from_numpy(v)


def assert_dyadic(vals):
    """The premise of the equality check: every value is an integer times 2^-20 below 2^20 in
    magnitude, and ``math.fsum`` of all of them is their exact sum."""
    ints = [int(v * (1 << 20)) for v in vals]
    assert all(i == v * (1 << 20) and abs(i) < 1 << 40 for i, v in zip(ints, vals))
    assert math.fsum(vals) * (1 << 20) == sum(ints)


def make_case(m: int, layout: str, seed: int = 0, part_dtype="i64", order_dtype="f64", two_by_two=False):
    """A case of ``m`` live rows: partition columns, order columns ``(col, valid, ascending,
    nulls_first)``, a dyadic value column and an int64 column with nulls, a selection (or None)."""
    rng = np.random.default_rng(7 * seed + 13 * LAYOUTS.index(layout) + m)
    dead = layout == "dead"
    live = 0 if dead else m
    n = m if layout not in ("sel",) else m + m // 4 + 3
    pos = np.arange(live)
    if layout == "one":
        pk = np.zeros(live, dtype=np.int64)
    elif layout == "each":
        pk = rng.permutation(live).astype(np.int64)
    elif layout == "heads":  # sorted positions 64 and T start a partition
        pk = (pos >= 64).astype(np.int64) + (pos >= T)
    elif layout == "span3":
        pk = (pos + T // 2) // (2 * T + 5)
    elif layout == "peers":
        pk = pos % 3
    else:
        pk = rng.integers(0, 5, live)
    ok = rng.integers(0, 1 if layout == "peers" else 7, live)
    rows = np.sort(rng.permutation(n)[:live]) if not dead else np.zeros(0, dtype=np.int64)
    shuffle = rng.permutation(live)

    def spread(x, fill=0):
        out = np.full(n, fill, dtype=np.int64)
        out[rows] = np.asarray(x)[shuffle]
        return out

    def typed(x, dt):
        td = DTYPES[dt]
        if dt in ("bool", "u8"):
            return torch.from_numpy((x % 2).astype(np.uint8)).to(td)
        return torch.from_numpy(x).to(td)

    nulls = layout == "nulls"
    mask = (lambda: torch.from_numpy(rng.random(n) >= 0.15)) if nulls else (lambda: None)
    parts = [(typed(spread(pk), part_dtype), mask())]
    orders = [(typed(spread(ok), order_dtype), mask(), True, True)]
    if nulls:  # float keys with the grouping rule's specials
        sp = np.array([0.0, -0.0, float("nan"), -float("nan"), 1.5, float("inf")])
        parts = [(torch.from_numpy(sp[spread(pk) % 6]), mask())]
    if two_by_two:
        parts.append((typed(spread(rng.integers(0, 3, live)), "i32"), mask()))
        orders = [(typed(spread(rng.integers(0, 3, live)), "i32"), mask(), False, False),
                  (typed(spread(ok), "f64"), mask(), True, False)]
    sel = None
    if layout == "sel" or dead:
        s = np.zeros(n, dtype=bool)
        s[rows] = True
        sel = torch.from_numpy(s)
    v = dyadic(rng, n)
    iv = torch.from_numpy(rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64))
    vvalid = torch.from_numpy(rng.random(n) >= 0.1)
    assert_dyadic(v.tolist())
    return {"n": n, "parts": parts, "orders": orders, "v": v, "iv": iv, "vvalid": vvalid, "sel": sel,
            "e": kernels.group_scale([v], [vvalid], sel)[0]}


def to_device(case, dev):
    mv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    out = dict(case)
    out["parts"] = [(mv(c), mv(k)) for c, k in case["parts"]]
    out["orders"] = [(mv(c), mv(k), a, f) for c, k, a, f in case["orders"]]
    for k in ("v", "iv", "vvalid", "sel"):
        out[k] = mv(case[k])
    return out


# ------------------------------------------------------------------------------------------
# the raw pipeline: every contract of ops/window.py on one case
# ------------------------------------------------------------------------------------------
def run_raw(case, blocks=None, frames=FRAMES):
    """name -> raw integer tensor (on the case's device).  10 prefix words (two passes), the four
    min / max scans, one finish per frame (12 words: two launches) and the ranking / shift words."""
    n, parts, orders = case["n"], case["parts"], case["orders"]
    v, iv, vv = case["v"], case["iv"], case["vvalid"]
    perm = kernels.sort_permutation([c for c, _ in parts] + [o[0] for o in orders], [k for _, k in parts] + [o[1] for o in orders],
                                    case["sel"], [True] * len(parts) + [o[2] for o in orders],
                                    [True] * len(parts) + [o[3] for o in orders], blocks=blocks)
    heads = kernels.window_heads([c for c, _ in parts], [k for _, k in parts], [o[0] for o in orders], [o[1] for o in orders],
                                 perm, n, blocks=blocks)
    bounds = kernels.window_bounds(heads, blocks=blocks)
    P, off = kernels.window_prefix([(wn.ROWS, None, None, 0), (wn.COUNT, None, vv, 0), (wn.SUM_F, v, vv, case["e"]),
                                    (wn.SUM_I, iv, vv, 0)], perm, n, blocks=blocks)
    assert off == [0, 1, 2, 9] and P.shape[0] == 10
    out = {"perm": perm, "heads": heads, "bounds": bounds, "P": P}
    scans = {}
    for is_max in (False, True):
        for back in (False, True):
            scans[(is_max, back)] = kernels.window_minmax(v, vv, perm, heads, is_max, back, blocks=blocks)
            out[f"scan{int(is_max)}{int(back)}"] = scans[(is_max, back)]
    for name, frame in frames.items():
        outs = [(wn.O_DIFF, P[w], 0) for w in range(10)]
        if name in PICKS:
            kind = wn.O_PICK_HI if PICKS[name] == "hi" else wn.O_PICK_LO
            outs += [(kind, scans[(False, PICKS[name] == "lo")], 0), (kind, scans[(True, PICKS[name] == "lo")], 0)]
        out["frame_" + name] = kernels.window_finish(bounds, perm, n, frame, outs, blocks=blocks)
    out["ranks"] = kernels.window_finish(bounds, perm, n, (True, None, 0),
                                         [(k, None, 0) for k in (wn.O_ROW_NUMBER, wn.O_RANK, wn.O_DENSE_RANK, wn.O_PART_SIZE,
                                                                 wn.O_PEER_END)] + [(wn.O_SHIFT, None, d) for d in SHIFTS],
                                         blocks=blocks)
    return out


def finalize(case, raw, frames=FRAMES):
    """The oracle's shape from the raw words: per live row a dict of values (None: null)."""
    live = raw["perm"].cpu().tolist()
    res = {r: {} for r in live}
    e = case["e"]
    for name in frames:
        w = raw["frame_" + name].cpu()
        cnt = w[:, 1]
        s = wn.sum_from_words(w[:, 2:9], e)
        for r in live:
            d = res[r]
            c = int(cnt[r])
            d[name + ".rows"] = int(w[r, 0])
            d[name + ".count"] = c
            d[name + ".sum"] = float(s[r]) if c else None
            d[name + ".isum"] = int(w[r, 9]) if c else None
        if name in PICKS:
            mn, mx = wn.minmax_from_keys(w[:, 10], torch.float64), wn.minmax_from_keys(w[:, 11], torch.float64)
            for r in live:
                c = res[r][name + ".count"]
                res[r][name + ".min"] = float(mn[r]) if c else None
                res[r][name + ".max"] = float(mx[r]) if c else None
    rk = raw["ranks"].cpu()
    for r in live:
        row = rk[r].tolist()
        res[r].update({"row_number": row[0], "rank": row[1], "dense_rank": row[2], "size": row[3], "peer_end": row[4]})
        for d, src in zip(SHIFTS, row[5:]):
            res[r][f"shift{d}"] = src
    return res


# ------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------
def _cmp_values(a, b) -> int:
    an, bn = a != a, b != b
    if an or bn:
        return int(an) - int(bn)  # NaN == NaN, NaN above everything
    return (a > b) - (a < b)  # (-0.0 == 0.0)


def _cmp_col(vals, ok, asc, nf, i, j) -> int:
    ni, nj = not ok[i], not ok[j]
    if ni or nj:
        return 0 if (ni and nj) else ((-1 if ni else 1) if nf else (1 if ni else -1))
    c = _cmp_values(vals[i], vals[j])
    return c if asc else -c


def oracle(case, frames=FRAMES):
    n = case["n"]
    lst = lambda c: c.tolist()  # noqa: E731
    okl = lambda k: [True] * n if k is None else k.tolist()  # noqa: E731
    pcols = [(lst(c), okl(k), True, True) for c, k in case["parts"]]
    ocols = [(lst(c), okl(k), a, f) for c, k, a, f in case["orders"]]
    sel = case["sel"]
    live = list(range(n)) if sel is None else [i for i, s in enumerate(sel.tolist()) if s]

    def cmp_with(cols):
        def cmp(i, j):
            for col in cols:
                c = _cmp_col(*col, i, j)
                if c:
                    return c
            return 0
        return cmp

    order = sorted(live, key=cmp_to_key(cmp_with(pcols + ocols)))
    same_part, same_peer = cmp_with(pcols), cmp_with(ocols)
    v, iv, vv = case["v"].tolist(), case["iv"].tolist(), case["vvalid"].tolist()
    res = {}
    a = 0
    while a < len(order):
        b = a
        while b + 1 < len(order) and same_part(order[a], order[b + 1]) == 0:
            b += 1
        part = order[a:b + 1]
        size = len(part)
        peer_lo, peer_hi, dense = [0] * size, [0] * size, [0] * size
        s = 0
        d = 0
        while s < size:
            t = s
            while t + 1 < size and same_peer(part[s], part[t + 1]) == 0:
                t += 1
            d += 1
            for k in range(s, t + 1):
                peer_lo[k], peer_hi[k], dense[k] = s, t, d
            s = t + 1
        vals = [v[r] if vv[r] else None for r in part]
        ints = [iv[r] if vv[r] else None for r in part]
        cache = {}

        def over(lo, hi):
            if (lo, hi) not in cache:
                xs = [x for x in vals[lo:hi + 1] if x is not None] if lo <= hi else []
                it = sum(x for x in ints[lo:hi + 1] if x is not None) if lo <= hi else 0
                it = (it + (I64 >> 1)) % I64 - (I64 >> 1)
                cache[(lo, hi)] = (max(hi - lo + 1, 0), len(xs), math.fsum(xs) if xs else None, it if xs else None,
                                   min(xs) if xs else None, max(xs) if xs else None)
            return cache[(lo, hi)]

        for k, r in enumerate(part):
            out = {"row_number": k + 1, "rank": peer_lo[k] + 1, "dense_rank": dense[k], "size": size, "peer_end": peer_hi[k] + 1}
            for dd in SHIFTS:
                out[f"shift{dd}"] = part[k + dd] if 0 <= k + dd < size else -1
            for name, (is_range, lo, hi) in frames.items():
                if is_range:
                    flo = 0 if lo is None else peer_lo[k]
                    fhi = size - 1 if hi is None else peer_hi[k]
                else:
                    flo = 0 if lo is None else max(k + lo, 0)
                    fhi = size - 1 if hi is None else min(k + hi, size - 1)
                rows, cnt, sm, it, mn, mx = over(flo, fhi)
                out.update({name + ".rows": rows, name + ".count": cnt, name + ".sum": sm, name + ".isum": it})
                if name in PICKS:
                    out.update({name + ".min": mn, name + ".max": mx})
            res[r] = out
        a = b + 1
    return order, res


_CACHE = {}


def cached(tag, build):
    """``build()`` computed once per ``tag`` and shared among the tests (cases, oracle and twin results)."""
    if tag not in _CACHE:
        _CACHE[tag] = build()
    return _CACHE[tag]


def reference(m, layout, **kw):
    """``(case, twin raw outputs, oracle order, oracle results)`` of one recipe, computed once."""
    def build():
        case = make_case(m, layout, **kw)
        order, res = oracle(case)
        return case, run_raw(case), order, res
    return cached((m, layout, tuple(sorted(kw.items()))), build)


def same_results(got, want):
    """Exact equality of two result maps (floats by value: the sums are exact, -0.0 cannot occur
    in a min / max of these columns unless it is in the column)."""
    assert got.keys() == want.keys()
    for r in want:
        assert got[r] == want[r], (r, {k: (got[r].get(k), want[r][k]) for k in want[r] if got[r].get(k) != want[r][k]})
