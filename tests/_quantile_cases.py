"""Shared by the quantile tests: the fp64 sort oracle and the value patterns.

The oracle is independent of the radix select: ``np.sort`` of the live, non-NaN values cast to
double, then element ``max(1, ceil(p * n)) - 1`` with ``p * n`` one double multiply (p = 0 the first
element, p = 1 the last)."""
import numpy as np

PROBS = [0.0, 1e-9, 0.25, 0.5, 0.5, 0.75, 1 - 1e-9, 1.0]  # unsorted, one duplicate
# 1024 rows are one grid-stride trip of a device block: 1025 / 2048 / 2049 put the vector-load /
# scalar-tail boundary on a trip edge
SIZES = [1, 63, 64, 65, 1025, 2048, 2049, 2373]


def oracle(x, probs, valid=None, sel=None):
    """``(values [Q] float64, live count)``; values all NaN when nothing is live."""
    v = np.asarray(x).astype(np.float64)
    live = ~np.isnan(v)
    if valid is not None:
        live &= np.asarray(valid, dtype=bool)
    if sel is not None:
        live &= np.asarray(sel, dtype=bool)
    s = np.sort(v[live])
    n = int(s.size)
    if n == 0:
        return np.full(len(probs), np.nan), 0
    out = []
    for p in probs:
        if p == 0.0:
            out.append(s[0])
        elif p == 1.0:
            out.append(s[-1])
        else:
            out.append(s[max(1, int(np.ceil(np.float64(p) * np.float64(n)))) - 1])
    return np.array(out, dtype=np.float64), n


def same(a, b):
    """``==`` on doubles, no tolerance (-0.0 == +0.0), NaN matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def patterns(n, seed=0):
    """name -> array of n values (float64 unless the name says otherwise)."""
    rng = np.random.default_rng(seed + n)
    j = np.arange(n, dtype=np.float64)
    special = np.array([np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308 / 4, np.finfo(np.float64).max,
                        -np.finfo(np.float64).max, 0.0, -0.0, 1.0])
    return {
        "constant": np.full(n, 3.25),
        "two_valued": np.where(j < (n + 1) // 2, 7.0, -2.0)[rng.permutation(n)],  # the tie straddles the median
        "signs_zero": np.where(rng.random(n) < 0.4, np.where(rng.random(n) < 0.5, -0.0, 0.0), rng.standard_normal(n)),
        "special": special[rng.integers(0, special.size, n)],
        "low_bits": (1.0 + j * 2.0 ** -52)[rng.permutation(n)],  # only the last pass tells them apart
        "sorted": np.sort(rng.standard_normal(n) * 1e3),
        "reverse": np.sort(rng.standard_normal(n) * 1e3)[::-1].copy(),
        "f32": (rng.standard_normal(n) * 10).astype(np.float32),
        "i32": rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
        "i64_big": rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64) | np.int64(1),  # beyond 2^53
    }
