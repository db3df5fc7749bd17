"""Shared by the exact Gram tests: inputs whose WLS statistics are exact on every path, and the
integer oracle they are compared with under ``==``.

Every generated value is a small integer (or, for the weights, a multiple of 1/2), chosen so that
every product a Gram kernel forms and every partial sum it keeps -- in bf16 x bf16 -> f32 MFMAs, in
fp8 x fp8 -> f32 MFMAs, in the exact-f32 and split-bf16 kernels, in f64 -- is exactly representable,
however the kernel orders or splits its sums.  The whole flat vector ``[count, Σw, Σw², Σwy, Σwy²,
Σw·x (d), Σw·x·y (d), packed upper Σw·x·xᵀ]`` then has ONE right answer in doubles, and the oracle
gets it in ``int64`` arithmetic on ``4·w``.

The bound that makes this true (``Case.bound``, asserted by ``test_gram_exact_cases.py``): with
``u = 2·w`` (an integer), for every integer shift ``s_j`` inside column j's own value range,

    Σ_live u·|x_i - s_i|·|x_j - s_j| < 2²⁴   and   Σ_live u·|x_i - s_i|·|y| < 2²⁴,   Σ_live u·y² < 2²⁴.

By Cauchy-Schwarz the cross terms are at most the largest diagonal one, and ``Σ u·(x - s)²`` is
convex in ``s``, so the bound is the maximum over the columns of the diagonal sums at the two ends of
the column's range (and the label's own sum).  An f32 accumulator then only ever holds a multiple of
1/2 (or, on the fp8 path, of 2¹² · 1/2) whose magnitude in those units is below 2²⁴: exact for any
chain length and any split.  (``Σ w·... < 2²⁴`` of the issue follows: ``w <= u``.)

Host only (numpy and torch on the CPU); the GPU test uploads what it needs.
"""
import functools

import numpy as np
import torch

LIMIT = 1 << 24
W_VALUES = np.array([0.5, 1.0, 2.0])
OFF_SLOTS = (3, 17, 30)  # columns j with j % 32 in OFF_SLOTS are off-centre: a few in every feature tile
ZERO_COL = 1             # the (centred) column that is sure to hold zeros (column 0 at d = 1)

# row counts of the tall paths: the 64-row superstep edge, the stream kernels' 1024-row flush, the
# patched tests' two-block wave map (40 supersteps + 5 rows), a ragged many-superstep size and a
# many-block planned grid (the largest size the bound allows with these value ranges)
TALL_N = [1, 63, 64, 65, 1023, 1024, 1025, 64 * 40 + 5, 4113, 70_001]
MID_N = [1023, 1024, 1025, 64 * 40 + 5, 4113]  # where blocks in {1, 2} makes one wave take several trips
TALL_D = [1, 8, 9, 32, 33, 64]
B_N = 4113
B_LIVE = (0, 63, 64, B_N - 1)


# ------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------
def layout_size(d):
    return 5 + 2 * d + d * (d + 1) // 2


def live_rows(n, w, sel):
    """Rows that count: selected (no selection: all) and of non-zero weight (no weights: all)."""
    live = np.ones(n, dtype=bool) if sel is None else np.asarray(sel, dtype=bool).copy()
    if w is not None:
        live &= np.asarray(w, dtype=np.float64) != 0
    return live


def _as_int(a, what):
    a = np.asarray(a, dtype=np.float64)
    r = np.rint(a)
    if not np.array_equal(a, r):
        raise ValueError(f"oracle: {what} must hold integers on the live rows")
    return r.astype(np.int64)


def _gram_int(Xi, u):
    """``(Xi * u) @ Xi.T`` in int64.  Small shapes: numpy's integer product.  Large ones: the f64
    product (exact here: every partial sum is an integer far below 2^53), accepted only after an
    int64 Freivalds check ``G v == X (u * (Xᵀ v))`` on two random integer vectors."""
    d, m = Xi.shape
    if d * d * m <= 30_000_000:
        return (Xi * u) @ Xi.T
    Xf = Xi.astype(np.float64)
    G = np.rint((Xf * u.astype(np.float64)) @ Xf.T).astype(np.int64)
    rng = np.random.default_rng(d * 7919 + m)
    for _ in range(2):
        v = rng.integers(-1024, 1025, d).astype(np.int64)
        if not np.array_equal(G @ v, Xi @ (u * (Xi.T @ v))):
            raise AssertionError("oracle: the f64 Gram product is not the integer one")
    return G


def oracle(X, y, w, sel, count_zero_weight=True):
    """The flat statistics ``float64[5 + 2d + d(d+1)/2]`` of integer features and labels, weights a
    multiple of 1/4: int64 sums on ``4·w``, scaled by a power of two at the end.  Dead rows
    (``sel == False``, ``w == 0`` or both) contribute nothing to any sum, whatever they hold (NaN
    and inf included).  The count (entry 0) is the one entry a zero weight does not settle:
    ``kernels.gram_stats`` and the d <= 64 kernels count every selected row, as Spark's WLS
    aggregator counts every instance (``count_zero_weight=True``); the d > 64 SYRK launcher counts
    the rows of non-zero weight (``False``; ops/device.py ``_gram_syrk``, pinned by
    test_gpu_syrk.py)."""
    X = np.asarray(X, dtype=np.float64)
    d, n = X.shape
    live = live_rows(n, w, sel)
    Xi = _as_int(X[:, live], "features")
    yi = _as_int(np.asarray(y, dtype=np.float64)[live], "labels")
    q = np.full(int(live.sum()), 4, dtype=np.int64) if w is None else _as_int(4.0 * np.asarray(w, dtype=np.float64)[live], "4 w")
    out = np.empty(layout_size(d), dtype=np.float64)
    out[0] = float(live.sum() if sel is None or not count_zero_weight else np.asarray(sel, dtype=bool).sum())
    if sel is None and count_zero_weight:
        out[0] = float(n)
    out[1] = float(q.sum()) / 4.0
    out[2] = float((q * q).sum()) / 16.0
    out[3] = float((q * yi).sum()) / 4.0
    out[4] = float((q * yi * yi).sum()) / 4.0
    out[5:5 + d] = (Xi @ q).astype(np.float64) / 4.0
    out[5 + d:5 + 2 * d] = (Xi @ (q * yi)).astype(np.float64) / 4.0
    G = _gram_int(Xi, q)
    assert np.abs(G).max(initial=0) < 1 << 52
    i, j = np.triu_indices(d)
    out[5 + 2 * d + i + j * (j + 1) // 2] = G[i, j].astype(np.float64) / 4.0
    return out


def oracle_one_row(x, y):
    """The statistics of ONE live row of unit weight, f64 products of f32 values (24 x 24 bits: exact
    in a double, and one term per sum)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[0]
    out = np.empty(layout_size(d), dtype=np.float64)
    out[:5] = [1.0, 1.0, 1.0, float(y), float(y) * float(y)]
    out[5:5 + d] = x
    out[5 + d:5 + 2 * d] = x * float(y)
    i, j = np.triu_indices(d)
    out[5 + 2 * d + i + j * (j + 1) // 2] = x[i] * x[j]
    return out


def f32_exact(v):
    """Where the doubles of ``v`` are f32-representable."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        return v.astype(np.float32).astype(np.float64) == v


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
class Case:
    """One generated input.  ``X`` f32 ``[d, n]`` (finite everywhere: the dead rows hold ordinary
    draws), ``y`` f32 ``[n]``, ``w`` f64 ``[n]`` with exact zeros, ``sel`` bool ``[n]``.  A test picks
    the mask / weight combination it runs: ``rows(False, False)`` = every row live, and so on; row 0
    is live in all of them."""

    ALL = ((False, False), (False, True), (True, False), (True, True))  # (weighted, masked)

    def __init__(self, name, X, y, w, sel, off_cols, zero_col, shift_free=False, combos=ALL):
        self.name, self.X, self.y, self.w, self.sel = name, X, y, w, sel
        self.combos = tuple(combos)  # the combinations this case is made for
        self.d, self.n = X.shape
        self.off_cols = list(off_cols)
        self.zero_col = zero_col
        self.shift_free = shift_free  # ops/shift.py never shifts these columns: the bound is taken at s = 0
        self._oracles = {}

    def rows(self, weighted, masked):
        return (self.w if weighted else None), (self.sel if masked else None)

    def oracle(self, weighted, masked, count_zero_weight=True):
        """The oracle of one combination (computed once, shared, never written to)."""
        key = (bool(weighted), bool(masked))
        if key not in self._oracles:
            w, sel = self.rows(*key)
            self._oracles[key] = torch.from_numpy(oracle(self.X.numpy(), self.y.numpy(), None if w is None else w.numpy(),
                                                         None if sel is None else sel.numpy()))
        ref = self._oracles[key]
        if not count_zero_weight:
            ref = ref.clone()
            ref[0] = float((~self.dead(*key)).sum())
        return ref

    def dead(self, weighted, masked):
        w, sel = self.rows(weighted, masked)
        return torch.from_numpy(~live_rows(self.n, None if w is None else w.numpy(), None if sel is None else sel.numpy()))

    def poisoned(self, weighted, masked):
        """``(X, y)`` with NaN / inf in the dead rows of this combination (alternating), for the
        paths that promise not to read them."""
        dead = self.dead(weighted, masked).nonzero().flatten()
        X, y = self.X.clone(), self.y.clone()
        X[:, dead[0::2]] = float("nan")
        X[:, dead[1::2]] = float("inf")
        y[dead[0::3]] = float("nan")
        return X, y

    def zero_dead(self, weighted, masked):
        """X with exact zeros in the dead rows of this combination (zero-dead storage)."""
        X = self.X.clone()
        X[:, self.dead(weighted, masked)] = 0.0
        return X

    @property
    def bound(self):
        """The largest of the sums of the module docstring, in units of 1/2, over the case's
        combinations (unweighted rows: u = 2)."""
        X = self.X.numpy().astype(np.float64)
        y = self.y.numpy().astype(np.float64)
        worst = 0.0
        for w, sel in (self.rows(*c) for c in self.combos):
            live = live_rows(self.n, None if w is None else w.numpy(), None if sel is None else sel.numpy())
            u = 2.0 * (np.ones(self.n) if w is None else w.numpy())
            u = np.where(live, u, 0.0)
            ends = [np.zeros(self.d)] if self.shift_free else [X.min(axis=1), X.max(axis=1)]
            for s in ends:
                worst = max(worst, float((((X - s[:, None]) ** 2) * u).sum(axis=1).max()))
            worst = max(worst, float((u * y * y).sum()))
        return worst

    def __repr__(self):
        return f"Case({self.name})"


def off_columns(d):
    return [j for j in range(d) if j % 32 in OFF_SLOTS]


def zero_rows(n):
    """Rows of the zero column that hold 0 in the rare-zero form: inside full supersteps (the
    patched companion covers only those), at most one per 2048-value entry on average."""
    full = n // 64
    rows = [1] if n > 1 else []
    if full >= 3:
        rows += [64 * (full // 2) + 5, 64 * full - 1]
    return rows


def _pairs_zero_sum(y, idx, rng):
    """Labels of rows ``idx`` in +-pairs: their sum is exactly 0 and their largest is exactly 7."""
    m = len(idx) // 2
    v = rng.integers(1, 8, m)
    if m:
        v[0] = 7
    y[idx] = 0
    y[idx[0:2 * m:2]] = v
    y[idx[1:2 * m:2]] = -v


@functools.lru_cache(maxsize=None)
def family_a(n, d, off="small", zeros="dense", label="plain", seed=0):
    """Family A: dense small integers.

    Centred columns: integers uniform in [-7, 7] (``zeros="rare"``: without 0, except the few
    ``zero_rows`` of column ``ZERO_COL`` -- the form the patched companion takes).  Off-centre
    columns (``off_columns``): ``off="small"``: integers in [0, 10] (rare: {1..4, 6..9}, which no
    integer shift near their mean 5 turns into zeros); ``off="hundred"``: 100 + k, k in [-7, 7];
    ``off="none"``: every column centred.  Row 0 is live in every combination and holds +-7 in
    every centred column (100 +- 7 in the ``hundred`` ones), nothing is larger after centring: the
    fp8 per-feature scale is exactly 7 / 448 = 2^-6.  The last row (n >= 3) is live too, with weight
    1/2, label 1 and +-1 in every centred column (100 +- 1): the least a live row can weigh, the row
    whose loss a relative measure sees least.  Labels: integers in [-7, 7];
    ``label="zero_sum"``: the selected rows' labels sum to exactly 0 with largest exactly 7 and so do
    the unselected rows', so the same holds over all rows (the fp8 label split is exact on it).
    Weights in {0.5, 1, 2} with about 10 % exact zeros; the selection leaves about 30 % dead."""
    rng = np.random.default_rng([n, d, seed, {"small": 0, "none": 1, "hundred": 2}[off], zeros == "rare", label == "zero_sum"])
    if zeros == "rare":
        X = rng.integers(1, 8, (d, n)) * rng.choice([-1, 1], (d, n))
    else:
        X = rng.integers(-7, 8, (d, n))
    offc = off_columns(d) if off != "none" else []
    for j in offc:
        if off == "hundred":
            X[j] = 100 + X[j]
        elif zeros == "rare":
            X[j] = rng.choice([1, 2, 3, 4, 6, 7, 8, 9], n)
        else:
            X[j] = rng.integers(0, 11, n)
    sign = rng.choice([-7, 7], d)
    for j in range(d):
        if j not in offc:
            X[j, 0] = sign[j]
        elif off == "hundred":
            X[j, 0] = 100 + sign[j]
    if n >= 3:  # the last row: the least a live row can weigh
        for j in range(d):
            if j not in offc:
                X[j, n - 1] = rng.choice([-1, 1])
            elif off == "hundred":
                X[j, n - 1] = 100 + rng.choice([-1, 1])
    zc = min(ZERO_COL, d - 1)
    if zc in offc:
        zc = 0
    zr = zero_rows(n)
    X[zc, zr] = 0
    sel = rng.random(n) >= 0.3
    w = rng.choice(W_VALUES, n)
    w[rng.random(n) < 0.1] = 0.0
    sel[0], w[0] = True, 1.0
    y = rng.integers(-7, 8, n)
    if n >= 3:
        sel[n - 1], w[n - 1], y[n - 1] = True, 0.5, 1
    if label == "zero_sum":
        _pairs_zero_sum(y, np.flatnonzero(sel), rng)
        _pairs_zero_sum(y, np.flatnonzero(~sel), rng)
    name = f"A-n{n}-d{d}-{off}-{zeros}-{label}"
    return Case(name, torch.from_numpy(X.astype(np.float32)), torch.from_numpy(y.astype(np.float32)),
                torch.from_numpy(w), torch.from_numpy(sel), offc, zc)


@functools.lru_cache(maxsize=None)
def family_b(d, seed=0):
    """Family B: few live rows, wide mantissas.  n = 4113, live rows 0, 63, 64 and n - 1 (the
    selection; the weights are non-zero exactly there).  Features: f32 integers with |x| <= 1023,
    most of them odd, so the split-bf16 path has a non-zero ``mid`` term (x = hi + mid, lo = 0).
    Labels: integers in [-7, 7].  Dead rows: every third holds +-(odd integers) -- symmetric, so the
    column stays centred and ops/shift.py leaves it unshifted --, the others 0; ``poisoned`` turns
    them into NaN / inf for the paths that promise not to read them."""
    n = B_N
    rng = np.random.default_rng([d, seed, 77])
    X = np.zeros((d, n), dtype=np.int64)
    junk = np.arange(n) % 3 == 1
    X[:, junk] = (2 * rng.integers(0, 512, (d, int(junk.sum()))) + 1) * rng.choice([-1, 1], (d, int(junk.sum())))
    live = np.array(B_LIVE)
    X[:, live] = (2 * rng.integers(0, 512, (d, 4)) + 1) * rng.choice([-1, 1], (d, 4))
    X[0, live] = [1023, -1023, 1022, 511]  # the extremes, an even value
    sel = np.zeros(n, dtype=bool)
    sel[live] = True
    w = np.zeros(n)
    w[live] = [1.0, 0.5, 2.0, 1.0]
    y = rng.integers(-7, 8, n)
    return Case(f"B-d{d}", torch.from_numpy(X.astype(np.float32)), torch.from_numpy(y.astype(np.float32)),
                torch.from_numpy(w), torch.from_numpy(sel), [], 0, shift_free=True,
                combos=((False, True), (True, False), (True, True)))  # (every row live: the dead rows' draws would count)


class OneRow:
    """The one-live-row variant of Family B: row ``live`` of n = 4113 is the only selected one.  The
    even columns hold arbitrary f32 values with 24 significant bits, the odd ones +-2^k; the dead
    rows hold 0 (every third: +- such values again, symmetric).  ``exact``: the entries of the flat
    vector whose exact value is f32-representable (``float32(p) == p`` for the f64 product ``p``;
    the five scalars always) -- those must come out ``==`` on the f32-class paths, the others keep
    the path's tolerance."""

    live = 63

    def __init__(self, d, seed=0):
        n = B_N
        rng = np.random.default_rng([d, seed, 78])

        def draw(m):
            v = np.empty((d, m), dtype=np.float32)
            mant = (rng.integers(1 << 23, 1 << 24, (d, m)) | 1).astype(np.float64)  # 24 bits, odd
            wide = mant * np.exp2(rng.integers(-3, 4, (d, m)) - 23.0)
            pow2 = np.exp2(rng.integers(-6, 7, (d, m)).astype(np.float64))
            v[:] = np.where(np.arange(d)[:, None] % 2 == 0, wide, pow2) * rng.choice([-1.0, 1.0], (d, m))
            return v

        X = np.zeros((d, n), dtype=np.float32)
        junk = np.arange(n) % 3 == 1
        X[:, junk] = draw(int(junk.sum()))
        X[:, self.live] = draw(1)[:, 0]
        sel = np.zeros(n, dtype=bool)
        sel[self.live] = True
        y = rng.integers(-7, 8, n).astype(np.float32)
        y[self.live] = 3.0  # x * 3 needs two more bits: not representable for the 24-bit columns
        self.name, self.d, self.n = f"B1-d{d}", d, n
        self.X, self.y, self.sel = torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(sel)
        self.ref = oracle_one_row(X[:, self.live], y[self.live])
        self.exact = f32_exact(self.ref)

    def shares(self):
        """(share of the Gram entries, share of Σx) in the ``==`` class."""
        d = self.d
        return float(self.exact[5 + 2 * d:].mean()), float(self.exact[5:5 + d].mean())


@functools.lru_cache(maxsize=None)
def one_row(d, seed=0):
    return OneRow(d, seed)


def split_bf16(x):
    """``(hi, mid, lo)`` of f32 values as the split-bf16 kernel cuts them: ``hi`` the top 16 bits
    of x, ``mid`` the top 16 bits of x - hi, ``lo`` the rest."""
    x = np.asarray(x, dtype=np.float32)

    def top(v):
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)

    hi = top(x)
    r = x - hi
    mid = top(r)
    return hi, mid, r - mid


# The shapes the tests run: one list, so that the CPU test checks exactly what the GPU test feeds.
WIDE_SHAPES = [(65, 77), (65, 4113), (65, 20_011), (300, 77), (300, 4113), (300, 20_011), (1100, 4113)]
SYRK_SHAPES = [(65, 700), (65, 9001), (257, 700), (257, 9001)]
PATCH_D = [32, 64]
PATCH_N = [n for n in TALL_N if n >= 64]
B_TALL_D = [9, 33, 64]
B_SYRK_D = [65, 257]
ONE_ROW_D = [10, 64, 66]
COLS_D = [1, 4, 8, 9, 33, 64]


def all_cases():
    """Every Family A / B case the GPU test feeds to a kernel."""
    out = [family_a(n, d) for d in sorted(set(TALL_D + COLS_D + [7])) for n in TALL_N]
    out += [family_a(n, d, zeros="rare") for d in PATCH_D for n in PATCH_N]
    for d, n in WIDE_SHAPES:
        out += [family_a(n, d, off=off, label=label) for off in ("none", "hundred") for label in ("plain", "zero_sum")]
    out += [family_a(n, d) for d, n in SYRK_SHAPES]
    out += [family_b(d) for d in B_TALL_D + B_SYRK_D]
    return out
