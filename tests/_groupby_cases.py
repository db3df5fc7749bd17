"""Shared cases of the grouped-aggregation tests: row patterns, the standard slot list, and a
plain-Python oracle that groups into a dict and uses ``len`` / ``math.fsum`` / ``min`` / ``max``."""
import math

import numpy as np
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb

NAN, INF = float("nan"), float("inf")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- oracle ------------------------------------------------------------------------------------
def key_order(v):
    """Sort key of one grouping value: null first, -0.0 = 0.0, every NaN equal and last."""
    if v is None:
        return (0, 0)
    if isinstance(v, float) and math.isnan(v):
        return (2, 0)
    return (1, v + 0.0 if isinstance(v, float) else v)


def value_order(v):
    """Order of MIN / MAX: -0.0 < 0.0, NaN the largest."""
    if isinstance(v, float):
        if math.isnan(v):
            return (1, 0, 0)
        return (0, v, 0 if (v == 0 and math.copysign(1.0, v) < 0) else 1)
    return (0, v, 1)


def oracle_sum(vals):
    if not vals:
        return None
    if any(math.isnan(v) for v in vals) or (INF in vals and -INF in vals):
        return NAN
    if INF in vals:
        return INF
    if -INF in vals:
        return -INF
    return math.fsum(vals)


def wrap64(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def oracle_groups(keys, sel):
    """{group order key: [row index...]} of the live rows; ``keys``: one tuple per row."""
    groups = {}
    for r, k in enumerate(keys):
        if sel is None or sel[r]:
            groups.setdefault(tuple(key_order(v) for v in k), []).append(r)
    return dict(sorted(groups.items()))


def oracle_cells(groups, ops_cols):
    """One row of cells per group (key order) for ``ops_cols`` = [(op, values, valid)] with python
    lists; a null cell is None.  Sums of floats are ``math.fsum``, of ints wrap like a Java long."""
    out = []
    for rows in groups.values():
        cells = [len(rows)]
        for op, vals, valid in ops_cols:
            live = [vals[r] for r in rows if valid is None or valid[r]] if vals is not None else None
            if op == gb.COUNT:
                cells.append(len([r for r in rows if valid is None or valid[r]]))
            elif op == gb.FIRST:
                cells.append(min(rows))
            elif op == gb.SUM_I:
                cells.append(wrap64(sum(live)) if live else None)
            elif op == gb.SUM_F:
                cells.append(oracle_sum([float(v) for v in live]))
            elif op == gb.MIN:
                cells.append(min(live, key=value_order) if live else None)
            elif op == gb.MAX:
                cells.append(max(live, key=value_order) if live else None)
        out.append(cells)
    return out


def same_cell(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        a, b = float(a), float(b)
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    return a == b


def assert_cells(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, (rg, rw) in enumerate(zip(got, want)):
        for c, (a, b) in enumerate(zip(rg, rw)):
            assert same_cell(a, b), f"group {g} cell {c}: got {a!r}, want {b!r}"


# ---- engines -----------------------------------------------------------------------------------
def finalise(acc, off, slots, row_offset=0):
    """Python cells (per kept group: rows, then one per slot) of raw accumulators, through the
    finalisation both engines share.  A COUNT slot of the same validity decides nullness: here a
    cell is null when its identity survived (MIN / MAX / FIRST) or when the sum saw no row, which
    the caller states by passing ``count`` slots: see ``null_by``."""
    acc = acc.cpu()
    keep = torch.nonzero(acc[:, 0] > 0).flatten()
    acc = acc[keep]
    cols = [acc[:, 0].tolist()]
    for (op, col, valid, e), w in zip(slots, off):
        if op in (gb.COUNT, gb.SUM_I):
            cols.append(acc[:, w].tolist())
        elif op == gb.FIRST:
            cols.append([v - row_offset for v in acc[:, w].tolist()])
        elif op == gb.SUM_F:
            cols.append(gb.finalize_sum(acc[:, w:w + 4], acc[:, w + 4], e).tolist())
        else:
            v = gb.keys_to_values(acc[:, w] ^ I64_MIN, col.dtype)
            cols.append(v.tolist())
    return [list(r) for r in zip(*cols)] if len(keep) else []


def null_by(cells, slots, counts):
    """Null out the value cells of groups whose matching count is 0.  ``counts[i]``: the cell
    index (1-based slot position) of the COUNT slot that shares slot i's validity, or None."""
    for row in cells:
        for i, c in enumerate(counts):
            if c is not None and row[c] == 0:
                row[1 + i] = None
    return cells


def scales(slots, sel):
    """The slots with the exponent of every SUM_F filled in (one ABSMAX pre-pass)."""
    need = [i for i, s in enumerate(slots) if s[0] == gb.SUM_F]
    es = gb.group_scale([slots[i][1] for i in need], [slots[i][2] for i in need], sel)
    slots = list(slots)
    for i, e in zip(need, es):
        slots[i] = slots[i][:3] + (e,)
    return slots


# ---- the standard frame --------------------------------------------------------------------------
def make_frame(n, pattern="mixed", seed=0):
    """Columns of n rows (host tensors): an int32 key by ``pattern``, values x f64 / y f32 / i i32 /
    l i64, a validity mask per column (each different), and a selection.  Dead and null rows hold
    NaN or garbage.  Magnitudes of the floats span less than 2^40, so their sums are exact."""
    rng = np.random.default_rng(seed + 7919 * n)
    r = np.arange(n)
    if pattern == "one":
        key = np.full(n, 42)
    elif pattern == "wave64":
        key = r % 64
    elif pattern == "alt":
        key = r % 2
    elif pattern == "holes":
        key = np.array([0, 5, 1000])[r % 3] - 500
    else:
        key = rng.integers(-20, 20, n)
    x = rng.integers(-1 << 20, 1 << 20, n) * 2.0 ** rng.integers(-20, 0, n)
    y = (rng.integers(-1 << 10, 1 << 10, n) * 2.0 ** rng.integers(-8, 0, n)).astype(np.float32)
    i = rng.integers(-1 << 31, 1 << 31, n).astype(np.int32)
    l = rng.integers(-1 << 62, 1 << 62, n)
    sel = rng.random(n) < 0.7
    vk, vx, vy, vl = (rng.random(n) < p for p in (0.95, 0.8, 0.9, 0.85))
    x[~vx] = NAN
    x[~sel] = NAN
    y[~sel] = -INF
    l[~vl] = I64_MAX
    t = torch.from_numpy
    return dict(key=t(key.astype(np.int32)), vk=t(vk), x=t(x), vx=t(vx), y=t(y), vy=t(vy), i=t(i), l=t(l), vl=t(vl),
                sel=t(sel))


def frame_slots(f):
    """13 slots (two chunks of a launch's 7 + ROWS): every op, every value dtype."""
    return [(gb.COUNT, None, f["vx"], 0), (gb.SUM_F, f["x"], f["vx"], None), (gb.MIN, f["x"], f["vx"], 0),
            (gb.MAX, f["x"], f["vx"], 0), (gb.COUNT, None, f["vy"], 0), (gb.SUM_F, f["y"], f["vy"], None),
            (gb.MAX, f["y"], f["vy"], 0), (gb.SUM_I, f["i"], None, 0), (gb.MIN, f["i"], None, 0),
            (gb.COUNT, None, f["vl"], 0), (gb.SUM_I, f["l"], f["vl"], 0), (gb.MAX, f["l"], f["vl"], 0),
            (gb.FIRST, None, None, 0)]


FRAME_COUNTS = [None, 1, 1, 1, None, 5, 5, None, None, None, 10, 10, None]  # cell of the COUNT that nulls slot i


def frame_oracle(f):
    py = {k: v.tolist() for k, v in f.items()}
    keys = [(k if ok else None,) for k, ok in zip(py["key"], py["vk"])]
    groups = oracle_groups(keys, py["sel"])
    ops_cols = [(gb.COUNT, None, py["vx"]), (gb.SUM_F, py["x"], py["vx"]), (gb.MIN, py["x"], py["vx"]),
                (gb.MAX, py["x"], py["vx"]), (gb.COUNT, None, py["vy"]), (gb.SUM_F, py["y"], py["vy"]),
                (gb.MAX, py["y"], py["vy"]), (gb.SUM_I, py["i"], None), (gb.MIN, py["i"], None),
                (gb.COUNT, None, py["vl"]), (gb.SUM_I, py["l"], py["vl"]), (gb.MAX, py["l"], py["vl"]),
                (gb.FIRST, None, None)]
    return oracle_cells(groups, ops_cols)


def to_device(f, dev):
    return {k: v.to(dev) for k, v in f.items()}


def run_frame(f, blocks=None, capacity=None, mode=None):
    """(gid, G, acc, off, slots) of the standard slots over the frame's tensors, on their device."""
    enc = gb.group_encode(f["key"], f["vk"], f["sel"], capacity=capacity, blocks=blocks, mode=mode)
    slots = scales(frame_slots(f), f["sel"])
    acc, off = gb.group_agg(enc.gid, enc.G, slots, f["sel"], blocks=blocks)
    return enc, acc, off, slots
