"""Shared cases of the window API tests (host and device sessions): one table, the same queries
through ``Window`` / ``Column.over`` and through SQL ``OVER``, the oracle's answer for every
column, and the groupBy identity."""
import numpy as np
import torch

import _window_cases as wc
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.window import Window

N = 240
SCHEMA = "id int, k string, ts double, price double, qty long, tag string"
KEYS = ("ams", "ber", "cph", None)


def make_rows(seed=5):
    rng = np.random.default_rng(seed)
    price = wc.dyadic(rng, N).tolist()
    rows = []
    for i in range(N):
        rows.append((i, KEYS[rng.integers(0, 4)], None if rng.random() < 0.1 else float(rng.integers(0, 9)),
                     None if rng.random() < 0.15 else price[i], int(rng.integers(-(1 << 40), 1 << 40)),
                     None if rng.random() < 0.1 else f"t{rng.integers(0, 50)}"))
    return rows


ROWS = make_rows()


def frame_df(spark):
    df = spark.createDataFrame(ROWS, SCHEMA)
    df.createOrReplaceTempView("trades")
    return df


def oracle_case():
    """The table as a case of ``_window_cases.oracle``: partitionBy(k) orderBy(ts desc nulls last)."""
    code = {k: i for i, k in enumerate(KEYS)}
    col = lambda j, dt, fill: torch.tensor([fill if r[j] is None else r[j] for r in ROWS], dtype=dt)  # noqa: E731
    ok = lambda j: torch.tensor([r[j] is not None for r in ROWS])  # noqa: E731
    return {"n": N, "parts": [(torch.tensor([code[r[1]] for r in ROWS]), ok(1))],
            "orders": [(col(2, torch.float64, 0.0), ok(2), False, False)],
            "v": col(3, torch.float64, 0.0), "vvalid": ok(3), "iv": col(4, torch.int64, 0), "sel": None, "e": 0}


W = Window.partitionBy("k").orderBy(F.desc("ts"))
OVER = "PARTITION BY k ORDER BY ts DESC"
UP, UF, CR = Window.unboundedPreceding, Window.unboundedFollowing, Window.currentRow
# oracle frame name -> (specification, SQL frame clause)
FRAME_SPECS = {
    "default": (W, ""),
    "whole": (W.rowsBetween(UP, UF), " ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING"),
    "running": (W.rowsBetween(UP, CR), " ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"),
    "slide": (W.rowsBetween(-3, 3), " ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING"),
    "ahead": (W.rowsBetween(1, 2), " ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING"),
    "rest": (W.rowsBetween(CR, UF), " ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING"),
}


def _ntile(r, size, n):
    q, rem = divmod(size, n)
    cut = rem * (q + 1)
    return (r - 1) // (q + 1) + 1 if r - 1 < cut else rem + (r - 1 - cut) // q + 1


def columns():
    """``(name, Column, SQL text, oracle row -> expected value)`` for every function and frame kind."""
    out = [
        ("rn", F.row_number().over(W), f"row_number() OVER ({OVER})", lambda o, r: o["row_number"]),
        ("rk", F.rank().over(W), f"rank() OVER ({OVER})", lambda o, r: o["rank"]),
        ("dr", F.dense_rank().over(W), f"dense_rank() OVER ({OVER})", lambda o, r: o["dense_rank"]),
        ("pr", F.percent_rank().over(W), f"percent_rank() OVER ({OVER})",
         lambda o, r: (o["rank"] - 1) / (o["size"] - 1) if o["size"] > 1 else 0.0),
        ("cd", F.cume_dist().over(W), f"cume_dist() OVER ({OVER})", lambda o, r: o["peer_end"] / o["size"]),
        ("nt", F.ntile(4).over(W), f"ntile(4) OVER ({OVER})", lambda o, r: _ntile(o["row_number"], o["size"], 4)),
        ("lg", F.lag("price").over(W), f"lag(price) OVER ({OVER})",
         lambda o, r: None if o["shift-1"] < 0 else ROWS[o["shift-1"]][3]),
        ("ld", F.lead("qty", 1, -7).over(W), f"lead(qty, 1, -7) OVER ({OVER})",
         lambda o, r: -7 if o["shift1"] < 0 else ROWS[o["shift1"]][4]),
        ("lt", F.lag("tag", 1, "none").over(W), f"lag(tag, 1, 'none') OVER ({OVER})",
         lambda o, r: "none" if o["shift-1"] < 0 else ROWS[o["shift-1"]][5]),
        ("all", F.count("*").over(Window.partitionBy("k")), "count(*) OVER (PARTITION BY k)", lambda o, r: o["size"]),
        ("psum", F.sum("price").over(Window.partitionBy("k")), "sum(price) OVER (PARTITION BY k)", lambda o, r: o["whole.sum"]),
        ("rsum", F.sum("price").over(W.rangeBetween(UP, CR)),
         f"sum(price) OVER ({OVER} RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)", lambda o, r: o["default.sum"]),
    ]
    for name, (spec, clause) in FRAME_SPECS.items():
        ov = f"OVER ({OVER}{clause})"
        out += [
            (f"{name}_c", F.count("price").over(spec), f"count(price) {ov}", lambda o, r, n=name: o[n + ".count"]),
            (f"{name}_s", F.sum("price").over(spec), f"sum(price) {ov}", lambda o, r, n=name: o[n + ".sum"]),
            (f"{name}_q", F.sum("qty").over(spec), f"sum(qty) {ov}",
             lambda o, r, n=name: _qty_sum(o, r, n)),
            (f"{name}_a", F.avg("price").over(spec), f"avg(price) {ov}",
             lambda o, r, n=name: None if not o[n + ".count"] else o[n + ".sum"] / o[n + ".count"]),
        ]
        if name in wc.PICKS:
            out += [
                (f"{name}_mn", F.min("price").over(spec), f"min(price) {ov}", lambda o, r, n=name: o[n + ".min"]),
                (f"{name}_mx", F.max("price").over(spec), f"max(price) {ov}", lambda o, r, n=name: o[n + ".max"]),
            ]
    return out


_QTY = {}


def _qty_sum(o, r, name):
    """sum(qty) of the frame: qty has no nulls, so the oracle's second run (validity all true) answers."""
    return _QTY[name][r]


def expected():
    """column name -> expected values in row order, from the plain-Python oracle."""
    def build():
        case = oracle_case()
        _, res = wc.oracle(case)
        every = dict(case, vvalid=torch.ones(N, dtype=torch.bool))
        _, res_q = wc.oracle(every)
        for name in FRAME_SPECS:
            _QTY[name] = {r: res_q[r][name + ".isum"] for r in range(N)}
        return {name: [fn(res[r], r) for r in range(N)] for name, _, _, fn in columns()}
    return wc.cached("api-expected", build)


def api_table(spark):
    df = frame_df(spark)
    return [tuple(r) for r in df.select("id", *[c.alias(n) for n, c, _, _ in columns()]).collect()]


def sql_table(spark):
    frame_df(spark)
    text = "SELECT id, " + ", ".join(f"{s} AS {n}" for n, _, s, _ in columns()) + " FROM trades"
    return [tuple(r) for r in spark.sql(text).collect()]


def nested_and_latest(spark):
    """``price - avg(price).over(w)`` and "latest record per key" through row_number() == 1."""
    df = frame_df(spark)
    wk = Window.partitionBy("k")
    a = [tuple(r) for r in df.select("id", (F.col("price") - F.avg("price").over(wk)).alias("d")).collect()]
    b = [tuple(r) for r in spark.sql("SELECT id, price - avg(price) OVER (PARTITION BY k) AS d FROM trades").collect()]
    latest = df.withColumn("rn", F.row_number().over(W)).filter(F.col("rn") == 1).drop("rn")
    c = [tuple(r) for r in latest.collect()]
    strs = df.select("id", F.count("*").over(Window.partitionBy("tag")).alias("per_tag"),
                     F.row_number().over(Window.partitionBy("k").orderBy("tag", "id")).alias("by_tag"))
    return a, b, c, [tuple(r) for r in strs.collect()]


# ------------------------------------------------------------------------------------------
# identity with groupBy
# ------------------------------------------------------------------------------------------
def identity_rows():
    rng = np.random.default_rng(9)
    nan, inf = float("nan"), float("inf")
    pool = [nan, -nan, inf, -inf, 1e300, -1e300, 1e-300, 5e-324, -0.0, 0.0, 1.5, -2.25, 1e308, 1e308, 3.0e-10]
    rows = []
    for i in range(400):
        k = None if rng.random() < 0.1 else int(rng.integers(0, 12))
        x = None if rng.random() < 0.1 else (pool[rng.integers(0, len(pool))] if rng.random() < 0.5 else float(rng.standard_normal()))
        if k is not None and k >= 9:  # some groups stay finite
            x = None if x is None else float(rng.standard_normal() * 10 ** float(rng.integers(-30, 30)))
        a = None if rng.random() < 0.1 else int(rng.integers(-(1 << 31), 1 << 31))
        b = None if rng.random() < 0.1 else int(rng.integers(-(1 << 62), 1 << 62))
        rows.append((i, k, x, a, b))
    return rows


def _bits(vals):
    ok = [v is not None for v in vals]
    t = torch.tensor([0.0 if v is None else v for v in vals], dtype=torch.float64)
    return ok, t.view(torch.int64)


def groupby_identity(spark):
    """sum / avg / min / max / count over partitionBy(k) equal groupBy(k) joined back, bit for bit."""
    rows = identity_rows()
    df = spark.createDataFrame(rows, "id int, k int, x double, a int, b long")
    wk = Window.partitionBy("k")
    fns = {"sum": F.sum, "avg": F.avg, "min": F.min, "max": F.max, "count": F.count}
    names = [(f, c) for c in ("x", "a", "b") for f in fns]
    win = df.select("id", "k", *[fns[f](c).over(wk).alias(f"{f}_{c}") for f, c in names]).collect()
    grp = df.groupBy("k").agg(*[fns[f](c).alias(f"{f}_{c}") for f, c in names]).collect()
    by_key = {r[0]: r for r in grp}
    assert len(win) == len(rows) and len(by_key) == 13
    for j, (f, c) in enumerate(names):
        got = [r[2 + j] for r in win]
        want = [by_key[r[1]][1 + j] for r in win]
        assert [type(v) for v in got] == [type(v) for v in want], (f, c)
        gok, gb = _bits([None if v is None else float(v) for v in got])
        wok, wb = _bits([None if v is None else float(v) for v in want])
        assert gok == wok and torch.equal(gb, wb), (f, c)
        if f in ("sum", "count", "min", "max") and c != "x":  # integers: exactly, not through a double
            assert got == want, (f, c)
    return win
