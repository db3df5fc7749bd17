"""Grouped aggregation on the host: the numpy twins of the ``groupby.hip`` kernels against a
plain-Python oracle (exact ``==``), the fixed-point sum's window, and the DataFrame / SQL surface
(``groupBy`` / ``agg`` / ``distinct`` / ``dropDuplicates`` / ``GROUP BY``), alone and on two ranks."""
import math
import multiprocessing as mp
import os
import random
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch

import _groupby_cases as gc
from conftest import data_path
from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb
from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.expressions import AnalysisException

NAN, INF = gc.NAN, gc.INF
TRIP = kernels.group_limits()[0]


# ---- twins against the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["mixed", "one", "wave64", "alt", "holes"])
@pytest.mark.parametrize("n", [0, 1, 65, TRIP + 1, 3 * TRIP + 77])
def test_twin_equals_oracle(n, pattern):
    f = gc.make_frame(n, pattern)
    enc, acc, off, slots = gc.run_frame(f)
    cells = gc.null_by(gc.finalise(acc, off, slots), slots, gc.FRAME_COUNTS)
    gc.assert_cells(cells, gc.frame_oracle(f))
    assert enc.mode == "direct"
    enc_h, acc_h, _, _ = gc.run_frame(f, mode="hash")  # the other encoding: the same groups
    keep, keep_h = acc[:, 0] > 0, acc_h[:, 0] > 0
    assert torch.equal(acc[keep], acc_h[keep_h]) and enc_h.mode == "hash"


def test_float_keys_fold_zero_and_nan_null_first():
    nan2 = np.array([0x7FF0000000000001, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)
    k = torch.from_numpy(np.concatenate([[0.0, -0.0, NAN], nan2, [INF, -INF, 1.5, 7.0, -2.5]]))  # (payloads kept)
    valid = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=torch.bool)
    enc = gb.group_encode(k, valid)
    # null, -inf, -2.5, 0, 1.5, +inf, NaN
    assert enc.G == 7 and enc.gid.tolist() == [3, 3, 6, 6, 6, 5, 1, 4, 0, 2]
    vals = gb.keys_to_values(enc.keys, torch.float64).tolist()[1:]
    assert vals[:5] == [-INF, -2.5, 0.0, 1.5, INF] and math.isnan(vals[5]) and math.copysign(1.0, vals[2]) == 1.0
    # MIN / MAX keep -0.0 below +0.0 and put NaN on top
    acc, off = gb.group_agg(None, 1, [(gb.MIN, k[:2], None), (gb.MAX, k[:2], None)])
    lo, hi = (gb.keys_to_values(acc[:, w] ^ gc.I64_MIN, torch.float64).item() for w in off)
    assert (math.copysign(1.0, lo), math.copysign(1.0, hi)) == (-1.0, 1.0)
    acc, off = gb.group_agg(None, 1, [(gb.MAX, k, valid)])
    assert math.isnan(gb.keys_to_values(acc[:, off[0]] ^ gc.I64_MIN, torch.float64).item())


def test_int64_extremes_bool_and_two_column_keys():
    k = torch.tensor([gc.I64_MAX, gc.I64_MIN, 0, gc.I64_MAX, gc.I64_MIN, -1], dtype=torch.int64)
    enc = gb.group_encode(k)
    assert enc.mode == "hash" and enc.gid.tolist() == [4, 1, 3, 4, 1, 2]
    assert enc.keys.tolist()[1:] == [gc.I64_MIN, -1, 0, gc.I64_MAX]
    b = torch.tensor([True, False, True, True], dtype=torch.bool)
    enc = gb.group_encode(b, torch.tensor([1, 1, 0, 1], dtype=torch.bool))
    assert enc.mode == "direct" and enc.gid.tolist() == [2, 1, 0, 2]
    # two columns: first the most significant, null first in each
    a = torch.tensor([2, 1, 2, 1, 1], dtype=torch.int32)
    c = torch.tensor([0.5, NAN, 0.5, -0.0, 0.0], dtype=torch.float64)
    va = torch.tensor([1, 1, 1, 0, 1], dtype=torch.bool)
    gid, G, kv = gb.group_encode_columns([a, c], [va, None])
    acc, _ = gb.group_agg(gid, G, [])
    keep = acc[:, 0] > 0
    rows = [(x if ox else None, y if oy else None) for (x, ox, y, oy) in
            zip(kv[0][0][keep].tolist(), kv[0][1][keep].tolist(), kv[1][0][keep].tolist(), kv[1][1][keep].tolist())]
    assert repr(rows) == repr([(None, 0.0), (1, 0.0), (1, NAN), (2, 0.5)]) and acc[keep, 0].tolist() == [1, 1, 1, 2]
    with pytest.raises(ValueError, match="63 bits"):
        wide = torch.tensor([0, (1 << 20) - 1], dtype=torch.int32)  # a direct range of 2^20 slots each
        gb.group_encode_columns([wide, wide, wide, wide])


def test_sum_flags_nulls_cancellation_and_wraparound():
    # groups 0..7: every combination of NaN (1), +inf (2), -inf (4) next to a finite value
    g, x = [], []
    for combo in range(8):
        vals = [1.25] + [v for bit, v in ((1, NAN), (2, INF), (4, -INF)) if combo & bit]
        g += [combo] * len(vals)
        x += vals
    g += [8, 8, 9, 9, 9]  # 8: only nulls; 9: x, -x cancellation next to a small term
    x += [5.0, 6.0, 1e16, -1e16, 0.125]
    valid = [True] * (len(g) - 5) + [False, False, True, True, True]
    gid = torch.tensor(g, dtype=torch.int32)
    xs, v = torch.tensor(x, dtype=torch.float64), torch.tensor(valid)
    slots = gc.scales([(gb.COUNT, None, v, 0), (gb.SUM_F, xs, v, None), (gb.MIN, xs, v, 0), (gb.MAX, xs, v, 0)], None)
    acc, off = gb.group_agg(gid, 10, slots)
    cells = gc.null_by(gc.finalise(acc, off, slots), slots, [None, 1, 1, 1])
    groups = gc.oracle_groups([(k,) for k in g], None)
    gc.assert_cells(cells, gc.oracle_cells(groups, [(gb.COUNT, None, valid), (gb.SUM_F, x, valid), (gb.MIN, x, valid),
                                                    (gb.MAX, x, valid)]))
    assert cells[8] == [2, 0, None, None, None] and cells[9][2] == 0.125
    # Java wraparound
    l = torch.tensor([gc.I64_MAX, 1, gc.I64_MIN, -1], dtype=torch.int64)
    acc, off = gb.group_agg(torch.tensor([0, 0, 1, 1], dtype=torch.int32), 2, [(gb.SUM_I, l, None)])
    assert acc[:, off[0]].tolist() == [gc.I64_MIN, gc.I64_MAX]
    i = torch.full((5,), 2 ** 31 - 1, dtype=torch.int32)
    acc, off = gb.group_agg(None, 1, [(gb.SUM_I, i, None)])
    assert acc[0, off[0]].item() == 5 * (2 ** 31 - 1)


def test_fixed_point_sum_equals_fsum_within_2_pow_60():
    rnd = random.Random(5)
    for trial in range(200):
        n = rnd.choice([1, 2, 7, 64, 1000])
        span = rnd.choice([0, 10, 40, 58])  # magnitudes within 2^60 of each other
        scale = rnd.choice([1.0, 1e-3, 123456.789, 2.0 ** -900, 2.0 ** 900])
        top = rnd.random() + 0.5
        xs = [top] + [rnd.choice([-1, 1]) * (rnd.random() + 0.5) * 2.0 ** rnd.randint(-span, 0) for _ in range(n - 1)]
        if trial % 5 == 0:
            xs = xs + [-v for v in xs[: n // 2]]  # cancellation
        xs = [v * scale for v in xs]
        x = torch.tensor(xs, dtype=torch.float64)
        (e,) = gb.group_scale([x], [None], None)
        assert e == math.frexp(max(abs(v) for v in xs))[1]
        acc, off = gb.group_agg(None, 1, [(gb.SUM_F, x, None, e)])
        w = off[0]
        assert gb.finalize_sum(acc[:, w:w + 4], acc[:, w + 4], e).item() == math.fsum(xs)


def test_fixed_point_window_bound_over_2_pow_200():
    rnd = random.Random(9)
    n, G = 600, 3
    xs = [rnd.choice([-1, 1]) * (rnd.random() + 0.5) * 2.0 ** rnd.randint(-200, 0) for _ in range(n)]
    xs[0], xs[1], xs[2], xs[3] = 1e300 * 2.0 ** -996, 1e-300 * 2.0 ** 796, -1e300 * 2.0 ** -996, 3.0 * 2.0 ** -190
    g = [r % G for r in range(n)]
    x = torch.tensor(xs, dtype=torch.float64)
    (e,) = gb.group_scale([x], [None], None)
    acc, off = gb.group_agg(torch.tensor(g, dtype=torch.int32), G, [(gb.SUM_F, x, None, e)])
    got = gb.finalize_sum(acc[:, 1:5], acc[:, 5], e).tolist()
    for k in range(G):
        part = [Fraction(v) for v, gg in zip(xs, g) if gg == k]
        exact = sum(part)
        ulp = math.ulp(got[k])
        assert abs(Fraction(got[k]) - exact) <= len(part) * Fraction(2) ** (e - 128) + Fraction(ulp) / 2


def test_shards_add_up_and_first_honours_row_offset():
    f = gc.make_frame(3000, "mixed", seed=3)
    enc, acc, off, slots = gc.run_frame(f)
    cut = 1337
    parts = []
    for lo, hi in ((0, cut), (cut, 3000)):
        sl = [(op, None if c is None else c[lo:hi], None if v is None else v[lo:hi], e) for op, c, v, e in slots]
        a, _ = gb.group_agg(enc.gid[lo:hi], enc.G, sl, f["sel"][lo:hi], row_offset=lo)
        parts.append(a)
    kinds = [gb.K_ADD] + gb.word_kinds([s[0] for s in slots])
    assert torch.equal(combine(parts[0], parts[1], kinds), acc)


def combine(a, b, kinds):
    out = a.clone()
    for w, k in enumerate(kinds):
        if k == gb.K_ADD:
            out[:, w] = a[:, w] + b[:, w]
        elif k == gb.K_OR:
            out[:, w] = a[:, w] | b[:, w]
        else:  # unsigned max / min through the sign-flipped words
            x, y = a[:, w] ^ gc.I64_MIN, b[:, w] ^ gc.I64_MIN
            out[:, w] = (torch.maximum(x, y) if k == gb.K_MAX else torch.minimum(x, y)) ^ gc.I64_MIN
    return out


# ---- API and SQL ---------------------------------------------------------------------------------
def lab_frame(spark):
    df = spark.read.format("csv").option("inferSchema", "true").option("header", "false").load(data_path("dataset-abstract.csv"))
    return df.withColumnRenamed("_c0", "guest").withColumnRenamed("_c1", "price")


def lab_rows():
    rows = []
    with open(data_path("dataset-abstract.csv")) as fh:
        for line in fh:
            a, b = line.strip().split(",")
            rows.append((int(a), float(b)))
    return rows


EDGE_ROWS = [("a", 1.0, None, True), ("b", 2.0, 1, False), (None, 3.0, 2, True), ("a", NAN, 3, None),
             ("b", -2.0, None, False), ("a", 1.0, None, True), (None, None, 2, True), ("c", None, None, None)]
EDGE_SCHEMA = "s string, x double, k int, b boolean"


def api_results(spark, lab=True):
    """Every API / SQL case as plain tuples (one list per case), for the host checks and the
    engine-to-engine comparisons."""
    out = {}
    rows = lambda df: [tuple(r) for r in df.collect()]  # noqa: E731
    if lab:
        df = lab_frame(spark)
        out["count"] = rows(df.groupBy("guest").count())
        out["agg"] = rows(df.groupBy("guest").agg(F.count("*"), F.count("price"), F.sum("price"), F.avg("price"),
                                                  F.min("price"), F.max("price"), F.sum("guest"), F.mean("guest")))
        out["agg_dict"] = rows(df.groupby("guest").agg({"price": "avg"}))
        out["global"] = rows(df.agg(F.count("*"), F.sum("price"), F.max("guest")))
        out["empty"] = rows(df.filter("guest > 1000").agg(F.count("*"), F.count("price"), F.sum("price"), F.avg("price"),
                                                        F.min("guest"), F.max("price")))
        out["filtered"] = rows(df.filter("price > 50").groupBy("guest").agg(F.sum("price").alias("total")))
        out["expr_key"] = rows(df.groupBy((df.col("guest") % 3).alias("m")).agg(F.sum(df.col("price") * 2)))
        out["distinct"] = rows(df.select("guest").distinct())
        out["dedupe"] = rows(df.dropDuplicates(["guest"]))
        out["dedupe_all"] = rows(df.union(df).dropDuplicates())
        df.createOrReplaceTempView("v")
        out["sql_group"] = rows(spark.sql("SELECT guest, count(*) c, avg(price) AS ap, max(price) FROM v WHERE price > 50 "
                                          "GROUP BY guest LIMIT 6"))
        out["sql_distinct"] = rows(spark.sql("SELECT DISTINCT guest FROM v"))
        out["sql_global"] = rows(spark.sql("SELECT count(*), min(price), sum(guest) FROM v"))
        out["sql_expr"] = rows(spark.sql("SELECT guest % 2 AS odd, count(price) FROM v GROUP BY guest % 2"))
    d = spark.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    out["edge_s"] = rows(d.groupBy("s").agg(F.sum("x"), F.avg("x"), F.count("k"), F.min("k"), F.max("x"), F.min("b")))
    out["edge_sk"] = rows(d.groupBy("s", "k").count())
    out["edge_b"] = rows(d.groupBy("b").sum())
    out["edge_x"] = rows(d.groupBy("x").agg(F.count("s")))
    out["edge_distinct"] = rows(d.select("s", "b").distinct())
    out["edge_dedupe"] = rows(d.dropDuplicates(["s"]))
    out["edge_dedupe_all"] = rows(d.dropDuplicates())
    return out


def test_api_on_the_lab_csv(cpu_session):
    df, rows = lab_frame(cpu_session), lab_rows()
    by = {}
    for g, p in rows:
        by.setdefault(g, []).append(p)
    r = df.groupBy("guest").count()
    assert [(f.name, f.dataType.simpleString(), f.nullable) for f in r.schema.fields] == \
        [("guest", "int", True), ("count", "bigint", False)]
    assert [tuple(x) for x in r.collect()] == [(g, len(by[g])) for g in sorted(by)]
    a = df.groupBy("guest").agg(F.count("*"), F.sum("price"), F.avg("price"), F.min("price"), F.max("price"), F.sum("guest"),
                                F.mean("guest"))
    assert [(f.name, f.dataType.simpleString(), f.nullable) for f in a.schema.fields] == [
        ("guest", "int", True), ("count(1)", "bigint", False), ("sum(price)", "double", True),
        ("avg(price)", "double", True), ("min(price)", "double", True), ("max(price)", "double", True),
        ("sum(guest)", "bigint", True), ("avg(guest)", "double", True)]
    want = [(g, len(by[g]), math.fsum(by[g]), math.fsum(by[g]) / len(by[g]), min(by[g]), max(by[g]), g * len(by[g]),
             float(g * len(by[g])) / len(by[g])) for g in sorted(by)]
    assert [tuple(x) for x in a.collect()] == want
    d = df.groupby("guest").agg({"price": "avg"})
    assert d.columns == ["guest", "avg(price)"] and [tuple(x) for x in d.collect()] == [(w[0], w[3]) for w in want]
    assert [tuple(x) for x in df.groupBy("guest").max().collect()] == [(g, max(by[g])) for g in sorted(by)]
    e = df.filter("guest > 1000").agg(F.count("*"), F.sum("price"), F.avg("price"), F.min("guest"))
    assert [tuple(x) for x in e.collect()] == [(0, None, None, None)]
    assert [tuple(x) for x in df.agg(F.count("price"), F.max("guest")).collect()] == [(len(rows), max(by))]
    assert [tuple(x) for x in df.select("guest").distinct().collect()] == [(g,) for g in sorted(by)]
    assert df.distinct().count() == len(set(rows))
    first = {}
    for g, p in rows:
        first.setdefault(g, p)
    kept = df.dropDuplicates(["guest"])
    assert [tuple(x) for x in kept.collect()] == [(g, p) for g, p in first.items()]  # row order, first rows
    assert kept._table().nrows == len(rows)  # no row moved: only the selection narrowed
    assert [tuple(x) for x in df.union(df).drop_duplicates().collect()] == list(dict.fromkeys(rows))


def test_sql_group_by_count_star_and_distinct(cpu_session):
    df, rows = lab_frame(cpu_session), lab_rows()
    df.createOrReplaceTempView("v")
    by = {}
    for g, p in rows:
        if p > 50:
            by.setdefault(g, []).append(p)
    q = cpu_session.sql("SELECT guest, count(*) c, avg(price) AS ap, max(price) FROM v WHERE price > 50 GROUP BY guest LIMIT 6")
    assert q.columns == ["guest", "c", "ap", "max(price)"]
    assert [tuple(x) for x in q.collect()] == [(g, len(by[g]), math.fsum(by[g]) / len(by[g]), max(by[g]))
                                                for g in sorted(by)][:6]
    d = cpu_session.sql("SELECT DISTINCT guest FROM v")
    assert [tuple(x) for x in d.collect()] == [(g,) for g in sorted({g for g, _ in rows})]
    assert len(d.collect()) < len(rows)  # (the keyword was once accepted and ignored)
    g = cpu_session.sql("SELECT count(*), min(price), sum(guest) FROM v")
    assert [tuple(x) for x in g.collect()] == [(len(rows), min(p for _, p in rows), sum(g for g, _ in rows))]
    o = cpu_session.sql("SELECT guest % 2 AS odd, count(price) FROM v GROUP BY guest % 2")
    assert [tuple(x) for x in o.collect()] == [(m, len([1 for g, _ in rows if g % 2 == m])) for m in (0, 1)]


def test_edge_frame_nulls_nan_strings_booleans(cpu_session):
    got = api_results(cpu_session, lab=False)
    assert repr(got["edge_s"]) == repr([(None, 3.0, 3.0, 2, 2, 3.0, True), ("a", NAN, NAN, 1, 3, NAN, True),
                                        ("b", 0.0, 0.0, 1, 1, 2.0, False), ("c", None, None, 0, None, None, None)])
    assert got["edge_sk"] == [(None, 2, 2), ("a", None, 2), ("a", 3, 1), ("b", None, 1), ("b", 1, 1), ("c", None, 1)]
    assert repr(got["edge_b"]) == repr([(None, NAN, 3), (False, 0.0, 1), (True, 5.0, 4)])
    assert repr(got["edge_x"]) == repr([(None, 1), (-2.0, 1), (1.0, 2), (2.0, 1), (3.0, 0), (NAN, 1)])
    assert got["edge_distinct"] == [(None, True), ("a", None), ("a", True), ("b", False), ("c", None)]
    assert [r[0] for r in got["edge_dedupe"]] == ["a", "b", None, "c"]
    assert len(got["edge_dedupe_all"]) == 7


def test_errors(cpu_session):
    df = lab_frame(cpu_session)
    df.createOrReplaceTempView("v")
    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    with pytest.raises(AnalysisException, match="only allowed in agg"):
        df.select(F.sum("price"))
    with pytest.raises(AnalysisException, match="only allowed in agg"):
        df.withColumn("t", F.count("*"))
    with pytest.raises(AnalysisException, match="only allowed in agg"):
        df.filter(F.max("price") > 3).count()
    with pytest.raises(AnalysisException, match="not supported yet"):
        d.agg(F.min("s"))
    with pytest.raises(AnalysisException, match="not supported yet"):
        d.groupBy("k").agg(F.max("s"))
    with pytest.raises(AnalysisException, match="numeric"):
        d.agg(F.sum("s"))
    with pytest.raises(AnalysisException, match="not a numeric column"):
        d.groupBy("k").avg("s")
    with pytest.raises(AnalysisException):
        df.groupBy("nope")
    with pytest.raises(AnalysisException):
        df.agg(F.sum("nope"))
    with pytest.raises(AnalysisException):
        df.dropDuplicates(["nope"])
    with pytest.raises(TypeError):
        df.dropDuplicates("guest")
    with pytest.raises(AnalysisException, match="neither present in the group by"):
        df.groupBy("guest").agg(df.col("price"))
    with pytest.raises(AnalysisException, match="neither present in the group by"):
        cpu_session.sql("SELECT price, count(*) FROM v GROUP BY guest")
    with pytest.raises(AnalysisException, match="neither present in the group by"):
        cpu_session.sql("SELECT guest, count(*) FROM v")
    with pytest.raises(AnalysisException, match="where clause"):
        cpu_session.sql("SELECT guest FROM v WHERE count(*) > 1")
    with pytest.raises(ValueError):
        df.groupBy("guest").agg()


def test_prune_columns_passes_key_and_input_references(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import Aggregate, prune_columns

    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    wide = d.withColumn("x2", d.col("x") * 2).withColumn("unused", d.col("k") + 1)
    agg = Aggregate(wide._plan, ["s"], [("sum", "x2", "t")])
    pruned = prune_columns(agg, {"t"})
    assert isinstance(pruned, Aggregate) and sorted(pruned.child.schema().names) == ["s", "x2"]
    assert "Aggregate [s] [t]" in pruned.describe()


# ---- two ranks (gloo) ------------------------------------------------------------------------
def _dp_rows():
    rng = np.random.default_rng(23)
    rows = []
    for j in range(120):
        k = None if j % 17 == 0 else int(rng.integers(-4, 5))
        x = None if j % 7 == 0 else (NAN if j == 50 else float(np.round(rng.standard_normal() * 10.0 ** rng.integers(-3, 4), 4)))
        rows.append((k, x, f"s{j % 5}" if j % 11 else None, float(j % 3), int(rng.integers(-2 ** 40, 2 ** 40))))
    return rows


_DP_SCHEMA = "k int, x double, s string, f double, l long"
_DP_SPLIT = 41


def _dp_results(spark, rows):
    df = spark.createDataFrame(rows, _DP_SCHEMA)
    t = lambda d: [tuple(r) for r in d.collect()]  # noqa: E731
    aggs = [F.count("*"), F.count("x"), F.sum("x"), F.avg("x"), F.min("x"), F.max("x"), F.sum("l"), F.max("l")]
    return (t(df.groupBy("k").agg(*aggs)), t(df.groupBy("s", "f").agg(*aggs)), t(df.groupBy("f").agg(F.sum("x"))),
            t(df.agg(*aggs)), t(df.filter("k > 100").agg(*aggs)), t(df.select("k", "s").distinct()),
            t(df.dropDuplicates(["k"])), t(df.dropDuplicates(["s", "f"])), t(df.filter("x > 0").dropDuplicates(["k"])),
            t(df.groupBy("l").count())[:5])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    rows = _dp_rows()
    mine = rows[:_DP_SPLIT] if rank == 0 else rows[_DP_SPLIT:]
    spark = SparkSession.builder().master("cpu").getOrCreate()
    q.put((rank, _dp_results(spark, mine)))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_equal_single_process(cpu_session):
    want = _dp_results(cpu_session, _dp_rows())
    assert len(want[0]) == 10 and len(want[6]) == 10
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, got in res:
        assert repr(got) == repr(want)  # exact, NaN cells included
