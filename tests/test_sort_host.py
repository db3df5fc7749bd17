"""Sorting on the host: the numpy twin of the ``sort.hip`` kernels against the plain-Python oracle
(the same permutation, ``torch.equal``), and the DataFrame / SQL surface (``orderBy`` / ``sort`` /
``sortWithinPartitions`` / ``ORDER BY``), alone and on two ranks."""
import math
import multiprocessing as mp
import os
import socket
from functools import cmp_to_key

import pytest
import torch

import _sort_cases as sc
from conftest import data_path
from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.expressions import AnalysisException

NAN, INF = sc.NAN, sc.INF
N = sc.TILE + 77  # (the twin has no tiles; the device tests take the tile's edges)


# ---- the twin against the oracle -----------------------------------------------------------------
def check(frame, ascending, nulls_first, want_live=None):
    stats = []
    got = sc.run(frame, ascending, nulls_first, stats=stats)
    assert got.dtype == torch.int64
    assert torch.equal(got, sc.oracle(frame, ascending, nulls_first))
    if want_live is not None:
        assert [s["live"] for s in stats] == want_live
    return got


@pytest.mark.parametrize("dtype", list(sc.DTYPES))
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_twin_equals_oracle(pattern, dtype):
    plain = sc.make_frame(N, [(pattern, dtype)], seed=1)
    for asc in (True, False):
        check(plain, asc, None)
    nulls = sc.make_frame(N, [(pattern, dtype)], nulls=True, seed=2)  # a 10% validity mask
    for asc, nf in sc.PLACEMENTS:
        check(nulls, asc, nf)
    picked = sc.make_frame(N, [(pattern, dtype)], nulls=True, selection=True, seed=3)  # and an 80% selection
    for asc, nf in sc.PLACEMENTS:
        check(picked, asc, nf)


@pytest.mark.parametrize("name", list(sc.MULTI))
def test_two_and_three_keys_ties_first(name):
    keys, asc, nf = sc.MULTI[name]
    check(sc.make_frame(N, keys, nulls=True, selection=True, seed=5), asc, nf)
    check(sc.make_frame(N, keys, seed=6), asc, nf)


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_small_frames(n):
    check(sc.make_frame(n, [("random64", "i64")], nulls=True, seed=n), True, None)
    check(sc.make_frame(n, [("floats", "f32"), ("ties", "i32")], nulls=True, selection=True, seed=n), [False, True], None)


def test_skipped_and_live_passes():
    eq = sc.make_frame(N, [("equal", "i64")], selection=True, seed=3)
    got = check(eq, True, None, want_live=[[]])  # every pass skipped: the identity over the live rows
    assert torch.equal(got, torch.nonzero(eq[2]).flatten())
    check(sc.make_frame(N, [("random64", "i64")], seed=4), True, None, want_live=[list(range(8))])
    only_null = sc.make_frame(N, [("equal", "f64")], nulls=True, seed=6)
    for asc, nf in sc.PLACEMENTS:
        check(only_null, asc, nf, want_live=[[8]])
    stats = []
    sc.run(([torch.arange(N, dtype=torch.int32) % 4096], [None], None), stats=stats)
    assert stats == [{"live": [0, 1]}]  # 4096 distinct non-negative int32 values: 2 of the 8 byte passes
    dead = (eq[0], eq[1], torch.zeros(N, dtype=torch.bool))
    assert sc.run(dead).numel() == 0


def test_float_rules_and_stability():
    nan2 = torch.tensor([0x7FF0000000000001, -0x7FFFFFFFFFEDD], dtype=torch.int64).view(torch.float64)  # payloads, a sign
    x = torch.cat([torch.tensor([0.0, -0.0, NAN, 1.5, -INF, INF, -0.0, 0.0], dtype=torch.float64), nan2])
    valid = torch.tensor([1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=torch.bool)
    # -inf, the zeros in row order, 1.5, +inf, the NaNs in row order; the null by its placement
    assert kernels.sort_permutation([x], [valid]).tolist() == [7, 4, 0, 1, 6, 3, 5, 2, 8, 9]
    assert kernels.sort_permutation([x], [valid], ascending=False).tolist() == [2, 8, 9, 5, 3, 0, 1, 6, 4, 7]
    assert kernels.sort_permutation([x], [valid], ascending=False, nulls_first=True).tolist() == [7, 2, 8, 9, 5, 3, 0, 1, 6, 4]
    assert kernels.sort_permutation([x], [valid], ascending=True, nulls_first=False).tolist() == [4, 0, 1, 6, 3, 5, 2, 8, 9, 7]


def test_limits_and_bad_arguments():
    threads, run, tile, bits = kernels.sort_limits()
    assert tile == threads * run and bits == 8
    x = torch.zeros(4)
    with pytest.raises(ValueError, match="no sort column"):
        kernels.sort_permutation([])
    with pytest.raises(ValueError, match="one per sort column"):
        kernels.sort_permutation([x, x], ascending=[True])
    with pytest.raises(TypeError):
        kernels.sort_permutation([x.to(torch.float16)])
    with pytest.raises(ValueError, match="one entry per row"):
        kernels.sort_permutation([x], [torch.ones(3, dtype=torch.bool)])


# ---- the API ---------------------------------------------------------------------------------------
def lab_frame(spark, name="dataset-full.csv"):
    df = spark.read.format("csv").option("inferSchema", "true").option("header", "false").load(data_path(name))
    return df.withColumnRenamed("_c0", "guest").withColumnRenamed("_c1", "price")


EDGE_ROWS = [("b", 2.5, 1, True), (None, NAN, None, False), ("a", None, 3, None), ("c", -0.0, 1, True), ("a", 0.0, 2, False),
             ("b", INF, None, True), ("a", -7.25, 3, None), (None, 2.5, 2, False), ("c", None, 1, True), ("b", -INF, 3, True)]
EDGE_SCHEMA = "s string, x double, k int, b boolean"


def _py_sorted(rows, orders):
    """``rows`` (tuples) by ``orders`` = (column index, ascending, nulls_first): the oracle's rules
    on collected rows."""
    def cmp(p, q):
        for i, asc, nf in orders:
            a, b = p[i], q[i]
            if a is None or b is None:
                c = 0 if (a is None and b is None) else ((-1 if a is None else 1) if nf else (1 if a is None else -1))
            else:
                c = sc._cmp_values(a, b) if not isinstance(a, str) else (a > b) - (a < b)
                c = c if asc else -c
            if c:
                return c
        return 0
    return sorted(rows, key=cmp_to_key(cmp))


def api_results(spark):
    """Every API / SQL case as plain tuples (one list per case), for the host checks and the
    engine-to-engine comparison."""
    out = {}
    rows = lambda df: [tuple(r) for r in df.collect()]  # noqa: E731
    lab = lab_frame(spark)
    out["lab_counts"] = rows(lab.groupBy("guest").count().orderBy(F.desc("count"), "guest"))
    out["lab_price"] = rows(lab.orderBy(F.desc("price"), "guest").limit(7))
    out["lab_filtered"] = rows(lab.filter("price > 100").sort("guest", F.col("price").desc()))
    d = spark.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    out["name"] = rows(d.orderBy("k"))
    out["two"] = rows(d.sort("k", "x"))
    out["list"] = rows(d.orderBy(["s", "x"], ascending=[False, True]))
    out["asc_false"] = rows(d.orderBy("x", ascending=False))
    out["asc_true_keeps"] = rows(d.orderBy(d.col("x").desc(), "k", ascending=True))
    c = F.col("x")
    for name, o in [("asc", c.asc()), ("desc", c.desc()), ("asc_nulls_first", c.asc_nulls_first()),
                    ("asc_nulls_last", c.asc_nulls_last()), ("desc_nulls_first", c.desc_nulls_first()),
                    ("desc_nulls_last", c.desc_nulls_last())]:
        out["m_" + name] = rows(d.orderBy(o))
        out["f_" + name] = rows(d.orderBy(getattr(F, name)("x")))
    out["string"] = rows(d.orderBy(F.desc_nulls_first("s"), "k"))
    out["bool"] = rows(d.orderBy("b", F.desc("k")))
    out["expr"] = rows(d.orderBy(-F.col("x")))
    out["expr2"] = rows(d.orderBy((F.col("k") * -1).desc(), F.col("s")))
    out["limit"] = rows(d.orderBy("x").limit(3))
    out["filter"] = rows(d.filter("k > 1").orderBy(F.desc("x")))
    out["within"] = rows(d.sortWithinPartitions("s", ascending=False))
    d.createOrReplaceTempView("edge")
    out["sql_alias"] = rows(spark.sql("SELECT k AS kk, x FROM edge ORDER BY kk, x DESC"))
    out["sql_ordinal"] = rows(spark.sql("SELECT s, x FROM edge ORDER BY 2 DESC, 1"))
    out["sql_view_col"] = rows(spark.sql("SELECT s FROM edge WHERE k > 0 ORDER BY x, s"))
    out["sql_nulls"] = rows(spark.sql("SELECT k, x FROM edge ORDER BY k DESC NULLS FIRST, x ASC NULLS LAST"))
    text = "SELECT k, count(*) c, sum(x) t FROM edge GROUP BY k ORDER BY c DESC, k LIMIT 3"
    out["sql_group"] = rows(spark.sql(text))
    out["sql_group_again"] = rows(spark.sql(text))  # the same text bound twice: the template cache
    out["sql_star"] = rows(spark.sql("SELECT * FROM edge e ORDER BY e.k DESC, s"))
    out["sql_distinct"] = rows(spark.sql("SELECT DISTINCT s FROM edge ORDER BY s DESC"))
    out["sql_expr"] = rows(spark.sql("SELECT s, x FROM edge ORDER BY -x, k"))
    return out


def test_api_rows_follow_the_rules(cpu_session):
    got = api_results(cpu_session)
    rep = lambda rows: repr(rows)  # noqa: E731  (NaN cells compare by their text)
    E = EDGE_ROWS
    assert rep(got["name"]) == rep(_py_sorted(E, [(2, True, True)]))
    assert rep(got["two"]) == rep(_py_sorted(E, [(2, True, True), (1, True, True)]))
    assert rep(got["list"]) == rep(_py_sorted(E, [(0, False, False), (1, True, True)]))
    assert rep(got["asc_false"]) == rep(_py_sorted(E, [(1, False, False)]))
    assert rep(got["asc_true_keeps"]) == rep(_py_sorted(E, [(1, False, False), (2, True, True)]))
    placements = {"asc": (True, True), "desc": (False, False), "asc_nulls_first": (True, True), "asc_nulls_last": (True, False),
                  "desc_nulls_first": (False, True), "desc_nulls_last": (False, False)}
    for name, (asc, nf) in placements.items():
        want = rep(_py_sorted(E, [(1, asc, nf)]))
        assert rep(got["m_" + name]) == want and rep(got["f_" + name]) == want, name
    assert rep(got["string"]) == rep(_py_sorted(E, [(0, False, True), (2, True, True)]))
    assert rep(got["bool"]) == rep(_py_sorted(E, [(3, True, True), (2, False, False)]))
    neg = [r + (None if r[1] is None else -r[1],) for r in E]
    assert rep(got["expr"]) == rep([r[:4] for r in _py_sorted(neg, [(4, True, True)])])
    negk = [r + (None if r[2] is None else -r[2],) for r in E]
    assert rep(got["expr2"]) == rep([r[:4] for r in _py_sorted(negk, [(4, False, False), (0, True, True)])])
    assert rep(got["limit"]) == rep(_py_sorted(E, [(1, True, True)])[:3])
    assert rep(got["filter"]) == rep(_py_sorted([r for r in E if r[2] is not None and r[2] > 1], [(1, False, False)]))
    assert rep(got["within"]) == rep(_py_sorted(E, [(0, False, False)]))
    # SQL
    assert rep(got["sql_alias"]) == rep([(r[2], r[1]) for r in _py_sorted(E, [(2, True, True), (1, False, False)])])
    assert rep(got["sql_ordinal"]) == rep([(r[0], r[1]) for r in _py_sorted(E, [(1, False, False), (0, True, True)])])
    live = [r for r in E if r[2] is not None and r[2] > 0]
    assert rep(got["sql_view_col"]) == rep([(r[0],) for r in _py_sorted(live, [(1, True, True), (0, True, True)])])
    assert rep(got["sql_nulls"]) == rep([(r[2], r[1]) for r in _py_sorted(E, [(2, False, True), (1, True, False)])])
    assert rep(got["sql_star"]) == rep(_py_sorted(E, [(2, False, False), (0, True, True)]))
    assert got["sql_distinct"] == [("c",), ("b",), ("a",), (None,)]
    assert rep(got["sql_expr"]) == rep([(r[0], r[1]) for r in _py_sorted(neg, [(4, True, True), (2, True, True)])])
    groups = {}
    for r in E:
        groups.setdefault(r[2], []).append(r[1])
    want = sorted(((k, len(v)) for k, v in groups.items()), key=lambda g: (-g[1], g[0] is not None, g[0] or 0))[:3]
    assert [(k, c) for k, c, _ in got["sql_group"]] == want
    assert rep(got["sql_group_again"]) == rep(got["sql_group"])


def test_lab_counts_by_count_then_guest(cpu_session):
    got = api_results(cpu_session)
    df = lab_frame(cpu_session)
    groups = [tuple(r) for r in df.groupBy("guest").count().collect()]
    assert len(groups) > 10
    assert got["lab_counts"] == sorted(groups, key=lambda g: (-g[1], g[0]))
    rows = [tuple(r) for r in df.collect()]
    assert got["lab_price"] == sorted(rows, key=lambda r: (-r[1], r[0]))[:7]
    assert got["lab_filtered"] == sorted([r for r in rows if r[1] > 100], key=lambda r: (r[0], -r[1]))


def test_schema_and_columns_unchanged_hidden_columns_gone(cpu_session):
    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    for s in (d.orderBy("k"), d.orderBy(-F.col("x"), "k"), d.sortWithinPartitions(F.col("x") + F.col("k"))):
        assert s.columns == d.columns and s.schema.simpleString() == d.schema.simpleString()
        assert s.count() == len(EDGE_ROWS)
        t = s._table()
        assert t.sel is None and t.nrows == len(EDGE_ROWS)  # compact
    d.createOrReplaceTempView("edge")
    q = cpu_session.sql("SELECT s FROM edge ORDER BY x")
    assert q.columns == ["s"] and q._table().schema.names == ["s"]


def test_explain_shows_the_sort_label(cpu_session, capsys):
    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    d.orderBy(F.desc("x"), "k").explain()
    assert "Sort [x DESC NULLS LAST, k ASC NULLS FIRST]" in capsys.readouterr().out
    d.createOrReplaceTempView("edge")
    cpu_session.sql("SELECT k FROM edge ORDER BY k DESC NULLS FIRST LIMIT 2").explain()
    out = capsys.readouterr().out
    assert "Sort [k DESC NULLS FIRST]" in out and out.index("Limit 2") < out.index("Sort [")


def test_prune_columns_passes_through_a_sort(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import Project, Sort, prune_columns

    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    wide = d.withColumn("x2", d.col("x") * 2).withColumn("unused", d.col("k") + 1).orderBy("x2")
    pruned = prune_columns(wide._plan, {"s"})
    assert isinstance(pruned, Project) and pruned.schema().names == ["s"]
    assert isinstance(pruned.child, Sort) and sorted(pruned.child.schema().names) == ["s", "x2"]
    assert prune_columns(wide._plan, set(wide.columns)) is wide._plan


def test_errors(cpu_session):
    d = cpu_session.createDataFrame(EDGE_ROWS, EDGE_SCHEMA)
    with pytest.raises(AnalysisException, match='Cannot resolve column name "nope"'):
        d.orderBy("nope")
    with pytest.raises(AnalysisException, match='Cannot resolve column name "nope"'):
        d.sort(F.desc("nope"))
    with pytest.raises(ValueError, match="ascending"):
        d.orderBy("k", "x", ascending=[True])
    with pytest.raises(ValueError):
        d.orderBy()
    from net.jgp.labs.sparkdq4ml_amd import VectorAssembler

    v = VectorAssembler().setInputCols(["x", "k"]).setOutputCol("features").transform(d.na.drop())
    with pytest.raises(AnalysisException, match="not an orderable data type"):
        v.orderBy("features")
    with pytest.raises(AnalysisException, match="aggregate"):
        d.orderBy(F.sum("x"))
    d.createOrReplaceTempView("edge")
    with pytest.raises(AnalysisException, match="aggregate"):
        cpu_session.sql("SELECT k, count(*) c FROM edge GROUP BY k ORDER BY sum(x)")
    with pytest.raises(AnalysisException, match="cannot resolve"):
        cpu_session.sql("SELECT k FROM edge ORDER BY nope")
    with pytest.raises(AnalysisException, match="cannot resolve"):
        cpu_session.sql("SELECT k, count(*) c FROM edge GROUP BY k ORDER BY x")
    with pytest.raises(AnalysisException, match="position 3"):
        cpu_session.sql("SELECT k, x FROM edge ORDER BY 3")
    with pytest.raises(AnalysisException):
        cpu_session.sql("SELECT k FROM edge ORDER BY k NULLS MIDDLE")


# ---- two ranks (gloo) ------------------------------------------------------------------------------
def _dp_rows():
    return [(j % 7 if j % 5 else None, float((j * 37) % 11) - 5.0, f"s{j % 3}") for j in range(90)]


_DP_SCHEMA = "k int, x double, s string"
_DP_SPLIT = 37


def _dp_results(spark, rows):
    df = spark.createDataFrame(rows, _DP_SCHEMA)
    t = lambda d: [tuple(r) for r in d.collect()]  # noqa: E731
    agg = df.groupBy("k").agg(F.count("*").alias("c"), F.sum("x").alias("t"))
    return (t(agg.orderBy(F.desc("c"), F.asc_nulls_last("k"))), t(agg.sort("t", "k")),
            t(df.groupBy("s", "k").count().orderBy(F.desc("s"), F.desc_nulls_first("k")).limit(5)))


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
    res = _dp_results(spark, mine)
    df = spark.createDataFrame(mine, _DP_SCHEMA)
    try:
        df.orderBy("k")
        raised = ""
    except AnalysisException as e:
        raised = str(e)
    local = [tuple(r) for r in df.sortWithinPartitions("x", "k")._table().to_rows()]  # this rank's rows, sorted
    q.put((rank, res, raised, local == _py_sorted(mine, [(1, True, True), (0, True, True)])))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_sort_an_aggregate_and_refuse_a_sharded_sort(cpu_session):
    want = _dp_results(cpu_session, _dp_rows())
    assert len(want[0]) == 8 and len(want[2]) == 5
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
    for _, got, raised, local_ok in res:
        assert repr(got) == repr(want)
        assert "global sort across ranks is not implemented" in raised and "sortWithinPartitions" in raised
        assert local_ok


_ = math
