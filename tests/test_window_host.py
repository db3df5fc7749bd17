"""Window functions on the host engine: the numpy twin of every ``window.hip`` contract against the
plain-Python oracle, the DataFrame API and SQL ``OVER`` against the oracle and against each other,
the errors, the identity with ``groupBy``, and a gloo world of two ranks."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

import _window_api_cases as ac
import _window_cases as wc
from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.ops import window as wn
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.expressions import AnalysisException
from net.jgp.labs.sparkdq4ml_amd.sql.window import Window

T = wc.T


# ---- the twin against the oracle -------------------------------------------------------------------
def check(m, layout, **kw):
    case, twin, order, want = wc.reference(m, layout, **kw)
    assert twin["perm"].tolist() == order
    wc.same_results(wc.finalize(case, twin), want)
    return case, twin


@pytest.mark.parametrize("layout", wc.LAYOUTS)
@pytest.mark.parametrize("m", wc.SIZES)
def test_twin_against_oracle(m, layout):
    check(m, layout)


@pytest.mark.parametrize("dtype", list(wc.DTYPES))
def test_twin_key_dtypes(dtype):
    check(2 * T + 1, "sel", part_dtype=dtype, order_dtype=dtype)


def test_twin_two_partition_and_two_order_columns():
    check(2 * T + 1, "nulls", two_by_two=True)


def test_the_dyadic_premise_is_checked():
    rng = __import__("numpy").random.default_rng(0)
    wc.assert_dyadic(wc.dyadic(rng, 1000).tolist())
    with pytest.raises(AssertionError):
        wc.assert_dyadic([0.1, 0.2, 0.3])


def test_limits_and_word_counts():
    threads, run, tile, keys, words = kernels.window_limits()
    assert tile == threads * run == T and words >= wn.SUM_WORDS == wn.word_count(wn.SUM_F)


def test_raw_contract_errors():
    perm = torch.arange(4)
    heads = kernels.window_heads([], [], [], [], perm, 4)
    assert heads.tolist() == [3, 0, 0, 0]
    bounds = kernels.window_bounds(heads)
    assert bounds.tolist() == [[0] * 4, [0] * 4, [3] * 4, [3] * 4, [1] * 4]
    with pytest.raises(ValueError):
        kernels.window_finish(bounds, perm, 4, (True, -1, 0), [(wn.O_ROW_NUMBER, None, 0)])
    with pytest.raises(ValueError):
        kernels.window_prefix([(wn.SUM_I, torch.zeros(4), None, 0)], perm, 4)
    with pytest.raises(ValueError):
        kernels.window_heads([], [], [], [], torch.arange(5), 4)
    assert wn.ntile(torch.arange(1, 11), torch.full((10,), 10), 3).tolist() == [1, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert wn.ntile(torch.arange(1, 3), torch.full((2,), 2), 5).tolist() == [1, 2]


# ---- the API and SQL --------------------------------------------------------------------------------
def _same(a, b):
    return a == b or (a != a and b != b)


def test_api_and_sql_give_the_oracles_table(cpu_session):
    want = ac.expected()
    api = ac.api_table(cpu_session)
    sql = ac.sql_table(cpu_session)
    assert [r[0] for r in api] == list(range(ac.N))
    assert repr(api) == repr(sql)  # both routes: the same table for one query
    for j, (name, _, _, _) in enumerate(ac.columns()):
        got = [r[1 + j] for r in api]
        assert all(_same(g, w) and type(g) is type(w) for g, w in zip(got, want[name])), \
            (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want[name])) if not _same(g, w)][:5])
    names = {n for n, _, _, _ in ac.columns()}
    assert {"rn", "rk", "dr", "pr", "cd", "nt", "lg", "ld", "lt"} <= names
    assert all(f"{f}_{s}" in names for f in ac.FRAME_SPECS for s in "csqa")


def test_result_types(cpu_session):
    df = ac.frame_df(cpu_session)
    w = ac.W
    out = df.select(F.count("price").over(w).alias("c"), F.sum("qty").over(w).alias("sq"), F.sum("id").over(w).alias("si"),
                    F.sum("price").over(w).alias("sp"), F.avg("qty").over(w).alias("aq"), F.min("qty").over(w).alias("mq"),
                    F.max("price").over(w).alias("mp"), F.row_number().over(w).alias("rn"), F.lag("tag").over(w).alias("lt"),
                    F.percent_rank().over(w).alias("pr"))
    types = {f.name: (f.dataType.simpleString(), f.nullable) for f in out.schema.fields}
    assert types == {"c": ("bigint", False), "sq": ("bigint", True), "si": ("bigint", True), "sp": ("double", True),
                     "aq": ("double", True), "mq": ("bigint", True), "mp": ("double", True), "rn": ("int", False),
                     "lt": ("string", True), "pr": ("double", False)}
    assert out.count() == ac.N


def test_nested_extraction_latest_per_key_and_strings(cpu_session):
    a, b, latest, strs = ac.nested_and_latest(cpu_session)
    assert repr(a) == repr(b)
    want = ac.expected()
    for (i, d), avg in zip(a, [None if not c else s / c for s, c in zip(want["whole_s"], want["whole_c"])]):
        p = ac.ROWS[i][3]
        assert d == (None if p is None or avg is None else p - avg)
    # the latest record per key: the first row of every partition in (ts desc nulls last, row) order
    assert sorted(r[0] for r in latest) == sorted(i for i, rn in enumerate(want["rn"]) if rn == 1)
    assert len(latest) == 4 and all(len(r) == 6 for r in latest)
    tags = [r[5] for r in ac.ROWS]
    assert [r[1] for r in strs] == [tags.count(t) for t in tags]
    for k in ac.KEYS:  # a string order key: by tag (nulls first), then id
        part = sorted((r for r in ac.ROWS if r[1] == k), key=lambda r: (r[5] is not None, r[5] or "", r[0]))
        assert [strs[r[0]][2] for r in part] == list(range(1, len(part) + 1))


def test_the_selection_vector_is_kept_and_no_row_moves(cpu_session):
    df = ac.frame_df(cpu_session).filter(F.col("id") % 3 != 0)
    out = df.withColumn("rn", F.row_number().over(ac.W)).withColumn("c", F.count("*").over(Window.partitionBy("k")))
    rows = [tuple(r) for r in out.collect()]
    assert [r[0] for r in rows] == [i for i in range(ac.N) if i % 3]
    live = [r for r in ac.ROWS if r[0] % 3]
    assert [r[7] for r in rows] == [sum(1 for x in live if x[1] == r[1]) for r in live]
    for k in ac.KEYS:
        assert sorted(r[6] for r in rows if r[1] == k) == list(range(1, sum(1 for x in live if x[1] == k) + 1))


def test_an_unpartitioned_window_and_shared_specifications(cpu_session):
    df = ac.frame_df(cpu_session)
    out = [tuple(r) for r in df.select("id", F.row_number().over(Window.orderBy("id")).alias("rn"),
                                       F.count("*").over(Window.partitionBy()).alias("n"),
                                       F.sum("id").over(Window.orderBy("id")).alias("run")).collect()]
    assert out == [(i, i + 1, ac.N, i * (i + 1) // 2) for i in range(ac.N)]


# ---- the errors -------------------------------------------------------------------------------------
def test_errors(cpu_session):
    spark = cpu_session
    df = ac.frame_df(spark)
    wk, w = Window.partitionBy("k"), ac.W

    def raises(what, build):
        with pytest.raises(AnalysisException, match=what):
            build()

    for fn in (F.row_number, F.rank, F.dense_rank, F.percent_rank, F.cume_dist, lambda: F.ntile(3), lambda: F.lag("price"),
               lambda: F.lead("price")):
        raises("requires window to be ordered", lambda fn=fn: fn().over(wk))
    raises("requires window to be ordered", lambda: spark.sql("SELECT row_number() OVER (PARTITION BY k) FROM trades"))
    raises("rangeBetween with numeric offsets is not implemented", lambda: F.sum("price").over(w.rangeBetween(-2, 0)))
    raises("rangeBetween with numeric offsets is not implemented",
           lambda: spark.sql(f"SELECT sum(price) OVER ({ac.OVER} RANGE BETWEEN 2 PRECEDING AND CURRENT ROW) FROM trades"))
    raises("bounded on both sides is not implemented", lambda: F.min("price").over(w.rowsBetween(-3, 3)))
    raises("bounded on both sides is not implemented", lambda: F.max("price").over(w.rowsBetween(0, 0)))
    raises("min / max of a string", lambda: df.select(F.min("tag").over(wk)))
    for name in ("first", "last", "nth_value"):
        raises("is not implemented", lambda name=name: spark.sql(f"SELECT {name}(price) OVER (PARTITION BY k) FROM trades"))
    raises("not allowed to use window functions inside WHERE", lambda: df.filter(F.row_number().over(w) == 1))
    raises("not allowed to use window functions inside WHERE",
           lambda: spark.sql(f"SELECT id FROM trades WHERE row_number() OVER ({ac.OVER}) = 1"))
    raises("not allowed in GROUP BY", lambda: df.groupBy(F.row_number().over(w)).count())
    raises("not allowed in GROUP BY",
           lambda: spark.sql(f"SELECT count(*) FROM trades GROUP BY rank() OVER ({ac.OVER})"))
    raises("requires an OVER clause", lambda: df.select(F.row_number()))
    raises("cannot start at UNBOUNDED FOLLOWING", lambda: w.rowsBetween(Window.unboundedFollowing, 0))
    raises("Buckets expression must be positive", lambda: F.ntile(0).over(w))
    raises("cannot resolve", lambda: df.select(F.sum("nope").over(wk)))
    raises("requires numeric types", lambda: df.select(F.sum("tag").over(wk)))
    # the unfinished list is the documented one
    text = open(os.path.join(os.path.dirname(__file__), "..", "docs", "PARITY.md")).read()
    for word in ("rangeBetween", "bounded on both sides", "first", "nth_value", "WHERE", "sharded"):
        assert word in text[text.index("K5w"):]


# ---- identity with groupBy ---------------------------------------------------------------------------
def test_groupby_identity(cpu_session):
    win = ac.groupby_identity(cpu_session)
    assert any(r[2] is not None and r[2] != r[2] for r in win)  # a NaN sum is among them
    assert any(r[2] in (float("inf"), -float("inf")) for r in win)


# ---- two ranks (gloo) ------------------------------------------------------------------------------
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
    spark = SparkSession.builder().master("cpu").getOrCreate()
    df = spark.createDataFrame(ac.ROWS[rank::2], ac.SCHEMA)
    df.createOrReplaceTempView("trades")
    raised = []
    for build in (lambda: df.select(F.row_number().over(ac.W)),
                  lambda: df.withColumn("s", F.col("price") - F.avg("price").over(Window.partitionBy("k"))),
                  lambda: spark.sql("SELECT sum(price) OVER (PARTITION BY k) FROM trades")):
        try:
            build()
            raised.append("")
        except AnalysisException as e:
            raised.append(str(e))
    q.put((rank, raised))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_a_window_over_a_sharded_input_raises():
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
    for _, raised in res:
        assert all("data-parallel (sharded) input" in r and "not implemented" in r for r in raised), raised
