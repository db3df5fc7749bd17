"""Exact quantiles on the CPU engine: the host radix select against the fp64 sort oracle, and the
public surface on top of it (``approxQuantile``, ``summary``, ``Imputer``, ``IqrRule``), single
process and as a 2-rank gloo run."""
import math
import multiprocessing as mp
import os
import socket
import threading

import numpy as np
import pytest
import torch

from _quantile_cases import PROBS, SIZES, oracle, patterns, same

NAN = float("nan")


# ---- the host radix form ---------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_host_radix_matches_sort_oracle(n):
    from net.jgp.labs.sparkdq4ml_amd.ops import kernels

    pats = patterns(n)
    rng = np.random.default_rng(n)
    valid, sel = rng.random(n) < 0.8, rng.random(n) < 0.7
    valid[0] = sel[0] = True
    names = list(pats)
    cols = []
    for k in names:
        x = pats[k].copy()
        if x.dtype.kind == "f":
            x[~(valid & sel)] = np.nan  # dead rows hold NaN
        cols.append(x)
    for vm, sm in ((None, None), (valid, sel)):
        v, c = kernels.quantiles([torch.from_numpy(x) for x in cols],
                                 None if vm is None else [torch.from_numpy(vm)] * len(cols),
                                 None if sm is None else torch.from_numpy(sm), PROBS)
        assert v.dtype == torch.float64 and c.dtype == torch.int64
        for i, k in enumerate(names):
            w, cnt = oracle(cols[i], PROBS, vm, sm)
            assert int(c[i]) == cnt and same(v[i].numpy(), w), k


def test_host_radix_empty_column_and_errors():
    from net.jgp.labs.sparkdq4ml_amd.ops import kernels

    x = torch.tensor([1.0, NAN, 3.0], dtype=torch.float64)
    v, c = kernels.quantiles([x, x], [None, torch.zeros(3, dtype=torch.bool)], None, [0.5, 1.0])
    assert v[0].tolist() == [1.0, 3.0] and c.tolist() == [2, 0] and bool(torch.isnan(v[1]).all())
    with pytest.raises(ValueError, match="probabilities per call"):
        kernels.quantiles([x], None, None, [0.5] * (kernels.MAX_QUANTILES + 1))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        kernels.quantiles([x], None, None, [-0.1])
    with pytest.raises(TypeError):
        kernels.quantiles([x.to(torch.float16)], None, None, [0.5])


def test_host_radix_two_shards_with_reduce():
    """The ``reduce`` hook: two shards (one of them empty in the second round) that add each
    other's per-pass histograms give the unsharded result on both sides."""
    from net.jgp.labs.sparkdq4ml_amd.ops import kernels

    n = 2373
    pats = patterns(n)
    cols = [pats[k] for k in ("signs_zero", "low_bits", "i64_big")]
    whole, cnt = kernels.quantiles([torch.from_numpy(c) for c in cols], None, None, PROBS)
    for split in (901, 0):
        bar = threading.Barrier(2, timeout=60)
        slot, out = [None, None], [None, None]

        def shard(r, split=split, bar=bar, slot=slot, out=out):
            lo, hi = (0, split) if r == 0 else (split, n)

            def reduce(h):
                slot[r] = h.clone()
                bar.wait()
                s = slot[0] + slot[1]
                bar.wait()
                return s

            out[r] = kernels.quantiles([torch.from_numpy(c[lo:hi].copy()) for c in cols], None, None, PROBS,
                                       reduce=reduce)

        ts = [threading.Thread(target=shard, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for r in range(2):
            assert out[r] is not None
            assert torch.equal(out[r][0].view(torch.int64), whole.view(torch.int64)) and torch.equal(out[r][1], cnt)


# ---- approxQuantile --------------------------------------------------------------------------
_ROWS = [(1, 10, 1.5, "a", True, None), (2, 20, None, "b", False, None), (3, 30, 3.5, None, True, None),
         (4, 2 ** 40, NAN, "d", True, None), (5, -7, -100.25, "e", False, None), (6, 0, 8.0, "f", True, None)]
_SCHEMA = "i int, l bigint, x double, s string, b boolean, z double"


def _frame(spark):
    return spark.createDataFrame(_ROWS, _SCHEMA)


def test_approx_quantile_shapes_and_values(cpu_session):
    df = _frame(cpu_session)
    one = df.approxQuantile("x", [0.0, 0.5, 1.0], 0.0)
    assert one == [-100.25, 1.5, 8.0] and all(isinstance(v, float) for v in one)  # null and NaN ignored
    many = df.stat.approxQuantile(["i", "l", "x"], [0.5, 0.25], 0.25)
    assert many == [[3.0, 2.0], [10.0, 0.0], [1.5, -100.25]]  # integral columns cast to double
    assert df.approxQuantile(("x",), [1.0], 0) == [[8.0]]
    assert df.approxQuantile("z", [0.5], 0.0) == []  # all-null: Spark 2.4's empty list
    assert df.approxQuantile(["x", "z"], [0.5], 0.0) == [[1.5], []]
    assert df.approxQuantile("x", [], 0.0) == []
    # more probabilities than one kernel call takes
    ps = [k / 39 for k in range(40)]
    w, _ = oracle([1.5, 3.5, -100.25, 8.0], ps)
    assert df.approxQuantile("x", ps, 0.0) == w.tolist()
    # a filter narrows the selection, the quantiles follow it
    assert df.filter("i > 2").approxQuantile("i", [0.0, 0.5], 0.0) == [3.0, 4.0]


def test_approx_quantile_errors(cpu_session):
    df = _frame(cpu_session)
    for bad in ([1.5], [-0.1], ["a"], 0.5, None):
        with pytest.raises(ValueError):
            df.approxQuantile("x", bad, 0.0)
    with pytest.raises(ValueError):
        df.approxQuantile("x", [0.5], -0.01)
    with pytest.raises(ValueError):
        df.approxQuantile("s", [0.5], 0.0)
    with pytest.raises(ValueError):
        df.approxQuantile("b", [0.5], 0.0)
    with pytest.raises(ValueError):
        df.approxQuantile("nope", [0.5], 0.0)
    with pytest.raises(ValueError):
        df.approxQuantile(3, [0.5], 0.0)


def test_approx_quantile_against_oracle_on_random_frame(cpu_session):
    rng = np.random.default_rng(5)
    n = 3001
    x = rng.standard_normal(n)
    x[rng.random(n) < 0.1] = np.nan
    k = rng.integers(-50, 50, n)
    df = cpu_session.createDataFrame({"x": torch.from_numpy(x), "k": torch.from_numpy(k)})
    got = df.approxQuantile(["x", "k"], PROBS, 0.0)
    assert same(got[0], oracle(x, PROBS)[0]) and same(got[1], oracle(k, PROBS)[0])


# ---- summary ---------------------------------------------------------------------------------
def _cells(df):
    return {r[0]: list(r)[1:] for r in df.collect()}


def test_summary_default_and_custom(cpu_session):
    df = _frame(cpu_session)
    s = df.summary()
    assert s.columns == ["summary", "i", "l", "x", "s", "z"]  # the boolean column is dropped
    assert [r[0] for r in s.collect()] == ["count", "mean", "stddev", "min", "25%", "50%", "75%", "max"]
    got, want = _cells(s), _cells(df.describe())
    for k in ("count", "mean", "stddev", "min", "max"):
        assert got[k] == want[k]
    # integral percentiles print in the column's own type, doubles as Java prints them, strings
    # and the all-null column are null
    assert got["25%"] == ["2", "0", "-100.25", None, None]
    assert got["50%"] == ["3", "10", "1.5", None, None]
    assert got["75%"] == ["5", "30", "3.5", None, None]
    c = df.summary("max", "33.3%", "count", "100%", "0%")
    assert [r[0] for r in c.collect()] == ["max", "33.3%", "count", "100%", "0%"]
    got = _cells(c)
    assert got["33.3%"] == ["2", "0", "1.5", None, None]
    assert got["100%"][:3] == ["6", str(2 ** 40), "8.0"] and got["0%"][:3] == ["1", "-7", "-100.25"]
    assert got["count"] == want["count"] and got["max"] == want["max"]
    assert all(f.dataType.simpleString() == "string" for f in c.schema.fields)


def test_summary_unknown_statistic(cpu_session):
    df = _frame(cpu_session)
    for bad in ("median", "p50", "abc%", "101%", "-1%"):
        with pytest.raises(ValueError):
            df.summary("count", bad)


# ---- Imputer ---------------------------------------------------------------------------------
def _imp_frame(spark):
    rows = [(1.0, 2.0, 1), (None, 4.0, 2), (3.0, NAN, 3), (NAN, 8.0, 4), (100.0, -1.0, 5), (5.0, -1.0, 6)]
    return spark.createDataFrame(rows, "a double, b double, k int")


def test_imputer_mean_and_median(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import Imputer, ImputerModel

    df = _imp_frame(cpu_session)
    imp = Imputer(inputCols=["a", "b"], outputCols=["a_i", "b_i"])
    assert imp.getStrategy() == "mean" and math.isnan(imp.getMissingValue()) and imp.uid.startswith("imputer_")
    m = imp.fit(df)
    assert isinstance(m, ImputerModel) and m.getInputCols() == ["a", "b"] and m.uid == imp.uid
    sur = m.surrogateDF
    assert sur.columns == ["a", "b"] and sur.count() == 1
    assert list(sur.collect()[0]) == [(1.0 + 3.0 + 100.0 + 5.0) / 4, (2.0 + 4.0 + 8.0 - 1.0 - 1.0) / 5]
    out = m.transform(df)
    assert out.columns == ["a", "b", "k", "a_i", "b_i"]
    rows = out.collect()
    assert [r["a_i"] for r in rows] == [1.0, 27.25, 3.0, 27.25, 100.0, 5.0]
    assert [r["b_i"] for r in rows] == [2.0, 4.0, 2.4, 8.0, -1.0, -1.0]
    assert [r["a"] for r in rows][1] is None  # the inputs stay as they were
    med = imp.setStrategy("median").fit(df)
    assert list(med.surrogateDF.collect()[0]) == [3.0, 2.0]  # rank ceil(n / 2) of the non-missing
    assert [r["a_i"] for r in med.transform(df).collect()] == [1.0, 3.0, 3.0, 3.0, 100.0, 5.0]


def test_imputer_custom_missing_value_and_in_place(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import Imputer

    df = _imp_frame(cpu_session)
    m = Imputer().setInputCols(["b"]).setOutputCols(["b"]).setStrategy("median").setMissingValue(-1.0).fit(df)
    assert list(m.surrogateDF.collect()[0]) == [4.0]  # of 2, 4, 8: NaN never counts
    got = [r["b"] for r in m.transform(df).collect()]
    assert got[:2] == [2.0, 4.0] and math.isnan(got[2]) and got[3:] == [8.0, 4.0, 4.0]  # NaN is no placeholder now
    assert m.transform(df).columns == ["a", "b", "k"]


def test_imputer_errors(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import Imputer
    from net.jgp.labs.sparkdq4ml_amd.sql.expressions import SparkException

    df = _imp_frame(cpu_session)
    with pytest.raises(ValueError, match="double or float"):
        Imputer(inputCols=["k"], outputCols=["k_i"]).fit(df)
    with pytest.raises(ValueError):
        Imputer(inputCols=["a", "b"], outputCols=["x"]).fit(df)
    with pytest.raises(ValueError):
        Imputer(inputCols=["a"], outputCols=["x"], strategy="mode")
    allmiss = cpu_session.createDataFrame([(None, 1.0), (NAN, 2.0)], "a double, b double")
    for strategy in ("mean", "median"):
        with pytest.raises(SparkException, match="surrogate cannot be computed"):
            Imputer(inputCols=["b", "a"], outputCols=["b_i", "a_i"], strategy=strategy).fit(allmiss)
    with pytest.raises(NotImplementedError):
        Imputer(inputCols=["a"], outputCols=["x"]).save("/nonexistent")
    with pytest.raises(NotImplementedError):
        Imputer(inputCols=["a"], outputCols=["x"]).fit(df).save("/nonexistent")


def test_imputer_float_column_keeps_its_type(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import Imputer

    df = cpu_session.createDataFrame({"f": torch.tensor([1.0, NAN, 4.0, 2.5], dtype=torch.float32)})
    assert df.schema["f"].dataType.simpleString() == "float"
    out = Imputer(inputCols=["f"], outputCols=["g"], strategy="median").fit(df).transform(df)
    assert out.schema["g"].dataType.simpleString() == "float"
    assert [r["g"] for r in out.collect()] == [1.0, 2.5, 4.0, 2.5]


def test_imputer_as_pipeline_stage(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import Imputer, LinearRegression, VectorAssembler
    from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline

    rng = np.random.default_rng(3)
    n = 400
    g = rng.uniform(1, 30, n)
    y = 5.0 * g + 20.0 + rng.standard_normal(n)
    holes = rng.random(n) < 0.15
    gm = g.copy()
    gm[holes] = np.nan
    df = cpu_session.createDataFrame({"guest": torch.from_numpy(gm), "label": torch.from_numpy(y)})
    pipe = Pipeline(stages=[Imputer(inputCols=["guest"], outputCols=["guest_f"], strategy="median"),
                            VectorAssembler(inputCols=["guest_f"], outputCol="features"), LinearRegression()])
    pm = pipe.fit(df)
    med = oracle(gm, [0.5])[0][0]
    filled = np.where(holes, med, g)
    ref_df = cpu_session.createDataFrame({"guest_f": torch.from_numpy(filled), "label": torch.from_numpy(y)})
    ref = LinearRegression().fit(VectorAssembler(inputCols=["guest_f"], outputCol="features").transform(ref_df))
    lr = pm.stages[-1]
    assert lr.coefficients.toArray().tolist() == ref.coefficients.toArray().tolist() and lr.intercept == ref.intercept
    assert pm.transform(df).count() == n


# ---- IqrRule ---------------------------------------------------------------------------------
def test_iqr_rule_bounds_and_contracts(cpu_session):
    from net.jgp.labs.sparkdq4ml_amd import DataTypes, IqrRule, callUDF
    from net.jgp.labs.sparkdq4ml_amd.dq.rules import RangeRule

    vals = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 1000.0, -500.0, None, NAN]
    df = cpu_session.createDataFrame([(v,) for v in vals], "x double")
    r = IqrRule.fit(df, "x")  # 10 values: Q1 = rank 3 = 2.0, Q3 = rank 8 = 7.0
    assert isinstance(r, RangeRule) and (r.q_lo, r.q_hi, r.k) == (2.0, 7.0, 1.5)
    assert (r.lo, r.hi, r.sentinel, r.name) == (2.0 - 7.5, 7.0 + 7.5, -1.0, "iqrRule")
    r2 = IqrRule.fit(df, "x", k=0.5, lower=0.1, upper=0.9, sentinel=-9.0, name="fence")
    assert (r2.q_lo, r2.q_hi) == (-500.0, 8.0) and (r2.lo, r2.hi) == (-500.0 - 254.0, 8.0 + 254.0)
    assert r2.sentinel == -9.0 and r2.name == "fence"
    cpu_session.udf().register("iqrRule", r, DataTypes.DoubleType)
    out = df.withColumn("q", callUDF("iqrRule", df.col("x")))
    got = [row["q"] for row in out.collect()]
    want = [r.call(v) for v in vals]  # the row contract
    assert same([NAN if g is None else g for g in got], [NAN if w is None else w for w in want])
    assert got[8] == -1.0 and got[9] == -1.0 and got[10] == -1.0 and math.isnan(got[11])  # null -> sentinel
    out.createOrReplaceTempView("t")
    assert cpu_session.sql("SELECT x FROM t WHERE q > 0").count() == 9  # 1..8 and NaN (above all in Spark SQL)
    with pytest.raises(ValueError):
        IqrRule.fit(cpu_session.createDataFrame([(None,)], "x double"), "x")
    with pytest.raises(ValueError):
        IqrRule.fit(df, "x", lower=0.8, upper=0.2)


# ---- two ranks (gloo) ------------------------------------------------------------------------
def _dp_rows():
    rng = np.random.default_rng(11)
    n = 100
    a = rng.standard_normal(n).round(3)
    rows = []
    for j in range(n):
        av = None if j % 7 == 0 else (NAN if j % 11 == 0 else float(a[j]))
        bv = float(j % 13) if j < 37 else None  # entirely null on rank 1
        rows.append((av, bv, int(rng.integers(-5, 6)), f"s{j % 9}"))
    return rows


_DP_SCHEMA = "a double, b double, k int, s string"
_DP_SPLIT = 37


def _dp_results(spark, rows):
    from net.jgp.labs.sparkdq4ml_amd import Imputer

    df = spark.createDataFrame(rows, _DP_SCHEMA)
    q = df.approxQuantile(["a", "b", "k"], PROBS, 0.0)
    s = [tuple(r) for r in df.summary().collect()]
    m = Imputer(inputCols=["a", "b"], outputCols=["a_i", "b_i"], strategy="median").fit(df)
    sur = [tuple(r) for r in m.surrogateDF.collect()]
    filled = [tuple(r) for r in m.transform(df).select("a_i", "b_i").collect()]
    mean = [tuple(r) for r in Imputer(inputCols=["b"], outputCols=["b_i"]).fit(df).surrogateDF.collect()]
    return q, s, sur, filled, mean


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
    assert want[0][1] and want[2]  # the half-null column still has values and a surrogate
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
