"""Window functions through the DataFrame API and SQL on a device session: the tables of the CPU
session, and a row_number() dedup that goes on into a fit."""
import os

import numpy as np
import pytest

import _window_api_cases as ac
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.window import Window

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(__file__), "..", "data")


@pytest.fixture(scope="module")
def host_tables():
    """The CPU session's answers, computed once for the module."""
    from net.jgp.labs.sparkdq4ml_amd import SparkSession

    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    s = SparkSession.builder().appName("test").master("cpu").getOrCreate()
    out = {"api": ac.api_table(s), "sql": ac.sql_table(s), "nested": ac.nested_and_latest(s)}
    s.stop()
    return out


def test_api_and_sql_tables_equal_the_cpu_sessions(host_tables, gpu_session):
    api = ac.api_table(gpu_session)
    assert repr(api) == repr(host_tables["api"])
    assert repr(ac.sql_table(gpu_session)) == repr(host_tables["sql"])
    want = ac.expected()
    for j, (name, _, _, _) in enumerate(ac.columns()):
        assert repr([r[1 + j] for r in api]) == repr(want[name]), name


def test_nested_latest_and_string_keys_equal_the_cpu_sessions(host_tables, gpu_session):
    assert repr(ac.nested_and_latest(gpu_session)) == repr(host_tables["nested"])


def test_a_filtered_device_frame_keeps_its_selection(gpu_session):
    df = ac.frame_df(gpu_session).filter(F.col("id") % 3 != 0)
    rows = [tuple(r) for r in df.withColumn("c", F.count("*").over(Window.partitionBy("k"))).collect()]
    live = [r for r in ac.ROWS if r[0] % 3]
    assert [r[0] for r in rows] == [r[0] for r in live]
    assert [r[6] for r in rows] == [sum(1 for x in live if x[1] == r[1]) for r in live]


def test_row_number_dedup_then_a_fit_on_the_lab_data(gpu_session):
    """Keep the latest record per guest count (the highest price), then fit price ~ guest."""
    from net.jgp.labs.sparkdq4ml_amd import LinearRegression, VectorAssembler

    spark = gpu_session
    df = spark.read().format("csv").option("inferSchema", "true").load(os.path.join(DATA, "dataset-full.csv"))
    df = df.withColumn("guest", df.col("_c0").cast("double")).withColumn("price", df.col("_c1").cast("double"))
    w = Window.partitionBy("guest").orderBy(F.desc("price"))
    top = df.withColumn("rn", F.row_number().over(w)).filter(F.col("rn") == 1).drop("rn")
    rows = [tuple(r) for r in top.select("guest", "price").collect()]
    every = [tuple(r) for r in df.select("guest", "price").collect()]
    best = {}
    for g, p in every:
        if p is not None and (g not in best or best[g] is None or p > best[g]):
            best[g] = p
        best.setdefault(g, None)
    assert sorted(rows, key=repr) == sorted(best.items(), key=repr) and 1 < len(rows) < len(every)
    feat = VectorAssembler().setInputCols(["guest"]).setOutputCol("features").transform(top.withColumn("label", F.col("price")))
    m = LinearRegression().setMaxIter(40).fit(feat)
    x = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    slope, icpt = np.polyfit(x[0], x[1], 1)
    assert abs(m.coefficients.toArray()[0] - slope) < 1e-6 * max(1.0, abs(slope))
    assert abs(m.intercept - icpt) < 1e-6 * max(1.0, abs(icpt))
