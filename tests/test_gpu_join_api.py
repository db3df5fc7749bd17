"""``DataFrame.join`` and SQL ``JOIN ... USING`` on the device session: every case of
``test_join_host.py`` collects the CPU engine's rows, row for row; a device string column travels
through an outer join as spans; a joined frame goes on into ``groupBy`` and into a fit; semi and
anti joins narrow the selection without a copy."""
import numpy as np
import pytest
import torch

from test_join_host import L_ROWS, R_ROWS, api_results, frames, py_join

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu_results():
    """The CPU engine's answers (computed before the device session exists)."""
    from net.jgp.labs.sparkdq4ml_amd import SparkSession

    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    s = SparkSession.builder().appName("test").master("cpu").getOrCreate()
    try:
        return api_results(s)
    finally:
        s.stop()


def test_every_case_equals_the_cpu_engine(cpu_results, gpu_session):
    got = api_results(gpu_session)
    assert sorted(got) == sorted(cpu_results)
    for name, want in cpu_results.items():
        assert repr(got[name]) == repr(want), name  # exact, NaN and null cells included
    assert len(got["k_full_outer"]) == len(py_join(L_ROWS, R_ROWS, [0], [0], "full_outer")) > len(L_ROWS)


def test_joined_frames_stay_on_the_device(gpu_session):
    L, R = frames(gpu_session)
    t = L.join(R, "k", "left")._table()
    assert t.device.type == "cuda" and t.sel is None and t.nrows == len(py_join(L_ROWS, R_ROWS, [0], [0], "left_outer"))
    for f, c in zip(t.schema.fields, t.columns):
        assert isinstance(c.values, list) or c.values.is_cuda, f.name


def test_semi_and_anti_narrow_the_selection_without_a_copy(gpu_session):
    L, R = frames(gpu_session)
    base = L._table()
    for how, keep in (("semi", [0, 1, 2, 4, 6]), ("anti", [3, 5, 7])):
        t = L.join(R, "k", how)._table()
        assert t.sel.is_cuda and t.nrows == base.nrows and torch.nonzero(t.sel).flatten().tolist() == keep
        assert all(a is b for a, b in zip(t.columns, base.columns))


def test_a_device_string_column_is_payload_of_an_outer_join(tmp_path):
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.sql.table import DeviceStringColumn

    n = 3000
    rng = np.random.default_rng(3)
    ks = rng.integers(0, 50, n)
    names = [f"name {i} of {k}" for i, k in enumerate(ks)]
    p = tmp_path / "named.csv"
    p.write_bytes(b"\r".join(f"{k},{i * 0.5},{s}".encode() for i, (k, s) in enumerate(zip(ks, names))))
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().master("mi355x[*]").config("dq4ml.csv.deviceThresholdBytes", "0").getOrCreate()
    try:
        df = spark.read().format("csv").option("inferSchema", "true").load(str(p)).toDF("k", "x", "name")
        src = df._table().columns[2]
        assert isinstance(src, DeviceStringColumn)
        probe = spark.createDataFrame([(7, 1), (99, 2), (None, 3), (7, 4), (0, 5)], "k int, tag int")
        j = probe.join(df, "k", "left")
        col = j._table().columns[3]  # k, tag, x, name
        assert isinstance(col, DeviceStringColumn) and not col.materialized and not src.materialized  # only spans moved
        got = [tuple(r) for r in j.collect()]
        rows = [(int(k), i * 0.5, s) for i, (k, s) in enumerate(zip(ks, names))]
        want = py_join([(7, 1), (99, 2), (None, 3), (7, 4), (0, 5)], rows, [0], [0], "left_outer")
        assert got == want and (99, 2, None, None) in got and len(got) > 100
    finally:
        spark.stop()


def test_a_joined_frame_goes_on_into_groupby_and_a_fit(gpu_session):
    from net.jgp.labs.sparkdq4ml_amd import LinearRegression, VectorAssembler
    from net.jgp.labs.sparkdq4ml_amd.sql import functions as F

    spark = gpu_session
    n = 5000
    rng = np.random.default_rng(11)
    g = rng.integers(0, 40, n)
    x = rng.normal(0, 3, n)
    slope = {int(k): 1.0 + 0.25 * k for k in range(40)}
    facts = spark.createDataFrame([(int(a), float(b)) for a, b in zip(g, x)], "g int, x double")
    dim = spark.createDataFrame([(k, v, 100.0 + k) for k, v in slope.items() if k != 13], "g long, slope double, base double")
    j = facts.join(dim, "g")  # the dimension-table case: unique right keys
    assert j.count() == int((g != 13).sum())
    by = {r[0]: (r[1], r[2]) for r in j.groupBy("g").agg(F.count("*").alias("n"), F.max("slope").alias("s")).collect()}
    assert by == {k: (int((g == k).sum()), slope[k]) for k in range(40) if k != 13}
    # the same rows made directly (the join's order: the left rows in row order): the two fits are the same computation
    rows = [(int(a), float(b), slope[int(a)], 100.0 + int(a)) for a, b in zip(g, x) if a != 13]
    direct = spark.createDataFrame(rows, "g int, x double, slope double, base double")
    assert [tuple(r) for r in j.collect()] == rows

    def fit(df):
        feat = df.withColumn("sx", F.col("slope") * F.col("x")).withColumn("label", F.col("slope") * F.col("x") + F.col("base"))
        va = VectorAssembler().setInputCols(["sx", "base"]).setOutputCol("features")
        m = LinearRegression().setMaxIter(50).fit(va.transform(feat))
        return m.coefficients.toArray(), m.intercept

    (cj, ij), (cd, idr) = fit(j), fit(direct)
    assert np.array_equal(cj, cd) and ij == idr
    assert abs(cj[0] - 1.0) < 1e-6 and abs(cj[1] - 1.0) < 1e-6  # y = sx + base
