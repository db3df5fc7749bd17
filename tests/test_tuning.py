"""ParamGridBuilder / CrossValidator / TrainValidationSplit / DataFrame.randomSplit on the CPU
engine: the statistics route against the generic (Spark-style) route on the same folds, the
route selection, the cancellation guard, the lab data and a 2-rank gloo run."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import data_path
from net.jgp.labs.sparkdq4ml_amd import (CrossValidator, CrossValidatorModel, LinearRegression, ParamGridBuilder,
                                         TrainValidationSplit, TrainValidationSplitModel, VectorAssembler, Vectors,
                                         callUDF)
from net.jgp.labs.sparkdq4ml_amd.models.evaluation import RegressionEvaluator
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import kernels

STAT_ROUTES = ("onepass", "masked")
CASES = {"d12": (2373, 12, 3, [773, 832, 768]), "d40": (3217, 40, 5, [704, 721, 448, 960, 384])}


def _data(n, d, seed=0, noise=1.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(d, n, generator=g, dtype=torch.float64)
    beta = torch.linspace(-1, 2, d, dtype=torch.float64)
    y = beta @ X + 5.0 + noise * torch.randn(n, generator=g, dtype=torch.float64)
    return X, y


def _grid():
    return ParamGridBuilder().addGrid("regParam", [0.0, 0.1, 1.0]).addGrid("elasticNetParam", [0.0, 1.0]).build()


def test_param_grid_builder():
    g = _grid()
    assert len(g) == 6 and g[0] == {"regParam": 0.0, "elasticNetParam": 0.0}
    assert g[1] == {"regParam": 0.0, "elasticNetParam": 1.0} and g[-1] == {"regParam": 1.0, "elasticNetParam": 1.0}
    b = ParamGridBuilder().baseOn({"maxIter": 7}).baseOn(("tol", 1e-3)).addGrid("regParam", [0.5, 2.0]).build()
    assert b == [{"maxIter": 7, "tol": 1e-3, "regParam": 0.5}, {"maxIter": 7, "tol": 1e-3, "regParam": 2.0}]
    assert ParamGridBuilder().build() == [{}]


def test_tuner_params():
    cv = CrossValidator()
    assert cv.getNumFolds() == 3 and cv.getParallelism() == 1 and cv.getCollectSubModels() is False
    assert isinstance(cv.getSeed(), int)
    with pytest.raises(ValueError):
        cv.setNumFolds(1)
    assert cv.setNumFolds(5).setSeed(7).setParallelism(4).getNumFolds() == 5
    tv = TrainValidationSplit()
    assert tv.getTrainRatio() == 0.75
    with pytest.raises(ValueError):
        tv.setTrainRatio(1.0)


@pytest.fixture(scope="module")
def frames():
    return {key: _data(n, d) for key, (n, d, _, _) in CASES.items()}


@pytest.mark.parametrize("key", list(CASES))
def test_fold_sizes(key):
    n, _, k, sizes = CASES[key]
    ids = kernels.fold_ids(n, k, 42, 64).numpy()
    assert np.bincount(ids, minlength=k).tolist() == sizes


@pytest.mark.parametrize("metric", ["rmse", "mse", "r2", "var"])
@pytest.mark.parametrize("key", list(CASES))
def test_statistics_route_equals_generic(cpu_session, frames, key, metric):
    n, d, k, _ = CASES[key]
    X, y = frames[key]
    cpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = cpu_session.createDataFrame({"features": X, "label": y})
    cv = CrossValidator(estimator=LinearRegression(), estimatorParamMaps=_grid(),
                        evaluator=RegressionEvaluator(metricName=metric), numFolds=k, seed=42)
    ms = cv.fit(df)
    assert isinstance(ms, CrossValidatorModel) and ms._cv_route in STAT_ROUTES
    cpu_session.conf.set("dq4ml.cv.onePass", "false")
    mg = cv.fit(df)
    assert mg._cv_route == "generic"
    assert len(ms.avgMetrics) == 6
    np.testing.assert_allclose(ms.avgMetrics, mg.avgMetrics, rtol=1e-9, atol=0)
    np.testing.assert_allclose(np.asarray(ms._foldMetrics), np.asarray(mg._foldMetrics), rtol=1e-9, atol=0)
    assert ms._bestIndex == mg._bestIndex
    for p in ("regParam", "elasticNetParam"):
        assert ms.bestModel.getOrDefault(p) == mg.bestModel.getOrDefault(p) == _grid()[ms._bestIndex][p]
    np.testing.assert_allclose(ms.bestModel.coefficients.toArray(), mg.bestModel.coefficients.toArray(),
                               rtol=1e-9, atol=1e-9)
    assert float(ms.bestModel.intercept) == pytest.approx(float(mg.bestModel.intercept), rel=1e-9)
    # the refit is the fit of the whole frame, with its lazy training summary
    ref = LinearRegression().copy(_grid()[ms._bestIndex]).fit(df)
    np.testing.assert_allclose(ms.bestModel.coefficients.toArray(), ref.coefficients.toArray(), rtol=1e-9, atol=1e-9)
    assert float(ms.bestModel.summary.rootMeanSquaredError) == pytest.approx(float(ref.summary.rootMeanSquaredError),
                                                                            rel=1e-9)
    assert ms.transform(df).count() == n


def test_through_origin_r2_and_submodels(cpu_session, frames):
    X, y = frames["d12"]
    cpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = cpu_session.createDataFrame({"features": X, "label": y})
    ev = RegressionEvaluator(metricName="r2").setThroughOrigin(True)
    cv = CrossValidator(estimator=LinearRegression(), estimatorParamMaps=_grid(), evaluator=ev, numFolds=3, seed=42,
                        collectSubModels=True)
    ms = cv.fit(df)
    cpu_session.conf.set("dq4ml.cv.onePass", "false")
    mg = cv.fit(df)
    assert ms._cv_route in STAT_ROUTES and mg._cv_route == "generic"
    np.testing.assert_allclose(ms.avgMetrics, mg.avgMetrics, rtol=1e-9, atol=0)
    assert len(ms.subModels) == 3 and len(ms.subModels[0]) == 6
    np.testing.assert_allclose(ms.subModels[1][3].coefficients.toArray(), mg.subModels[1][3].coefficients.toArray(),
                               rtol=1e-9, atol=1e-9)


def _with_weight(spark, X, y):
    w = torch.rand(X.shape[1], generator=torch.Generator().manual_seed(5), dtype=torch.float64) + 0.5
    return spark.createDataFrame({"features": X, "label": y, "w": w, "label2": y * 2.0})


def _manual_rmse(X, y, k, seed, granule, fit):
    ids = kernels.fold_ids(X.shape[1], k, seed, granule).numpy()
    out = []
    for f in range(k):
        tr, va = ids != f, ids == f
        coef, icpt = fit(X[:, tr], y[tr])
        r = y[va] - (coef @ X[:, va] + icpt)
        out.append(float(np.sqrt(np.mean(r * r))))
    return out


@pytest.mark.parametrize("case", ["mae", "huber", "pipeline", "weightCol", "labelCol-grid"])
def test_generic_routes(cpu_session, frames, case):
    X, y = frames["d12"]
    cpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = _with_weight(cpu_session, X, y)
    est, ev = LinearRegression(), RegressionEvaluator(metricName="rmse")
    grid = ParamGridBuilder().addGrid("regParam", [0.0, 0.1]).build()
    if case == "mae":
        ev = RegressionEvaluator(metricName="mae")
    elif case == "huber":
        est = LinearRegression(loss="huber", maxIter=30)
    elif case == "pipeline":
        parts = cpu_session.createDataFrame({"a": X[0], "b": X[1], "label": y})
        df = parts
        est = Pipeline(stages=[VectorAssembler().setInputCols(["a", "b"]).setOutputCol("features"),
                               LinearRegression()])
    elif case == "weightCol":
        est = LinearRegression(weightCol="w")
    else:
        grid = ParamGridBuilder().addGrid("labelCol", ["label", "label2"]).build()
    m = CrossValidator(estimator=est, estimatorParamMaps=grid, evaluator=ev, numFolds=3, seed=42).fit(df)
    assert m._cv_route == "generic"
    assert len(m.avgMetrics) == 2 and len(m._foldMetrics) == 3
    assert all(np.isfinite(v) and v > 0 for row in m._foldMetrics for v in row)
    assert "prediction" in m.transform(df).columns
    if case == "pipeline":  # an unregularised 2-feature fit per fold, checked against numpy least squares
        def ols(Xt, yt):
            A = np.vstack([Xt, np.ones(Xt.shape[1])]).T
            s = np.linalg.lstsq(A, yt, rcond=None)[0]
            return s[:-1], s[-1]

        want = _manual_rmse(X[:2].numpy(), y.numpy(), 3, 42, 64, ols)
        np.testing.assert_allclose([row[0] for row in m._foldMetrics], want, rtol=1e-9)


def test_cancellation_guard_falls_back(cpu_session):
    X, y = _data(2373, 12, noise=0.0)  # a noiseless label: SSE is pure rounding of the raw moments
    cpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = cpu_session.createDataFrame({"features": X, "label": y})
    grid = ParamGridBuilder().addGrid("regParam", [0.0]).build()
    m = CrossValidator(estimator=LinearRegression(), estimatorParamMaps=grid,
                       evaluator=RegressionEvaluator(metricName="rmse"), numFolds=3, seed=42).fit(df)
    assert m._cv_route == "generic"
    assert 0 <= m.avgMetrics[0] < 1e-9


def _lab_frame(spark, name):
    from net.jgp.labs.sparkdq4ml_amd.dq.rules import register_lab_rules

    register_lab_rules(spark)
    df = spark.read().format("csv").option("inferSchema", "true").load(data_path(name))
    df = df.withColumnRenamed("_c0", "guest").withColumnRenamed("_c1", "price")
    df = df.withColumn("price_no_min", callUDF("minimumPriceRule", df.col("price")))
    df.createOrReplaceTempView("price")
    df = spark.sql("SELECT cast(guest as int) guest, price_no_min AS price FROM price WHERE price_no_min > 0")
    df = df.withColumn("price_correct_correl", callUDF("priceCorrelationRule", df.col("price"), df.col("guest")))
    df.createOrReplaceTempView("price")
    df = spark.sql("SELECT guest, price_correct_correl AS price FROM price WHERE price_correct_correl > 0")
    df = df.withColumn("label", df.col("price"))
    return VectorAssembler().setInputCols(["guest"]).setOutputCol("features").transform(df)


@pytest.mark.parametrize("name,rows", [("dataset-full.csv", 1024), ("dataset-abstract.csv", 24)])
def test_lab_data_cross_validation(cpu_session, name, rows):
    df = _lab_frame(cpu_session, name)
    assert df.count() == rows
    grid = ParamGridBuilder().addGrid("regParam", [0.1, 1.0]).build()
    lr = LinearRegression().setMaxIter(40).setElasticNetParam(1)
    m = CrossValidator(estimator=lr, estimatorParamMaps=grid, evaluator=RegressionEvaluator(), numFolds=3,
                       seed=42).fit(df)
    assert m._cv_route in STAT_ROUTES
    assert m.transform(df).count() == rows
    assert np.isfinite(float(m.bestModel.predict(Vectors.dense(40.0))))
    # hand-rolled: the same masks (few rows: granule 1 over the PHYSICAL rows of the executed
    # table), a compacted training frame per fold, numpy scoring
    tbl = df._table()
    live = tbl.sel_mask().numpy()
    guest = tbl.column("guest").values.to(torch.float64).numpy()
    price = tbl.column("price").values.to(torch.float64).numpy()
    ids = kernels.fold_ids(tbl.nrows, 3, 42, 1).numpy()
    assert all(int((live & (ids == f)).sum()) > 0 for f in range(3))
    want = np.zeros((3, 2))
    for f in range(3):
        tr, va = live & (ids != f), live & (ids == f)
        tdf = cpu_session.createDataFrame({"features": torch.from_numpy(guest[tr]).unsqueeze(0),
                                           "label": torch.from_numpy(price[tr])})
        for j, pm in enumerate(grid):
            fm = lr.copy(pm).fit(tdf)
            r = price[va] - (float(fm.coefficients.toArray()[0]) * guest[va] + float(fm.intercept))
            want[f, j] = np.sqrt(np.mean(r * r))
    np.testing.assert_allclose(m.avgMetrics, want.mean(0), rtol=1e-9)
    assert m._bestIndex == int(np.argmin(want.mean(0)))


def test_random_split(cpu_session):
    X, y = _data(1000, 3)
    rid = torch.arange(1000, dtype=torch.int64)
    df = cpu_session.createDataFrame({"features": X, "label": y, "rid": rid}).filter("rid % 7 != 0")
    total = df.count()
    a, b = df.randomSplit([3, 1], 42)
    ra = [r.rid for r in a.select("rid").collect()]
    rb = [r.rid for r in b.select("rid").collect()]
    assert len(ra) + len(rb) == total == a.count() + b.count()
    assert not set(ra) & set(rb) and set(ra) | set(rb) == {i for i in range(1000) if i % 7}
    ids = kernels.fold_ids(1000, [3, 1], 42, 1).numpy()
    assert ra == [i for i in range(1000) if i % 7 and ids[i] == 0]
    assert rb == [i for i in range(1000) if i % 7 and ids[i] == 1]
    assert 0.70 < len(ra) / total < 0.80
    a2, b2 = df.randomSplit([0.75, 0.25], 42)
    assert [r.rid for r in a2.select("rid").collect()] == ra and b2.count() == len(rb)
    c, _ = df.randomSplit([3, 1], 43)
    assert [r.rid for r in c.select("rid").collect()] != ra
    assert sum(p.count() for p in df.randomSplit([1, 1, 2])) == total  # seed drawn on the host
    with pytest.raises(ValueError):
        df.randomSplit([1, -1], 1)


@pytest.mark.parametrize("route", ["statistics", "generic"])
def test_train_validation_split(cpu_session, route):
    X, y = _data(3000, 5)
    df = cpu_session.createDataFrame({"features": X, "label": y})
    if route == "generic":
        cpu_session.conf.set("dq4ml.cv.onePass", "false")
    grid = ParamGridBuilder().addGrid("regParam", [0.0, 0.5]).build()
    m = TrainValidationSplit(estimator=LinearRegression(), estimatorParamMaps=grid,
                             evaluator=RegressionEvaluator(metricName="rmse"), trainRatio=0.8, seed=11).fit(df)
    assert isinstance(m, TrainValidationSplitModel)
    assert (m._cv_route in STAT_ROUTES) if route == "statistics" else m._cv_route == "generic"
    train, val = df.randomSplit([0.8, 0.2], 11)  # 3000 rows: granule 1, the split's own rule
    want = []
    for pm in grid:
        fm = LinearRegression().copy(pm).fit(train)
        want.append(RegressionEvaluator(metricName="rmse").evaluate(fm.transform(val)))
    np.testing.assert_allclose(m.validationMetrics, want, rtol=1e-9)
    assert m.bestModel.getOrDefault("regParam") == grid[int(np.argmin(want))]["regParam"]
    assert m.transform(df).count() == 3000


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
    X, y = _data(5000, 6)
    n = X.shape[1]
    lo, hi = rank * n // world, (rank + 1) * n // world
    spark = SparkSession.builder().master("cpu").getOrCreate()
    spark.conf.set("dq4ml.cv.foldGranule", "64")
    df = spark.createDataFrame({"features": X[:, lo:hi].contiguous(), "label": y[lo:hi].contiguous()})
    cv = CrossValidator(estimator=LinearRegression(), estimatorParamMaps=_grid(), evaluator=RegressionEvaluator(),
                        numFolds=3, seed=42)
    ms = cv.fit(df)
    spark.conf.set("dq4ml.cv.onePass", "false")
    mg = cv.fit(df)
    q.put((rank, ms._cv_route, mg._cv_route, list(ms.avgMetrics), list(mg.avgMetrics),
           ms.bestModel.coefficients.toArray().tolist(), mg.bestModel.coefficients.toArray().tolist()))
    comm.barrier()
    comm.shutdown()


def test_cross_validation_two_ranks():
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
    for _, rs, rg, avg_s, avg_g, coef_s, coef_g in res:
        assert rs in STAT_ROUTES and rg == "generic"
        np.testing.assert_allclose(avg_s, avg_g, rtol=1e-9)
        np.testing.assert_allclose(coef_s, coef_g, rtol=1e-9, atol=1e-9)
    assert res[0][3] == res[1][3] and res[0][5] == res[1][5]  # identical on both ranks, bit for bit
