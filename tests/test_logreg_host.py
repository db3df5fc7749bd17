"""Logistic regression on the host: the fp64 twin of the device pass against an mpmath oracle, fits
on the CPU engine against the optimum found by plain Newton steps, Spark's post-processing, the API
and a two-rank (gloo) fit.

FIT_BOUND is the asserted distance |fit - beta*|_inf: 10x the largest distance measured for these
fits, 1.35e-8 (profiles/logreg.md lists them); the stopping rule (tol 1e-12), not the arithmetic, sets it.
"""
import multiprocessing as mp
import os
import socket

import mpmath
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import (CrossValidator, LogisticRegression, MulticlassClassificationEvaluator,
                                         ParamGridBuilder, VectorAssembler, Vectors)
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import logreg as L

FIT_BOUND = 1.4e-7


def data(K, n=500, d=5, seed=0):
    """Features [n, d] and labels from a Gumbel-noised linear model over max(K, 2) classes."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * rng.uniform(0.5, 3.0, d) + rng.normal(size=d)
    B = rng.normal(size=(max(K, 2), d))
    return X, np.argmax((X - X.mean(axis=0)) @ B.T + rng.gumbel(size=(n, max(K, 2))), axis=1).astype(np.float64)


def newton(X, y, K, reg, w=None, steps=12):
    """(coef [K, d], intercept [K], last |gradient|_inf) of the optimum of Spark's scaled L2
    objective -- weighted mean loss, features over Spark's weighted std -- by Newton steps
    (minimum-norm: the multinomial intercepts are free up to a shift)."""
    n, d = X.shape
    w = np.ones(n) if w is None else w
    W = w.sum()
    mean = w @ X / W
    std = np.sqrt(w @ (X - mean) ** 2 / (W - (w * w).sum() / W))
    Z = np.c_[X / std, np.ones(n)]
    C = max(K, 2)
    Y = np.eye(C)[y.astype(int)][:, C - K:]
    pen = np.tile(np.r_[np.full(d, reg), 0.0], K)
    B = np.zeros((K, d + 1))
    for _ in range(steps):
        M = Z @ B.T
        P = 1.0 / (1.0 + np.exp(-M)) if K == 1 else np.exp(M - M.max(axis=1, keepdims=True))
        P = P if K == 1 else P / P.sum(axis=1, keepdims=True)
        g = ((w[:, None] * (P - Y)).T @ Z / W).reshape(-1) + pen * B.reshape(-1)
        H = np.diag(pen)
        for a in range(K):
            for b in range(K):
                wgt = P[:, a] * ((1.0 if a == b else 0.0) - P[:, b]) if K > 1 else P[:, 0] * (1.0 - P[:, 0])
                H[a * (d + 1):(a + 1) * (d + 1), b * (d + 1):(b + 1) * (d + 1)] += (Z * (w * wgt)[:, None]).T @ Z / W
        B -= np.linalg.lstsq(H, g, rcond=None)[0].reshape(K, d + 1)
    return B[:, :d] / std, B[:, d] - (B[:, d].mean() if K > 1 else 0.0), np.abs(g).max()


def weights(n, seed=1):
    """Non-unit weights that sum to less than 1 (a fit must not depend on their scale)."""
    u = np.random.default_rng(seed).uniform(0.5, 3.0, n)
    return u / (2.0 * u.sum())


def frame(spark, X, y, w=None):
    rows = [(Vectors.dense(*X[i]), float(y[i])) + (() if w is None else (float(w[i]),)) for i in range(len(y))]
    return spark.createDataFrame(rows, ["features", "label"] + ([] if w is None else ["weight"]))


def fitted(m):
    return m.coefficientMatrix.toArray(), m.interceptVector.toArray()


@pytest.mark.parametrize("K,scale", [(1, 1.0), (1, 800.0), (3, 1.0), (5, 800.0)])
def test_twin_equals_mpmath_oracle(K, scale):
    mpmath.mp.dps = 50
    rng = np.random.default_rng(K)
    d, n, C = 3, 40, max(K, 2)
    X, y, w = rng.uniform(-1, 1, (d, n)), rng.integers(0, C, n), rng.uniform(0.5, 2.0, n)
    coef = rng.normal(size=(K, d + 1)) * scale
    mp, f = mpmath.mpf, mpmath
    M = [[sum(mp(coef[c, j]) * mp(X[j, r]) for j in range(d)) + mp(coef[c, d]) for r in range(n)] for c in range(K)]
    M = [[mp(0)] * n] + M if K == 1 else M
    ls = [f.log(sum(f.exp(M[c][r] - max(M[k][r] for k in range(C))) for c in range(C))) + max(M[k][r] for k in range(C))
          for r in range(n)]
    P = np.array([[f.exp(M[c][r] - ls[r]) for r in range(n)] for c in range(C)])
    loss = [mp(w[r]) * (ls[r] - M[y[r]][r]) for r in range(n)]
    mult = np.array([[mp(w[r]) * (P[c, r] - (1 if y[r] == c else 0)) for r in range(n)] for c in range(C - K, C)])
    Xe = np.vstack([X, np.ones(n)])
    want = np.array([sum(mult[c, r] * mp(Xe[j, r]) for r in range(n)) for c in range(K) for j in range(d + 1)]
                    + [sum(loss), sum(mp(v) for v in w), mp(n), mp(0)])
    S = np.array([sum(abs(mult[c, r] * mp(Xe[j, r])) for r in range(n)) for c in range(K) for j in range(d + 1)]
                 + [sum(abs(v) for v in loss), sum(w), 0, 0])
    got = L.logreg_pass_host(X, y.astype(np.float64), w, None, coef, L.GRAD).numpy()
    assert np.isfinite(got).all()
    assert all(abs(mp(got[i]) - want[i]) <= mp(1e-12) * S[i] for i in range(got.size))
    _, prob, pred = L.logreg_pass_host(X, None, None, None, coef, L.PREDICT)
    assert np.abs(prob.numpy() - P.astype(np.float64)).max() <= 1e-12
    assert (pred.numpy() == np.argmax(P.astype(np.float64), axis=0)).all()


@pytest.mark.parametrize("K,weighted", [(1, False), (3, False), (1, True), (3, True)])
def test_l2_fit_reaches_the_newton_optimum(cpu_session, K, weighted):
    X, y = data(K)
    w = weights(len(y)) if weighted else None
    coef, icpt, gmax = newton(X, y, K, 0.1, w)
    assert gmax <= 1e-15
    lr = LogisticRegression(regParam=0.1, tol=1e-12, family="auto", weightCol="weight" if weighted else None)
    m = lr.fit(frame(cpu_session, X, y, w))
    gc, gi = fitted(m)
    dist = max(np.abs(gc - coef).max(), np.abs(gi - icpt).max())
    print("fit distance", K, weighted, dist)
    assert m.numClasses == max(K, 2) and dist <= FIT_BOUND
    assert m.summary.objectiveHistory[-1] <= m.summary.objectiveHistory[0]


def test_l1_fit_meets_the_subgradient_conditions(cpu_session):
    X, y = data(1)
    n = len(y)
    m = LogisticRegression(regParam=0.1, elasticNetParam=1.0, tol=1e-12).fit(frame(cpu_session, X, y))
    beta, b = m.coefficients.toArray(), float(m.intercept)
    std = X.std(axis=0, ddof=1)
    p = 1.0 / (1.0 + np.exp(-(X @ beta + b)))
    g = (X / std).T @ (p - y) / n  # gradient of the mean loss in the scaled space
    zero = beta == 0.0
    assert zero.any() and not zero.all()
    assert (np.abs(g[zero]) <= 0.1 + FIT_BOUND).all()
    assert np.abs(g[~zero] + np.sign(beta[~zero]) * 0.1).max() <= FIT_BOUND and abs((p - y).mean()) <= FIT_BOUND


def test_spark_post_processing(cpu_session):
    X, y = data(3, n=200)
    gc, gi = fitted(LogisticRegression(maxIter=30).fit(frame(cpu_session, X, y)))
    assert np.abs(gc.mean(axis=0)).max() <= 1e-15 and abs(gi.mean()) <= 1e-15  # regParam 0: both centred
    gc, gi = fitted(LogisticRegression(regParam=0.1, standardization=False).fit(frame(cpu_session, X, y)))
    assert abs(gi.mean()) <= 1e-15
    for lab, family, want in ((1.0, "auto", [np.inf]), (0.0, "auto", [-np.inf]), (2.0, "multinomial", [0, 0, np.inf])):
        m = LogisticRegression(family=family).fit(frame(cpu_session, X[:20], np.full(20, lab)))
        gc, gi = fitted(m)
        assert not gc.any() and gi.tolist() == want and m.summary.objectiveHistory == []
    assert m.predict(Vectors.dense(*X[0])) == 2.0


def test_params_errors_pipeline_and_evaluator(cpu_session, tmp_path):
    lr = LogisticRegression(maxIter=7, regParam=0.25, family="multinomial")
    assert (lr.getMaxIter(), lr.getTol(), lr.getThreshold(), lr.getElasticNetParam()) == (7, 1e-6, 0.5, 0.0)
    lr.save(str(tmp_path / "lr"))
    assert LogisticRegression.load(str(tmp_path / "lr")).getRegParam() == 0.25
    for bad in (lambda: lr.setThresholds([0.5, 0.5]), lambda: lr.setLowerBoundsOnCoefficients(None),
                lambda: LogisticRegression(family="poisson")):
        with pytest.raises((NotImplementedError, ValueError, TypeError)):
            bad()
    X, y = data(3, n=120)
    df = frame(cpu_session, X, y, np.ones(len(y)))
    with pytest.raises(ValueError, match="binomial"):
        LogisticRegression(family="binomial").fit(df)
    with pytest.raises(ValueError, match="class ind"):
        LogisticRegression().fit(frame(cpu_session, X, y - 0.5))
    cols = cpu_session.createDataFrame([tuple(float(v) for v in X[i]) + (float(y[i]),) for i in range(len(y))],
                                       ["a", "b", "c", "d", "e", "label"])
    model = Pipeline(stages=[VectorAssembler(inputCols=list("abcde"), outputCol="features"),
                             LogisticRegression(weightCol=None)]).fit(cols)
    out = model.transform(cols)
    m = LogisticRegression(weightCol="weight").fit(df)
    with pytest.raises(RuntimeError):
        m.coefficients
    with pytest.raises(NotImplementedError):
        m.save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError):
        m.summary.roc
    pr = np.array([r[0].toArray() for r in out.select("probability").collect()])
    pred = np.array([r[0] for r in out.select("prediction").collect()])
    np.testing.assert_allclose(pr, [m.predictProbability(Vectors.dense(*x)).toArray() for x in X], atol=1e-9)
    assert (pred == pr.argmax(axis=1)).all() and m.summary.accuracy == m.evaluate(df).accuracy == (pred == y).mean()
    # confusion matrix [[2, 1, 0], [0, 1, 1], [1, 0, 2]]: rows = label
    cm = cpu_session.createDataFrame([(0.0, 0.0), (0.0, 0.0), (0.0, 1.0), (1.0, 1.0), (1.0, 2.0), (2.0, 0.0), (2.0, 2.0),
                                      (2.0, 2.0)], ["label", "prediction"])
    prec, rec = np.array([2 / 3, 1 / 2, 2 / 3]), np.array([2 / 3, 1 / 2, 2 / 3])
    wt = np.array([3, 2, 3]) / 8
    for name, want in (("accuracy", 5 / 8), ("weightedPrecision", (wt * prec).sum()), ("weightedRecall", (wt * rec).sum()),
                       ("f1", (wt * 2 * prec * rec / (prec + rec)).sum())):
        assert MulticlassClassificationEvaluator(metricName=name).evaluate(cm) == pytest.approx(want, rel=1e-14)
    assert MulticlassClassificationEvaluator().getMetricName() == "f1"
    lr = LogisticRegression(maxIter=10)
    grid = ParamGridBuilder().addGrid("regParam", [0.01, 10.0]).build()
    cv = CrossValidator(estimator=lr, estimatorParamMaps=grid, numFolds=3,
                        evaluator=MulticlassClassificationEvaluator(metricName="accuracy")).fit(df)
    assert cv.avgMetrics[0] > cv.avgMetrics[1] and cv.bestModel.numClasses == 3


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    X, y = data(3)
    part = slice(0, 260) if rank == 0 else slice(260, None)
    m = LogisticRegression(regParam=0.1, tol=1e-12).fit(frame(spark, X[part], y[part]))
    q.put((rank, m.coefficientMatrix.toArray().tolist(), m.interceptVector.toArray().tolist()))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_fit_equals_the_single_process_fit():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    coef, icpt, _ = newton(*data(3), 3, 0.1)
    for _, gc, gi in res:
        assert max(np.abs(np.array(gc) - coef).max(), np.abs(np.array(gi) - icpt).max()) <= FIT_BOUND
    assert res[0][1:] == res[1][1:]
