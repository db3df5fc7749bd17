"""LogisticRegression on the device: the fit against the Newton optimum of tests/test_logreg_host.py
(same recorded bound), its columns and accuracy against the CPU engine's, and the composite route
beyond the fused kernel's range."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import LogisticRegression, SparkSession  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops import logreg as L  # noqa: E402
from test_logreg_host import FIT_BOUND, data, fitted, frame, newton, weights  # noqa: E402


def _fit(master, X, y, w, **params):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().appName("test").master(master).getOrCreate()
    try:
        df = frame(spark, X, y, w)
        m = LogisticRegression(**params).fit(df)
        rows = m.transform(df).select("rawPrediction", "probability", "prediction").collect()
        cols = [np.array([np.asarray(r[i].toArray() if i < 2 else r[i]) for r in rows]) for i in range(3)]
        return fitted(m), cols, float(m.summary.accuracy), m.summary.route
    finally:
        spark.stop()


@pytest.mark.parametrize("K,weighted", [(1, False), (3, False), (3, True)])
def test_device_fit_reaches_the_newton_optimum_and_equals_the_cpu_engine(K, weighted):
    X, y = data(K)
    w = weights(len(y)) if weighted else None
    params = dict(regParam=0.1, tol=1e-12, weightCol="weight" if weighted else None)
    coef, icpt, _ = newton(X, y, K, 0.1, w)
    (gc, gi), gcols, gacc, groute = _fit("mi355x[*]", X, y, w, **params)
    dist = max(np.abs(gc - coef).max(), np.abs(gi - icpt).max())
    print("device fit distance", K, weighted, dist)
    assert groute == "fused" and dist <= FIT_BOUND
    _, ccols, cacc, croute = _fit("cpu", X, y, w, **params)
    assert croute == "host" and gacc == cacc
    np.testing.assert_array_equal(gcols[2], ccols[2])
    for a, b in zip(gcols[:2], ccols[:2]):  # (two fits FIT_BOUND from one optimum; |x| <= ~12 here)
        assert np.abs(a - b).max() <= 2 * FIT_BOUND * (np.abs(X).sum(axis=1).max() + 1)


@pytest.mark.parametrize("d,K", [(65, 3), (3, 65)])
def test_wide_inputs_take_the_composite(d, K):
    rng = np.random.default_rng(d + K)
    n = 300
    X = torch.from_numpy(rng.uniform(-1, 1, (d, n)))
    y, w = torch.from_numpy(rng.integers(0, K, n).astype(np.float64)), torch.from_numpy(rng.uniform(0.5, 2, n))
    C = rng.normal(size=(K, d + 1))
    assert L.route(X.cuda(), K) == "composite" and L.route(X[:64].cuda(), min(K, 64)) == "fused" and L.route(X, K) == "host"
    want = L.logreg_pass_host(X, y, w, None, C, L.GRAD)
    got = L.composite_pass(X.cuda(), y.cuda(), w.cuda(), None, C, L.GRAD).cpu()
    assert ((got - want).abs() <= 1e-12 * n * (1 + want.abs())).all()
    for a, b in zip(L.predict(X.cuda(), None, C), L.logreg_pass_host(X, None, None, None, C, L.PREDICT)):
        assert (a.cpu() - b).abs().max() <= 1e-12 * (d + 1) * 8
