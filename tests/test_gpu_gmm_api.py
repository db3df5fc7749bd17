"""GaussianMixture on the device against the CPU engine on the same data and seed: equal iteration
counts and predictions, parameters to 1e-9 (fp64 rounding differences of the passes, about 1e-13
relative, carried through at most five M-steps whose smallest weight is near 1 / k), the transform
columns, the summary and the route it reports."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import GaussianMixture, SparkSession, Vectors  # noqa: E402


def _fit(master, pts, **params):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().appName("test").master(master).getOrCreate()
    try:
        df = spark.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"])
        m = GaussianMixture(**params).fit(df)
        out = m.transform(df)
        assert out.columns == ["features", "prediction", "probability"]
        pred = np.array([r[0] for r in out.select("prediction").collect()])
        prob = np.array([r[0].toArray() for r in out.select("probability").collect()])
        s = m.summary
        return dict(w=np.array(m.weights), mu=np.array([g.mean.toArray() for g in m.gaussians]),
                    cov=np.array([g.cov.toArray() for g in m.gaussians]), pred=pred, prob=prob, route=s.route,
                    its=int(s.numIter), ll=float(s.logLikelihood), sizes=s.clusterSizes, k=int(s.k))
    finally:
        spark.stop()


@pytest.mark.parametrize("d,k,route", [(3, 3, "fused"), (20, 8, "fused"), (33, 2, "composite"), (3, 17, "composite")])
def test_device_equals_cpu_engine(d, k, route):
    rng = np.random.default_rng(100 * d + k)
    n = 700
    lab = rng.integers(0, min(k, 8), n)
    # (narrow blobs: with unit noise the starting Gaussians of d = 20 and 33 have logdet > 60, every
    # density falls below EPS, all responsibilities tie at 1 / k and the arg-max is decided by rounding)
    pts = (rng.normal(size=(8, d))[lab] * 0.5 + 0.1 * rng.normal(size=(n, d))).astype(np.float32).astype(np.float64)
    want = _fit("cpu", pts, k=k, seed=3, maxIter=5)
    got = _fit("mi355x[*]", pts, k=k, seed=3, maxIter=5)
    assert (want["route"], got["route"]) == ("host", route) and got["its"] == want["its"] and got["k"] == k
    np.testing.assert_array_equal(got["pred"], want["pred"])
    assert got["sizes"] == want["sizes"] == np.bincount(want["pred"], minlength=k).tolist()
    for name in ("w", "mu", "cov", "prob"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-9, atol=1e-9)
    assert got["ll"] == pytest.approx(want["ll"], rel=1e-9)
    np.testing.assert_array_equal(got["prob"].argmax(axis=1), got["pred"])
