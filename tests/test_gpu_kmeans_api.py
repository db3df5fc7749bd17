"""KMeans on the device against the CPU engine on the same data and seed: equal assignments,
centres to 1e-12 of the fp64 sum of absolute terms, and the route the summary reports."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import KMeans, SparkSession, Vectors  # noqa: E402


def _fit(master, pts, **params):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().appName("test").master(master).getOrCreate()
    try:
        df = spark.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"])
        m = KMeans(**params).fit(df)
        pred = np.array([r[0] for r in m.transform(df).select("prediction").collect()])
        return np.array(m.clusterCenters()), pred, float(m.computeCost(df)), m.summary.route, int(m.summary.numIter)
    finally:
        spark.stop()


@pytest.mark.parametrize("d,k,route", [(3, 3, "fused"), (33, 17, "fused"), (65, 3, "composite"), (3, 65, "composite")])
@pytest.mark.parametrize("init", ["k-means||", "random"])
def test_device_equals_cpu_engine(d, k, route, init):
    rng = np.random.default_rng(100 * d + k)
    n = 700
    lab = rng.integers(0, min(k, 8), n)
    pts = (rng.normal(size=(8, d))[lab] * 6 + rng.normal(size=(n, d))).astype(np.float32).astype(np.float64)
    cw, pw, costw, rw, itw = _fit("cpu", pts, k=k, seed=3, initMode=init)
    cg, pg, costg, rg, itg = _fit("mi355x[*]", pts, k=k, seed=3, initMode=init)
    assert (rw, rg) == ("host", route) and itw == itg
    np.testing.assert_array_equal(pg, pw)
    S = np.stack([np.abs(pts[pw == c]).sum(axis=0) for c in range(k)])
    assert (np.abs(cg - cw) <= 1e-12 * np.maximum(S, 1e-300)).all()
    assert costg == pytest.approx(costw, rel=1e-12)
