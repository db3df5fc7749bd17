"""MultilayerPerceptronClassifier on the device: the fit against the CPU engine's from the same
initialWeights, the prediction column and its dead rows, and the routes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import MultilayerPerceptronClassifier, SparkSession, Vectors  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops import mlp as M  # noqa: E402
from test_logreg_host import FIT_BOUND  # noqa: E402
from test_mlp_host import blobs  # noqa: E402


def _fit(master, X, y, **params):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().appName("test").master(master).getOrCreate()
    try:
        rows = [(Vectors.dense(*X[i]) if i != 2 else None, float(y[i])) for i in range(len(y))]  # row 2: no features
        df = spark.createDataFrame(rows, ["features", "label"])
        m = MultilayerPerceptronClassifier(**params).fit(df)
        out = m.transform(df)
        return m.weights.toArray(), [r[0] for r in out.select("prediction").collect()], out.columns, m.route
    finally:
        spark.stop()


@pytest.mark.parametrize("layers", ([2, 5, 2], [2, 6, 4, 2]), ids=str)
def test_device_fit_equals_the_cpu_engine(layers):
    X, y = blobs()
    params = dict(layers=layers, maxIter=25, initialWeights=Vectors.dense(*M.random_weights(layers, 11)))
    gw, gpred, gcols, groute = _fit("mi355x[*]", X, y, **params)
    cw, cpred, ccols, croute = _fit("cpu", X, y, **params)
    dist = np.abs(gw - cw).max()
    print("device fit - cpu fit", layers, dist)
    assert (groute, croute) == ("fused", "host") and gcols == ccols == ["features", "label", "prediction"]
    # (the distance that tests/test_gpu_logreg_api.py allows between a device and a CPU fit)
    assert dist <= 2 * FIT_BOUND
    assert gpred == cpred and gpred[2] is None and set(gpred) == {0.0, 1.0, None}


def test_routes():
    X = torch.zeros(8, 50)
    assert M.route(X.cuda(), [8, 8, 3]) == "fused" and M.route(X.cuda().double(), [8, 32, 32, 32]) == "fused"
    for layers in ([8, 33, 3], [8, 3], [8, 4, 4, 4, 3], [9, 8, 3]):
        assert M.route(X.cuda(), layers) == "composite"
    assert M.route(torch.zeros(65, 50).cuda(), [65, 8, 3]) == "composite" and M.route(X, [8, 8, 3]) == "host"
    rng = np.random.default_rng(1)
    layers, n = [8, 33, 3], 300
    Xr, y = torch.from_numpy(rng.uniform(-1, 1, (8, n))), torch.from_numpy(rng.integers(0, 3, n).astype(np.float64))
    w = rng.normal(size=M.weight_count(layers))
    want = M.mlp_pass_host(Xr, y, None, w, layers, M.GRAD)
    scale = M.mlp_pass_host(Xr, y, None, w, layers, M.GRAD, absolute=True)
    got = M.composite_pass(Xr.cuda(), y.cuda(), None, w, layers, M.GRAD).cpu()
    assert ((got - want).abs()[:-2] <= 1e-12 * scale[:-2]).all() and torch.equal(got[-2:], want[-2:])
    assert torch.equal(M.predict(Xr.cuda(), None, w, layers).cpu(), M.mlp_pass_host(Xr, None, None, w, layers, M.PREDICT))
