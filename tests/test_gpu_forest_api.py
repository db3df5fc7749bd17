"""RandomForestRegressor / RandomForestClassifier on the device against the CPU engine: the same forest
tree for tree and node for node, the same transform columns, and the routes of ops/forest.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import RandomForestClassifier, RandomForestRegressor, Vectors  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops import forest as F, tree as T  # noqa: E402


def _rows(n=300):
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (n, 6))
    y = np.floor(2.0 * (X[:, 2] > 0.25) + (X[:, 0] > -0.5) + (rng.random(n) < 0.1))
    return [(Vectors.dense(*x), float(v)) for x, v in zip(X, y)]


@pytest.mark.parametrize("est,strategy", [(RandomForestRegressor, "onethird"), (RandomForestClassifier, "sqrt")])
def test_device_fit_equals_cpu_fit(gpu_session, cpu_session, est, strategy):
    fits = [est(numTrees=5, maxDepth=4, featureSubsetStrategy=strategy, subsamplingRate=0.8, seed=3).fit(
        s.createDataFrame(_rows(), ["features", "label"])) for s in (gpu_session, cpu_session)]
    assert (fits[0].route, fits[1].route) == ("fused", "host") and fits[0].getNumTrees == 5
    for g, c in zip(fits[0]._trees, fits[1]._trees):
        assert g.feature.size > 7
        for name in ("feature", "threshold", "left", "right", "count", "node_id"):
            np.testing.assert_array_equal(getattr(g, name), getattr(c, name))
        for name in ("gain", "impurity", "prediction"):
            np.testing.assert_allclose(getattr(g, name), getattr(c, name), rtol=0, atol=1e-12)
    outs = [m.transform(s.createDataFrame(_rows(), ["features", "label"])).collect() for m, s in zip(fits, (gpu_session, cpu_session))]
    for a, b in zip(*outs):
        for col in ("prediction", "probability", "rawPrediction")[:3 if est is RandomForestClassifier else 1]:
            np.testing.assert_allclose(np.asarray(a[col].toArray() if col != "prediction" else a[col]),
                                       np.asarray(b[col].toArray() if col != "prediction" else b[col]), rtol=0, atol=1e-12)


def test_routes():
    X = torch.zeros(6, 300, device="cuda")
    assert F.route(X, T.REG, 32, 0, 0, 2) == F.route(X, T.CLS, 256, 16, 0, 3) == "fused" and F.route(X.cpu(), T.REG, 32, 0, 0, 2) == "host"
    wide = torch.zeros(64, 8, device="cuda")
    assert F.route(wide, T.REG, 32, 0, 0, 22) == "fused"  # a third of the features fits where all 64 do not
    for args in ((torch.zeros(65, 8, device="cuda"), T.REG, 32, 0, 0, 22), (X, T.CLS, 32, 17, 0, 3), (wide, T.REG, 32, 0, 0, 64),
                 (X.to(torch.float16), T.REG, 32, 0, 0, 2)):
        with pytest.raises(NotImplementedError, match="no composite route"):
            F.route(*args)
    y = torch.zeros(8, device="cuda")
    with pytest.raises(NotImplementedError, match="no composite route"):
        F.fit(torch.zeros(65, 8, device="cuda"), y, None, T.REG, T.VARIANCE)
    with pytest.raises(ValueError, match="host tensors"):
        F.fit(X, X[0], None, T.REG, T.VARIANCE, how="host")
