"""CrossValidator on the device engine against the CPU engine on the same data: the one-pass
route (fp64 statistics) and the masked route (bf16 statistics)."""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import (CrossValidator, LinearRegression, ParamGridBuilder, SparkSession,
                                         TrainValidationSplit)
from net.jgp.labs.sparkdq4ml_amd.models.evaluation import RegressionEvaluator

pytestmark = pytest.mark.gpu

N, D, K = 20_011, 32, 5
BF16_RTOL = 1e-3  # the bound smoke() states for bf16 statistics


def _grid():
    return ParamGridBuilder().addGrid("regParam", [0.0, 0.1, 1.0]).addGrid("elasticNetParam", [0.0, 1.0]).build()


def _cv():
    return CrossValidator(estimator=LinearRegression(), estimatorParamMaps=_grid(),
                          evaluator=RegressionEvaluator(metricName="rmse"), numFolds=K, seed=42)


def _tvs():
    return TrainValidationSplit(estimator=LinearRegression(), estimatorParamMaps=_grid(),
                                evaluator=RegressionEvaluator(metricName="r2"), trainRatio=0.8, seed=42)


@pytest.fixture(scope="module")
def reference():
    """The data (f32 features, so both engines read the same values) and the CPU engine's result."""
    g = torch.Generator().manual_seed(7)
    X = torch.randn(D, N, generator=g, dtype=torch.float64).to(torch.float32)
    y = torch.linspace(-1, 2, D, dtype=torch.float64) @ X.double() + 5.0 + torch.randn(N, generator=g,
                                                                                       dtype=torch.float64)
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    cpu = SparkSession.builder().appName("test").master("cpu").getOrCreate()
    cpu.conf.set("dq4ml.cv.foldGranule", "64")
    df = cpu.createDataFrame({"features": X, "label": y})
    m, t = _cv().fit(df), _tvs().fit(df)
    ref = {"avg": list(m.avgMetrics), "best": m._bestIndex, "coef": m.bestModel.coefficients.toArray().copy(),
           "icpt": float(m.bestModel.intercept), "tvs": list(t.validationMetrics), "tvs_best": t._bestIndex}
    cpu.stop()
    return X, y, ref


def _check(m, ref, rtol):
    np.testing.assert_allclose(m.avgMetrics, ref["avg"], rtol=rtol, atol=0)
    assert m._bestIndex == ref["best"]
    np.testing.assert_allclose(m.bestModel.coefficients.toArray(), ref["coef"], rtol=rtol, atol=rtol)
    assert float(m.bestModel.intercept) == pytest.approx(ref["icpt"], rel=rtol)


def test_cross_validator_onepass_fp64(reference, gpu_session):
    X, y, ref = reference
    gpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = gpu_session.createDataFrame({"features": X.cuda(), "label": y.cuda()})
    m = _cv().fit(df)
    assert m._cv_route == "onepass"
    _check(m, ref, 1e-9)
    assert m.transform(df).count() == N
    assert float(m.bestModel.summary.rootMeanSquaredError) > 0
    t = _tvs().fit(df)
    assert t._cv_route == "onepass" and t._bestIndex == ref["tvs_best"]
    np.testing.assert_allclose(t.validationMetrics, ref["tvs"], rtol=1e-9, atol=0)


def test_cross_validator_masked_bf16(reference, gpu_session):
    X, y, ref = reference
    gpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    df = gpu_session.createDataFrame({"features": X.cuda(), "label": y.cuda()})
    cv = _cv()
    cv.setEstimator(LinearRegression().setGramDtype("bf16"))
    m = cv.fit(df)
    assert m._cv_route == "masked"
    _check(m, ref, BF16_RTOL)


def test_cross_validator_generic_on_device(reference, gpu_session):
    X, y, ref = reference
    gpu_session.conf.set("dq4ml.cv.foldGranule", "64")
    gpu_session.conf.set("dq4ml.cv.onePass", "false")
    df = gpu_session.createDataFrame({"features": X.cuda(), "label": y.cuda()})
    m = _cv().fit(df)
    assert m._cv_route == "generic"
    _check(m, ref, 1e-9)
