"""GeneralizedLinearRegression on the device: the fused IRLS route against the CPU engine and the
stand-alone IRLS of _glm_cases.py, the composite route for d > 64, the hand-back of a singular
iteration, the label-domain errors, transform and summary.

Tolerances: coefficients to ``rtol = 1e-6, atol = 1e-8`` (the project's GPU-vs-CPU solver tolerance,
tests/test_gpu_pipeline.py) with equal ``numIterations`` on the seeds of ``_glm_cases.FIT_SEEDS``,
where the oracle's last two max |delta| are a factor 10 away from tol.
"""
import numpy as np
import pytest
import torch

import _glm_cases as C

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import GeneralizedLinearRegression, SparkSession, Vectors  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops import glm  # noqa: E402

COLS = ["features", "label", "weight"]
SUMMARY = ("deviance", "nullDeviance", "dispersion", "aic", "numInstances", "rank", "degreesOfFreedom",
           "residualDegreeOfFreedomNull", "numIterations")


def _session(master):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    return SparkSession.builder().appName("test").master(master).getOrCreate()


def _run(master, rows, cols, body, **params):
    """Fit on a fresh session of ``master`` and return what ``body(model, df)`` extracts."""
    if master != "cpu" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    spark = _session(master)
    try:
        df = spark.createDataFrame(rows, cols)
        return body(GeneralizedLinearRegression(**params).fit(df), df)
    finally:
        spark.stop()


def _beta(m, df=None):
    return np.concatenate([m.coefficients.toArray(), [float(m.intercept)]])


def _beta_its_route(m, df):
    return _beta(m), int(m.summary.numIterations), m.summary.route


@pytest.mark.parametrize("family,link", C.PAIRS, ids=C.PAIR_IDS)
def test_device_fit_equals_cpu_engine_and_oracle(family, link):
    case = C.fit_case(family, link)
    rows = C.rows_of(case, Vectors)
    Xr = np.asarray(case["X"], dtype=np.float64).T
    for tol, max_iter in ((1e-12, 50), (1e-6, 25)):
        coef, icpt, its, deltas = C.oracle_irls(Xr, case["y"], case["w"], family, link, tol=tol, max_iter=max_iter)
        want = np.concatenate([coef, [icpt]])
        kw = dict(family=family, link=link, weightCol="weight", tol=tol, maxIter=max_iter)
        cb, cits, croute = _run("cpu", rows, COLS, _beta_its_route, **kw)
        gb, gits, groute = _run("mi355x[*]", rows, COLS, _beta_its_route, **kw)
        assert (croute, groute) == ("host", "fused")
        np.testing.assert_allclose(gb, cb, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(gb, want, rtol=1e-6, atol=1e-8)
        if tol == 1e-6:
            assert (family, link) == ("gaussian", "identity") or C.clear_of_tol(deltas)
            assert gits == cits == its
        else:
            assert its < max_iter and gits <= max_iter


def test_reg_param_no_intercept_and_max_iter():
    case = C.fit_case("binomial", "logit")
    rows = C.rows_of(case, Vectors)
    Xr = np.asarray(case["X"], dtype=np.float64).T
    for kw, okw in ((dict(regParam=0.3, tol=1e-12, maxIter=50), dict(reg=0.3, tol=1e-12, max_iter=50)),
                    (dict(fitIntercept=False, tol=1e-12, maxIter=50), dict(fit_icpt=False, tol=1e-12, max_iter=50)),
                    (dict(maxIter=2), dict(max_iter=2))):
        coef, icpt, its, _ = C.oracle_irls(Xr, case["y"], case["w"], "binomial", "logit", **okw)
        gb, gits, route = _run("mi355x[*]", rows, COLS, _beta_its_route, family="binomial", weightCol="weight", **kw)
        assert route == "fused"
        np.testing.assert_allclose(gb, np.concatenate([coef, [icpt]]), rtol=1e-6, atol=1e-8)
        if "maxIter" in kw and kw["maxIter"] == 2:
            assert gits == its == 2


def test_wide_input_takes_the_composite_route():
    d, n = 70, 400
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(d, n))
    y = rng.poisson(np.exp((rng.normal(size=d) * 0.1) @ X + 0.3)).astype(np.float64)
    rows = [(Vectors.dense(X[:, i]), float(y[i])) for i in range(n)]
    want = C.oracle_irls(X.T, y, None, "poisson", "log", tol=1e-12, max_iter=50)
    kw = dict(family="poisson", tol=1e-12, maxIter=50)
    gb, _, route = _run("mi355x[*]", rows, COLS[:2], _beta_its_route, **kw)
    cb, _, croute = _run("cpu", rows, COLS[:2], _beta_its_route, **kw)
    assert route == croute == "composite"
    np.testing.assert_allclose(gb, np.concatenate([want[0], [want[1]]]), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(gb, cb, rtol=1e-6, atol=1e-8)


def test_singular_iteration_is_handed_back_to_the_host_route():
    """Two identical feature columns, regParam = 0: the device Cholesky reports a system that is not
    positive definite, and the fit is re-run by the host driver (Spark's quasi-Newton fallback)
    instead of returning whatever the failed solve left.  The two coefficients of the twin columns
    are not determined, their sum and every prediction are: those are compared, to 1e-4 -- the
    fallback solver stops on a 1e-6 relative change of its objective."""
    case = C.fit_case("poisson", "log")
    X = np.asarray(case["X"], dtype=np.float64)
    X = np.vstack([X[:1], X])  # feature 0 twice
    rows = [(Vectors.dense(X[:, i]), float(case["y"][i])) for i in range(X.shape[1])]

    def body(m, df):
        return _beta(m), m.summary.route, np.array([r[0] for r in m.transform(df).select("prediction").collect()])
    gb, route, gp = _run("mi355x[*]", rows, COLS[:2], body, family="poisson")
    cb, _, cp = _run("cpu", rows, COLS[:2], body, family="poisson")
    assert route == "fused->host"
    assert np.all(np.isfinite(gb))
    np.testing.assert_allclose(gp, cp, rtol=1e-4)
    np.testing.assert_allclose(np.concatenate([[gb[0] + gb[1]], gb[2:]]), np.concatenate([[cb[0] + cb[1]], cb[2:]]),
                               rtol=1e-4, atol=1e-6)
    free = C.oracle_irls(X[1:].T, case["y"], None, "poisson", "log")
    np.testing.assert_allclose(np.concatenate([[gb[0] + gb[1]], gb[2:]]), np.concatenate([free[0], [free[1]]]),
                               rtol=1e-3, atol=1e-5)


def test_label_domain_errors_surface_at_first_read():
    case = C.fit_case("binomial", "logit")
    rows = C.rows_of(case, Vectors)

    def with_label(v):
        return [(f, v if i == 5 else y, w) for i, (f, y, w) in enumerate(rows)]
    for family, bad, what in (("binomial", 1.5, "Binomial family should be in range"),
                              ("poisson", -1.0, "Poisson family should be non-negative"),
                              ("gamma", 0.0, "Gamma family should be positive")):
        with pytest.raises(ValueError, match=what):
            _run("mi355x[*]", with_label(bad), COLS, lambda m, df: None, family=family, weightCol="weight")
    # in a filtered row it is no error
    rows5 = [(f, -1.0 if i == 5 else y + 1.0, w, i) for i, (f, y, w) in enumerate(rows)]
    spark = _session("mi355x[*]")
    try:
        df = spark.createDataFrame(rows5, COLS + ["i"]).filter("i != 5")
        m = GeneralizedLinearRegression(family="poisson", weightCol="weight").fit(df)
        assert m.summary.route == "fused" and m.summary.numInstances == len(rows) - 1
    finally:
        spark.stop()


@pytest.mark.parametrize("family,link", [("binomial", "logit"), ("gamma", "inverse"), ("gaussian", "log")], ids=lambda v: v)
def test_transform_and_summary_match_the_cpu_engine(family, link):
    case = C.fit_case(family, link)
    rows = C.rows_of(case, Vectors)
    rows = [(f, None if i % 11 == 0 else y, w) for i, (f, y, w) in enumerate(rows)]  # null labels: selected away

    def body(m, df):
        s = m.summary
        out = m.transform(df)
        assert out.columns == COLS + ["prediction", "eta"]
        pred = np.array([[r[3], r[4]] for r in out.collect()])
        res = {k: np.array([r[0] for r in s.residuals(k).collect()], dtype=np.float64)
               for k in ("deviance", "pearson", "working", "response")}
        ev = m.evaluate(df)
        return ({k: float(getattr(s, k)) for k in SUMMARY}, np.asarray(s.coefficientStandardErrors), np.asarray(s.tValues),
                np.asarray(s.pValues), pred, res, float(ev.deviance), float(m.predict(Vectors.dense(case["X"][:, 0]))))
    kw = dict(family=family, link=link, weightCol="weight", linkPredictionCol="eta", tol=1e-12, maxIter=50)
    g = _run("mi355x[*]", rows, COLS, body, **kw)
    c = _run("cpu", rows, COLS, body, **kw)
    for k in SUMMARY:
        assert g[0][k] == pytest.approx(c[0][k], rel=1e-6, abs=1e-9), k
    assert g[0]["numInstances"] == sum(1 for r in rows if r[1] is not None)
    for i in (1, 2):
        np.testing.assert_allclose(g[i], c[i], rtol=1e-5)
    np.testing.assert_allclose(g[3], c[3], rtol=1e-4, atol=1e-12)
    np.testing.assert_allclose(g[4], c[4], rtol=1e-6, atol=1e-9)
    for k in g[5]:
        np.testing.assert_allclose(g[5][k], c[5][k], rtol=1e-5, atol=1e-8, equal_nan=True)
    assert g[6] == pytest.approx(c[6], rel=1e-6) and g[7] == pytest.approx(c[7], rel=1e-6)


def test_fused_limits_route_through_ops_glm():
    """``ops.glm.fit`` on device tensors: f32 features take the fused route, a forced composite route
    agrees with it, and an unknown route is refused."""
    case = C.make_case("poisson", "log", 5000, 33, 3, weights=True, dead=True, xdtype=np.float32)
    X = torch.as_tensor(case["X"]).cuda()
    y, w, sel = (torch.as_tensor(case[k]).cuda() for k in ("y", "w", "sel"))
    a = glm.fit(X, y, w, sel, "poisson", "log", True, 0.0, 50, 1e-12)
    b = glm.fit(torch.nan_to_num(X), torch.nan_to_num(y), w, sel, "poisson", "log", True, 0.0, 50, 1e-12, route="composite")
    assert (a.route, b.route) == ("fused", "composite")
    np.testing.assert_allclose(np.append(a.coefficients, a.intercept), np.append(b.coefficients, b.intercept),
                               rtol=1e-6, atol=1e-8)
    live = case["sel"]
    want = C.oracle_irls(np.asarray(case["X"], dtype=np.float64).T[live], case["y"][live], case["w"][live], "poisson", "log",
                         tol=1e-12, max_iter=50)
    np.testing.assert_allclose(np.append(a.coefficients, a.intercept), np.append(want[0], want[1]), rtol=1e-6, atol=1e-8)
    with pytest.raises(ValueError, match="unknown route"):
        glm.fit(X, y, w, sel, "poisson", "log", True, 0.0, 5, 1e-6, route="magic")
