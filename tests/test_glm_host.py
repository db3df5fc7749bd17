"""GeneralizedLinearRegression on the CPU engine: the fp64 twin of the fused pass against a 40-digit
oracle, fits against a stand-alone IRLS, the summary, the Params API, every error, Pipeline,
regParam and a two-rank (gloo) fit.

Twin bound.  ``|got_k - ref_k| <= 1e-12 * S_k`` with ``S_k`` the sum of the absolute per-row terms of
component k (tests/test_gpu_rowops.py: the project's bound for f64 row reductions).  The inputs keep
``|eta| <= 4`` and ``mu`` away from the clamps, where fp64 numpy stays below 7e-16 * S_k.

Fit tolerance.  Coefficients to ``rtol = 1e-6, atol = 1e-8`` at ``tol = 1e-12, maxIter = 50`` (the
project's solver tolerance, tests/test_gpu_pipeline.py); at the default ``tol = 1e-6`` the iteration
counts must be equal, on seeds where the oracle's last two max |delta| are each a factor 10 away
from tol (asserted).
"""
import multiprocessing as mp
import os
import socket

import mpmath
import numpy as np
import pytest
import torch

import _glm_cases as C

from net.jgp.labs.sparkdq4ml_amd import (GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                                         LinearRegression, Vectors)
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import glm, kernels

mpmath.mp.dps = 40
M = mpmath.mpf


# ---- the 40-digit oracle of the pass --------------------------------------------------------------
def _mp_working(family, link, eta, y, w, mode):
    ln, ex, sq = mpmath.log, mpmath.exp, mpmath.sqrt
    lk = {"identity": lambda m: m, "log": ln, "logit": lambda m: ln(m / (1 - m)), "inverse": lambda m: 1 / m, "sqrt": sq}
    un = {"identity": lambda e: e, "log": ex, "logit": lambda e: 1 / (1 + ex(-e)), "inverse": lambda e: 1 / e,
          "sqrt": lambda e: e * e}
    dl = {"identity": lambda m: M(1), "log": lambda m: 1 / m, "logit": lambda m: 1 / (m * (1 - m)),
          "inverse": lambda m: -1 / (m * m), "sqrt": lambda m: 1 / (2 * sq(m))}
    var = {"gaussian": lambda m: M(1), "binomial": lambda m: m * (1 - m), "poisson": lambda m: m, "gamma": lambda m: m * m}
    if mode == C.INIT:
        mu0 = {"gaussian": y, "gamma": y, "binomial": (w * y + M("0.5")) / (w + 1),
               "poisson": max(y, M("0.1"))}[family]
        return lk[link](mu0), w
    mu = un[link](eta)
    eps = M(10) ** -16
    lo, hi = {"gaussian": (None, None), "binomial": (eps, 1 - eps)}.get(family, (eps, None))
    assert (lo is None or mu > lo) and (hi is None or mu < hi), "the oracle's inputs stay off the clamps"
    g = dl[link](mu)
    return eta + (y - mu) * g, w / (g * g * var[family](mu))


def _mp_flat(case, mode):
    X, beta = case["X"], case["beta"]
    d, n = X.shape
    cnt, s = 0, [M(0)] * 4
    a, ab = [M(0)] * d, [M(0)] * d
    aa = [[M(0)] * d for _ in range(d)]
    for r in range(n):
        if case["sel"] is not None and not case["sel"][r]:
            continue
        x = [M(float(X[j, r])) for j in range(d)]
        y = M(float(case["y"][r]))
        w = M(1) if case["w"] is None else M(float(case["w"][r]))
        eta = sum((x[j] * M(float(beta[j])) for j in range(d)), M(float(beta[d])))
        z, wp = _mp_working(case["family"], case["link"], eta, y, w, mode)
        cnt += 1
        s = [s[0] + wp, s[1] + wp * wp, s[2] + wp * z, s[3] + wp * z * z]
        for j in range(d):
            a[j] += wp * x[j]
            ab[j] += wp * x[j] * z
            for i in range(j + 1):
                aa[i][j] += wp * x[i] * x[j]
    flat = [M(cnt)] + s + a + ab + [aa[i][j] for j in range(d) for i in range(j + 1)]
    return flat


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)


@pytest.mark.parametrize("family,link", C.PAIRS, ids=C.PAIR_IDS)
def test_twin_against_40_digit_oracle(family, link):
    for weights, dead, xdt in ((False, False, np.float64), (True, True, np.float32)):
        case = C.make_case(family, link, 333, 5, 11, weights=weights, dead=dead, xdtype=xdt)
        eta = case["beta"][:5] @ np.where(np.isnan(case["X"]), 0.0, case["X"]).astype(np.float64) + case["beta"][5]
        assert np.max(np.abs(eta)) <= 4.0
        for mode in (C.INIT, C.STEP):
            got = kernels.glm_pass(_t(case["X"]), _t(case["y"]), _t(case["w"]), _t(case["sel"], torch.bool),
                                   case["beta"], family, link, mode).numpy()
            ref = _mp_flat(case, mode)
            S = C.abs_sums(case, case["beta"], mode)
            err = np.array([float(abs(M(float(g)) - r)) for g, r in zip(got, ref)])
            assert len(ref) == got.shape[0] == S.shape[0]
            print(f"{family}/{link} weights={weights} dead={dead} mode={mode}: max |d|/S = {np.max(err / S):.3e}")
            assert np.all(np.isfinite(got)) and np.all(err <= C.TOL * S), np.max(err / S)


def test_twin_rejects_bad_operands():
    case = C.make_case("poisson", "log", 20, 3, 1)
    X, y = _t(case["X"]), _t(case["y"])
    with pytest.raises(ValueError, match="row-count mismatch"):
        kernels.glm_pass(X, y[:5], None, None, case["beta"], "poisson", "log", C.STEP)
    with pytest.raises(ValueError, match="beta must hold"):
        kernels.glm_pass(X, y, None, None, case["beta"][:2], "poisson", "log", C.STEP)
    with pytest.raises(ValueError, match="mode must be"):
        kernels.glm_pass(X, y, None, None, case["beta"], "poisson", "log", 5)
    with pytest.raises(ValueError, match="does not support the logit link"):
        kernels.glm_pass(X, y, None, None, case["beta"], "poisson", "logit", C.STEP)


# ---- fits -----------------------------------------------------------------------------------------
def _df(spark, case, with_weight=True):
    cols = ["features", "label", "weight"] if with_weight else ["features", "label"]
    return spark.createDataFrame(C.rows_of(case, Vectors, with_weight), cols)


def _beta(model):
    return np.concatenate([model.coefficients.toArray(), [float(model.intercept)]])


@pytest.mark.parametrize("family,link", C.PAIRS, ids=C.PAIR_IDS)
def test_fit_against_independent_irls(cpu_session, family, link):
    case = C.fit_case(family, link)
    df = _df(cpu_session, case)
    Xr = np.asarray(case["X"], dtype=np.float64).T
    coef, icpt, its, deltas = C.oracle_irls(Xr, case["y"], case["w"], family, link, tol=1e-12, max_iter=50)
    assert its < 50 or (family, link) == ("gaussian", "identity")
    m = GeneralizedLinearRegression(family=family, link=link, weightCol="weight", tol=1e-12, maxIter=50).fit(df)
    np.testing.assert_allclose(_beta(m), np.concatenate([coef, [icpt]]), rtol=1e-6, atol=1e-8)
    # default tol: the iteration counts agree, on a seed that keeps tol out of reach of the last bits
    coef, icpt, its, deltas = C.oracle_irls(Xr, case["y"], case["w"], family, link)
    m = GeneralizedLinearRegression(family=family, link=link, weightCol="weight").fit(df)
    if (family, link) == ("gaussian", "identity"):
        assert its == 0 and m.summary.numIterations == 0
    else:
        assert C.clear_of_tol(deltas), deltas
        assert m.summary.numIterations == its
    np.testing.assert_allclose(_beta(m), np.concatenate([coef, [icpt]]), rtol=1e-6, atol=1e-8)
    assert m.numFeatures == C.FIT_D and m.summary.solver == "irls"


def test_default_link_no_intercept_and_max_iter(cpu_session):
    case = C.fit_case("poisson", "log")
    df = _df(cpu_session, case, with_weight=False)
    Xr = np.asarray(case["X"], dtype=np.float64).T
    coef, icpt, its, _ = C.oracle_irls(Xr, case["y"], None, "poisson", "log", fit_icpt=False, tol=1e-12, max_iter=50)
    m = GeneralizedLinearRegression(family="poisson", fitIntercept=False, tol=1e-12, maxIter=50).fit(df)
    np.testing.assert_allclose(m.coefficients.toArray(), coef, rtol=1e-6, atol=1e-8)
    assert float(m.intercept) == 0.0 and icpt == 0.0
    coef2, icpt2, its2, _ = C.oracle_irls(Xr, case["y"], None, "poisson", "log", max_iter=2)
    m2 = GeneralizedLinearRegression(family="poisson", maxIter=2).fit(df)
    assert m2.summary.numIterations == its2 == 2
    np.testing.assert_allclose(_beta(m2), np.concatenate([coef2, [icpt2]]), rtol=1e-6, atol=1e-8)


def test_reg_param(cpu_session):
    for family, link in (("binomial", "logit"), ("gamma", "log")):
        case = C.fit_case(family, link)
        Xr = np.asarray(case["X"], dtype=np.float64).T
        coef, icpt, its, _ = C.oracle_irls(Xr, case["y"], case["w"], family, link, tol=1e-12, max_iter=50, reg=0.3)
        free = C.oracle_irls(Xr, case["y"], case["w"], family, link, tol=1e-12, max_iter=50)[0]
        assert np.linalg.norm(coef) < 0.9 * np.linalg.norm(free)  # the penalty bites
        m = GeneralizedLinearRegression(family=family, link=link, weightCol="weight", tol=1e-12, maxIter=50,
                                        regParam=0.3).fit(_df(cpu_session, case))
        np.testing.assert_allclose(_beta(m), np.concatenate([coef, [icpt]]), rtol=1e-6, atol=1e-8)


def test_wide_input_takes_the_composite_route(cpu_session):
    d, n = 70, 400
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(d, n))
    coef = rng.normal(size=d) * 0.1
    y = rng.poisson(np.exp(coef @ X + 0.3)).astype(np.float64)
    res = glm.fit(torch.as_tensor(X), torch.as_tensor(y), None, None, "poisson", None, True, 0.0, 50, 1e-12)
    assert res.route == "composite"
    want = C.oracle_irls(X.T, y, None, "poisson", "log", tol=1e-12, max_iter=50)
    np.testing.assert_allclose(np.concatenate([res.coefficients, [res.intercept]]),
                               np.concatenate([want[0], [want[1]]]), rtol=1e-6, atol=1e-8)
    with pytest.raises(ValueError, match="only supports number of features <= 4096. Found 4097"):
        glm.fit(torch.zeros(4097, 2), torch.zeros(2), None, None, "poisson", None, True, 0.0, 5, 1e-6)


# ---- summary --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,link", [("gaussian", "log"), ("binomial", "logit"), ("poisson", "log"),
                                         ("gamma", "inverse")], ids=lambda v: v)
def test_summary_identities(cpu_session, family, link):
    from scipy import stats

    case = C.fit_case(family, link)
    df = _df(cpu_session, case)
    m = GeneralizedLinearRegression(family=family, link=link, weightCol="weight", tol=1e-12, maxIter=50,
                                    linkPredictionCol="eta").fit(df)
    s = m.summary
    X, y, w = np.asarray(case["X"], dtype=np.float64), case["y"], case["w"]
    n, d = y.shape[0], X.shape[0]
    eta = m.coefficients.toArray() @ X + float(m.intercept)
    mu = C.np_unlink(link, eta)
    dev = C.np_unit_deviance(family, y, mu, w)
    assert s.deviance == pytest.approx(dev.sum(), rel=1e-10)
    mu0 = np.full(n, (w * y).sum() / w.sum())
    assert s.nullDeviance == pytest.approx(C.np_unit_deviance(family, y, mu0, w).sum(), rel=1e-10)
    assert s.nullDeviance > s.deviance
    assert (s.numInstances, s.rank, s.degreesOfFreedom, s.residualDegreeOfFreedom, s.residualDegreeOfFreedomNull) == \
        (n, d + 1, n - d - 1, n - d - 1, n - 1)
    pearson = (w * (y - mu) ** 2 / C.np_variance(family, mu)).sum()
    disp = 1.0 if family in ("binomial", "poisson") else pearson / (n - d - 1)
    assert s.dispersion == pytest.approx(disp, rel=1e-10)
    # standard errors from the last solve's weights: w' at the fitted coefficients
    g = C.np_dlink(link, mu)
    wp = w / (g * g * C.np_variance(family, mu))
    A = np.vstack([X, np.ones(n)])
    se = np.sqrt(disp * np.diag(np.linalg.inv((A * wp) @ A.T)))
    np.testing.assert_allclose(s.coefficientStandardErrors, se, rtol=1e-6)
    tv = np.concatenate([m.coefficients.toArray(), [float(m.intercept)]]) / se
    np.testing.assert_allclose(s.tValues, tv, rtol=1e-6)
    pv = 2 * (1 - stats.norm.cdf(np.abs(tv))) if family in ("binomial", "poisson") else \
        2 * (1 - stats.t.cdf(np.abs(tv), n - d - 1))
    np.testing.assert_allclose(s.pValues, pv, rtol=1e-5, atol=1e-12)
    # aic: Spark's log-likelihoods, written with scipy
    if family == "gaussian":
        ll = -2 * stats.norm.logpdf(y, mu, np.sqrt(dev.sum() / n / w)).sum()  # = n (log(2 pi dev / n) + 1) - sum log w
        aic = ll + 2
    elif family == "binomial":
        aic = -2 * stats.binom.logpmf(np.round(y * w), np.round(w), mu).sum()
    elif family == "poisson":
        aic = -2 * (w * stats.poisson.logpmf(np.trunc(y), mu)).sum()
    else:
        dsp = dev.sum() / w.sum()
        aic = -2 * (w * stats.gamma.logpdf(y, 1 / dsp, scale=mu * dsp)).sum() + 2
    assert s.aic == pytest.approx(aic + 2 * (d + 1), rel=1e-9)
    # residuals, predictions
    r = y - mu
    want = {"deviance": np.sign(r) * np.sqrt(np.maximum(dev, 0)), "pearson": r * np.sqrt(w) / np.sqrt(C.np_variance(family, mu)),
            "working": r * g, "response": r}
    for kind, ref in want.items():
        rows = s.residuals(kind).collect()
        assert s.residuals(kind).columns == [kind + "Residuals"]
        np.testing.assert_allclose([x[0] for x in rows], ref, rtol=1e-9, atol=1e-12)
    assert s.residuals().columns == ["devianceResiduals"]
    out = m.transform(df)
    assert out.columns == ["features", "label", "weight", "prediction", "eta"]
    rows = out.collect()
    np.testing.assert_allclose([x[3] for x in rows], mu, rtol=1e-12)
    np.testing.assert_allclose([x[4] for x in rows], eta, rtol=1e-12, atol=1e-14)
    assert float(m.predict(Vectors.dense(X[:, 0]))) == pytest.approx(mu[0], rel=1e-12)
    ev = m.evaluate(df)
    assert ev.deviance == pytest.approx(float(s.deviance), rel=1e-12) and not hasattr(ev, "numIterations")


def test_gaussian_identity_equals_linear_regression(cpu_session):
    case = C.fit_case("gaussian", "identity")
    df = _df(cpu_session, case)
    m = GeneralizedLinearRegression(weightCol="weight").fit(df)
    lr = LinearRegression(weightCol="weight", regParam=0.0).fit(df)
    np.testing.assert_allclose(m.coefficients.toArray(), lr.coefficients.toArray(), rtol=1e-9)
    assert float(m.intercept) == pytest.approx(float(lr.intercept), rel=1e-9)
    assert m.summary.numIterations == 0
    # the inference columns on unit weights (LinearRegression's residual sum of squares is the
    # unweighted one, the GLM dispersion is the weighted Pearson statistic)
    df = _df(cpu_session, case, with_weight=False)
    m, lr = GeneralizedLinearRegression().fit(df), LinearRegression(regParam=0.0).fit(df)
    np.testing.assert_allclose(_beta(m), np.concatenate([lr.coefficients.toArray(), [float(lr.intercept)]]), rtol=1e-9)
    assert m.summary.deviance == pytest.approx(float(lr.summary.meanSquaredError) * C.FIT_N, rel=1e-9)
    np.testing.assert_allclose(m.summary.coefficientStandardErrors, lr.summary.coefficientStandardErrors, rtol=1e-7)
    np.testing.assert_allclose(m.summary.tValues, lr.summary.tValues, rtol=1e-7)
    np.testing.assert_allclose(m.summary.pValues, lr.summary.pValues, rtol=1e-6, atol=1e-12)


def test_nulls_and_selection(cpu_session):
    """A null label leaves the fit like a filtered row; a filter is a selection, not a copy."""
    case = C.fit_case("binomial", "logit")
    rows = C.rows_of(case, Vectors)
    rows_null = [(f, None if i % 7 == 0 else y, w) for i, (f, y, w) in enumerate(rows)]
    keep = [r for i, r in enumerate(rows) if i % 7 != 0]
    cols = ["features", "label", "weight"]
    est = GeneralizedLinearRegression(family="binomial", weightCol="weight", tol=1e-12, maxIter=50)
    a = est.fit(cpu_session.createDataFrame(keep, cols))
    b = est.fit(cpu_session.createDataFrame(rows_null, cols))
    c = est.fit(cpu_session.createDataFrame([(f, y, w, i) for i, (f, y, w) in enumerate(rows)],
                                            cols + ["i"]).filter("i % 7 != 0"))
    for other in (b, c):
        np.testing.assert_allclose(_beta(other), _beta(a), rtol=1e-9, atol=1e-12)
        assert other.summary.numInstances == len(keep)
        assert other.summary.deviance == pytest.approx(float(a.summary.deviance), rel=1e-9)
    with pytest.raises(Exception, match="null weight"):
        est.fit(cpu_session.createDataFrame([(f, y, None if i == 3 else w) for i, (f, y, w) in enumerate(rows)], cols))


# ---- Params, errors, Pipeline ---------------------------------------------------------------------
def test_params_api(tmp_path):
    est = GeneralizedLinearRegression()
    assert (est.getFamily(), est.getMaxIter(), est.getTol(), est.getRegParam(), est.getFitIntercept(), est.getSolver(),
            est.getFeaturesCol(), est.getLabelCol(), est.getPredictionCol()) == \
        ("gaussian", 25, 1e-6, 0.0, True, "irls", "features", "label", "prediction")
    assert not est.isSet("link") and not est.isDefined("linkPredictionCol") and not est.isDefined("weightCol")
    est.setFamily("Poisson").setLink("LOG").setMaxIter(7).setTol(1e-9).setRegParam(0.5).setWeightCol("w") \
       .setLinkPredictionCol("eta").setFitIntercept(False)
    assert est.getFamily() == "poisson" and est.getLink() == "log" and est.getMaxIter() == 7
    text = est.explainParams()
    for name in ("family", "link", "linkPredictionCol", "maxIter", "regParam", "solver", "tol", "weightCol"):
        assert f"\n{name}: " in "\n" + text
    assert "current: poisson" in text
    path = str(tmp_path / "glr")
    est.save(path)
    back = GeneralizedLinearRegression.load(path)
    assert back.uid == est.uid and back.extractParamMap() == est.extractParamMap()
    est.write().overwrite().save(path)
    with pytest.raises(IOError, match="already exists"):
        est.write().save(path)
    kw = GeneralizedLinearRegression(family="gamma", link=None, maxIter=3)
    assert kw.getFamily() == "gamma" and not kw.isSet("link") and kw.getMaxIter() == 3
    assert kw.copy({"maxIter": 9}).getMaxIter() == 9 and kw.getMaxIter() == 3


def test_every_error(cpu_session, tmp_path):
    def raises(exc, what, fn):
        with pytest.raises(exc, match=what):
            fn()

    G = GeneralizedLinearRegression
    raises(ValueError, "parameter family given invalid value", lambda: G(family="cauchy"))
    raises(ValueError, "parameter link given invalid value", lambda: G(link="cubic"))
    raises(ValueError, "parameter solver given invalid value", lambda: G(solver="l-bfgs"))
    raises(ValueError, "parameter maxIter given invalid value", lambda: G(maxIter=-1))
    raises(ValueError, "parameter regParam given invalid value", lambda: G(regParam=-0.1))
    raises(NotImplementedError, "offsetCol is not implemented", lambda: G(offsetCol="o"))
    raises(NotImplementedError, "offsetCol is not implemented", lambda: G().setOffsetCol("o"))
    raises(NotImplementedError, "variancePower is not implemented", lambda: G().setVariancePower(1.5))
    raises(NotImplementedError, "linkPower is not implemented", lambda: G().setLinkPower(0.5))
    case = C.fit_case("binomial", "logit")
    df = _df(cpu_session, case)
    raises(NotImplementedError, "tweedie family .* is not implemented", lambda: G(family="tweedie").fit(df))
    raises(NotImplementedError, "probit link is not implemented", lambda: G(family="binomial", link="probit").fit(df))
    raises(NotImplementedError, "cloglog link is not implemented", lambda: G(family="binomial", link="cloglog").fit(df))
    raises(ValueError, "binomial family does not support the log link", lambda: G(family="binomial", link="log").fit(df))
    raises(ValueError, "gaussian family does not support the logit link", lambda: G(link="logit").fit(df))
    m = G(family="binomial").fit(df)
    raises(NotImplementedError, "persistence of the fitted model is not implemented", lambda: m.save(str(tmp_path / "m")))
    raises(NotImplementedError, "persistence of the fitted model is not implemented", lambda: m.write())
    raises(NotImplementedError, "persistence of the fitted model is not implemented",
           lambda: GeneralizedLinearRegressionModel.load(str(tmp_path / "m")))
    raises(ValueError, "residuals type student is not supported", lambda: m.summary.residuals("student"))
    raises(RuntimeError, "No training summary", lambda: GeneralizedLinearRegressionModel("u", [1.0], 0.0).summary)
    raises(ValueError, 'Field "nope" does not exist', lambda: G(featuresCol="nope").fit(df))
    raises(ValueError, "must be of type numeric", lambda: G(labelCol="features").fit(df))
    # label domains
    rows = C.rows_of(case, Vectors)
    cols = ["features", "label", "weight"]

    def with_label(v):
        return cpu_session.createDataFrame([(f, v if i == 5 else y, w) for i, (f, y, w) in enumerate(rows)], cols)
    raises(ValueError, "Binomial family should be in range \\[0, 1\\]", lambda: G(family="binomial").fit(with_label(1.5)))
    raises(ValueError, "Binomial family should be in range \\[0, 1\\]", lambda: G(family="binomial").fit(with_label(-0.5)))
    raises(ValueError, "Poisson family should be non-negative", lambda: G(family="poisson").fit(with_label(-1.0)))
    raises(ValueError, "Gamma family should be positive", lambda: G(family="gamma").fit(with_label(0.0)))
    # a bad label in a filtered row is no error
    df5 = cpu_session.createDataFrame([(f, -1.0 if i == 5 else y + 1.0, w, i) for i, (f, y, w) in enumerate(rows)],
                                      cols + ["i"]).filter("i != 5")
    assert G(family="poisson").fit(df5).summary.numInstances == len(rows) - 1
    # the documented limits are the ones that raise
    text = open(os.path.join(os.path.dirname(__file__), "..", "docs", "PARITY.md")).read()
    for word in ("offsetCol", "tweedie", "probit", "cloglog", "persistence"):
        assert word in text[text.index("K5i"):]


def test_pipeline_and_cross_validator(cpu_session, tmp_path):
    from net.jgp.labs.sparkdq4ml_amd import CrossValidator, ParamGridBuilder, VectorAssembler
    from net.jgp.labs.sparkdq4ml_amd.models.evaluation import RegressionEvaluator

    case = C.fit_case("poisson", "log")
    X = np.asarray(case["X"], dtype=np.float64)
    names = [f"x{j}" for j in range(X.shape[0])]
    df = cpu_session.createDataFrame([tuple(float(v) for v in X[:, i]) + (float(case["y"][i]),) for i in range(X.shape[1])],
                                     names + ["label"])
    glr = GeneralizedLinearRegression(family="poisson", tol=1e-12, maxIter=50)
    pipe = Pipeline([VectorAssembler().setInputCols(names).setOutputCol("features"), glr])
    pm = pipe.fit(df)
    want = C.oracle_irls(X.T, case["y"], None, "poisson", "log", tol=1e-12, max_iter=50)
    np.testing.assert_allclose(_beta(pm.stages[1]), np.concatenate([want[0], [want[1]]]), rtol=1e-6, atol=1e-8)
    assert "prediction" in pm.transform(df).columns
    path = str(tmp_path / "pipe")
    pipe.save(path)
    back = Pipeline.load(path)
    assert isinstance(back.getStages()[1], GeneralizedLinearRegression) and back.getStages()[1].getFamily() == "poisson"
    feat = pm.stages[0].transform(df)
    grid = ParamGridBuilder().addGrid("regParam", [0.0, 5.0]).build()
    cv = CrossValidator(estimator=glr, estimatorParamMaps=grid, evaluator=RegressionEvaluator(), numFolds=3, seed=3)
    cvm = cv.fit(feat)
    assert len(cvm.avgMetrics) == 2 and cvm.avgMetrics[0] < cvm.avgMetrics[1]  # rmse: the heavy penalty loses
    assert isinstance(cvm.bestModel, GeneralizedLinearRegressionModel)


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import GeneralizedLinearRegression, SparkSession, Vectors
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    case = C.fit_case("gamma", "inverse")
    rows = C.rows_of(case, Vectors)[rank::world]
    m = GeneralizedLinearRegression(family="gamma", weightCol="weight").fit(
        spark.createDataFrame(rows, ["features", "label", "weight"]))
    s = m.summary
    q.put((rank, list(m.coefficients.toArray()) + [float(m.intercept)], int(s.numIterations), float(s.deviance),
           float(s.nullDeviance), float(s.aic), int(s.numInstances), list(s.coefficientStandardErrors)))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_fit_equals_the_single_process_fit(cpu_session):
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
    case = C.fit_case("gamma", "inverse")
    m = GeneralizedLinearRegression(family="gamma", weightCol="weight").fit(_df(cpu_session, case))
    s = m.summary
    for _, beta, its, dev, null_dev, aic, n, se in res:
        np.testing.assert_allclose(beta, _beta(m), rtol=1e-9)
        assert its == s.numIterations and n == s.numInstances
        assert dev == pytest.approx(float(s.deviance), rel=1e-9) and null_dev == pytest.approx(float(s.nullDeviance), rel=1e-9)
        assert aic == pytest.approx(float(s.aic), rel=1e-9)
        np.testing.assert_allclose(se, s.coefficientStandardErrors, rtol=1e-7)
