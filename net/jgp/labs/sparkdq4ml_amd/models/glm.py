"""``org.apache.spark.ml.regression.GeneralizedLinearRegression`` (Spark 2.4 semantics), fitted by
IRLS (iteratively reweighted least squares).

Families gaussian / binomial / poisson / gamma with the links of ``ops/glm.py``; each IRLS
iteration is one pass over the features for the statistics of the working response and weights
plus one small weighted least-squares solve.  On the device, for up to 64 f32 / f64 features, the
reweighting is fused into the f64 Gram pass (``csrc/hip/glm_irls.hip``) and the whole loop is
enqueued with one host read per batch of iterations; wider inputs and the CPU engine run the host
loop of ``ops/glm.py``.

Not implemented, each raising an error that says so: persistence of the fitted model,
``offsetCol``, the tweedie family with ``variancePower`` / ``linkPower``, the probit and cloglog
links.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ..ops import glm as G
from ..ops import kernels
from ..ops.layout import TiledBF16, TiledWide
from ..parallel import comm
from ..runtime.checks import defer, verify
from ..sql.dataframe import DataFrame
from ..sql.expressions import ColRef, EvalContext, Expr
from ..sql.plan import Project
from ..sql.table import ColumnData
from ..sql.types import DoubleType
from ..utils import tracing
from .linalg import DenseVector, Vector
from .param import Param, Params, param_accessors
from .regression import (_CallableDF, _CallableVector, _features_label, _fit_checks, _jarr, _JavaFloat, _JavaInt,
                         _num_features, _weight_of)

__all__ = ["GeneralizedLinearRegression", "GeneralizedLinearRegressionModel", "GeneralizedLinearRegressionSummary",
           "GeneralizedLinearRegressionTrainingSummary"]

_OUT_OF_SCOPE_PARAMS = ("offsetCol", "variancePower", "linkPower")
_OUT_OF_SCOPE_LINKS = ("probit", "cloglog")
_RESIDUAL_TYPES = ("deviance", "pearson", "working", "response")


def _not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"GeneralizedLinearRegression: {what} is not implemented")


def _family_ok(v) -> bool:
    return isinstance(v, str) and v.lower() in tuple(G.SUPPORTED) + ("tweedie",)


def _link_ok(v) -> bool:
    return v is None or (isinstance(v, str) and v.lower() in tuple(G.LINKS) + _OUT_OF_SCOPE_LINKS)


class _GLRParams(Params):
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "labelCol": Param("labelCol", "label column name", "label"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "linkPredictionCol": Param("linkPredictionCol", "link prediction (linear predictor) column name", None,
                                   has_default=False),
        "family": Param("family", "The name of family which is a description of the error distribution to be used "
                                  "in the model. Supported options: gaussian (default), binomial, poisson, gamma.",
                        "gaussian", _family_ok),
        "link": Param("link", "The name of link function which provides the relationship between the linear "
                              "predictor and the mean of the distribution function. Supported options: identity, "
                              "log, inverse, logit, sqrt.", None, _link_ok, has_default=False),
        "fitIntercept": Param("fitIntercept", "whether to fit an intercept term", True),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 25, lambda v: v >= 0, converter=int),
        "tol": Param("tol", "the convergence tolerance for iterative algorithms (>= 0)", 1e-6, lambda v: v >= 0,
                     converter=float),
        "regParam": Param("regParam", "regularization parameter for L2 regularization (>= 0)", 0.0, lambda v: v >= 0,
                          converter=float),
        "weightCol": Param("weightCol", "weight column name. If this is not set or empty, we treat all instance "
                                        "weights as 1.0", None, has_default=False),
        "solver": Param("solver", "The solver algorithm for optimization. Supported options: irls", "irls",
                        lambda v: v == "irls"),
    }

    def set(self, name, value):
        if name in _OUT_OF_SCOPE_PARAMS:
            raise _not_implemented(name)
        if name == "family" and isinstance(value, str):
            value = value.lower()
        if name == "link" and isinstance(value, str):
            value = value.lower()
        return super().set(name, value)

    _set = set

    def _family_link(self):
        """(family, link) of the params; raises for what is out of scope or unsupported."""
        family = self.getOrDefault("family")
        if family == "tweedie":
            raise _not_implemented("the tweedie family (variancePower / linkPower)")
        link = self.getOrDefault("link") if self.isSet("link") else None
        if link in _OUT_OF_SCOPE_LINKS:
            raise _not_implemented(f"the {link} link")
        return family, G.resolve_link(family, link)


for _name in _OUT_OF_SCOPE_PARAMS:  # setOffsetCol(...) etc. exist and say what they are
    setattr(_GLRParams, "set" + _name[0].upper() + _name[1:],
            (lambda n: lambda self, v: self.set(n, v))(_name))


def _dense_features(X) -> torch.Tensor:
    """The column's features as a dense f32 / f64 feature-major matrix (the tiled bf16 / fp8
    storages are not an input of the fused pass)."""
    v = X.values
    if isinstance(v, (TiledBF16, TiledWide)):
        v = v.to_dense()
    if v.dtype == torch.bfloat16 or v.dtype == torch.float16:
        v = v.to(torch.float32)
    elif v.dtype not in (torch.float32, torch.float64):
        v = v.to(torch.float64)
    return v


def _label_checks(family: str, yv: torch.Tensor, live: Optional[torch.Tensor]) -> list:
    """The family's label domain as a pending device flag."""
    if family == "binomial":
        bad, msg = (yv < 0) | (yv > 1), "The response variable of Binomial family should be in range [0, 1]."
    elif family == "poisson":
        bad, msg = yv < 0, "The response variable of Poisson family should be non-negative."
    elif family == "gamma":
        bad, msg = yv <= 0, "The response variable of Gamma family should be positive."
    else:
        return []
    if live is not None:
        bad = bad & live
    c = defer(bad.any(), lambda: ValueError("requirement failed: " + msg))
    return [] if c is None else [c]


def _rows(params, tbl, y):
    """(label f32 / f64, weight | None, selection | None): null labels merged into the selection."""
    w = _weight_of(params, tbl)
    sel = tbl.sel
    yv = y.values
    if yv.dtype not in (torch.float32, torch.float64):
        yv = yv.to(torch.float64)
    if y.valid is not None:
        sel = y.valid if sel is None else (sel & y.valid)
    return yv, w, sel


@param_accessors
class GeneralizedLinearRegression(_GLRParams):
    uid_prefix = "glm"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k in _OUT_OF_SCOPE_PARAMS:
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "GeneralizedLinearRegressionModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.regression.GeneralizedLinearRegression")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "GeneralizedLinearRegressionModel":
        family, link = self._family_link()
        tbl, X, y = _features_label(self, df)
        d = _num_features(X)
        if d <= 0:
            raise ValueError("requirement failed: The number of features must be positive.")
        if d > G.MAX_FEATURES:
            raise ValueError(f"requirement failed: Currently, GeneralizedLinearRegression only supports number of "
                             f"features <= {G.MAX_FEATURES}. Found {d} in the input dataset.")
        checks = _fit_checks(self, tbl, X)
        yv, w, sel = _rows(self, tbl, y)
        checks += _label_checks(family, yv, sel)
        Xv = _dense_features(X)
        with tracing.span("glm"):
            try:
                res = G.fit(Xv, yv, w, sel, family, link, bool(self.getOrDefault("fitIntercept")),
                            float(self.getOrDefault("regParam")), int(self.getOrDefault("maxIter")),
                            float(self.getOrDefault("tol")))
            except Exception:
                verify(checks)  # a data error of the input explains a failed solve: it goes first
                raise
        verify(checks)  # the fit has read its state: the flags cost one small copy
        tracing.add_rows("glm", tbl.nrows)
        model = GeneralizedLinearRegressionModel(self.uid, DenseVector(res.coefficients), res.intercept)
        self.copyValues(model)
        model._link_v = link
        model._set_summary(GeneralizedLinearRegressionTrainingSummary(model, df, res))
        return model


class GlmPredictExpr(Expr):
    """``unlink(features . coef + intercept)``, or the linear predictor itself (``eta=True``)."""

    def __init__(self, features: str, coef: np.ndarray, intercept: float, link: str, eta: bool = False):
        self.features, self.coef, self.intercept, self.link, self.eta = features, coef, intercept, link, eta

    def children(self):
        return [ColRef(self.features)]

    def data_type(self, schema):
        return DoubleType()

    def nullable(self, schema):
        return False

    def sql_name(self):
        return "linkPrediction" if self.eta else "prediction"

    def eval(self, ctx: EvalContext) -> ColumnData:
        X = ctx.table.column(self.features)
        with tracing.span("predict"):
            eta = kernels.predict(X.values, self.coef, self.intercept)
            out = eta if self.eta else G.unlink(self.link, eta)
            return ColumnData(DoubleType(), out, X.valid, checks=list(X.checks))


class _GlmResidualExpr(Expr):
    def __init__(self, model: "GeneralizedLinearRegressionModel", kind: str):
        self.m, self.kind = model, kind

    def children(self):
        cols = [ColRef(self.m.getOrDefault("featuresCol")), ColRef(self.m.getOrDefault("labelCol"))]
        if self.m._weight_name():
            cols.append(ColRef(self.m._weight_name()))
        return cols

    def data_type(self, schema):
        return DoubleType()

    def nullable(self, schema):
        return True

    def sql_name(self):
        return self.kind + "Residuals"

    def eval(self, ctx: EvalContext) -> ColumnData:
        m = self.m
        tbl = ctx.table
        X, y = tbl.column(m.getOrDefault("featuresCol")), tbl.column(m.getOrDefault("labelCol"))
        yv = y.values.to(torch.float64)
        eta = kernels.predict(X.values, m._coefficients.toArray(), float(m._intercept))
        mu = G.unlink(m._link, eta)
        w = torch.ones_like(yv)
        if m._weight_name():
            w = tbl.column(m._weight_name()).values.to(torch.float64)
        family = m.getOrDefault("family")
        r = yv - mu
        if self.kind == "deviance":
            dev = torch.clamp(G.unit_deviance(family, yv, mu, w), min=0.0)
            out = torch.sign(r) * torch.sqrt(dev)
        elif self.kind == "pearson":
            out = r * torch.sqrt(w) / torch.sqrt(G.variance(family, mu))
        elif self.kind == "working":
            out = r * G.dlink(m._link, mu)
        else:
            out = r
        valid = X.valid
        if y.valid is not None:
            valid = y.valid if valid is None else (valid & y.valid)
        return ColumnData(DoubleType(), out, valid, checks=list(X.checks))


@param_accessors
class GeneralizedLinearRegressionModel(_GLRParams):
    uid_prefix = "glm"

    def __init__(self, uid: Optional[str], coefficients, intercept: float):
        super().__init__(uid)
        self._coef_v = coefficients if isinstance(coefficients, Vector) else DenseVector(coefficients)
        self._icpt_v = _JavaFloat(intercept)
        self._summary = None
        self._link_v = None

    @property
    def _coefficients(self) -> Vector:
        return self._coef_v

    @property
    def _intercept(self):
        return self._icpt_v

    @property
    def _link(self) -> str:
        if self._link_v is None:
            self._link_v = self._family_link()[1]
        return self._link_v

    def _weight_name(self):
        return self.getOrDefault("weightCol") if self.isSet("weightCol") and self.getOrDefault("weightCol") else None

    @property
    def coefficients(self):
        return _CallableVector(self._coef_v.toArray())

    @property
    def intercept(self):
        return self._icpt_v

    @property
    def numFeatures(self):
        return _JavaInt(len(self._coef_v))

    def _set_summary(self, s):
        self._summary = s
        return self

    @property
    def hasSummary(self):
        return self._summary is not None

    @property
    def summary(self) -> "GeneralizedLinearRegressionTrainingSummary":
        if self._summary is None:
            raise RuntimeError(f"No training summary available for this {type(self).__name__}")
        return self._summary

    def predict(self, features) -> float:
        v = features.toArray() if isinstance(features, Vector) else np.asarray(features, dtype=np.float64)
        eta = float(np.dot(self._coef_v.toArray(), v)) + float(self._icpt_v)
        return _JavaFloat(float(G.unlink(self._link, torch.tensor(eta, dtype=torch.float64))))

    def transform(self, df: DataFrame) -> DataFrame:
        from ..sql.expressions import Alias

        fc, pc = self.getOrDefault("featuresCol"), self.getOrDefault("predictionCol")
        lpc = self.getOrDefault("linkPredictionCol") if self.isSet("linkPredictionCol") else None
        ColRef(fc).data_type(df.schema)
        new = []
        coef, icpt = self._coef_v.toArray(), float(self._icpt_v)
        if pc:
            new.append(Alias(GlmPredictExpr(fc, coef, icpt, self._link), pc))
        if lpc:
            new.append(Alias(GlmPredictExpr(fc, coef, icpt, self._link, eta=True), lpc))
        if not new:
            return df
        drop = {pc, lpc}
        exprs = [ColRef(n) for n in df.columns if n not in drop] + new
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    def evaluate(self, df: DataFrame) -> "GeneralizedLinearRegressionSummary":
        return GeneralizedLinearRegressionSummary(self, df)

    # persistence: out of scope ---------------------------------------------------------------
    def write(self):
        raise _not_implemented("persistence of the fitted model")

    def save(self, path):
        self.write()

    @classmethod
    def read(cls):
        raise _not_implemented("persistence of the fitted model")

    @classmethod
    def load(cls, path):
        cls.read()

    def __repr__(self):
        return f"GeneralizedLinearRegressionModel: uid={self.uid}, numFeatures={len(self._coef_v)}"


class GeneralizedLinearRegressionSummary:
    """Goodness of fit of a model on a DataFrame, computed at first read: one ``predict`` pass plus
    elementwise torch on the engine's device (not a hot path), summed over the ranks."""

    def __init__(self, model: GeneralizedLinearRegressionModel, df: DataFrame):
        self._model, self._df = model, df
        self._s = None
        self._pred_df = None

    def __call__(self):  # Java spelling: model.summary()
        return self

    @property
    def predictions(self) -> DataFrame:
        if self._pred_df is None:
            self._pred_df = self._model.transform(self._df)
        return self._pred_df

    @property
    def predictionCol(self):
        return self._model.getOrDefault("predictionCol")

    def _sums(self) -> dict:
        if self._s is not None:
            return self._s
        m = self._model
        family, link = m.getOrDefault("family"), m._link
        tbl = self._df._table()
        X, y = tbl.column(m.getOrDefault("featuresCol")), tbl.column(m.getOrDefault("labelCol"))
        yv, w, sel = _rows(m, tbl, y)
        eta = kernels.predict(X.values, m._coef_v.toArray(), float(m._icpt_v))
        if sel is not None:
            yv, eta = yv[sel], eta[sel]
            w = None if w is None else w[sel]
        yv = yv.to(torch.float64)
        w = torch.ones_like(yv) if w is None else w.to(torch.float64)
        mu = G.unlink(link, eta)
        r = yv - mu
        one = torch.stack([torch.tensor(float(yv.numel()), dtype=torch.float64, device=yv.device), w.sum(),
                           (w * yv).sum(), G.unit_deviance(family, yv, mu, w).sum(),
                           (w * r * r / G.variance(family, mu)).sum(), torch.log(w).sum()])
        n, wsum, wy, dev, pearson, logw = (float(v) for v in comm.all_reduce_sum(one).cpu().tolist())
        # the intercept-only model and the log-likelihood need the global sums above
        if m.getOrDefault("fitIntercept"):
            mu0 = torch.full_like(yv, wy / wsum)
        else:
            mu0 = G.unlink(link, torch.zeros_like(yv))
        if family == "gaussian":
            ll = torch.zeros((), dtype=torch.float64, device=yv.device)
        elif family == "binomial":
            wt = torch.round(w)
            k = torch.round(yv * w)
            lp = (torch.lgamma(wt + 1) - torch.lgamma(k + 1) - torch.lgamma(wt - k + 1)
                  + torch.xlogy(k, mu) + torch.xlogy(wt - k, 1.0 - mu))
            ll = torch.where(wt == 0, torch.zeros_like(lp), lp).sum()
        elif family == "poisson":
            k = torch.trunc(yv)
            ll = (w * (torch.xlogy(k, mu) - mu - torch.lgamma(k + 1))).sum()
        else:  # gamma: shape 1 / disp, scale mu disp, disp = deviance / weightSum
            disp = dev / wsum
            a, s = 1.0 / disp, mu * disp
            ll = (w * ((a - 1.0) * torch.log(yv) - yv / s - a * torch.log(s) - math.lgamma(a))).sum()
        two = torch.stack([G.unit_deviance(family, yv, mu0, w).sum(), ll])
        null_dev, ll = (float(v) for v in comm.all_reduce_sum(two).cpu().tolist())
        if family == "gaussian":
            aic = n * (np.log(dev / n * 2.0 * np.pi) + 1.0) + 2.0 - logw
        elif family == "gamma":
            aic = -2.0 * ll + 2.0
        else:
            aic = -2.0 * ll
        self._s = {"n": n, "wsum": wsum, "deviance": dev, "pearson": pearson, "nullDeviance": null_dev, "aic": aic}
        return self._s

    @property
    def numInstances(self):
        return _JavaInt(int(round(self._sums()["n"])))

    @property
    def rank(self):
        return _JavaInt(len(self._model._coef_v) + (1 if self._model.getOrDefault("fitIntercept") else 0))

    @property
    def degreesOfFreedom(self):
        return _JavaInt(self.numInstances - self.rank)

    @property
    def residualDegreeOfFreedom(self):
        return self.degreesOfFreedom

    @property
    def residualDegreeOfFreedomNull(self):
        return _JavaInt(self.numInstances - (1 if self._model.getOrDefault("fitIntercept") else 0))

    @property
    def deviance(self):
        return _JavaFloat(self._sums()["deviance"])

    @property
    def nullDeviance(self):
        return _JavaFloat(self._sums()["nullDeviance"])

    @property
    def dispersion(self):
        if self._model.getOrDefault("family") in ("binomial", "poisson"):
            return _JavaFloat(1.0)
        return _JavaFloat(self._sums()["pearson"] / self.degreesOfFreedom)

    @property
    def aic(self):
        return _JavaFloat(self._sums()["aic"] + 2.0 * self.rank)

    def residuals(self, residualsType: str = "deviance") -> DataFrame:
        from ..sql.expressions import Alias

        if residualsType not in _RESIDUAL_TYPES:
            raise ValueError(f"The residuals type {residualsType} is not supported by Generalized Linear Regression.")
        e = _GlmResidualExpr(self._model, residualsType)
        return _CallableDF(Project(self._df._plan, [Alias(e, residualsType + "Residuals")]), self._df.sparkSession)


class GeneralizedLinearRegressionTrainingSummary(GeneralizedLinearRegressionSummary):
    def __init__(self, model, df, res: "G.IrlsResult"):
        super().__init__(model, df)
        self._res = res

    @property
    def numIterations(self):
        return _JavaInt(self._res.iterations)

    @property
    def solver(self):
        return "irls"

    @property
    def route(self) -> str:
        """Which route of ``ops/glm.py`` fitted the model (engine diagnostic, not Spark's):
        "fused", "host", "composite", or "fused->host" after a handed-back device solve."""
        return self._res.route

    @property
    def coefficientStandardErrors(self):
        """sqrt(dispersion * diag((X' W' X + reg)^-1)) from the last solve's statistics, intercept last."""
        return _jarr(np.sqrt(float(self.dispersion) * np.asarray(self._res.wls.diagInvAtWA, dtype=np.float64)))

    @property
    def tValues(self):
        est = self._model._coef_v.toArray()
        if self._model.getOrDefault("fitIntercept"):
            est = np.concatenate([est, [float(self._model._icpt_v)]])
        return _jarr(est / self.coefficientStandardErrors)

    @property
    def pValues(self):
        from scipy.stats import norm, t as student_t

        tv = np.abs(np.asarray(self.tValues))
        if self._model.getOrDefault("family") in ("binomial", "poisson"):
            return _jarr(2.0 * (1.0 - norm.cdf(tv)))
        return _jarr(2.0 * (1.0 - student_t.cdf(tv, float(self.degreesOfFreedom))))
