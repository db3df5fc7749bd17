"""``org.apache.spark.ml.tuning``: ``ParamGridBuilder``, ``CrossValidator`` and
``TrainValidationSplit`` with their models.

Spark fits every (fold, paramMap) pair and scores it with one more pass.  Here a normal-equation
``LinearRegression`` is solved from the flat additive statistics vector of the Gram kernels, so
when one pass yields one such vector per fold (``ops.kernels.gram_stats_folds``)

* the training statistics of fold f are ``total - fold_f``;
* every (fold, paramMap) model is a solve (``optim.fit_wls_flat``), no data pass;
* rmse / mse / r2 / var of the validation fold are closed forms of ``fold_f``'s own moments and
  the coefficients;
* the best model is the solve on ``total``.

Routes (kept on the fitted model as ``_cv_route``):

``onepass``  the fold statistics come from the one-pass ``gram_folds`` kernel (64-row granules);
``masked``   the same statistics from k masked ``gram_stats`` passes (any granule, any gramDtype,
             any storage; the CPU engine);
``generic``  everything the statistics cannot express (pipelines, huber, l-bfgs, mae, weights,
             non-solve params in the grid): per fold, train and validation DataFrames over the
             SAME columns with a narrowed selection vector, then fit / transform / evaluate.

All routes draw the folds from one rule (``ops.kernels.fold_ids``), so they partition the rows
identically.  docs/DESIGN.md has the rule, the granule choice and the cancellation guard."""
from __future__ import annotations

import itertools
from typing import List, Optional

import numpy as np

from ..ops import kernels
from ..parallel import comm
from ..runtime.checks import verify
from ..sql.dataframe import DataFrame
from .evaluation import RegressionEvaluator
from .linalg import DenseVector
from .optim import MAX_NUM_FEATURES, fit_wls_flat, packed_upper_indices
from .param import Param, Params, param_accessors
from .pipeline import Pipeline

__all__ = ["ParamGridBuilder", "CrossValidator", "CrossValidatorModel", "TrainValidationSplit",
           "TrainValidationSplitModel"]

# params of LinearRegression that only change the solve on fixed statistics
_SOLVE_PARAMS = frozenset(("regParam", "elasticNetParam", "fitIntercept", "standardization", "maxIter", "tol",
                           "solver"))
_STAT_METRICS = ("rmse", "mse", "r2", "var")
# validation SSE below this fraction of the fold's raw Σy² has lost its digits to cancellation
# (raw moments; docs/DESIGN.md): the fit then takes the generic route
CANCEL_GUARD = 1e-9


def _pname(p) -> str:
    return p.name if isinstance(p, Param) else str(p)


class ParamGridBuilder:
    """Builder of a param grid: the cartesian product of the ``addGrid`` value lists, every map
    extended by the ``baseOn`` pairs.  Params are named by string (or ``Param``)."""

    def __init__(self):
        self._grid = {}

    def addGrid(self, param, values):
        self._grid[_pname(param)] = list(values)
        return self

    def baseOn(self, *args):
        if len(args) == 1 and isinstance(args[0], dict):
            pairs = list(args[0].items())
        else:
            pairs = list(args)
        for p, v in pairs:
            self.addGrid(p, [v])
        return self

    def build(self) -> List[dict]:
        names = list(self._grid)
        return [dict(zip(names, vals)) for vals in itertools.product(*(self._grid[n] for n in names))]


# ---------------------------------------------------------------------------------------------
# shared machinery
# ---------------------------------------------------------------------------------------------
def _default_seed(name: str) -> int:
    h = 0
    for ch in name:  # java.lang.String.hashCode of the class name, as Spark seeds its tuners
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


def _granule(session, nrows: int, k: int) -> int:
    """``dq4ml.cv.foldGranule`` = auto | 1 | 64; auto: 64 when every fold expects >= 64 granules."""
    v = str(session.conf.get("dq4ml.cv.foldGranule", "auto")).lower() if session is not None else "auto"
    if v == "auto":
        return 64 if nrows >= 64 * 64 * k else 1
    if v not in ("1", "64"):
        raise ValueError(f"dq4ml.cv.foldGranule must be auto, 1 or 64, not {v!r}")
    return int(v)


def _one_pass_conf(session) -> bool:
    v = session.conf.get("dq4ml.cv.onePass", "true") if session is not None else "true"
    return str(v).lower() not in ("false", "0")


def _stats_eligible(est, maps, ev, session) -> bool:
    from .regression import LinearRegression

    if type(est) is not LinearRegression or not isinstance(ev, RegressionEvaluator) or not _one_pass_conf(session):
        return False
    if any(not set(m) <= _SOLVE_PARAMS for m in maps):
        return False
    for m in maps or [{}]:
        e = est.copy(m) if m else est
        if e.getOrDefault("loss") != "squaredError" or e.getOrDefault("solver") not in ("auto", "normal"):
            return False
    if est.isSet("weightCol") and est.getOrDefault("weightCol"):
        return False
    return (ev.getOrDefault("metricName") in _STAT_METRICS
            and ev.getOrDefault("labelCol") == est.getOrDefault("labelCol")
            and ev.getOrDefault("predictionCol") == est.getOrDefault("predictionCol"))


class _FoldMoments:
    """One fold's statistics unpacked for the metric closed forms."""

    def __init__(self, flat: np.ndarray, d: int):
        self.n, self.bSum, self.bb = float(flat[0]), float(flat[3]), float(flat[4])
        self.a, self.ab = flat[5:5 + d], flat[5 + d:5 + 2 * d]
        I, J = packed_upper_indices(d)
        self.AA = np.zeros((d, d))
        self.AA[I, J] = flat[5 + 2 * d:]
        self.AA[J, I] = flat[5 + 2 * d:]

    def sums(self, beta: np.ndarray, b: float):
        """(SSE, Σp, Σp²) of predictions p = βᵀx + b over the fold's rows."""
        ba = float(beta @ self.a)
        spp = float(beta @ self.AA @ beta) + 2.0 * b * ba + b * b * self.n
        sse = self.bb - 2.0 * float(beta @ self.ab) - 2.0 * b * self.bSum + spp
        return sse, ba + b * self.n, spp

    def metric(self, name: str, through_origin: bool, sse: float, sp: float, spp: float) -> float:
        n = self.n
        if name == "mse":
            return sse / n
        if name == "rmse":
            return float(np.sqrt(max(sse, 0.0) / n))
        mean_y = self.bSum / n
        if name == "var":
            return (spp - 2.0 * mean_y * sp + n * mean_y ** 2) / n
        if through_origin:
            return 1.0 - sse / self.bb
        return 1.0 - sse / (self.bb - n * mean_y ** 2)


def _solve(est, flat: np.ndarray, d: int):
    from .regression import _wls_args

    return fit_wls_flat(flat, *_wls_args(est, d)[1:])


def _plain_model(est, wls):
    from .regression import LinearRegressionModel

    m = LinearRegressionModel(est.uid, DenseVector(np.asarray(wls.coefficients, dtype=np.float64)),
                              float(wls.intercept))
    est.copyValues(m)
    return m


def _stats_fit(est, maps, ev, df, classes, seed, cross: bool):
    """The statistics routes.  ``classes``: k (equal folds) or weights.  ``cross``: k-fold (train
    on total - fold f, validate on fold f, for every f) or a single split (train on class 0,
    validate on class 1).  Returns (route, metrics [folds][maps], best index, best model, sub-models)
    or None when the fit must take the generic route (solver not normal-equation at this d, an
    empty class, or the cancellation guard)."""
    from .regression import (LinearRegressionModel, LinearRegressionTrainingSummary, _features_label, _fit_checks,
                             _gram_dtype, _num_features)

    tbl, X, y = _features_label(est, df)
    d = _num_features(X)
    if d <= 0:
        raise ValueError("requirement failed: The number of features must be positive.")
    for m in maps or [{}]:
        if d > MAX_NUM_FEATURES and (est.copy(m) if m else est).getOrDefault("solver") == "auto":
            return None  # auto picks l-bfgs above 4096 features
    checks = _fit_checks(est, tbl, X)
    sel = tbl.sel
    if y.valid is not None:
        sel = y.valid if sel is None else (sel & y.valid)
    k = classes if isinstance(classes, int) else len(classes)
    granule = _granule(df.sparkSession, tbl.nrows, k)
    gd = _gram_dtype(est, df)
    Xv = X.values
    route = kernels.folds_route(Xv, granule, gd)
    stats = kernels.gram_stats_folds(Xv, y.values, sel, classes, seed, granule, gd)
    stats = comm.all_reduce_sum(stats)  # one all-reduce of the whole [k, P] tensor
    host = stats.detach().cpu().numpy()  # one D2H
    verify(checks)
    if np.any(host[:, 0] <= 0):
        return None
    total = host.sum(axis=0)
    pairs = [(total - host[f], host[f]) for f in range(k)] if cross else [(host[0], host[1])]
    name, origin = ev.getOrDefault("metricName"), bool(ev.getOrDefault("throughOrigin"))
    ests = [est.copy(m) for m in (maps or [{}])]
    metrics, subs = [], []
    for train, val in pairs:
        fm = _FoldMoments(val, d)
        row, srow = [], []
        for e in ests:
            wls, _ = _solve(e, train, d)
            beta, b = np.asarray(wls.coefficients, dtype=np.float64), float(wls.intercept)
            sse, sp, spp = fm.sums(beta, b)
            if not sse > CANCEL_GUARD * fm.bb:
                return None  # cancellation guard: the raw moments cannot resolve this residual
            row.append(fm.metric(name, origin, sse, sp, spp))
            srow.append(_plain_model(e, wls))
        metrics.append(row)
        subs.append(srow)
    avg = np.mean(np.asarray(metrics, dtype=np.float64), axis=0)
    best = int(np.argmax(avg) if ev.isLargerBetter() else np.argmin(avg))
    be = ests[best]
    # the refit: a solve on the total statistics, with the usual lazy training summary
    wls, gstats = _solve(be, total, d)
    model = LinearRegressionModel(be.uid, None, 0.0)
    be.copyValues(model)
    model._coefficients = DenseVector(wls.coefficients)
    model._intercept = float(wls.intercept)
    model._set_summary(LinearRegressionTrainingSummary(model, df, wls, wls.objectiveHistory, stats=gstats,
                                                       solver=wls.solver))
    return route, metrics, best, model, subs


def _fit_with(est, df, pm):
    """``est.fit(df)`` under param map ``pm``; a Pipeline hands each param to the stages that
    declare it."""
    if isinstance(est, Pipeline):
        stages, used = [], set()
        for s in est.getStages():
            sub = {n: v for n, v in pm.items() if isinstance(s, Params) and n in s.params_list()}
            used |= set(sub)
            stages.append(s.copy(sub) if sub else s)
        missing = set(pm) - used
        if missing:
            raise KeyError(f"Param {sorted(missing)[0]} does not exist.")
        return Pipeline(stages, uid=est.uid).fit(df)
    return (est.copy(pm) if pm else est).fit(df)


def _generic_fit(est, maps, ev, df, classes, seed, cross: bool, collect: bool):
    """Spark's loop over fold DataFrames that share the executed table's columns."""
    tbl = df._table()  # the plan runs once
    k = classes if isinstance(classes, int) else len(classes)
    granule = _granule(df.sparkSession, tbl.nrows, k)
    ids = kernels.fold_ids(tbl.nrows, classes, seed, granule, tbl.device)
    splits = [(ids != f, ids == f) for f in range(k)] if cross else [(ids == 0, ids == 1)]
    metrics, subs = [], []
    for tm, vm in splits:
        train, val = df._narrowed(tbl, tm), df._narrowed(tbl, vm)
        row, srow = [], []
        for pm in (maps or [{}]):
            m = _fit_with(est, train, pm)
            row.append(float(ev.evaluate(m.transform(val))))
            srow.append(m if collect else None)
        metrics.append(row)
        subs.append(srow)
    avg = np.mean(np.asarray(metrics, dtype=np.float64), axis=0)
    best = int(np.argmax(avg) if ev.isLargerBetter() else np.argmin(avg))
    model = _fit_with(est, df, (maps or [{}])[best])
    return "generic", metrics, best, model, subs


def _tune(self, df, classes, cross: bool):
    est, ev = self.getOrDefault("estimator"), self.getOrDefault("evaluator")
    maps = [{_pname(p): v for p, v in m.items()} for m in (self.getOrDefault("estimatorParamMaps") or [{}])]
    seed, collect = int(self.getOrDefault("seed")), bool(self.getOrDefault("collectSubModels"))
    res = None
    if _stats_eligible(est, maps, ev, getattr(df, "sparkSession", None)):
        res = _stats_fit(est, maps, ev, df, classes, seed, cross)
    if res is None:
        res = _generic_fit(est, maps, ev, df, classes, seed, cross, collect)
    route, metrics, best, model, subs = res
    return route, metrics, best, model, (subs if collect else None)


class _TunerParams(Params):
    _params = {
        "estimator": Param("estimator", "estimator to be cross-validated", None, has_default=False),
        "estimatorParamMaps": Param("estimatorParamMaps", "param maps for the estimator", None, has_default=False),
        "evaluator": Param("evaluator", "evaluator used to select hyper-parameters that maximize the validated "
                                        "metric", None, has_default=False),
        "seed": Param("seed", "random seed", 0, converter=int),
        "parallelism": Param("parallelism", "the number of threads to use when running parallel algorithms (>= 1); "
                                            "accepted, unused: the statistics routes need no data pass per model",
                             1, lambda v: v >= 1, converter=int),
        "collectSubModels": Param("collectSubModels", "whether to collect a list of sub-models trained during "
                                                      "tuning", False, converter=bool),
    }

    def _init(self, kw):
        self._paramMap.setdefault("seed", _default_seed("org.apache.spark.ml.tuning." + type(self).__name__))
        for k, v in kw.items():
            if v is not None:
                self.set(k, v)

    def set(self, name, value):
        if name in ("estimator", "evaluator", "estimatorParamMaps"):
            self._paramMap[name] = list(value) if name == "estimatorParamMaps" else value
            return self
        return super().set(name, value)


class _TunedModel(Params):
    """Common part of the two tuned models: ``transform`` delegates to ``bestModel``."""

    def __init__(self, best_model, uid=None):
        super().__init__(uid)
        self.bestModel = best_model
        self.subModels = None
        self._cv_route = None

    def transform(self, df: DataFrame) -> DataFrame:
        return self.bestModel.transform(df)


@param_accessors
class CrossValidator(_TunerParams):
    """K-fold cross-validation.  ``numFolds`` >= 2 (at most 16)."""

    uid_prefix = "cv"
    _params = {"numFolds": Param("numFolds", "number of folds for cross validation (>= 2)", 3,
                                 lambda v: 2 <= v <= kernels.MAX_FOLDS, converter=int)}

    def __init__(self, estimator=None, estimatorParamMaps=None, evaluator=None, numFolds=None, seed=None,
                 parallelism=None, collectSubModels=None, uid=None):
        super().__init__(uid)
        self._init(dict(estimator=estimator, estimatorParamMaps=estimatorParamMaps, evaluator=evaluator,
                        numFolds=numFolds, seed=seed, parallelism=parallelism, collectSubModels=collectSubModels))

    def fit(self, dataset: DataFrame, params=None) -> "CrossValidatorModel":
        cv = self.copy(params) if params else self
        route, metrics, best, model, subs = _tune(cv, dataset, int(cv.getOrDefault("numFolds")), True)
        out = CrossValidatorModel(model, list(np.mean(np.asarray(metrics, dtype=np.float64), axis=0)), uid=cv.uid)
        cv.copyValues(out)
        out.subModels, out._cv_route, out._foldMetrics, out._bestIndex = subs, route, metrics, best
        return out


@param_accessors
class CrossValidatorModel(_TunedModel):
    uid_prefix = "cv"
    _params = dict(_TunerParams._params, **CrossValidator._params)

    def __init__(self, bestModel, avgMetrics: Optional[list] = None, uid=None):
        super().__init__(bestModel, uid)
        self.avgMetrics = [float(v) for v in (avgMetrics or [])]


@param_accessors
class TrainValidationSplit(_TunerParams):
    """One random split: train on ``trainRatio`` of the rows, validate on the rest."""

    uid_prefix = "tvs"
    _params = {"trainRatio": Param("trainRatio", "ratio between train and validation data. Must be between 0 and 1.",
                                   0.75, lambda v: 0 < v < 1, converter=float)}

    def __init__(self, estimator=None, estimatorParamMaps=None, evaluator=None, trainRatio=None, seed=None,
                 parallelism=None, collectSubModels=None, uid=None):
        super().__init__(uid)
        self._init(dict(estimator=estimator, estimatorParamMaps=estimatorParamMaps, evaluator=evaluator,
                        trainRatio=trainRatio, seed=seed, parallelism=parallelism, collectSubModels=collectSubModels))

    def fit(self, dataset: DataFrame, params=None) -> "TrainValidationSplitModel":
        tv = self.copy(params) if params else self
        r = float(tv.getOrDefault("trainRatio"))
        route, metrics, best, model, subs = _tune(tv, dataset, [r, 1.0 - r], False)
        out = TrainValidationSplitModel(model, metrics[0], uid=tv.uid)
        tv.copyValues(out)
        out.subModels, out._cv_route, out._bestIndex = (subs[0] if subs else None), route, best
        return out


@param_accessors
class TrainValidationSplitModel(_TunedModel):
    uid_prefix = "tvs"
    _params = dict(_TunerParams._params, **TrainValidationSplit._params)

    def __init__(self, bestModel, validationMetrics: Optional[list] = None, uid=None):
        super().__init__(bestModel, uid)
        self.validationMetrics = [float(v) for v in (validationMetrics or [])]
