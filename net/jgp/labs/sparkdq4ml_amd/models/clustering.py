"""``org.apache.spark.ml.clustering``: ``KMeans`` (Spark 2.4 semantics, euclidean distance) and, in
the second half of this file, ``GaussianMixture``.

The Lloyd iterations, the seeding and the routes are ``ops/kmeans.py``'s: on the device, for dense
f32 / f64 features with d <= 64 and k <= 64, one iteration is one launch of ``csrc/hip/kmeans.hip``
and the loop is enqueued with one host read per batch; wider inputs take the torch composite and
the CPU engine the fp64 twin.  Starting centres come from the project's own seeded rule, so they
agree with Spark's in distribution, not bit for bit.

Not implemented, each raising an error that says so: ``distanceMeasure="cosine"``, persistence of
the fitted model, ``weightCol`` (a Spark 3 feature).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ops import gmm as G
from ..ops import kmeans as K
from ..sql.dataframe import DataFrame
from ..sql.expressions import Alias, ColRef, EvalContext, Expr
from ..sql.plan import Project
from ..sql.table import ColumnData
from ..sql.types import IntegerType, VectorUDT
from ..utils import tracing
from .glm import _dense_features
from .linalg import DenseMatrix, DenseVector, SparseVector
from .param import Param, Params, param_accessors
from .regression import _JavaFloat, _JavaInt

__all__ = ["KMeans", "KMeansModel", "KMeansSummary", "GaussianMixture", "GaussianMixtureModel", "GaussianMixtureSummary",
           "MultivariateGaussian"]


def _not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"KMeans: {what} is not implemented")


class _KMeansParams(Params):
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "k": Param("k", "The number of clusters to create. Must be > 1.", 2, lambda v: v > 1, converter=int),
        "initMode": Param("initMode", "The initialization algorithm. Supported options: 'random' and 'k-means||'.",
                          "k-means||", lambda v: v in ("random", "k-means||")),
        "initSteps": Param("initSteps", "The number of steps for k-means|| initialization mode. Must be > 0.", 2,
                           lambda v: v > 0, converter=int),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 20, lambda v: v >= 0, converter=int),
        "tol": Param("tol", "the convergence tolerance for iterative algorithms (>= 0)", 1e-4, lambda v: v >= 0,
                     converter=float),
        "seed": Param("seed", "random seed", -1689246527, converter=int),
        "distanceMeasure": Param("distanceMeasure", "The distance measure. Supported options: 'euclidean' and 'cosine'.",
                                 "euclidean", lambda v: v in ("euclidean", "cosine")),
    }

    def set(self, name, value):
        if name == "weightCol":
            raise _not_implemented("weightCol (a Spark 3 feature)")
        return super().set(name, value)

    _set = set

    def setWeightCol(self, v):
        return self.set("weightCol", v)


def _features(params, df: DataFrame):
    """(table, dense feature-major features, selection with null vectors merged in)."""
    fc = params.getOrDefault("featuresCol")
    ColRef(fc).data_type(df.schema)
    tbl = df._table()
    X = tbl.column(fc)
    sel = tbl.sel
    if X.valid is not None:
        sel = X.valid if sel is None else (sel & X.valid)
    return tbl, _dense_features(X), sel


@param_accessors
class KMeans(_KMeansParams):
    uid_prefix = "kmeans"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k == "weightCol":
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "KMeansModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.clustering.KMeans")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "KMeansModel":
        if self.getOrDefault("distanceMeasure") == "cosine":
            raise _not_implemented('distanceMeasure="cosine"')
        tbl, Xv, sel = _features(self, df)
        with tracing.span("kmeans"):
            res = K.fit(Xv, sel, self.getOrDefault("k"), self.getOrDefault("initMode"), self.getOrDefault("initSteps"),
                        self.getOrDefault("maxIter"), self.getOrDefault("tol"), self.getOrDefault("seed"))
        tracing.add_rows("kmeans", tbl.nrows)
        model = KMeansModel(self.uid, res.centers)
        self.copyValues(model)
        model._summary = KMeansSummary(model, df, res)
        return model


class KMeansPredictExpr(Expr):
    """The index of the nearest centre of a features column (the ASSIGN pass)."""

    def __init__(self, features: str, centers: np.ndarray):
        self.features, self.centers = features, centers

    def children(self):
        return [ColRef(self.features)]

    def data_type(self, schema):
        return IntegerType()

    def sql_name(self):
        return "prediction"

    def eval(self, ctx: EvalContext) -> ColumnData:
        X = ctx.table.column(self.features)
        with tracing.span("kmeans_predict"):
            idx, _ = K.assign(_dense_features(X), X.valid, self.centers)
            return ColumnData(IntegerType(), idx, X.valid, checks=list(X.checks))


@param_accessors
class KMeansModel(_KMeansParams):
    uid_prefix = "kmeans"

    def __init__(self, uid: Optional[str], centers):
        super().__init__(uid)
        self._centers = np.array(centers, dtype=np.float64)
        self._summary = None

    def clusterCenters(self):
        return [c.copy() for c in self._centers]

    def predict(self, features) -> int:
        v = features.toArray() if isinstance(features, DenseVector) else np.asarray(features, dtype=np.float64)
        return _JavaInt(int(np.argmin(((self._centers - v[None, :]) ** 2).sum(axis=1))))

    @property
    def hasSummary(self):
        return self._summary is not None

    @property
    def summary(self) -> "KMeansSummary":
        if self._summary is None:
            raise RuntimeError(f"No training summary available for this {type(self).__name__}")
        return self._summary

    def transform(self, df: DataFrame) -> DataFrame:
        fc, pc = self.getOrDefault("featuresCol"), self.getOrDefault("predictionCol")
        ColRef(fc).data_type(df.schema)
        exprs = [ColRef(n) for n in df.columns if n != pc] + [Alias(KMeansPredictExpr(fc, self._centers), pc)]
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    def computeCost(self, df: DataFrame) -> float:
        """Sum of squared distances of the rows to their nearest centre, over the ranks."""
        from ..parallel import comm

        _, Xv, sel = _features(self, df)
        _, cost = K.assign(Xv, sel, self._centers)
        return _JavaFloat(float(comm.all_reduce_sum(cost.sum().reshape(1)).cpu()[0]))

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
        return f"KMeansModel: uid={self.uid}, k={self._centers.shape[0]}, numFeatures={self._centers.shape[1]}"


class KMeansSummary:
    """Spark 2.4's ``KMeansSummary``; the predictions and sizes are computed at first read."""

    def __init__(self, model: KMeansModel, df: DataFrame, res: "K.KMeansResult"):
        self._model, self._df, self._res = model, df, res
        self._pred = self._sizes = None

    def __call__(self):  # Java spelling: model.summary()
        return self

    @property
    def k(self):
        return _JavaInt(self._model._centers.shape[0])

    @property
    def predictionCol(self):
        return self._model.getOrDefault("predictionCol")

    @property
    def featuresCol(self):
        return self._model.getOrDefault("featuresCol")

    @property
    def predictions(self) -> DataFrame:
        if self._pred is None:
            self._pred = self._model.transform(self._df)
        return self._pred

    @property
    def cluster(self) -> DataFrame:
        return self.predictions.select(self.predictionCol)

    @property
    def clusterSizes(self):
        if self._sizes is None:
            from ..parallel import comm

            _, Xv, sel = _features(self._model, self._df)
            idx, _ = K.assign(Xv, sel, self._model._centers)
            cnt = torch.bincount(idx[idx >= 0].to(torch.long), minlength=int(self.k)).to(torch.float64)
            self._sizes = [int(v) for v in comm.all_reduce_sum(cnt).cpu().tolist()]
        return list(self._sizes)

    @property
    def trainingCost(self):
        """The cost of the last iteration's assignment (against the centres it started from)."""
        return _JavaFloat(self._res.cost)

    @property
    def numIter(self):
        return _JavaInt(self._res.iterations)

    @property
    def route(self) -> str:
        """Which route of ``ops/kmeans.py`` ran the iterations (engine diagnostic, not Spark's)."""
        return self._res.route


# ------------------------------------------------------------------------------------------
# GaussianMixture (Spark 2.4 semantics)
# ------------------------------------------------------------------------------------------
# The EM pass, the start and the routes are ``ops/gmm.py``'s: on the device, for dense f32 / f64
# features with d <= 32 and k <= 16 (k <= 8 beyond d = 16), one iteration is one launch of
# ``csrc/hip/gmm.hip`` and the host closes it with the M-step; wider inputs take the torch composite
# and the CPU engine the fp64 twin.  The start uses the project's own seeded rule, so it agrees with
# Spark's in distribution, not bit for bit.
#
# Not implemented, each raising an error that says so: persistence of the fitted model,
# ``weightCol`` (a Spark 3 feature), sparse vectors.
def _gmm_not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"GaussianMixture: {what} is not implemented")


class _GaussianMixtureParams(Params):
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "probabilityCol": Param("probabilityCol", "Column name for predicted class conditional probabilities.",
                                "probability"),
        "k": Param("k", "Number of independent Gaussians in the mixture model. Must be > 1.", 2, lambda v: v > 1,
                   converter=int),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 100, lambda v: v >= 0, converter=int),
        "tol": Param("tol", "the convergence tolerance for iterative algorithms (>= 0)", 0.01, lambda v: v >= 0,
                     converter=float),
        "seed": Param("seed", "random seed", 538009335, converter=int),
    }

    def set(self, name, value):
        if name == "weightCol":
            raise _gmm_not_implemented("weightCol (a Spark 3 feature)")
        return super().set(name, value)

    _set = set

    def setWeightCol(self, v):
        return self.set("weightCol", v)


def _dense_array(features) -> np.ndarray:
    if isinstance(features, SparseVector):
        raise _gmm_not_implemented("sparse feature vectors")
    return features.toArray() if isinstance(features, DenseVector) else np.asarray(features, dtype=np.float64)


class MultivariateGaussian:
    """One Gaussian of a fitted mixture, evaluated by ``ops/gmm.gaussian_params``."""

    def __init__(self, mean: np.ndarray, cov: np.ndarray):
        self._mean, self._cov = np.array(mean, dtype=np.float64), np.array(cov, dtype=np.float64)
        self._W, self._u = G.gaussian_params(self._mean, self._cov)

    @property
    def mean(self) -> DenseVector:
        return DenseVector(self._mean)

    @property
    def cov(self) -> DenseMatrix:
        d = self._mean.size
        return DenseMatrix(d, d, self._cov.reshape(-1), True)

    def logpdf(self, x) -> float:
        z = self._W @ (_dense_array(x) - self._mean)
        return _JavaFloat(self._u - 0.5 * float(z @ z))

    def pdf(self, x) -> float:
        return _JavaFloat(float(np.exp(self.logpdf(x))))


@param_accessors
class GaussianMixture(_GaussianMixtureParams):
    uid_prefix = "GaussianMixture"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k == "weightCol":
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "GaussianMixtureModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.clustering.GaussianMixture")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "GaussianMixtureModel":
        tbl, Xv, sel = _features(self, df)
        with tracing.span("gmm"):
            res = G.fit(Xv, sel, self.getOrDefault("k"), self.getOrDefault("maxIter"), self.getOrDefault("tol"),
                        self.getOrDefault("seed"))
        tracing.add_rows("gmm", tbl.nrows)
        model = GaussianMixtureModel(self.uid, res.weights, res.means, res.covs)
        self.copyValues(model)
        model._summary, model._session = GaussianMixtureSummary(model, df, res), df.sparkSession
        return model


class _AssignPass:
    """One ASSIGN pass per table, shared by the two output columns of a transform."""

    def __init__(self, features: str, model: "GaussianMixtureModel"):
        self.features, self.model = features, model
        self._table = self._out = None

    def of(self, table):
        if self._table is not table:
            X = table.column(self.features)
            m = self.model
            with tracing.span("gmm_predict"):
                idx, prob, _ = G.assign(_dense_features(X), X.valid, m._weights, m._means, m._covs)
            self._out, self._table = (idx, prob, X), table
        return self._out


class GaussianMixturePredictExpr(Expr):
    """Column ``which`` (0 prediction, 1 probability) of a mixture's ASSIGN pass."""

    def __init__(self, run: _AssignPass, which: int):
        self.run, self.which = run, which

    def children(self):
        return [ColRef(self.run.features)]

    def data_type(self, schema):
        return VectorUDT() if self.which else IntegerType()

    def sql_name(self):
        return ("prediction", "probability")[self.which]

    def eval(self, ctx: EvalContext) -> ColumnData:
        out = self.run.of(ctx.table)
        X = out[2]
        return ColumnData(self.data_type(None), out[self.which], X.valid, checks=list(X.checks))


@param_accessors
class GaussianMixtureModel(_GaussianMixtureParams):
    uid_prefix = "GaussianMixture"

    def __init__(self, uid: Optional[str], weights, means, covs):
        super().__init__(uid)
        self._weights = np.array(weights, dtype=np.float64)
        self._means, self._covs = np.array(means, dtype=np.float64), np.array(covs, dtype=np.float64)
        self._summary = self._session = None

    @property
    def weights(self):
        return [float(w) for w in self._weights]

    @property
    def gaussians(self):
        return [MultivariateGaussian(m, c) for m, c in zip(self._means, self._covs)]

    @property
    def gaussiansDF(self) -> DataFrame:
        """One row per Gaussian: ``mean`` (vector) and ``cov`` -- the engine has no matrix column
        type, so the covariance is the vector of its d x d entries, row-major."""
        if self._session is None:
            raise RuntimeError("gaussiansDF needs the session of the fit: this model was not fitted")
        return self._session.createDataFrame([(DenseVector(m), DenseVector(c.reshape(-1)))
                                        for m, c in zip(self._means, self._covs)], ["mean", "cov"])

    def _local(self, features):
        x = _dense_array(features).reshape(-1, 1)
        return G.em_pass_host(x, None, self._weights, self._means, self._covs, G.ASSIGN)

    def predict(self, features) -> int:
        return _JavaInt(int(self._local(features)[0][0]))

    def predictProbability(self, features) -> DenseVector:
        return DenseVector(self._local(features)[1][:, 0].numpy())

    @property
    def hasSummary(self):
        return self._summary is not None

    @property
    def summary(self) -> "GaussianMixtureSummary":
        if self._summary is None:
            raise RuntimeError(f"No training summary available for this {type(self).__name__}")
        return self._summary

    def transform(self, df: DataFrame) -> DataFrame:
        g = self.getOrDefault
        ColRef(g("featuresCol")).data_type(df.schema)
        run = _AssignPass(g("featuresCol"), self)
        names = [g("predictionCol"), g("probabilityCol")]
        new = [Alias(GaussianMixturePredictExpr(run, i), n) for i, n in enumerate(names) if n]
        exprs = [ColRef(n) for n in df.columns if n not in names] + new
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    # persistence: out of scope ---------------------------------------------------------------
    def write(self):
        raise _gmm_not_implemented("persistence of the fitted model")

    def save(self, path):
        self.write()

    @classmethod
    def read(cls):
        raise _gmm_not_implemented("persistence of the fitted model")

    @classmethod
    def load(cls, path):
        cls.read()

    def __repr__(self):
        return f"GaussianMixtureModel: uid={self.uid}, k={self._weights.size}, numFeatures={self._means.shape[1]}"


class GaussianMixtureSummary:
    """Spark 2.4's ``GaussianMixtureSummary``; the predictions and sizes are computed at first read."""

    def __init__(self, model: GaussianMixtureModel, df: DataFrame, res: "G.GmmResult"):
        self._model, self._df, self._res = model, df, res
        self._pred = self._sizes = None

    def __call__(self):  # Java spelling: model.summary()
        return self

    @property
    def k(self):
        return _JavaInt(self._model._weights.size)

    @property
    def predictionCol(self):
        return self._model.getOrDefault("predictionCol")

    @property
    def probabilityCol(self):
        return self._model.getOrDefault("probabilityCol")

    @property
    def featuresCol(self):
        return self._model.getOrDefault("featuresCol")

    @property
    def predictions(self) -> DataFrame:
        if self._pred is None:
            self._pred = self._model.transform(self._df)
        return self._pred

    @property
    def cluster(self) -> DataFrame:
        return self.predictions.select(self.predictionCol)

    @property
    def probability(self) -> DataFrame:
        return self.predictions.select(self.probabilityCol)

    @property
    def clusterSizes(self):
        if self._sizes is None:
            from ..parallel import comm

            m = self._model
            _, Xv, sel = _features(m, self._df)
            idx, _, _ = G.assign(Xv, sel, m._weights, m._means, m._covs)
            cnt = torch.bincount(idx[idx >= 0].to(torch.long), minlength=int(self.k)).to(torch.float64)
            self._sizes = [int(v) for v in comm.all_reduce_sum(cnt).cpu().tolist()]
        return list(self._sizes)

    @property
    def logLikelihood(self):
        """The log-likelihood of the last iteration's E-step (against the parameters it started from)."""
        return _JavaFloat(self._res.log_likelihood)

    @property
    def numIter(self):
        return _JavaInt(self._res.iterations)

    @property
    def route(self) -> str:
        """Which route of ``ops/gmm.py`` ran the iterations (engine diagnostic, not Spark's)."""
        return self._res.route
