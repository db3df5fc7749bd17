"""``org.apache.spark.ml.classification.LogisticRegression`` and ``MultilayerPerceptronClassifier``
(Spark 2.4 semantics).

The loss / gradient evaluations, the routes and the fit are ``ops/logreg.py``'s: on the device, for
dense f32 / f64 features with d <= 64 and at most 64 classes, one evaluation is one launch of
``csrc/hip/logreg.hip`` under Breeze's L-BFGS / OWLQN (``qn_device.minimize``); wider inputs take the
torch composite and the CPU engine the fp64 twin.  ``transform`` adds ``rawPrediction``,
``probability`` and ``prediction`` from one PREDICT pass.

Not implemented, each raising an error that says so: ``thresholds``, bound constraints
(``lowerBoundsOnCoefficients`` ...), persistence of the fitted model, the binary summary's ROC / PR
curves and ``areaUnderROC``, sparse vectors in the local ``predict*`` methods (vector columns are
dense).  ``aggregationDepth`` is accepted and ignored.

``MultilayerPerceptronClassifier``: the evaluations, the routes and the fit are ``ops/mlp.py``'s: on
the device, for one or two hidden layers with d <= 64 and widths and classes <= 32, one evaluation
is one launch of ``csrc/hip/mlp.hip`` under Breeze's L-BFGS; other shapes take the torch composite
and the CPU engine the fp64 twin.  Not implemented, each raising an error that says so:
``solver="gd"``, sparse vectors, persistence of the fitted model, ``rawPredictionCol`` and
``probabilityCol`` (Spark 3's).  ``blockSize`` is accepted and ignored: the objective is the plain
mean over the live rows, Spark's value whenever every block is full.  ``stepSize`` belongs to ``gd``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ops import logreg as L
from ..ops import mlp as M
from ..sql.dataframe import DataFrame
from ..sql.expressions import Alias, ColRef, EvalContext, Expr
from ..sql.plan import Project
from ..sql.table import ColumnData
from ..sql.types import DoubleType, VectorUDT
from ..utils import tracing
from .glm import _dense_features, _rows
from .linalg import DenseMatrix, DenseVector, SparseVector
from .param import Param, Params, param_accessors
from .regression import _JavaFloat, _JavaInt

__all__ = ["LogisticRegression", "LogisticRegressionModel", "LogisticRegressionTrainingSummary",
           "MultilayerPerceptronClassifier", "MultilayerPerceptronClassificationModel"]

_OUT_OF_SCOPE_PARAMS = ("thresholds", "lowerBoundsOnCoefficients", "upperBoundsOnCoefficients",
                        "lowerBoundsOnIntercepts", "upperBoundsOnIntercepts")


def _not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"LogisticRegression: {what} is not implemented")


class _LRParams(Params):
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "labelCol": Param("labelCol", "label column name", "label"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "probabilityCol": Param("probabilityCol", "Column name for predicted class conditional probabilities.",
                                "probability"),
        "rawPredictionCol": Param("rawPredictionCol", "raw prediction (a.k.a. confidence) column name", "rawPrediction"),
        "weightCol": Param("weightCol", "weight column name. If this is not set or empty, we treat all instance "
                                        "weights as 1.0", None),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 100, lambda v: v >= 0, converter=int),
        "regParam": Param("regParam", "regularization parameter (>= 0)", 0.0, lambda v: v >= 0, converter=float),
        "elasticNetParam": Param("elasticNetParam", "the ElasticNet mixing parameter, in range [0, 1]", 0.0,
                                 lambda v: 0 <= v <= 1, converter=float),
        "tol": Param("tol", "the convergence tolerance for iterative algorithms (>= 0)", 1e-6, lambda v: v >= 0,
                     converter=float),
        "fitIntercept": Param("fitIntercept", "whether to fit an intercept term", True, converter=bool),
        "standardization": Param("standardization", "whether to standardize the training features before fitting "
                                                    "the model", True, converter=bool),
        "threshold": Param("threshold", "threshold in binary classification prediction, in range [0, 1]", 0.5,
                           lambda v: 0 <= v <= 1, converter=float),
        "family": Param("family", "The name of family which is a description of the label distribution to be used "
                                  "in the model. Supported options: auto, binomial, multinomial.", "auto",
                        lambda v: v in ("auto", "binomial", "multinomial")),
        "aggregationDepth": Param("aggregationDepth", "suggested depth for treeAggregate (>= 2); ignored", 2,
                                  lambda v: v >= 2, converter=int),
    }

    def set(self, name, value):
        if name in _OUT_OF_SCOPE_PARAMS:
            raise _not_implemented(name)
        return super().set(name, value)

    _set = set


for _name in _OUT_OF_SCOPE_PARAMS:  # setThresholds(...) etc. exist and say what they are
    setattr(_LRParams, "set" + _name[0].upper() + _name[1:], (lambda n: lambda self, v: self.set(n, v))(_name))


def _operands(params, df: DataFrame, need_label: bool):
    """(table, dense feature-major features, label | None, weight | None, selection)."""
    fc = params.getOrDefault("featuresCol")
    ColRef(fc).data_type(df.schema)
    tbl = df._table()
    X = tbl.column(fc)
    y = w = None
    sel = tbl.sel
    if need_label:
        y, w, sel = _rows(params, tbl, tbl.column(params.getOrDefault("labelCol")))
    if X.valid is not None:
        sel = X.valid if sel is None else (sel & X.valid)
    return tbl, _dense_features(X), y, w, sel


@param_accessors
class LogisticRegression(_LRParams):
    uid_prefix = "logreg"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k in _OUT_OF_SCOPE_PARAMS:
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "LogisticRegressionModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.classification.LogisticRegression")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "LogisticRegressionModel":
        tbl, Xv, y, w, sel = _operands(self, df, True)
        g = self.getOrDefault
        with tracing.span("logreg"):
            res = L.fit(Xv, y, w, sel, g("family"), g("regParam"), g("elasticNetParam"), g("maxIter"), g("tol"),
                        g("fitIntercept"), g("standardization"))
        tracing.add_rows("logreg", tbl.nrows)
        model = LogisticRegressionModel(self.uid, res.coef, res.intercept, res.num_classes)
        self.copyValues(model)
        model._summary = LogisticRegressionTrainingSummary(model, df, res)
        return model


class _PredictPass:
    """One PREDICT pass per table, shared by the three output columns of a transform."""

    def __init__(self, features: str, coef: np.ndarray, threshold: float):
        self.features, self.coef, self.threshold = features, coef, threshold
        self._table = self._out = None

    def of(self, table):
        if self._table is not table:
            X = table.column(self.features)
            with tracing.span("logreg_predict"):
                self._out = L.predict(_dense_features(X), X.valid, self.coef, self.threshold) + (X,)
            self._table = table
        return self._out


class LogregPredictExpr(Expr):
    """Column ``which`` (0 raw, 1 probability, 2 prediction) of a model's PREDICT pass."""

    def __init__(self, run: _PredictPass, which: int):
        self.run, self.which = run, which

    def children(self):
        return [ColRef(self.run.features)]

    def data_type(self, schema):
        return DoubleType() if self.which == 2 else VectorUDT()

    def sql_name(self):
        return ("rawPrediction", "probability", "prediction")[self.which]

    def eval(self, ctx: EvalContext) -> ColumnData:
        out = self.run.of(ctx.table)
        X = out[3]
        return ColumnData(self.data_type(None), out[self.which], X.valid, checks=list(X.checks))


@param_accessors
class LogisticRegressionModel(_LRParams):
    uid_prefix = "logreg"

    def __init__(self, uid: Optional[str], coef, intercept, num_classes: int):
        super().__init__(uid)
        self._coef = np.array(coef, dtype=np.float64).reshape(len(intercept), -1)  # [K, d]; K = 1: binomial
        self._icpt = np.array(intercept, dtype=np.float64)
        self._classes = int(num_classes)
        self._summary = None

    @property
    def _multinomial(self) -> bool:
        return self._coef.shape[0] > 1

    def _packed(self) -> np.ndarray:
        return np.concatenate([self._coef, self._icpt[:, None]], axis=1)

    @property
    def coefficients(self):
        if self._multinomial:
            raise RuntimeError("Multinomial models contain a matrix of coefficients, use coefficientMatrix instead.")
        return DenseVector(self._coef[0])

    @property
    def intercept(self):
        if self._multinomial:
            raise RuntimeError("Multinomial models contain a vector of intercepts, use interceptVector instead.")
        return _JavaFloat(self._icpt[0])

    @property
    def coefficientMatrix(self):
        K, d = self._coef.shape
        return DenseMatrix(K, d, self._coef.reshape(-1), True)

    @property
    def interceptVector(self):
        return DenseVector(self._icpt)

    @property
    def numClasses(self):
        return _JavaInt(self._classes)

    @property
    def numFeatures(self):
        return _JavaInt(self._coef.shape[1])

    def _local(self, features):
        if isinstance(features, SparseVector):
            raise _not_implemented("sparse feature vectors")
        v = features.toArray() if isinstance(features, DenseVector) else np.asarray(features, dtype=np.float64)
        return L.logreg_pass_host(v.reshape(-1, 1), None, None, None, self._packed(), L.PREDICT,
                                  self.getOrDefault("threshold"))

    def predictRaw(self, features):
        return DenseVector(self._local(features)[0][:, 0].numpy())

    def predictProbability(self, features):
        return DenseVector(self._local(features)[1][:, 0].numpy())

    def predict(self, features) -> float:
        return _JavaFloat(float(self._local(features)[2][0]))

    @property
    def hasSummary(self):
        return self._summary is not None

    @property
    def summary(self) -> "LogisticRegressionTrainingSummary":
        if self._summary is None:
            raise RuntimeError(f"No training summary available for this {type(self).__name__}")
        return self._summary

    def transform(self, df: DataFrame) -> DataFrame:
        g = self.getOrDefault
        ColRef(g("featuresCol")).data_type(df.schema)
        run = _PredictPass(g("featuresCol"), self._packed(), g("threshold"))
        names = [g("rawPredictionCol"), g("probabilityCol"), g("predictionCol")]
        new = [Alias(LogregPredictExpr(run, i), n) for i, n in enumerate(names) if n]
        exprs = [ColRef(n) for n in df.columns if n not in names] + new
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    def evaluate(self, df: DataFrame) -> "LogisticRegressionSummary":
        return LogisticRegressionSummary(self, df)

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
        return f"LogisticRegressionModel: uid = {self.uid}, numClasses = {self._classes}, numFeatures = {self._coef.shape[1]}"


class LogisticRegressionSummary:
    """Spark 2.4's ``LogisticRegressionSummary``; the predictions are computed at first read."""

    def __init__(self, model: LogisticRegressionModel, df: DataFrame):
        self._model, self._df = model, df
        self._pred = None

    def __call__(self):  # Java spelling: model.summary()
        return self

    @property
    def predictions(self) -> DataFrame:
        if self._pred is None:
            self._pred = self._model.transform(self._df)
        return self._pred

    @property
    def labelCol(self):
        return self._model.getOrDefault("labelCol")

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
    def labels(self):
        return [float(c) for c in range(int(self._model.numClasses))]

    def _metric(self, name: str) -> float:
        from .evaluation import MulticlassClassificationEvaluator

        ev = MulticlassClassificationEvaluator(predictionCol=self.predictionCol, labelCol=self.labelCol, metricName=name)
        return _JavaFloat(ev.evaluate(self.predictions))

    @property
    def accuracy(self):
        return self._metric("accuracy")

    @property
    def weightedPrecision(self):
        return self._metric("weightedPrecision")

    @property
    def weightedRecall(self):
        return self._metric("weightedRecall")

    @property
    def weightedFMeasure(self):
        return self._metric("f1")

    def _binary_curves(self, *_):
        raise _not_implemented("the binary summary's ROC / PR curves and areaUnderROC")

    roc = pr = areaUnderROC = fMeasureByThreshold = precisionByThreshold = recallByThreshold = property(_binary_curves)


class LogisticRegressionTrainingSummary(LogisticRegressionSummary):
    def __init__(self, model: LogisticRegressionModel, df: DataFrame, res: "L.LogregResult"):
        super().__init__(model, df)
        self._res = res

    @property
    def objectiveHistory(self):
        return list(self._res.objective_history)

    @property
    def totalIterations(self):
        return _JavaInt(len(self._res.objective_history))

    @property
    def route(self) -> str:
        """Which route of ``ops/logreg.py`` ran the evaluations (engine diagnostic, not Spark's)."""
        return self._res.route


# ---- MultilayerPerceptronClassifier ------------------------------------------------------------------
_MLP_OUT_OF_SCOPE_PARAMS = ("rawPredictionCol", "probabilityCol")


def _mlp_not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"MultilayerPerceptronClassifier: {what} is not implemented")


def _mlp_layers(v) -> list:
    return [int(x) for x in v]


def _mlp_vector(v) -> np.ndarray:
    if isinstance(v, SparseVector):
        raise _mlp_not_implemented("sparse vectors")
    return np.array(v.toArray() if isinstance(v, DenseVector) else v, dtype=np.float64).reshape(-1)


class _MLPParams(Params):
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "labelCol": Param("labelCol", "label column name", "label"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "layers": Param("layers", "Sizes of layers from input layer to output layer. E.g., Array(780, 100, 10) means "
                                  "780 inputs, one hidden layer with 100 neurons and output layer of 10 neurons.", None,
                        lambda v: len(v) >= 2 and all(x > 0 for x in v), converter=_mlp_layers),
        "blockSize": Param("blockSize", "Block size for stacking input data in matrices; accepted and ignored", 128,
                           lambda v: v > 0, converter=int),
        "solver": Param("solver", "The solver algorithm for optimization. Supported options: l-bfgs, gd.", "l-bfgs",
                        lambda v: v in ("l-bfgs", "gd")),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 100, lambda v: v >= 0, converter=int),
        "tol": Param("tol", "the convergence tolerance for iterative algorithms (>= 0)", 1e-6, lambda v: v >= 0,
                     converter=float),
        "seed": Param("seed", "random seed", -763139545, converter=int),
        "stepSize": Param("stepSize", "Step size to be used for each iteration of optimization (> 0); solver gd only", 0.03,
                          lambda v: v > 0, converter=float),
        "initialWeights": Param("initialWeights", "The initial weights of the model", None, converter=_mlp_vector),
    }

    def set(self, name, value):
        if name in _MLP_OUT_OF_SCOPE_PARAMS:
            raise _mlp_not_implemented(name)
        return super().set(name, value)

    _set = set


for _name in _MLP_OUT_OF_SCOPE_PARAMS:
    setattr(_MLPParams, "set" + _name[0].upper() + _name[1:], (lambda n: lambda self, v: self.set(n, v))(_name))


@param_accessors
class MultilayerPerceptronClassifier(_MLPParams):
    uid_prefix = "mlpc"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k in _MLP_OUT_OF_SCOPE_PARAMS:
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "MultilayerPerceptronClassificationModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.classification.MultilayerPerceptronClassifier")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "MultilayerPerceptronClassificationModel":
        g = self.getOrDefault
        layers, init = g("layers"), g("initialWeights")
        if layers is None:
            raise ValueError("MultilayerPerceptronClassifier: layers must be set")
        if g("solver") == "gd":
            raise _mlp_not_implemented('solver="gd"')
        if init is not None and init.size != M.weight_count(layers):
            raise ValueError(f"MultilayerPerceptronClassifier: initialWeights must have length {M.weight_count(layers)} "
                             f"for layers {layers}, found {init.size}")
        tbl, Xv, y, _, sel = _operands(self, df, True)
        with tracing.span("mlp"):
            res = M.fit(Xv, y, sel, layers, g("maxIter"), g("tol"), g("seed"), init)
        tracing.add_rows("mlp", tbl.nrows)
        model = MultilayerPerceptronClassificationModel(self.uid, layers, res.weights)
        self.copyValues(model)
        model._route, model._objective_history = res.route, res.objective_history
        return model


class MlpPredictExpr(Expr):
    """The prediction column of a model's PREDICT pass."""

    def __init__(self, features: str, layers: list, weights: np.ndarray):
        self.features, self.layers, self.weights = features, layers, weights

    def children(self):
        return [ColRef(self.features)]

    def data_type(self, schema):
        return DoubleType()

    def sql_name(self):
        return "prediction"

    def eval(self, ctx: EvalContext) -> ColumnData:
        X = ctx.table.column(self.features)
        with tracing.span("mlp_predict"):
            pred = M.predict(_dense_features(X), X.valid, self.weights, self.layers)
        return ColumnData(DoubleType(), pred, X.valid, checks=list(X.checks))


@param_accessors
class MultilayerPerceptronClassificationModel(_MLPParams):
    """A Spark 2.4 ``PredictionModel``: the prediction column only."""
    uid_prefix = "mlpc"

    def __init__(self, uid: Optional[str], layers, weights):
        super().__init__(uid)
        self._layers = _mlp_layers(layers)
        self._weights = _mlp_vector(weights)
        if self._weights.size != M.weight_count(self._layers):
            raise ValueError(f"MultilayerPerceptronClassificationModel: weights must have length "
                             f"{M.weight_count(self._layers)} for layers {self._layers}")
        self._route, self._objective_history = None, []

    @property
    def layers(self):
        return list(self._layers)

    @property
    def weights(self):
        return DenseVector(self._weights)

    @property
    def numFeatures(self):
        return _JavaInt(self._layers[0])

    @property
    def route(self) -> Optional[str]:
        """Which route of ``ops/mlp.py`` ran the fit's evaluations (engine diagnostic, not Spark's)."""
        return self._route

    def predict(self, features) -> float:
        v = _mlp_vector(features)
        return _JavaFloat(float(M.mlp_pass_host(v.reshape(-1, 1), None, None, self._weights, self._layers, M.PREDICT)[0]))

    def transform(self, df: DataFrame) -> DataFrame:
        fc, pc = self.getOrDefault("featuresCol"), self.getOrDefault("predictionCol")
        ColRef(fc).data_type(df.schema)
        exprs = [ColRef(n) for n in df.columns if n != pc] + [Alias(MlpPredictExpr(fc, self._layers, self._weights), pc)]
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    # persistence: out of scope ---------------------------------------------------------------
    def write(self):
        raise _mlp_not_implemented("persistence of the fitted model")

    def save(self, path):
        self.write()

    @classmethod
    def read(cls):
        raise _mlp_not_implemented("persistence of the fitted model")

    @classmethod
    def load(cls, path):
        cls.read()

    def __repr__(self):
        return f"MultilayerPerceptronClassificationModel: uid = {self.uid}, layers = {self._layers}"
