"""``org.apache.spark.ml.regression.DecisionTreeRegressor`` and
``org.apache.spark.ml.classification.DecisionTreeClassifier`` (Spark 2.4 semantics, continuous
features).

The thresholds, the level passes, the routes and the fit are ``ops/tree.py``'s: on the device, for
dense f32 / f64 features with d <= 64, at most 256 bins and 16 classes, a level is one histogram
launch per node group of ``csrc/hip/tree.hip`` plus a split search and a routing pass, with one host
read of the node records per level; other device shapes take the torch composite and the CPU engine
the fp64 twins.  ``transform`` walks the tree over the raw features (``tree_predict_kernel``) and adds
``prediction`` (and, for the classifier, ``rawPrediction`` = the leaf's class counts and
``probability`` = counts / n).

Not implemented, each raising an error that says so: ``thresholds``, ``varianceCol``, ``weightCol``,
categorical features, sparse vectors, persistence of the fitted model.  ``maxMemoryInMB``,
``cacheNodeIds`` and ``checkpointInterval`` are accepted and ignored.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ops import tree as T
from ..sql.dataframe import DataFrame
from ..sql.expressions import Alias, ColRef, EvalContext, Expr
from ..sql.plan import Project
from ..sql.table import ColumnData
from ..sql.types import DoubleType, VectorUDT
from ..utils import tracing
from .glm import _dense_features
from .linalg import DenseVector, SparseVector
from .param import Param, Params, param_accessors
from .regression import _JavaFloat, _JavaInt

__all__ = ["DecisionTreeRegressor", "DecisionTreeRegressionModel", "DecisionTreeClassifier",
           "DecisionTreeClassificationModel"]

_OUT_OF_SCOPE_PARAMS = ("thresholds", "varianceCol", "weightCol", "categoricalFeaturesInfo")


class _TreeParams(Params):
    _who = "DecisionTree"
    _params = {
        "featuresCol": Param("featuresCol", "features column name", "features"),
        "labelCol": Param("labelCol", "label column name", "label"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "maxDepth": Param("maxDepth", "Maximum depth of the tree. (>= 0) E.g., depth 0 means 1 leaf node; depth 1 means "
                                      "1 internal node + 2 leaf nodes.", 5, lambda v: 0 <= v <= 30, converter=int),
        "maxBins": Param("maxBins", "Max number of bins for discretizing continuous features. Must be >= 2.", 32,
                         lambda v: v >= 2, converter=int),
        "minInstancesPerNode": Param("minInstancesPerNode", "Minimum number of instances each child must have after "
                                                            "split. Should be >= 1.", 1, lambda v: v >= 1, converter=int),
        "minInfoGain": Param("minInfoGain", "Minimum information gain for a split to be considered at a tree node.", 0.0,
                             lambda v: v >= 0, converter=float),
        "seed": Param("seed", "random seed", 926680331, converter=int),
        "maxMemoryInMB": Param("maxMemoryInMB", "Maximum memory in MB allocated to histogram aggregation; ignored", 256,
                               lambda v: v >= 0, converter=int),
        "cacheNodeIds": Param("cacheNodeIds", "whether to cache node ids; ignored", False, converter=bool),
        "checkpointInterval": Param("checkpointInterval", "checkpoint interval (>= 1) or -1; ignored", 10,
                                    lambda v: v == -1 or v >= 1, converter=int),
    }

    def _not_implemented(self, what: str) -> NotImplementedError:
        return NotImplementedError(f"{self._who}: {what} is not implemented")

    def set(self, name, value):
        if name in _OUT_OF_SCOPE_PARAMS:
            raise self._not_implemented("categorical features" if name == "categoricalFeaturesInfo" else name)
        return super().set(name, value)

    _set = set


for _name in _OUT_OF_SCOPE_PARAMS:  # setThresholds(...) etc. exist and say what they are
    setattr(_TreeParams, "set" + _name[0].upper() + _name[1:], (lambda n: lambda self, v: self.set(n, v))(_name))


def _operands(params, df: DataFrame):
    """(table, dense feature-major features, label, selection with null labels / vectors merged in)."""
    fc, lc = params.getOrDefault("featuresCol"), params.getOrDefault("labelCol")
    ColRef(fc).data_type(df.schema)
    ColRef(lc).data_type(df.schema)
    tbl = df._table()
    X, y = tbl.column(fc), tbl.column(lc)
    sel = tbl.sel
    for v in (X.valid, y.valid):
        if v is not None:
            sel = v if sel is None else (sel & v)
    return tbl, _dense_features(X), y.values, sel


class _TreeEstimator(_TreeParams):
    _kind = T.REG
    _spark_class = ""

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None or k in _OUT_OF_SCOPE_PARAMS:
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None):
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, self._spark_class)

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame):
        tbl, Xv, y, sel = _operands(self, df)
        g = self.getOrDefault
        with tracing.span("tree"):
            res = T.fit(Xv, y, sel, self._kind, T.IMPURITIES[g("impurity")], g("maxDepth"), g("maxBins"),
                        g("minInstancesPerNode"), g("minInfoGain"), g("seed"))
        tracing.add_rows("tree", tbl.nrows)
        model = self._model_class(self.uid, res)
        self.copyValues(model)
        return model


class _LeafWalk:
    """One prediction walk per table, shared by the output columns of a transform."""

    def __init__(self, features: str, tree: "T.TreeResult"):
        self.features, self.tree = features, tree
        self._table = self._out = None

    def of(self, table):
        if self._table is not table:
            X = table.column(self.features)
            with tracing.span("tree_predict"):
                Xv = _dense_features(X)
                leaf = T.predict(Xv, X.valid, self.tree).to(torch.int64).clamp(min=0)
                pred = torch.as_tensor(self.tree.prediction, device=leaf.device)[leaf]
                raw = prob = None
                if self.tree.kind == T.CLS:
                    cc = torch.as_tensor(self.tree.class_counts, dtype=torch.float64, device=leaf.device)
                    raw = cc[leaf].t().contiguous()  # [classes, n], as the vector columns are stored
                    prob = raw / raw.sum(dim=0, keepdim=True)
            self._out, self._table = (raw, prob, pred, X), table
        return self._out


class TreePredictExpr(Expr):
    """Column ``which`` (0 rawPrediction, 1 probability, 2 prediction) of a model's walk."""

    def __init__(self, run: _LeafWalk, which: int):
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


class _TreeModel(_TreeParams):
    def __init__(self, uid: Optional[str], tree: "T.TreeResult"):
        super().__init__(uid)
        self._tree = tree

    @property
    def numNodes(self):
        return _JavaInt(self._tree.feature.size)

    @property
    def depth(self):
        return _JavaInt(self._tree.depth)

    @property
    def numFeatures(self):
        return _JavaInt(self._tree.num_features)

    @property
    def route(self) -> str:
        """Which route of ``ops/tree.py`` ran the fit (engine diagnostic, not Spark's)."""
        return self._tree.route

    @property
    def featureImportances(self):
        """Per feature, the sum of gain x node count over its splits, normalised to 1."""
        t = self._tree
        imp = np.zeros(t.num_features)
        inner = t.feature >= 0
        np.add.at(imp, t.feature[inner], t.gain[inner] * t.count[inner])
        return DenseVector(imp / imp.sum() if imp.sum() > 0 else imp)

    def _leaf(self, features) -> int:
        if isinstance(features, SparseVector):
            raise self._not_implemented("sparse feature vectors")
        v = features.toArray() if isinstance(features, DenseVector) else np.asarray(features, dtype=np.float64)
        return int(T.predict(torch.from_numpy(np.array(v, dtype=np.float64).reshape(-1, 1)), None, self._tree)[0])

    def predict(self, features) -> float:
        return _JavaFloat(float(self._tree.prediction[self._leaf(features)]))

    @property
    def toDebugString(self) -> str:
        t = self._tree
        lines = [f"{type(self).__name__} (uid={self.uid}) of depth {int(self.depth)} with {int(self.numNodes)} nodes"]

        def walk(i: int, indent: int):
            pad = " " * indent
            if t.feature[i] < 0:
                lines.append(f"{pad}Predict: {float(t.prediction[i])!r}")
                return
            lines.append(f"{pad}If (feature {int(t.feature[i])} <= {float(t.threshold[i])!r})")
            walk(int(t.left[i]), indent + 1)
            lines.append(f"{pad}Else (feature {int(t.feature[i])} > {float(t.threshold[i])!r})")
            walk(int(t.right[i]), indent + 1)

        walk(0, 2)
        return "\n".join(lines) + "\n"

    def _columns(self):
        return [(2, self.getOrDefault("predictionCol"))]

    def transform(self, df: DataFrame) -> DataFrame:
        fc = self.getOrDefault("featuresCol")
        ColRef(fc).data_type(df.schema)
        run = _LeafWalk(fc, self._tree)
        cols = [(w, n) for w, n in self._columns() if n]
        names = [n for _, n in cols]
        exprs = [ColRef(n) for n in df.columns if n not in names] + [Alias(TreePredictExpr(run, w), n) for w, n in cols]
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    # persistence: out of scope ---------------------------------------------------------------
    def write(self):
        raise self._not_implemented("persistence of the fitted model")

    def save(self, path):
        self.write()

    @classmethod
    def read(cls):
        raise NotImplementedError(f"{cls._who}: persistence of the fitted model is not implemented")

    @classmethod
    def load(cls, path):
        cls.read()

    def __repr__(self):
        return f"{type(self).__name__} (uid={self.uid}) of depth {int(self.depth)} with {int(self.numNodes)} nodes"


_REG_PARAMS = {"impurity": Param("impurity", "Criterion used for information gain calculation. Supported options: "
                                             "variance", "variance", lambda v: v == "variance")}
_CLS_PARAMS = {
    "impurity": Param("impurity", "Criterion used for information gain calculation. Supported options: entropy, gini",
                      "gini", lambda v: v in ("gini", "entropy")),
    "probabilityCol": Param("probabilityCol", "Column name for predicted class conditional probabilities.", "probability"),
    "rawPredictionCol": Param("rawPredictionCol", "raw prediction (a.k.a. confidence) column name", "rawPrediction"),
}


@param_accessors
class DecisionTreeRegressionModel(_TreeModel):
    uid_prefix, _who, _params = "dtr", "DecisionTreeRegressor", _REG_PARAMS


@param_accessors
class DecisionTreeRegressor(_TreeEstimator):
    uid_prefix, _who, _params = "dtr", "DecisionTreeRegressor", _REG_PARAMS
    _kind, _spark_class = T.REG, "org.apache.spark.ml.regression.DecisionTreeRegressor"
    _model_class = DecisionTreeRegressionModel


@param_accessors
class DecisionTreeClassificationModel(_TreeModel):
    uid_prefix, _who, _params = "dtc", "DecisionTreeClassifier", _CLS_PARAMS

    @property
    def numClasses(self):
        return _JavaInt(self._tree.num_classes)

    def predictRaw(self, features):
        return DenseVector(np.array(self._tree.class_counts[self._leaf(features)], dtype=np.float64))

    def predictProbability(self, features):
        c = np.array(self._tree.class_counts[self._leaf(features)], dtype=np.float64)
        return DenseVector(c / c.sum())

    def _columns(self):
        g = self.getOrDefault
        return [(0, g("rawPredictionCol")), (1, g("probabilityCol")), (2, g("predictionCol"))]


@param_accessors
class DecisionTreeClassifier(_TreeEstimator):
    uid_prefix, _who, _params = "dtc", "DecisionTreeClassifier", _CLS_PARAMS
    _kind, _spark_class = T.CLS, "org.apache.spark.ml.classification.DecisionTreeClassifier"
    _model_class = DecisionTreeClassificationModel
