"""``org.apache.spark.ml.regression.RandomForestRegressor`` and
``org.apache.spark.ml.classification.RandomForestClassifier`` (Spark 2.4 semantics, continuous
features).

The bag rule, the per-node feature subsets, the level passes and the fit are ``ops/forest.py``'s: on
the device one histogram launch per slot group serves the open nodes of all trees
(``csrc/hip/forest.hip``), with one host read of the node records per level; the CPU engine runs the
twins and grows the same forest node for node.  ``transform`` walks every tree over the raw features
in one pass (``forest_predict_kernel``): ``prediction`` is the mean of the trees' leaf means, or the
first maximal class of ``rawPrediction`` = the sum over the trees of each leaf's class
probabilities, with ``probability`` = raw / sum raw.

Not implemented, each raising an error that says so: ``thresholds``, ``varianceCol``, ``weightCol``,
categorical features, sparse vectors, persistence of the fitted model.  ``maxMemoryInMB``,
``cacheNodeIds`` and ``checkpointInterval`` are accepted and ignored.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from ..ops import forest as F, tree as T
from ..sql.dataframe import DataFrame
from ..sql.expressions import Alias, ColRef
from ..sql.plan import Project
from ..utils import tracing
from .glm import _dense_features
from .linalg import DenseVector, SparseVector
from .param import Param, param_accessors
from .regression import _JavaFloat, _JavaInt
from .tree import (_CLS_PARAMS, _REG_PARAMS, DecisionTreeClassificationModel, DecisionTreeRegressionModel, TreePredictExpr,
                   _operands, _TreeEstimator, _TreeModel)

__all__ = ["RandomForestRegressor", "RandomForestRegressionModel", "RandomForestClassifier",
           "RandomForestClassificationModel"]

_FOREST_PARAMS = {
    "numTrees": Param("numTrees", "Number of trees to train (>= 1).", 20, lambda v: v >= 1, converter=int),
    "featureSubsetStrategy": Param("featureSubsetStrategy", "The number of features to consider for splits at each tree "
                                   "node. Supported options: auto, all, onethird, sqrt, log2, (0.0-1.0], [1-n].", "auto",
                                   lambda v: F.features_per_node(v, 1 << 20, T.REG, 2) >= 1, converter=str),
    "subsamplingRate": Param("subsamplingRate", "Fraction of the training data used for learning each decision tree, in "
                             "range (0, 1].", 1.0, lambda v: 0.0 < v <= 1.0, converter=float),
}


class _ForestEstimator(_TreeEstimator):
    def _train(self, df: DataFrame):
        tbl, Xv, y, sel = _operands(self, df)
        g = self.getOrDefault
        with tracing.span("forest"):
            res = F.fit(Xv, y, sel, self._kind, T.IMPURITIES[g("impurity")], g("numTrees"), g("featureSubsetStrategy"),
                        g("subsamplingRate"), g("maxDepth"), g("maxBins"), g("minInstancesPerNode"), g("minInfoGain"),
                        g("seed"))
        tracing.add_rows("forest", tbl.nrows)
        model = self._model_class(self.uid, res)
        self.copyValues(model)
        return model


class _ForestWalk:
    """One walk of all trees per table, shared by the output columns of a transform."""

    def __init__(self, features: str, kind: int, count: int, tabs):
        self.features, self.kind, self.count, self.tabs = features, kind, count, tabs
        self._table = self._out = None

    def of(self, table):
        if self._table is not table:
            X = table.column(self.features)
            with tracing.span("forest_predict"):
                raw = F.predict(_dense_features(X), X.valid, self.tabs)  # [C, n]
                if self.kind == T.CLS:
                    prob = raw / raw.sum(dim=0, keepdim=True)
                    # the first maximum (dead rows hold NaN: any index)
                    pred = torch.argmax(torch.nan_to_num(raw, nan=0.0), dim=0).to(torch.float64)
                else:
                    raw, prob, pred = None, None, raw[0] / float(self.count)
            self._out, self._table = (raw, prob, pred, X), table
        return self._out


class _ForestModel(_TreeModel):
    _tree_model = None

    def __init__(self, uid: Optional[str], trees: List["T.TreeResult"]):
        super().__init__(uid, trees[0])
        self._trees = list(trees)
        self._tabs = F.tables(self._trees)

    @property
    def trees(self):
        return [self.copyValues(self._tree_model(None, t)) for t in self._trees]

    @property
    def treeWeights(self):
        return [1.0] * len(self._trees)

    @property
    def getNumTrees(self):
        return _JavaInt(len(self._trees))

    @property
    def totalNumNodes(self):
        return _JavaInt(sum(t.feature.size for t in self._trees))

    @property
    def numNodes(self):
        raise AttributeError(f"{type(self).__name__} has totalNumNodes; numNodes and depth belong to each of its trees")

    depth = numNodes

    @property
    def featureImportances(self):
        """Each tree's importances (gain x node count per feature, normalised), summed and normalised."""
        total = np.zeros(int(self.numFeatures))
        for m in self.trees:
            total += m.featureImportances.toArray()
        return DenseVector(total / total.sum() if total.sum() > 0 else total)

    def _raw(self, features) -> np.ndarray:
        if isinstance(features, SparseVector):
            raise self._not_implemented("sparse feature vectors")
        v = features.toArray() if isinstance(features, DenseVector) else np.asarray(features, dtype=np.float64)
        return F.predict(torch.from_numpy(np.array(v, dtype=np.float64).reshape(-1, 1)), None, self._tabs)[:, 0].numpy()

    def predict(self, features) -> float:
        raw = self._raw(features)
        return _JavaFloat(float(np.argmax(raw)) if self._tree.kind == T.CLS else float(raw[0] / len(self._trees)))

    @property
    def toDebugString(self) -> str:
        lines = [repr(self)]
        for k, m in enumerate(self.trees):
            lines.append(f"  Tree {k} (weight 1.0):")
            lines += ["  " + s for s in m.toDebugString.splitlines()[1:]]
        return "\n".join(lines) + "\n"

    def transform(self, df: DataFrame) -> DataFrame:
        fc = self.getOrDefault("featuresCol")
        ColRef(fc).data_type(df.schema)
        run = _ForestWalk(fc, self._tree.kind, len(self._trees), self._tabs)
        cols = [(w, n) for w, n in self._columns() if n]
        names = [n for _, n in cols]
        exprs = [ColRef(n) for n in df.columns if n not in names] + [Alias(TreePredictExpr(run, w), n) for w, n in cols]
        return DataFrame(Project(df._plan, exprs), df.sparkSession)

    def __repr__(self):
        return f"{type(self).__name__} (uid={self.uid}) with {len(self._trees)} trees"


@param_accessors
class RandomForestRegressionModel(_ForestModel):
    uid_prefix, _who, _params = "rfr", "RandomForestRegressor", {**_REG_PARAMS, **_FOREST_PARAMS}
    _tree_model = DecisionTreeRegressionModel


@param_accessors
class RandomForestRegressor(_ForestEstimator):
    uid_prefix, _who, _params = "rfr", "RandomForestRegressor", {**_REG_PARAMS, **_FOREST_PARAMS}
    _kind, _spark_class = T.REG, "org.apache.spark.ml.regression.RandomForestRegressor"
    _model_class = RandomForestRegressionModel


@param_accessors
class RandomForestClassificationModel(_ForestModel):
    uid_prefix, _who, _params = "rfc", "RandomForestClassifier", {**_CLS_PARAMS, **_FOREST_PARAMS}
    _tree_model = DecisionTreeClassificationModel

    @property
    def numClasses(self):
        return _JavaInt(self._tree.num_classes)

    def predictRaw(self, features):
        return DenseVector(self._raw(features))

    def predictProbability(self, features):
        raw = self._raw(features)
        return DenseVector(raw / raw.sum())

    def _columns(self):
        g = self.getOrDefault
        return [(0, g("rawPredictionCol")), (1, g("probabilityCol")), (2, g("predictionCol"))]


@param_accessors
class RandomForestClassifier(_ForestEstimator):
    uid_prefix, _who, _params = "rfc", "RandomForestClassifier", {**_CLS_PARAMS, **_FOREST_PARAMS}
    _kind, _spark_class = T.CLS, "org.apache.spark.ml.classification.RandomForestClassifier"
    _model_class = RandomForestClassificationModel
