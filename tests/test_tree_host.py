"""Decision trees on the host: the thresholds against hand-worked cases, the fp64 twins of the level
passes against a plain Python oracle (``fractions.Fraction`` where equality is exact, ``math.fsum`` /
``math.log2`` for entropy), the estimators on the CPU engine and a two-rank (gloo) fit."""
import math
import multiprocessing as mp
import os
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import (DecisionTreeClassificationModel, DecisionTreeClassifier, DecisionTreeRegressor,
                                         VectorAssembler, Vectors)
from net.jgp.labs.sparkdq4ml_amd.models.linalg import SparseVector
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import tree as T


@pytest.mark.parametrize("col,max_bins,want", [
    ([1, 2, 2, 4, 8], 32, [1.5, 3.0, 6.0]),                       # m <= numSplits: every midpoint
    ([5, 5, 5, 5], 32, []),                                       # a constant feature: none
    # counts 6, 1, 1, 2, 2 of values 0..4, three splits wanted: stride 3.  i = 1: prev 6, cur 7, target
    # 3: 3 < 4 cuts at 0.5 (target 6); i = 2: prev 7, cur 8: 1 < 2 cuts at 1.5 (target 9); i = 3: prev 8,
    # cur 10: 1 < 1 fails; i = 4: prev 10, cur 12: 1 < 3 cuts at 3.5
    ([0] * 6 + [1, 2, 3, 3, 4, 4], 4, [0.5, 1.5, 3.5]),
])
def test_find_splits_hand_worked(col, max_bins, want):
    got = T.find_splits(np.array(col, dtype=np.float64)[:, None], max_bins, len(col))
    np.testing.assert_array_equal(got[0], want)


def _oracle_imp(ys, impurity):
    n = len(ys)
    if impurity == T.VARIANCE:
        return (sum(Fraction(v) ** 2 for v in ys) - sum(Fraction(v) for v in ys) ** 2 / n) / n
    cnt = [ys.count(k) for k in sorted(set(ys))]
    if impurity == T.GINI:
        return 1 - sum(Fraction(c, n) ** 2 for c in cnt)
    return -math.fsum(c / n * math.log2(c / n) for c in cnt)


def _oracle_gains(B, ys, nsplit, impurity, min_rows, min_gain):
    """{(feature, bin): gain} of the valid splits."""
    n, out = len(ys), {}
    for f, ns in enumerate(nsplit):
        for b in range(ns):
            L, R = [y for y, r in zip(ys, B) if r[f] <= b], [y for y, r in zip(ys, B) if r[f] > b]
            if len(L) < min_rows or len(R) < min_rows:
                continue
            gain = (_oracle_imp(ys, impurity) - Fraction(len(L), n) * _oracle_imp(L, impurity)
                    - Fraction(len(R), n) * _oracle_imp(R, impurity))
            if gain >= min_gain:
                out[f, b] = gain
    return out


@pytest.mark.parametrize("min_rows,min_gain", [(1, 0.0), (6, 0.0), (1, 0.3)])
@pytest.mark.parametrize("impurity", [T.VARIANCE, T.GINI, T.ENTROPY])
def test_hist_and_split_twins_equal_the_oracle(impurity, min_rows, min_gain):
    """Counts, the parent impurity (16 rows per node, dyadic labels) and the leaf flags are exact.
    Child sizes are not powers of two, so what divides by them is not exact in f64: those lie
    within 1e-14 of the exact value (a few ulp of quantities below 4).  The chosen split is the
    lowest (feature, split) among the exactly maximal ones: feature 1 copies feature 0 and never
    wins.  Node 1's labels follow feature 0 alone, so its best split leaves two pure children."""
    kind = T.REG if impurity == T.VARIANCE else T.CLS
    rng = np.random.default_rng(5)
    n, d, nb = 40, 3, 4
    B = rng.integers(0, nb, (n, 4)).astype(np.uint8)
    B[:, 1] = B[:, 0]                                    # a tie: feature 0 wins
    node = np.where(np.arange(n) >= 32, -1, np.arange(n) % 2).astype(np.int32)  # two open nodes, 8 rows in neither
    ys = ((B[:, 0] >= 2) * 2.0 + (B[:, 2] >= 3) * (node != 1)) * (0.25 if kind == T.REG else 1.0)
    classes, e = int(ys.max()) + 1, int(np.frexp(np.abs(ys).max())[1])
    H = T.hist_host(torch.from_numpy(B), torch.from_numpy(node), torch.from_numpy(ys), kind, 2, d, nb, classes, e)
    nsplit = [3, 3, 2]
    rec = T.split_host(H, nsplit, kind, impurity, e, min_rows, min_gain, False, False)
    near = lambda a, b: a == pytest.approx(float(b), abs=1e-14)  # noqa: E731
    for s in range(2):
        rows = [r for r in range(n) if node[r] == s]
        yl = [float(ys[r]) for r in rows]
        gains = _oracle_gains(B[rows], yl, nsplit, impurity, min_rows, min_gain)
        pimp = _oracle_imp(yl, impurity)
        assert rec[s, 4] == 16 and (near(rec[s, 3], pimp) if impurity == T.ENTROPY else rec[s, 3] == float(pimp))
        if not gains:
            assert rec[s, 0] == -1 and rec[s, 10] == 1
            continue
        f, b = int(rec[s, 0]), int(rec[s, 1])
        top = max(gains.values())
        assert (f, b) == min(k for k, g in gains.items() if (near(float(g), top) if impurity == T.ENTROPY else g == top))
        assert near(rec[s, 2], gains[f, b])
        assert rec[s, 10] == (0.0 if gains[f, b] > 0 else 1.0)
        L, R = [y for y, r in zip(yl, B[rows]) if r[f] <= b], [y for y, r in zip(yl, B[rows]) if r[f] > b]
        assert (rec[s, 6], rec[s, 7]) == (len(L), len(R))
        assert near(rec[s, 8], _oracle_imp(L, impurity)) and near(rec[s, 9], _oracle_imp(R, impurity))
        assert rec[s, 11] == float(_oracle_imp(L, impurity) == 0) and rec[s, 12] == float(_oracle_imp(R, impurity) == 0)
    if min_rows == 1 and min_gain == 0.0:  # node 1 splits feature 0 at its label step: both children are pure leaves
        assert rec[1, :2].tolist() == [0.0, 1.0] and rec[1, 8:13].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]
    assert T.split_host(H, nsplit, kind, impurity, e, 1, 0.0, True, True)[:, 10].tolist() == [1.0, 1.0]  # maxDepth 0
    comp = T.composite_hist(torch.from_numpy(B), torch.from_numpy(node), torch.from_numpy(ys), kind, 2, d, nb, classes)
    crec = T.split_stats(comp.numpy(), nsplit, kind, impurity, e, min_rows, min_gain, False, False)
    np.testing.assert_allclose(crec, rec, rtol=0, atol=1e-13)


def _steps(n=48, seed=2):
    X = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    return X, 3.0 * (X[:, 2] > 0.25) + (X[:, 0] > -0.5)


def _between(X, rows, f, cut, t):
    """t separates the node's rows at `cut`: it lies between their neighbouring values of feature f."""
    col = X[rows, f]
    return col[col <= cut].max() < t < col[col > cut].min()


@pytest.mark.parametrize("est", [DecisionTreeRegressor, DecisionTreeClassifier])
def test_fit_recovers_the_thresholds(cpu_session, est):
    X, y = _steps()
    df = cpu_session.createDataFrame([(Vectors.dense(*x), float(v)) for x, v in zip(X, y)], ["features", "label"])
    m = est(maxBins=64).fit(df)  # 48 rows: every midpoint is a candidate
    t = m._tree
    assert t.feature[0] == 2 and _between(X, slice(None), 2, 0.25, t.threshold[0]) and m.route == "host"
    for c, rows in ((t.left[0], X[:, 2] <= 0.25), (t.right[0], X[:, 2] > 0.25)):
        assert t.feature[c] == 0 and _between(X, rows, 0, -0.5, t.threshold[c])
    assert (m.numNodes, m.depth, m.numFeatures) == (7, 2, 3) and sorted(t.node_id) == [1, 2, 3, 4, 5, 6, 7]
    rows = m.transform(df).collect()
    assert [r["prediction"] for r in rows] == list(y)
    imp = m.featureImportances.toArray()
    assert imp.sum() == pytest.approx(1.0, abs=1e-15) and imp[1] == 0 and imp[0] > 0 and imp[2] > 0
    s = m.toDebugString.splitlines()
    assert s[1] == f"  If (feature 2 <= {float(t.threshold[0])!r})" and s[2].startswith("   If (feature 0 <= ")
    assert s[3] == "    Predict: 0.0" and f"  Else (feature 2 > {float(t.threshold[0])!r})" in s
    assert m.predict(Vectors.dense(0.0, 0.0, 0.9)) == 4.0
    if est is DecisionTreeClassifier:
        assert m.numClasses == 5 and m.predictRaw(Vectors.dense(0.0, 0.0, 0.9)).toArray()[4] == (y == 4).sum()
        assert all(r["probability"].toArray()[int(r["label"])] == 1.0 and r["rawPrediction"].toArray().sum() > 0 for r in rows)
    assert est(maxDepth=0).fit(df).numNodes == 1


def test_params_and_errors(cpu_session, tmp_path):
    r, c = DecisionTreeRegressor(), DecisionTreeClassifier(maxMemoryInMB=64, cacheNodeIds=True, checkpointInterval=5)
    assert (r.getMaxDepth(), r.getMaxBins(), r.getMinInstancesPerNode(), r.getMinInfoGain()) == (5, 32, 1, 0.0)
    assert (r.getImpurity(), c.getImpurity(), c.getRawPredictionCol(), c.getProbabilityCol()) == (
        "variance", "gini", "rawPrediction", "probability")
    for bad in (dict(maxDepth=31), dict(maxDepth=-1), dict(maxBins=1), dict(minInstancesPerNode=0), dict(impurity="gini")):
        with pytest.raises((ValueError, TypeError)):
            DecisionTreeRegressor(**bad)
    for name in ("thresholds", "varianceCol", "weightCol"):
        with pytest.raises(NotImplementedError, match=name):
            DecisionTreeClassifier(**{name: "x"})
    with pytest.raises(NotImplementedError, match="categorical"):
        r.setCategoricalFeaturesInfo({0: 3})
    X, y = _steps()
    rows = [(Vectors.dense(*x), float(v)) for x, v in zip(X, y)]
    m = c.fit(cpu_session.createDataFrame(rows, ["features", "label"]))
    with pytest.raises(NotImplementedError, match="sparse"):
        m.predict(SparseVector(3, [0], [1.0]))
    with pytest.raises(NotImplementedError, match="persistence"):
        m.save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="persistence"):
        DecisionTreeClassificationModel.load(str(tmp_path / "m"))
    for label, feat, est, msg in ((float("nan"), 0.0, r, "label"), (1.0, float("nan"), r, "NaN feature"),
                                  (0.5, 0.0, c, "integers"), (-1.0, 0.0, c, "integers")):
        df = cpu_session.createDataFrame(rows + [(Vectors.dense(feat, 0.0, 0.0), label)], ["features", "label"])
        with pytest.raises(ValueError, match=msg):
            est.fit(df)


def test_shapes_beyond_the_kernels():
    """More than 256 bins (the bin matrix widens to int16) and more than 16 classes (the node record
    widens) are served by the twins: the same tree as the shape the kernels would serve."""
    x = np.random.default_rng(0).uniform(-1, 1, (1, 2000))
    X, y = torch.from_numpy(x), torch.from_numpy((x[0] > 0.9).astype(np.float64))
    a, b = (T.fit(X, y, None, T.REG, T.VARIANCE, 2, mb) for mb in (256, 512))
    assert a.threshold[0] == b.threshold[0] and 0.89 < b.threshold[0] < 0.91 and b.count[1:3].tolist() == a.count[1:3].tolist()
    assert b.prediction[1] == 0.0 and b.prediction[2] > 0.95 and T.bin_host(X, None, *T.pack_splits([np.linspace(-1, 1, 400)]))[0].max() > 255
    lab = np.floor((x[0] + 1) * 10).clip(0, 19)  # 20 classes, each an interval of x
    t = T.fit(X, torch.from_numpy(lab), None, T.CLS, T.GINI, 6, 64)
    assert t.num_classes == 20 and t.class_counts.shape[1] == 20
    np.testing.assert_array_equal(t.class_counts[0], np.bincount(lab.astype(int), minlength=20))
    leaf = T.predict(X, None, t).numpy()
    # 19 class boundaries, each inside one of 63 bins of about 32 rows that loses at most half its rows: >= 85 % right
    assert (t.prediction[leaf] == lab).mean() > 0.8 and (t.class_counts[t.left[0]] + t.class_counts[t.right[0]] == t.class_counts[0]).all()


def test_pipeline_stage(cpu_session):
    X, y = _steps()
    df = cpu_session.createDataFrame([(*map(float, x), float(v)) for x, v in zip(X, y)], ["a", "b", "c", "label"])
    pipe = Pipeline(stages=[VectorAssembler(inputCols=["a", "b", "c"], outputCol="features"), DecisionTreeRegressor(maxBins=64)])
    assert [r[0] for r in pipe.fit(df).transform(df).select("prediction").collect()] == list(y)


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    X, y = _steps(120)
    lo, hi = (0, 63) if rank == 0 else (63, 120)
    df = spark.createDataFrame([(Vectors.dense(*x), float(v) + 0.125 * x[1]) for x, v in zip(X[lo:hi], y[lo:hi])],
                               ["features", "label"])
    t = DecisionTreeRegressor(maxDepth=4).fit(df)._tree
    q.put((rank, t.feature.tolist(), t.threshold.tolist(), t.gain.tolist(), t.prediction.tolist(), t.count.tolist()))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_fit_equals_the_single_process_fit(cpu_session):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X, y = _steps(120)
    df = cpu_session.createDataFrame([(Vectors.dense(*x), float(v) + 0.125 * x[1]) for x, v in zip(X, y)], ["features", "label"])
    t = DecisionTreeRegressor(maxDepth=4).fit(df)._tree
    for got in res:  # node for node, bit for bit: the words are integers
        assert got[1:] == (t.feature.tolist(), t.threshold.tolist(), t.gain.tolist(), t.prediction.tolist(), t.count.tolist())
