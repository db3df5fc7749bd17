"""Random forests on the host: the twins of the level passes against a plain Python oracle (``int`` /
``Fraction`` sums over rows repeated by their bag count), the bag and subset rules, the estimators on
the CPU engine against DecisionTree* and a two-rank (gloo) fit."""
import multiprocessing as mp
import os
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import (DecisionTreeClassifier, DecisionTreeRegressor, RandomForestClassificationModel,
                                         RandomForestClassifier, RandomForestRegressor, VectorAssembler, Vectors)
from net.jgp.labs.sparkdq4ml_amd.models.linalg import SparseVector
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import forest as F, tree as T


@pytest.mark.parametrize("kind", [T.REG, T.CLS])
def test_twins_equal_the_oracle(kind):
    """Labels are multiples of 1/4, so every sum of the oracle is exact in f64 too."""
    rng = np.random.default_rng(3)
    n, d, m, nb, trees, classes = 200, 5, 2, 4, 3, 3
    B = rng.integers(0, nb, (n, 8)).astype(np.uint8)
    live = rng.random(n) < 0.9
    y = rng.integers(0, classes, n).astype(np.float64) * (0.25 if kind == T.REG else 1.0)
    node = F.bag_host(n, 7, torch.from_numpy(live), F.tree_seeds(5, trees), F.bag_thresholds(trees, 1.0)).numpy()
    cnt = node >> F.COUNT_SHIFT
    assert ((node >= 0) <= live).all() and cnt.max() >= 3 and (node[node >= 0] & F.SLOT_MASK == np.nonzero(node >= 0)[0]).all()
    slots = [(t, half) for t in range(trees) for half in (0, 1)]  # two open slots per tree: even and odd rows
    node = np.where(node >= 0, (cnt << F.COUNT_SHIFT) | (2 * (node & F.SLOT_MASK) + np.arange(n) % 2), -1).astype(np.int32)
    feats = np.stack([F.node_subset(1, t, 2 + h, d, m) for t, h in slots])
    e = int(np.frexp(np.abs(y).max())[1])
    H = F.hist_host(B, node, y, kind, d, m, nb, classes, e, [F._mask(f) for f in feats]).numpy()
    for s, (t, h) in enumerate(slots):
        rows = [r for r in range(n) if node[t, r] >= 0 and r % 2 == h for _ in range(cnt[t, r])]
        for p, f in enumerate(feats[s]):
            for b in range(nb):
                ys = [Fraction(y[r]) for r in rows if B[r, f] == b]
                if kind == T.CLS:
                    assert H[s, p, b].tolist() == [ys.count(k) for k in range(classes)]
                else:
                    assert H[s, p, b, 0] == len(ys) and T.limbs_to_f64(H[s, p, b, 1:5], e) == sum(ys)
                    assert T.limbs_to_f64(H[s, p, b, 5:9], 2 * e) == sum(v * v for v in ys)
    rec = F.split_host(H, feats, [3] * d, kind, T.VARIANCE if kind == T.REG else T.GINI, e, 1, 0.0, False, False)
    assert all(r[0] in fs or r[0] == -1 for r, fs in zip(rec, feats)) and (rec[:, 4] == H[:, 0].sum(axis=1)[:, :1 if kind == T.REG else classes].sum(axis=1)).all()
    tab = np.stack([rec[:, 0], rec[:, 1], np.arange(6) * 2, np.where(np.arange(6) % 3 == 0, -1, np.arange(6) * 2 + 1)], axis=1).astype(np.int32)
    got = F.route_host(torch.from_numpy(B), torch.from_numpy(node), tab).numpy()
    for t in range(trees):
        for r in range(n):
            want = -1
            if node[t, r] >= 0 and tab[node[t, r] & F.SLOT_MASK, 0] >= 0:
                f, b, lo, hi = tab[node[t, r] & F.SLOT_MASK]
                child = lo if B[r, f] <= b else hi
                want = -1 if child < 0 else (cnt[t, r] << F.COUNT_SHIFT) | child
            assert got[t, r] == want
    # the walk: two trees of three and one node, values added in tree order
    X = torch.from_numpy(rng.uniform(-1, 1, (d, n)))
    tabs = (np.array([1, -1, -1, -1]), np.array([0.1, 0, 0, 0]), np.array([1, -1, -1, -1]), np.array([2, -1, -1, -1]),
            np.array([0, 3]), np.array([[0.0, 0.0], [0.1, 0.7], [0.2, 0.3], [1e-17, 0.5]]))
    out = F.predict_host(X, torch.from_numpy(live), *tabs).numpy()
    for r in range(n):
        leaf = 1 if X[1, r] <= 0.1 else 2
        want = [0.0 + tabs[5][leaf, k] + tabs[5][3, k] for k in range(2)] if live[r] else [np.nan] * 2
        np.testing.assert_array_equal(out[:, r], want)


def test_bag_rule():
    one = F.bag_host(1000, 0, None, F.tree_seeds(1, 1), F.bag_thresholds(1, 1.0)).numpy()
    assert (one == 1 << F.COUNT_SHIFT).all()
    many = F.bag_host(100000, 0, None, F.tree_seeds(1, 20), F.bag_thresholds(20, 1.0)).numpy()
    c = np.where(many >= 0, many >> F.COUNT_SHIFT, 0)
    assert abs(c.mean() - 1.0) < 0.02 and abs(c[0].mean() - 1.0) < 0.02 and (many[5][many[5] >= 0] & F.SLOT_MASK == 5).all()
    thr = F.bag_thresholds(20, 1.0)
    assert thr.size <= 15 and (np.diff(thr.astype(np.int64)) >= 0).all() and thr[0] == int(np.exp(-1.0) * 2 ** 32)
    half = F.bag_host(100000, 0, None, F.tree_seeds(1, 1), F.bag_thresholds(1, 0.5)).numpy()
    assert set(np.unique(half)) == {-1, 1 << F.COUNT_SHIFT} and abs((half >= 0).mean() - 0.5) < 0.01


@pytest.mark.parametrize("d", [1, 9, 64])
def test_feature_subsets(d):
    log2 = {1: 1, 9: 4, 64: 6}[d]
    want = {"all": d, "sqrt": {1: 1, 9: 3, 64: 8}[d], "log2": log2, "onethird": {1: 1, 9: 3, 64: 22}[d], "1": 1, str(d): d,
            "0.5": {1: 1, 9: 5, 64: 32}[d], "1.0": d}
    for s, m in want.items():
        assert F.features_per_node(s, d, T.REG, 20) == m, s
    assert F.features_per_node("auto", d, T.REG, 1) == d and F.features_per_node("auto", d, T.CLS, 20) == want["sqrt"]
    assert F.features_per_node("auto", d, T.REG, 20) == want["onethird"]
    for bad in ("0", str(d + 1), "1.5", "0.0", "cube"):
        with pytest.raises(ValueError):
            F.features_per_node(bad, d, T.REG, 20)
    for m in sorted(set(want.values())):
        subs = [F.node_subset(7, t, i, d, m) for t in (0, 1) for i in (1, 2, 3, 12)]
        assert all(s.size == m and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < d for s in subs)
        assert all((a == b).all() for a, b in zip(subs, [F.node_subset(7, t, i, d, m) for t in (0, 1) for i in (1, 2, 3, 12)]))
        if 1 < m < d and d == 64:
            assert len({tuple(s) for s in subs}) == len(subs)  # nodes and trees differ


def _blobs(n=240, seed=2, classes=False):
    """Three blobs along features 0 and 2 of six; the label is the blob (0 / 1 / 2), noisy for regression."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    X = rng.normal(size=(n, 6))
    X[:, 0] += 2.5 * (k == 1)
    X[:, 2] += 2.5 * (k == 2)
    return X, k.astype(np.float64) + (0.0 if classes else 0.3 * rng.normal(size=n)), k


def _df(s, X, y):
    return s.createDataFrame([(Vectors.dense(*x), float(v)) for x, v in zip(X, y)], ["features", "label"])


@pytest.mark.parametrize("forest,tree", [(RandomForestRegressor, DecisionTreeRegressor), (RandomForestClassifier, DecisionTreeClassifier)])
def test_one_tree_is_the_decision_tree(cpu_session, forest, tree):
    X, y, _ = _blobs(classes=forest is RandomForestClassifier)
    df = _df(cpu_session, X, y)
    f = forest(numTrees=1, featureSubsetStrategy="all", subsamplingRate=1.0, maxDepth=4, seed=3).fit(df)
    a, b = f._trees[0], tree(maxDepth=4, seed=3).fit(df)._tree
    assert a.feature.size > 7 and f.getNumTrees == 1 and f.route == "host"
    for name in ("feature", "threshold", "left", "right", "gain", "impurity", "count", "prediction", "node_id"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    assert [r["prediction"] for r in f.transform(df).collect()] == [r["prediction"] for r in tree(maxDepth=4, seed=3).fit(df).transform(df).collect()]


@pytest.mark.parametrize("est", [RandomForestRegressor, RandomForestClassifier])
def test_forest_beats_its_worst_tree(cpu_session, est):
    cls = est is RandomForestClassifier
    X, y, k = _blobs(classes=cls)
    Xt, yt, kt = _blobs(seed=9, classes=cls)
    m = est(numTrees=20, maxDepth=3, seed=11).fit(_df(cpu_session, X, y))
    test = _df(cpu_session, Xt, yt)
    err = lambda rows: np.mean([(r["prediction"] != t) if cls else (r["prediction"] - t) ** 2 for r, t in zip(rows, kt)])  # noqa: E731
    whole, single = err(m.transform(test).collect()), [err(t.transform(test).collect()) for t in m.trees]
    assert whole < max(single) and whole < np.mean(single) and len(single) == 20 == m.getNumTrees
    imp = m.featureImportances.toArray()
    assert imp.sum() == pytest.approx(1.0, abs=1e-12) and (imp >= 0).all() and imp[0] + imp[2] > 0.5
    assert m.totalNumNodes == sum(t.numNodes for t in m.trees) and m.treeWeights == [1.0] * 20 and m.numFeatures == 6
    assert m.toDebugString.count("Tree ") == 20 and "Tree 19 (weight 1.0):" in m.toDebugString
    row = m.transform(test).collect()[0]
    assert m.predict(Vectors.dense(*Xt[0])) == row["prediction"]
    if cls:
        raw = m.predictRaw(Vectors.dense(*Xt[0])).toArray()
        assert m.numClasses == 3 and raw.sum() == pytest.approx(20.0, abs=1e-12) and (raw == row["rawPrediction"].toArray()).all()
        assert (m.predictProbability(Vectors.dense(*Xt[0])).toArray() == row["probability"].toArray()).all()
        assert row["prediction"] == float(np.argmax(raw))


def test_params_errors_and_pipeline(cpu_session, tmp_path):
    r, c = RandomForestRegressor(), RandomForestClassifier(maxMemoryInMB=64, cacheNodeIds=True, checkpointInterval=5)
    assert (r.getNumTrees(), r.getFeatureSubsetStrategy(), r.getSubsamplingRate(), r.getMaxDepth(), c.getImpurity()) == (
        20, "auto", 1.0, 5, "gini")
    for bad in (dict(numTrees=0), dict(subsamplingRate=0.0), dict(subsamplingRate=1.5), dict(featureSubsetStrategy="cube"),
                dict(maxBins=1), dict(impurity="gini")):
        with pytest.raises((ValueError, TypeError)):
            RandomForestRegressor(**bad)
    for name in ("thresholds", "weightCol"):
        with pytest.raises(NotImplementedError, match=name):
            RandomForestClassifier(**{name: "x"})
    with pytest.raises(NotImplementedError, match="categorical"):
        r.setCategoricalFeaturesInfo({0: 3})
    X, y, _ = _blobs(60, classes=True)
    m = c.setNumTrees(3).fit(_df(cpu_session, X, y))
    with pytest.raises(NotImplementedError, match="sparse"):
        m.predict(SparseVector(6, [0], [1.0]))
    with pytest.raises(NotImplementedError, match="persistence"):
        m.save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="persistence"):
        RandomForestClassificationModel.load(str(tmp_path / "m"))
    with pytest.raises(ValueError, match="featureSubsetStrategy"):
        RandomForestRegressor(featureSubsetStrategy="7").fit(_df(cpu_session, X, y))
    with pytest.raises(ValueError, match="NaN feature"):
        r.fit(_df(cpu_session, np.vstack([X, np.full((1, 6), np.nan)]), np.append(y, 1.0)))
    df = cpu_session.createDataFrame([(*map(float, x), float(v)) for x, v in zip(X, y)], [*"abcdef", "label"])
    pipe = Pipeline(stages=[VectorAssembler(inputCols=list("abcdef"), outputCol="features"), RandomForestRegressor(numTrees=4)])
    assert len(pipe.fit(df).transform(df).select("prediction").collect()) == 60


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _fit_lists(spark, lo, hi):
    X, y, _ = _blobs(120)
    m = RandomForestRegressor(numTrees=4, maxDepth=3, subsamplingRate=0.7, seed=5).fit(_df(spark, X[lo:hi], y[lo:hi]))
    return [(t.feature.tolist(), t.threshold.tolist(), t.gain.tolist(), t.prediction.tolist(), t.count.tolist()) for t in m._trees]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    q.put((rank, _fit_lists(SparkSession.builder().master("cpu").getOrCreate(), *((0, 63) if rank == 0 else (63, 120)))))
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
    want = _fit_lists(cpu_session, 0, 120)
    assert len(want) == 4 and len(want[0][0]) > 3
    for _, got in res:  # tree for tree, node for node, bit for bit: the words are integers
        assert got == want
