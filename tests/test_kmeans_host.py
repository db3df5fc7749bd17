"""k-means on the host: the fp64 twin of the device pass against a brute-force ``math.fsum`` oracle,
the KMeans API on the CPU engine and a two-rank (gloo) fit."""
import math
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import KMeans, KMeansModel, VectorAssembler, Vectors
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import kmeans as K


@pytest.mark.parametrize("d,k,n", [(1, 2, 5), (3, 4, 40), (17, 5, 70)])
def test_twin_equals_bruteforce_oracle(d, k, n):
    rng = np.random.default_rng(d + k + n)
    X, C = rng.integers(-8, 9, (d, n)).astype(np.float64), rng.integers(-8, 9, (k, d)).astype(np.float64)
    C[1] = C[0]
    live = rng.random(n) < 0.8
    Xn = np.where(live[None, :], X, np.nan)
    d2 = [[math.fsum((X[j, r] - C[c, j]) ** 2 for j in range(d)) for c in range(k)] for r in range(n)]
    a = np.array([int(np.argmin(row)) if live[r] else -1 for r, row in enumerate(d2)])
    got_a, got_c = K.lloyd_pass_host(torch.from_numpy(Xn), torch.from_numpy(live), C, K.ASSIGN)
    np.testing.assert_array_equal(got_a.numpy(), a)
    np.testing.assert_array_equal(got_c.numpy(), [min(row) if live[r] else 0.0 for r, row in enumerate(d2)])
    st = K.lloyd_pass_host(torch.from_numpy(Xn), torch.from_numpy(live), C, K.STEP).numpy()
    for c in range(k):
        assert st[k * d + c] == (a == c).sum()
        np.testing.assert_array_equal(st[c * d:(c + 1) * d], [math.fsum(X[j, a == c]) for j in range(d)])
    assert st[k * d + 1] == 0 and st[-1] == live.sum() and st[-2] == math.fsum(got_c.numpy())
    comp = K.composite_pass(torch.from_numpy(Xn), torch.from_numpy(live), C, K.STEP).numpy()
    np.testing.assert_array_equal(comp, st)
    new, cost, moved, done = K.update_host(st, C, 1e-4)
    np.testing.assert_array_equal(new[1], C[1])  # the empty centre stays
    assert cost == st[-2] and done == (moved <= 1e-8)


def _blobs(n_per=40, seed=3):
    rng = np.random.default_rng(seed)
    means = np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 5.0], [0.0, 30.0, -5.0]])
    pts = np.concatenate([m + rng.normal(size=(n_per + 5 * i, 3)) for i, m in enumerate(means)])
    lab = np.concatenate([np.full(n_per + 5 * i, i) for i in range(3)])
    p = rng.permutation(len(pts))
    return pts[p], lab[p]


@pytest.mark.parametrize("init", ["k-means||", "random"])
def test_blobs_are_recovered(cpu_session, init):
    pts, lab = _blobs()
    df = cpu_session.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"])
    m = KMeans(k=3, initMode=init, seed=7, maxIter=40).fit(df)
    pred = np.array([r[0] for r in m.transform(df).select("prediction").collect()])
    assert len({(a, b) for a, b in zip(lab, pred)}) == 3  # a bijection between blobs and clusters
    assert sorted(m.summary.clusterSizes) == [40, 45, 50] and m.summary.k == 3 and m.hasSummary
    want = np.array([pts[lab == i].mean(axis=0) for i in range(3)])
    got = np.array(m.clusterCenters())
    np.testing.assert_allclose(got[np.argsort(got[:, 0] + got[:, 1])], want[np.argsort(want[:, 0] + want[:, 1])],
                               rtol=1e-12, atol=1e-12)
    assert m.computeCost(df) == pytest.approx(float(m.summary.trainingCost), rel=1e-12)
    assert 1 <= m.summary.numIter <= 40 and m.summary.route == "host"
    assert m.predict(Vectors.dense(20.0, 0.0, 5.0)) == pred[np.argmax(lab == 1)]


def test_params_defaults_and_errors(cpu_session, tmp_path):
    km = KMeans()
    assert (km.getK(), km.getInitMode(), km.getInitSteps(), km.getMaxIter(), km.getTol()) == (2, "k-means||", 2, 20, 1e-4)
    assert km.getFeaturesCol() == "features" and km.getPredictionCol() == "prediction"
    assert km.getDistanceMeasure() == "euclidean"
    for bad in (dict(k=1), dict(initMode="kmeans++"), dict(initSteps=0), dict(maxIter=-1), dict(distanceMeasure="l1")):
        with pytest.raises((ValueError, TypeError)):
            KMeans(**bad)
    df = cpu_session.createDataFrame([(Vectors.dense(float(i), 1.0),) for i in range(6)], ["features"])
    with pytest.raises(NotImplementedError, match="cosine"):
        KMeans(distanceMeasure="cosine").fit(df)
    with pytest.raises(NotImplementedError, match="weightCol"):
        KMeans().setWeightCol("w")
    with pytest.raises(NotImplementedError, match="persistence"):
        KMeans().fit(df).save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="persistence"):
        KMeansModel.load(str(tmp_path / "m"))
    KMeans(k=4, seed=5).save(str(tmp_path / "est"))
    back = KMeans.load(str(tmp_path / "est"))
    assert back.getK() == 4 and back.getSeed() == 5


def test_seeding_is_deterministic_and_seed_dependent():
    pts, _ = _blobs(200)
    X = torch.from_numpy(pts.T.copy())
    for mode in ("random", "k-means||"):
        a, b = (K.seed_centers(X, None, 3, mode, 2, 11) for _ in range(2))
        np.testing.assert_array_equal(a, b)
        assert a.shape == (3, 3)
    assert not np.array_equal(K.seed_centers(X, None, 3, "random", 2, 11), K.seed_centers(X, None, 3, "random", 2, 12))
    sel = torch.ones(X.shape[1], dtype=torch.bool)
    sel[np.argsort(K.row_uniforms(11, X.shape[1]).numpy())[:3]] = False  # the rows a full selection picks
    c = K.seed_centers(X, sel, 3, "random", 2, 11)
    assert not any((c[:, None, :] == K.seed_centers(X, None, 3, "random", 2, 11)[None]).all(axis=2).ravel())


def test_pipeline_stage(cpu_session):
    pts, lab = _blobs()
    df = cpu_session.createDataFrame([tuple(float(v) for v in p) for p in pts], ["a", "b", "c"])
    pipe = Pipeline(stages=[VectorAssembler(inputCols=["a", "b", "c"], outputCol="features"), KMeans(k=3, seed=7)])
    out = pipe.fit(df).transform(df)
    pred = np.array([r[0] for r in out.select("prediction").collect()])
    assert out.schema["prediction"].dataType.typeName() == "integer"
    assert len({(a, b) for a, b in zip(lab, pred)}) == 3


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _worker(rank, world, port, init, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    pts, _ = _blobs()
    half = len(pts) // 2 + 3  # contiguous shards: global row numbers are the single process's
    mine = pts[:half] if rank == 0 else pts[half:]
    df = spark.createDataFrame([(Vectors.dense(*p),) for p in mine], ["features"])
    m = KMeans(k=3, initMode=init, seed=7, maxIter=40).fit(df)
    q.put((rank, np.array(m.clusterCenters()).tolist(), int(m.summary.numIter), float(m.summary.trainingCost),
           float(m.computeCost(df)), list(m.summary.clusterSizes),
           [r[0] for r in m.transform(df).select("prediction").collect()]))
    comm.barrier()
    comm.shutdown()


@pytest.mark.parametrize("init", ["k-means||", "random"])
def test_two_ranks_fit_equals_the_single_process_fit(cpu_session, init):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, init, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    pts, _ = _blobs()
    df = cpu_session.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"])
    m = KMeans(k=3, initMode=init, seed=7, maxIter=40).fit(df)
    want = [r[0] for r in m.transform(df).select("prediction").collect()]
    for _, centers, its, tcost, cost, sizes, pred in res:
        assert pred == want  # (collect gathers the shards in rank order)
        np.testing.assert_allclose(centers, np.array(m.clusterCenters()), rtol=1e-12, atol=1e-12)
        assert its == m.summary.numIter and sizes == m.summary.clusterSizes
        assert tcost == pytest.approx(float(m.summary.trainingCost), rel=1e-12)
        assert cost == pytest.approx(float(m.computeCost(df)), rel=1e-12)
