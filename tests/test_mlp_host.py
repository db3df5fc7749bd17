"""The multilayer perceptron on the host: the fp64 twin of the device pass against an mpmath oracle
(to a tenth of the kernel tests' bound), the flat weight layout against a hand-worked network, the
composite route, fits on the CPU engine, the API and a two-rank (gloo) fit."""
import multiprocessing as mp
import os
import socket

import mpmath
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import (CrossValidator, MulticlassClassificationEvaluator, MultilayerPerceptronClassifier,
                                         ParamGridBuilder, VectorAssembler, Vectors)
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import mlp as M


def blobs(n=240, seed=0):
    """XOR-like blobs: class = sign(x0) != sign(x1), which no linear model separates."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 4, n)
    X = np.c_[np.where(c & 1, 1.0, -1.0), np.where(c & 2, 1.0, -1.0)] + 0.2 * rng.normal(size=(n, 2))
    return X, ((c & 1) ^ (c >> 1)).astype(np.float64)


def frame(spark, X, y):
    return spark.createDataFrame([(Vectors.dense(*X[i]), float(y[i])) for i in range(len(y))], ["features", "label"])


def oracle(X, y, live, w, layers):
    """(statistics, sums of the absolute per-row terms) at 40 digits."""
    mpmath.mp.dps = 40
    f, mpf = mpmath, mpmath.mpf
    P, K = M.weight_count(layers), layers[-1]
    want, S = [mpf(0)] * (P + 3), [mpf(0)] * (P + 3)
    for r in range(X.shape[1]):
        if not live[r]:
            continue
        want[P + 1] += 1
        if not (0 <= y[r] < K and y[r] == np.floor(y[r])):
            want[P + 2] += 1
            continue
        acts, off, offs = [[mpf(v) for v in X[:, r]]], 0, []
        for l, (i, o) in enumerate(zip(layers[:-1], layers[1:])):
            z = [sum(mpf(w[off + j * o + u]) * acts[-1][j] for j in range(i)) + mpf(w[off + i * o + u]) for u in range(o)]
            acts.append(z if l == len(layers) - 2 else [1 / (1 + f.exp(-v)) for v in z])
            offs.append(off)
            off += (i + 1) * o
        z = acts.pop()
        lse = f.log(sum(f.exp(v) for v in z))
        loss = lse - z[int(y[r])]
        want[P] += loss
        S[P] += abs(loss)
        delta = [f.exp(v - lse) - (1 if u == int(y[r]) else 0) for u, v in enumerate(z)]
        for l in range(len(layers) - 2, -1, -1):
            i, o, off = layers[l], layers[l + 1], offs[l]
            for u in range(o):
                for j in range(i):
                    want[off + j * o + u] += delta[u] * acts[l][j]
                    S[off + j * o + u] += abs(delta[u] * acts[l][j])
                want[off + i * o + u] += delta[u]
                S[off + i * o + u] += abs(delta[u])
            delta = [sum(mpf(w[off + j * o + u]) * delta[u] for u in range(o)) * acts[l][j] * (1 - acts[l][j])
                     for j in range(i)]
    return want, S


@pytest.mark.parametrize("layers", ([2, 2, 2], [3, 4, 3, 2], [1, 1, 2]), ids=str)
def test_twin_equals_mpmath_oracle_within_a_tenth_of_the_kernel_bound(layers):
    rng = np.random.default_rng(sum(layers))
    n = 20
    X, y = rng.uniform(-1, 1, (layers[0], n)), rng.integers(0, layers[-1], n).astype(np.float64)
    live = np.ones(n, dtype=bool)
    live[3], X[:, 3], y[3], y[5] = False, np.nan, np.nan, 7.0  # a dead row and a bad label
    w = np.concatenate([rng.normal(size=(i + 1) * o) / np.sqrt(i) for i, o in zip(layers[:-1], layers[1:])])
    want, S = oracle(X, y, live, w, layers)
    got = M.mlp_pass_host(X, y, live, w, layers, M.GRAD).numpy()
    Sa = M.mlp_pass_host(X, y, live, w, layers, M.GRAD, absolute=True).numpy()
    P = M.weight_count(layers)
    ratio = max(float(abs(mpmath.mpf(got[i]) - want[i]) / (mpmath.mpf(1e-12) * S[i])) for i in range(P + 1))
    print("twin error / kernel bound", layers, ratio)
    assert ratio <= 0.1 and got[P + 1] == 19 and got[P + 2] == 1
    assert all(abs(mpmath.mpf(Sa[i]) - S[i]) <= mpmath.mpf(1e-12) * S[i] for i in range(P + 1))
    Xt, yt, lt = torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(live)
    comp = M.composite_pass(Xt, yt, lt, w, layers, M.GRAD).numpy()
    assert (np.abs(comp - got) <= 1e-12 * np.maximum(Sa, 1.0)).all()
    assert torch.equal(M.composite_pass(Xt, None, lt, w, layers, M.PREDICT), M.mlp_pass_host(X, None, live, w, layers, M.PREDICT))


def test_flat_layout_of_a_hand_worked_network():
    # W1 = [[1, 2], [3, 4]] (row = output unit), b1 = [0, -1]; W2 = [[1, -1], [0, 2]], b2 = [0.5, 0]
    w = np.array([1, 3, 2, 4, 0, -1, 1, 0, -1, 2, 0.5, 0], dtype=np.float64)
    x = np.array([[1.0], [-1.0]])
    a = 1 / (1 + np.exp(-np.array([1 * 1 + 2 * -1 + 0, 3 * 1 + 4 * -1 - 1])))
    z = np.array([a[0] - a[1] + 0.5, 2 * a[1]])
    p = np.exp(z) / np.exp(z).sum()
    d2 = p - [0, 1]
    d1 = np.array([1 * d2[0] + 0 * d2[1], -1 * d2[0] + 2 * d2[1]]) * a * (1 - a)
    want = np.concatenate([np.outer(x[:, 0], d1).reshape(-1), d1, np.outer(a, d2).reshape(-1), d2, [-np.log(p[1]), 1, 0]])
    got = M.mlp_pass_host(x, np.array([1.0]), None, w, [2, 2, 2], M.GRAD).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-16)
    assert M.weight_count([2, 2, 2]) == 12 and M.mlp_pass_host(x, None, None, w, [2, 2, 2], M.PREDICT)[0] == z.argmax()


def test_fit_separates_xor_blobs_and_is_reproducible(cpu_session):
    X, y = blobs()
    df = frame(cpu_session, X, y)
    mlp = MultilayerPerceptronClassifier(layers=[2, 5, 2], seed=7, maxIter=200)
    m = mlp.fit(df)
    pred = np.array([r[0] for r in m.transform(df).select("prediction").collect()])
    assert (pred == y).mean() >= 0.99 and m.route == "host" and m.numFeatures == 2 and m.layers == [2, 5, 2]
    assert m.predict(Vectors.dense(*X[0])) == pred[0]
    assert np.array_equal(mlp.fit(df).weights.toArray(), m.weights.toArray())  # the seed fixes the start
    w0 = M.random_weights([2, 5, 2], 3)
    bound = np.repeat([2.4 / np.sqrt(2), 2.4 / np.sqrt(5)], [15, 12])
    assert (np.abs(w0) <= bound).all() and np.abs(w0 / bound).max() > 0.8
    fits = [MultilayerPerceptronClassifier(layers=[2, 5, 2], initialWeights=Vectors.dense(*w0), maxIter=20).fit(df)
            for _ in range(2)]
    assert np.array_equal(fits[0].weights.toArray(), fits[1].weights.toArray())
    assert not np.array_equal(fits[0].weights.toArray(), w0)


def test_params_errors_pipeline_and_evaluator(cpu_session, tmp_path):
    mlp = MultilayerPerceptronClassifier(layers=[2, 3, 2])
    assert (mlp.getBlockSize(), mlp.getSolver(), mlp.getMaxIter(), mlp.getTol(), mlp.getStepSize()) == (128, "l-bfgs", 100, 1e-6, 0.03)
    assert (mlp.getFeaturesCol(), mlp.getLabelCol(), mlp.getPredictionCol(), mlp.getInitialWeights()) == ("features", "label", "prediction", None)
    mlp.save(str(tmp_path / "mlp"))
    assert MultilayerPerceptronClassifier.load(str(tmp_path / "mlp")).getLayers() == [2, 3, 2]
    for bad in (lambda: mlp.setLayers([2]), lambda: mlp.setLayers([2, 0, 2]), lambda: mlp.setSolver("adam"),
                lambda: mlp.setRawPredictionCol("raw"), lambda: MultilayerPerceptronClassifier(probabilityCol="p")):
        with pytest.raises((NotImplementedError, ValueError)):
            bad()
    X, y = blobs(120)
    df = frame(cpu_session, X, y)
    with pytest.raises(NotImplementedError, match="gd"):
        MultilayerPerceptronClassifier(layers=[2, 3, 2], solver="gd").fit(df)
    with pytest.raises(ValueError, match="length 17"):
        MultilayerPerceptronClassifier(layers=[2, 3, 2], initialWeights=Vectors.dense(*np.zeros(16))).fit(df)
    with pytest.raises(ValueError, match="feature width"):
        MultilayerPerceptronClassifier(layers=[3, 3, 2]).fit(df)
    with pytest.raises(ValueError, match="class ind"):
        MultilayerPerceptronClassifier(layers=[2, 3, 2]).fit(frame(cpu_session, X, y + 2))
    with pytest.raises(NotImplementedError, match="sparse"):
        MultilayerPerceptronClassifier(layers=[2, 3, 2], initialWeights=Vectors.sparse(17, [0], [1.0]))
    cols = cpu_session.createDataFrame([(float(X[i, 0]), float(X[i, 1]), float(y[i])) for i in range(len(y))],
                                       ["a", "b", "label"])
    model = Pipeline(stages=[VectorAssembler(inputCols=["a", "b"], outputCol="features"),
                             MultilayerPerceptronClassifier(layers=[2, 4, 2], seed=1)]).fit(cols)
    out = model.transform(cols)
    assert out.columns[-1] == "prediction"
    acc = MulticlassClassificationEvaluator(metricName="accuracy").evaluate(out)
    assert acc >= 0.95
    m = model.stages[-1]
    with pytest.raises(NotImplementedError):
        m.save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="sparse"):
        m.predict(Vectors.sparse(2, [0], [1.0]))
    grid = ParamGridBuilder().addGrid("maxIter", [0, 100]).build()
    cv = CrossValidator(estimator=MultilayerPerceptronClassifier(layers=[2, 4, 2], seed=1), estimatorParamMaps=grid,
                        numFolds=3, evaluator=MulticlassClassificationEvaluator(metricName="accuracy")).fit(df)
    assert cv.avgMetrics[1] > cv.avgMetrics[0] and cv.bestModel.layers == [2, 4, 2]


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    X, y = blobs()
    part = slice(0, 130) if rank == 0 else slice(130, None)
    m = MultilayerPerceptronClassifier(layers=[2, 5, 2], seed=7, maxIter=15).fit(frame(spark, X[part], y[part]))
    q.put((rank, m.weights.toArray().tolist()))
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
    X, y = blobs()
    one = MultilayerPerceptronClassifier(layers=[2, 5, 2], seed=7, maxIter=15).fit(frame(cpu_session, X, y)).weights.toArray()
    assert res[0][1] == res[1][1]
    # (the two ranks sum their statistics in another order: rounding, carried through 15 iterations)
    assert np.abs(np.array(res[0][1]) - one).max() <= 1e-9 * max(1.0, np.abs(one).max())
