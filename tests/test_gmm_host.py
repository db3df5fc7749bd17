"""Gaussian mixtures on the host: the fp64 twin of the device pass against a 40-digit mpmath oracle,
the GaussianMixture API on the CPU engine and a two-rank (gloo) fit.

The oracle test also fixes the tolerance of tests/test_gpu_gmm.py: the twin's worst error, relative to
S (the sum of the absolute per-row terms of each statistic), measured 5.4e-16 and is asserted to stay
below 1e-13, so the kernel is held to the project's 1e-12 S against the twin.
"""
import multiprocessing as mp
import os
import socket

import mpmath
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import GaussianMixture, GaussianMixtureModel, VectorAssembler, Vectors
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import gmm as G

mpmath.mp.dps = 40
M = mpmath.mpf


def _oracle(X, live, w, mu, cov):
    """(statistics, S) of one E-step in 40 digits, the eigen rule included."""
    d, n = X.shape
    k = len(w)
    eps = M(2) ** -52
    gauss = []
    for j in range(k):
        lam, U = mpmath.eigsy(mpmath.matrix(cov[j].tolist()))
        keep = [i for i in range(d) if lam[i] > eps * max(lam) * d]
        W = [[U[a, i] / mpmath.sqrt(lam[i]) for a in range(d)] for i in keep]
        gauss.append((W, -(d * mpmath.log(2 * mpmath.pi) + sum(mpmath.log(lam[i]) for i in keep)) / 2))
    tri = [(a, b) for a in range(d) for b in range(a, d)]
    sw, sm = [M(0)] * k, [[M(0)] * d for _ in range(k)]
    S, Sabs = [[M(0)] * len(tri) for _ in range(k)], [[M(0)] * len(tri) for _ in range(k)]
    smabs, ll, llabs, rows = [[M(0)] * d for _ in range(k)], M(0), M(0), []
    for r in np.flatnonzero(live):
        x = [M(float(v)) for v in X[:, r]]
        p = []
        for j, (W, u) in enumerate(gauss):
            z = [sum(Wi[a] * (x[a] - M(float(mu[j][a]))) for a in range(d)) for Wi in W]
            p.append(eps + M(float(w[j])) * mpmath.exp(u - sum(v * v for v in z) / 2))
        P = sum(p)
        rows.append((r, [v / P for v in p], mpmath.log(P)))
        ll, llabs = ll + mpmath.log(P), llabs + abs(mpmath.log(P))
        for j in range(k):
            rj = p[j] / P
            sw[j] += rj
            for a in range(d):
                sm[j][a] += rj * x[a]
                smabs[j][a] += rj * abs(x[a])
            for t, (a, b) in enumerate(tri):
                S[j][t] += rj * x[a] * x[b]
                Sabs[j][t] += rj * abs(x[a] * x[b])
    flat = lambda *parts: [v for part in parts for v in part]  # noqa: E731
    stats = flat(sw, flat(*sm), flat(*S), [ll, M(int(live.sum()))])
    bound = flat(sw, flat(*smabs), flat(*Sabs), [llabs, M(1)])
    return stats, bound, rows


@pytest.mark.parametrize("d,k,n", [(1, 2, 9), (3, 3, 14), (17, 3, 12)])
def test_twin_equals_mpmath_oracle(d, k, n):
    rng = np.random.default_rng(10 * d + k)
    X = rng.uniform(-1, 1, (d, n))
    X[:, 1] = 1e3  # so far from every component that every p_j is EPS
    live = np.ones(n, dtype=bool)
    live[2] = False
    w = rng.dirichlet(np.ones(k))
    mu = rng.uniform(-1, 1, (k, d))
    A = rng.uniform(-1, 1, (k, d, d))
    cov = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(d)
    if d > 1:  # a singular component: the pseudo-inverse ignores feature 1
        cov[1] = np.diag(np.where(np.arange(d) == 1, 0.0, rng.uniform(0.5, 1.5, d)))
    Xn = np.where(live[None, :], X, np.nan)
    want, bound, rows = _oracle(X, live, w, mu, cov)
    got = G.em_pass_host(torch.from_numpy(Xn), torch.from_numpy(live), w, mu, cov, G.STEP).numpy()
    assert got.size == G.stats_size(k, d) == len(want) and got[-1] == n - 1
    worst = max(float(abs(M(float(g)) - t) / b) for g, t, b in zip(got, want, bound))
    print(f"twin vs oracle, d={d} k={k}: worst error / S = {worst:.2e}")
    assert worst <= 1e-13
    idx, prob, logp = (t.numpy() for t in G.em_pass_host(torch.from_numpy(Xn), torch.from_numpy(live), w, mu, cov, G.ASSIGN))
    assert idx[2] == -1 and (prob[:, 2] == 0).all() and logp[2] == 0
    np.testing.assert_array_equal(prob[:, 1], np.full(k, 1.0 / k))
    assert logp[1] == np.log(k * G.EPS) and idx[1] == 0  # all equal: the first maximum
    for r, rr, lp in rows:
        assert idx[r] == int(np.argmax([float(v) for v in rr])) or r == 1
        assert max(abs(M(float(prob[j, r])) - rr[j]) for j in range(k)) <= 1e-13 and abs(M(float(logp[r])) - lp) <= 1e-13 * abs(lp)
    comp = G.composite_pass(torch.from_numpy(Xn), torch.from_numpy(live), w, mu, cov, G.STEP).numpy()
    assert (np.abs(comp - got) <= 1e-13 * np.array([float(b) for b in bound])).all()


def test_gaussian_rule_and_m_step():
    W, u = G.gaussian_params([1.0, 2.0], [[4.0, 0.0], [0.0, 0.0]])  # singular: logdet and W skip the zero eigenvalue
    assert u == -0.5 * (2 * np.log(2 * np.pi) + np.log(4.0))
    np.testing.assert_allclose(np.abs(W).sum(axis=1), [0.0, 0.5])
    with pytest.raises(ValueError, match="no non-zero singular values"):
        G.gaussian_params([0.0, 0.0], np.zeros((2, 2)))
    stats = np.array([2.0, 6.0,  2.0, 4.0, 6.0, 18.0,  10.0, 4.0, 20.0, 12.0, 36.0, 120.0,  -7.0, 8.0])
    w, mu, cov = G.m_step_host(stats, 2, 2)
    np.testing.assert_array_equal(w, [0.25, 0.75])
    np.testing.assert_array_equal(mu, [[1.0, 2.0], [1.0, 3.0]])
    np.testing.assert_array_equal(cov, [[[4.0, 0.0], [0.0, 6.0]], [[1.0, 3.0], [3.0, 11.0]]])


def test_loop_stops_as_sparks_while():
    seen = []

    def step(w, mu, cov):  # log-likelihoods -50, -49.5, -49.495: |ll - prev| <= 0.01 after the third pass
        seen.append(w.copy())
        return torch.tensor([1.0, 3.0, 1.0, 3.0, 2.0, 12.0, (-50.0, -49.5, -49.495, -40.0)[len(seen) - 1], 4.0],
                            dtype=torch.float64)

    res = G.em(step, [0.5, 0.5], [[0.0], [1.0]], [[[1.0]], [[1.0]]], 100, 0.01, "host")
    assert res.iterations == 3 and res.log_likelihood == -49.495 and len(seen) == 3
    np.testing.assert_array_equal(res.weights, [0.25, 0.75])
    assert G.em(step, [0.5, 0.5], [[0.0], [1.0]], [[[1.0]], [[1.0]]], 0, 0.01, "host").iterations == 0
    seen.clear()
    assert G.em(step, [0.5, 0.5], [[0.0], [1.0]], [[[1.0]], [[1.0]]], 2, 0.01, "host").iterations == 2  # maxIter


def _blobs(n_per=60, seed=3):
    rng = np.random.default_rng(seed)
    means = np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 5.0], [0.0, 30.0, -5.0]])
    scale = np.array([[1.0, 1.0, 1.0], [2.0, 0.5, 1.0], [0.5, 1.0, 3.0]])
    pts = np.concatenate([m + s * rng.normal(size=(n_per + 20 * i, 3)) for i, (m, s) in enumerate(zip(means, scale))])
    lab = np.concatenate([np.full(n_per + 20 * i, i) for i in range(3)])
    p = rng.permutation(len(pts))
    return pts[p], lab[p]


def test_blobs_are_recovered(cpu_session):
    pts, lab = _blobs()
    df = cpu_session.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"])
    m = GaussianMixture(k=3, seed=7).fit(df)
    out = m.transform(df)
    pred = np.array([r[0] for r in out.select("prediction").collect()])
    prob = np.array([r[0].toArray() for r in out.select("probability").collect()])
    assert len({(a, b) for a, b in zip(lab, pred)}) == 3  # a bijection between blobs and components
    np.testing.assert_array_equal(prob.argmax(axis=1), pred)
    np.testing.assert_allclose(prob.sum(axis=1), 1.0, rtol=1e-14)
    assert out.schema["prediction"].dataType.typeName() == "integer"
    s = m.summary
    assert sorted(s.clusterSizes) == [60, 80, 100] and s.k == 3 and m.hasSummary and s.route == "host"
    assert 1 <= s.numIter <= 100 and s.logLikelihood < 0 and s.probabilityCol == "probability"
    assert s.cluster.columns == ["prediction"] and s.probability.columns == ["probability"]
    for i in range(3):  # well separated: the responsibilities are 0 / 1, the moments those of the blob
        j = pred[np.argmax(lab == i)]
        g = m.gaussians[j]
        np.testing.assert_allclose(m.weights[j], (lab == i).mean(), rtol=1e-9)
        np.testing.assert_allclose(g.mean.toArray(), pts[lab == i].mean(axis=0), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(g.cov.toArray(), np.cov(pts[lab == i].T, bias=True), rtol=1e-8, atol=1e-8)
        x = pts[np.argmax(lab == i)]
        assert m.predict(Vectors.dense(*x)) == j and m.predictProbability(Vectors.dense(*x)).toArray().argmax() == j
        assert g.pdf(Vectors.dense(*x)) == pytest.approx(np.exp(g.logpdf(x)))
    assert m.gaussiansDF.columns == ["mean", "cov"] and m.gaussiansDF.count() == 3


def test_params_defaults_and_errors(cpu_session, tmp_path):
    gm = GaussianMixture()
    assert (gm.getK(), gm.getMaxIter(), gm.getTol()) == (2, 100, 0.01)
    assert (gm.getFeaturesCol(), gm.getPredictionCol(), gm.getProbabilityCol()) == ("features", "prediction", "probability")
    for bad in (dict(k=1), dict(maxIter=-1), dict(tol=-1.0)):
        with pytest.raises((ValueError, TypeError)):
            GaussianMixture(**bad)
    df = cpu_session.createDataFrame([(Vectors.dense(float(i), 1.0),) for i in range(12)], ["features"])
    with pytest.raises(ValueError, match="at least 15 rows"):
        GaussianMixture(k=3).fit(df)
    with pytest.raises(NotImplementedError, match="weightCol"):
        GaussianMixture().setWeightCol("w")
    m = GaussianMixture(seed=1).fit(df)  # feature 1 is constant: singular covariances, the pseudo-inverse
    with pytest.raises(NotImplementedError, match="sparse"):
        m.predict(Vectors.sparse(2, [0], [1.0]))
    with pytest.raises(NotImplementedError, match="persistence"):
        m.save(str(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="persistence"):
        GaussianMixtureModel.load(str(tmp_path / "m"))
    GaussianMixture(k=4, seed=5).save(str(tmp_path / "est"))
    back = GaussianMixture.load(str(tmp_path / "est"))
    assert back.getK() == 4 and back.getSeed() == 5


def test_pipeline_stage(cpu_session):
    pts, lab = _blobs()
    df = cpu_session.createDataFrame([tuple(float(v) for v in p) for p in pts], ["a", "b", "c"])
    pipe = Pipeline(stages=[VectorAssembler(inputCols=["a", "b", "c"], outputCol="features"), GaussianMixture(k=3, seed=7)])
    pred = np.array([r[0] for r in pipe.fit(df).transform(df).select("prediction").collect()])
    assert len({(a, b) for a, b in zip(lab, pred)}) == 3


# ---- two ranks (gloo) -----------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init(backend="gloo")
    spark = SparkSession.builder().master("cpu").getOrCreate()
    pts, _ = _blobs()
    half = len(pts) // 2 + 3  # contiguous shards: global row numbers are the single process's
    df = spark.createDataFrame([(Vectors.dense(*p),) for p in (pts[:half] if rank == 0 else pts[half:])], ["features"])
    m = GaussianMixture(k=3, seed=7).fit(df)
    q.put((rank, m.weights, [g.mean.toArray().tolist() for g in m.gaussians], [g.cov.toArray().tolist() for g in m.gaussians],
           int(m.summary.numIter), float(m.summary.logLikelihood), list(m.summary.clusterSizes)))
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
    pts, _ = _blobs()
    m = GaussianMixture(k=3, seed=7).fit(cpu_session.createDataFrame([(Vectors.dense(*p),) for p in pts], ["features"]))
    for _, w, means, covs, its, ll, sizes in res:
        np.testing.assert_allclose(w, m.weights, rtol=1e-12)
        np.testing.assert_allclose(means, [g.mean.toArray() for g in m.gaussians], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(covs, [g.cov.toArray() for g in m.gaussians], rtol=1e-10, atol=1e-10)
        assert its == m.summary.numIter and sizes == m.summary.clusterSizes
        assert ll == pytest.approx(float(m.summary.logLikelihood), rel=1e-12)
