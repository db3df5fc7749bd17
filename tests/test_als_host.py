"""ALS on the host: the fp64 twin of the device half-step against extended-precision normal
equations, the segment builder against a plain grouping, fits on the CPU engine, the API."""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd import ALS, ALSModel, SparkSession
from net.jgp.labs.sparkdq4ml_amd.models.pipeline import Pipeline
from net.jgp.labs.sparkdq4ml_amd.ops import als as A

C = A.CHUNK
LENGTHS = (0, 1, 3, 4, 5, C - 1, C, C + 1, 3 * C + 7)


def table(rank, lengths=LENGTHS, sources=300, seed=0, dtype=np.float32):
    """(offsets, src, rating, Y): one segment per length, half-integer ratings, unit-norm factors."""
    rng = np.random.default_rng(seed + rank)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    src = rng.integers(0, sources, off[-1]).astype(np.int32)
    rating = rng.integers(1, 11, off[-1]) / 2.0
    Y = rng.normal(size=(sources, rank))
    Y = (Y / np.linalg.norm(Y, axis=1, keepdims=True)).astype(dtype)
    return torch.from_numpy(off), torch.from_numpy(src), torch.from_numpy(rating), torch.from_numpy(Y)


def residual_ratio(off, src, rating, Y, reg, X):
    """The largest ``|A* x - b*| / (|A*| |x| + |b*|)`` over the solved systems and their components,
    with the normal equations of the stored factors in ``np.longdouble``; an empty segment must
    hold zeros."""
    ld = np.longdouble
    off, src = off.numpy(), src.numpy()
    Yl, rl, Xl = Y.numpy().astype(ld), rating.numpy().astype(ld), np.asarray(X).astype(ld)
    worst = 0.0
    for d in range(off.size - 1):
        o0, o1 = off[d], off[d + 1]
        if o0 == o1:
            assert not Xl[d].any()
            continue
        Ys, r, ridge = Yl[src[o0:o1]], rl[o0:o1], ld(reg) * ld(o1 - o0) * np.eye(Yl.shape[1], dtype=ld)
        res = np.abs((Ys.T @ Ys + ridge) @ Xl[d] - Ys.T @ r)
        scale = (np.abs(Ys).T @ np.abs(Ys) + ridge) @ np.abs(Xl[d]) + np.abs(Ys).T @ np.abs(r)
        worst = max(worst, float((res / scale).max()))
    return worst


@pytest.mark.parametrize("reg", (0.1, 1e-6))
@pytest.mark.parametrize("rank", (1, 2, 10, 15, 16, 17, 33, 64))
def test_twin_meets_the_bound(rank, reg):
    off, src, rating, Y = table(rank, dtype=np.float64 if rank % 2 else np.float32)
    X, fails = A.als_half_step_host(off, src, rating, Y, reg, np.float64)
    ratio = residual_ratio(off, src, rating, Y, reg, X) / 1e-12
    print("twin residual / bound", rank, reg, ratio)
    assert fails == 0 and ratio <= 1.0
    X32, _ = A.als_half_step_host(off, src, rating, Y, reg, np.float32)
    assert np.array_equal(X32, X.astype(np.float32))  # rounded once, at the store


def test_segment_builder():
    rng = np.random.default_rng(3)
    dst, src = rng.integers(0, 7, 500), rng.integers(0, 11, 500)
    dst[dst == 4] = 5  # destination 4 stays empty
    rating = rng.normal(size=500)
    seg = A.build_segments(torch.from_numpy(dst), torch.from_numpy(src), torch.from_numpy(rating), 7, 11)
    assert seg.offsets.dtype == torch.int64 and seg.src.dtype == torch.int32 and seg.rating.dtype == torch.float64
    for d in range(7):
        rows = [i for i in range(500) if dst[i] == d]  # in row order
        o0, o1 = int(seg.offsets[d]), int(seg.offsets[d + 1])
        assert seg.src[o0:o1].tolist() == src[rows].tolist() and seg.rating[o0:o1].tolist() == rating[rows].tolist()
    assert int(seg.offsets[-1]) == 500


@pytest.fixture(scope="module")
def spark():
    s = SparkSession.builder().appName("test").master("cpu").getOrCreate()
    yield s
    s.stop()


def ratings(spark, users=12, items=9, seed=0):
    """Every cell of a rank-3 matrix; ids that are not dense."""
    rng = np.random.default_rng(seed)
    R = rng.normal(size=(users, 3)) @ rng.normal(size=(items, 3)).T
    rows = [(10 * u + 3, float(2 * i), float(R[u, i])) for u in range(users) for i in range(items)]
    return spark.createDataFrame(rows, ["user", "item", "rating"]), R


def test_full_matrix_is_reproduced(spark):
    df, R = ratings(spark)
    m = ALS(rank=3, maxIter=20, regParam=1e-4, seed=5).fit(df.filter("rating > -100"))
    got = np.array([r[0] for r in m.transform(df).select("prediction").collect()]).reshape(R.shape)
    print("relative error", np.abs(got - R).max() / np.abs(R).max())
    assert np.abs(got - R).max() <= 1e-3 * np.abs(R).max() and m.rank == 3 and m.route == "host"
    uf, itf = m.userFactors.collect(), m.itemFactors.collect()
    assert [r[0] for r in uf] == [10 * u + 3 for u in range(12)] and [r[0] for r in itf] == [2 * i for i in range(9)]
    assert m.userFactors.columns == ["id", "features"] and len(uf[0][1].toArray()) == 3
    again = ALS(rank=3, maxIter=20, regParam=1e-4, seed=5).fit(df)
    assert np.array_equal(again._user_factors, m._user_factors) and np.array_equal(again._item_factors, m._item_factors)
    other = ALS(rank=3, maxIter=20, regParam=1e-4, seed=6).fit(df)
    assert not np.array_equal(other._user_factors, m._user_factors)


def test_dead_rows_and_cold_start(spark):
    df, _ = ratings(spark)
    extra = spark.createDataFrame([(7, 0.0, 1e9), (3, 1.0, 5.0)], ["user", "item", "rating"])
    m = ALS(rank=2, maxIter=3, seed=1).fit(df.union(extra).filter("rating < 1000"))
    assert 7 not in m._user_ids and 1 in m._item_ids  # a dead row's id is not a user; the live row's item is one
    new = spark.createDataFrame([(3, 0.0), (4, 0.0), (13, 5.0), (None, 2.0)], ["user", "item"])
    pred = [r[2] for r in m.transform(new).collect()]
    assert m.transform(new).columns == ["user", "item", "prediction"]
    assert np.isfinite(pred[0]) and all(np.isnan(p) for p in pred[1:])
    dropped = m.setColdStartStrategy("drop").transform(new).collect()
    assert len(dropped) == 1 and dropped[0][0] == 3 and dropped[0][2] == pred[0]
    assert isinstance(Pipeline(stages=[ALS(rank=2, maxIter=1)]).fit(df).stages[0], ALSModel)


def test_params_and_errors(spark, tmp_path):
    als = ALS()
    want = dict(rank=10, maxIter=10, regParam=0.1, userCol="user", itemCol="item", ratingCol="rating",
                predictionCol="prediction", coldStartStrategy="nan")
    assert {k: als.getOrDefault(k) for k in want} == want
    ALS(numUserBlocks=4, numItemBlocks=4, checkpointInterval=2, intermediateStorageLevel="MEMORY_ONLY",
        finalStorageLevel="MEMORY_ONLY", implicitPrefs=False, nonnegative=False)
    for kw in (dict(implicitPrefs=True), dict(alpha=2.0), dict(nonnegative=True)):
        with pytest.raises(NotImplementedError, match="not implemented"):
            ALS(**kw)
    with pytest.raises(Exception):
        ALS(coldStartStrategy="zero")
    df, _ = ratings(spark)
    m = ALS(rank=2, maxIter=1).fit(df)
    for call in (m.write, lambda: m.save(str(tmp_path / "m")), ALSModel.read, lambda: m.recommendForAllUsers(3),
                 lambda: m.recommendForAllItems(3)):
        with pytest.raises(NotImplementedError, match="not implemented"):
            call()
    bad = {"a value is not an integer": [(0.5, 1, 1.0)], "out of range": [(2.0 ** 31, 1, 1.0)], "null id": [(None, 1, 1.0), (1, 1, 2.0)],
           "null rating": [(1, 1, None), (1, 2, 2.0)]}
    for msg, rows in bad.items():
        with pytest.raises(ValueError, match=msg):
            ALS(maxIter=1).fit(spark.createDataFrame(rows, ["user", "item", "rating"]))
    with pytest.raises(Exception, match="numeric"):
        ALS(maxIter=1).fit(spark.createDataFrame([("a", 1, 1.0)], ["user", "item", "rating"]))
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import LocalRelation
    from net.jgp.labs.sparkdq4ml_amd.sql.dataframe import DataFrame

    sharded = DataFrame(LocalRelation(df._table(), sharded=True), spark)
    with pytest.raises(Exception, match="shuffle"):
        ALS(maxIter=1).fit(sharded)
    with pytest.raises(ArithmeticError, match="pivot"):  # one rating cannot fix two components
        ALS(rank=2, maxIter=1, regParam=0.0).fit(spark.createDataFrame([(1, 1, 1.0)], ["user", "item", "rating"]))
