"""ALS on the device: the fit against the CPU engine's, the transform under both cold-start
strategies, the factor frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd import ALS, SparkSession  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops import als as A  # noqa: E402

PARAMS = dict(rank=5, maxIter=6, regParam=0.05, seed=3)


def data(users=60, items=40, n=900, seed=2):
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, users, n), rng.integers(0, items, n)
    r = np.round(2.0 * (3.0 + np.sin(u) + np.cos(i) + 0.3 * rng.normal(size=n))) / 2.0
    return 7 * u + 1, 3 * i, r  # ids that are not dense


def _fit(master, u, i, r):
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    spark = SparkSession.builder().appName("test").master(master).getOrCreate()
    try:
        rows = [(int(a), int(b), float(c)) for a, b, c in zip(u, i, r)] + [(5, 0, 1e9)]  # the last row is filtered out
        df = spark.createDataFrame(rows, ["user", "item", "rating"]).filter("rating < 1000")
        m = ALS(**PARAMS).fit(df)
        new = spark.createDataFrame([(int(u[0]), int(i[0])), (5, int(i[0])), (int(u[1]), 1)], ["user", "item"])
        nan = [r[2] for r in m.transform(new).collect()]
        drop = [tuple(r) for r in m.setColdStartStrategy("drop").transform(new).collect()]
        uf, itf = m.userFactors.collect(), m.itemFactors.collect()
        return (m._user_factors, m._item_factors, m.route, nan, drop, [r[0] for r in uf], [r[0] for r in itf],
                np.array([r[1].toArray() for r in uf]))
    finally:
        spark.stop()


def test_device_fit_equals_the_cpu_engine():
    u, i, r = data()
    gU, gV, groute, gnan, gdrop, guid, giid, guf = _fit("mi355x[*]", u, i, r)
    cU, cV, croute, cnan, cdrop, cuid, ciid, _ = _fit("cpu", u, i, r)
    # The tolerance.  Both engines solve in f64 and store f32, so they part only where their f64
    # solutions round to different f32 neighbours: a perturbation of one f32 ulp of a component,
    # which later iterations propagate.  Rounding every stored component to f32 at all perturbs it
    # by up to half an ulp, and what THAT costs is measured here: the twin's fit with f32 storage
    # against the same fit with f64 storage.  A flipped rounding is at most twice such a
    # perturbation and happens in few components, so the engines may differ by twice that figure.
    _, ud = np.unique(u, return_inverse=True)
    _, idn = np.unique(i, return_inverse=True)
    args = (torch.from_numpy(ud), torch.from_numpy(idn), torch.from_numpy(r), ud.max() + 1, idn.max() + 1, PARAMS["rank"],
            PARAMS["maxIter"], PARAMS["regParam"], PARAMS["seed"], "host")
    f32, f64 = A.fit(*args, storage=np.float32), A.fit(*args, storage=np.float64)
    tol = 2.0 * max(np.abs(f32.user_factors - f64.user_factors).max(), np.abs(f32.item_factors - f64.item_factors).max())
    dist = max(np.abs(gU - cU).max(), np.abs(gV - cV).max())
    print("device fit - cpu fit", dist, "tolerance (2 x f32 storage against f64 storage)", tol)
    assert (groute, croute) == ("fused", "host") and np.array_equal(cU, f32.user_factors)
    assert dist <= tol
    # transform: NaN for an id the fit did not see (user 5 only has the dead row, item 1 none), dropped under "drop"
    for nan, drop in ((gnan, gdrop), (cnan, cdrop)):
        assert np.isfinite(nan[0]) and np.isnan(nan[1]) and np.isnan(nan[2])
        assert len(drop) == 1 and drop[0][:2] == (int(u[0]), int(i[0])) and drop[0][2] == nan[0]
    assert abs(gnan[0] - cnan[0]) <= 2 * PARAMS["rank"] * tol * max(np.abs(cU).max(), np.abs(cV).max()) + np.spacing(np.float32(abs(cnan[0])))
    # the factor frames: ids in key order, the rows of the factors
    assert guid == cuid == sorted(set(u.tolist())) and giid == ciid == sorted(set(i.tolist()))
    assert np.array_equal(guf, gU.astype(np.float64))
