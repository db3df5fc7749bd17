"""The fused logistic pass (csrc/hip/logreg.hip) against its fp64 twin (ops/logreg.py).

Bound: |got - ref| <= 1e-12 S, S the fp64 sum of the absolute per-row terms of the statistic (the
project's bound for f64 row reductions, tests/test_gpu_rowops.py); counts are exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, kernels, kmeans as KM, logreg as L  # noqa: E402

NS = ((1, None), (63, None), (64, None), (65, None), (1061, 2))


def _case(d, K, n, seed, dead, big=False):
    """Features, labels, weights, selection (dead rows hold NaN everywhere) and coefficients."""
    rng = np.random.default_rng(seed)
    classes = max(K, 2)
    X = rng.uniform(-1, 1, (d, n)).astype(np.float32).astype(np.float64)
    y = rng.integers(0, classes, n).astype(np.float64)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32).astype(np.float64)
    live = rng.random(n) < 0.8 if dead else np.ones(n, dtype=bool)
    live[0] = True
    C = rng.normal(size=(K, d + 1)) * (800.0 / np.sqrt(d) if big else 1.0)
    for a in (X, y[None], w[None]):
        a[:, ~live] = np.nan
    return X, y, w, live, C


def _bound(X, y, w, live, C):
    """1e-12 S per statistic: S sums |w (p - [y = c]) x_j|, |w (p - [y = c])|, |row loss|, w."""
    K, d = C.shape[0], X.shape[0]
    Xz, wz = np.where(live, X, 0.0), np.where(live, w, 0.0)
    _, p, _ = (t.numpy() for t in L.logreg_pass_host(Xz, None, None, None, C, L.PREDICT))
    M = C[:, :d] @ Xz + C[:, d:]
    M = np.concatenate([-M, M]) if K == 1 else M
    yi = np.where(live, y, 0).astype(int)
    p[yi, np.arange(yi.size)] -= 1.0
    mult = np.abs(wz * p)[-K:]
    mx = M.max(axis=0)
    loss = np.abs(wz * (mx + np.log(np.exp(M - mx).sum(axis=0)) - M[yi, np.arange(yi.size)]))
    S = np.concatenate([np.concatenate([mult @ np.abs(Xz).T, mult.sum(axis=1)[:, None]], axis=1).reshape(-1),
                        [loss.sum(), wz.sum(), 0.0, 0.0]])
    return 1e-12 * S


@pytest.mark.parametrize("rows", ["plain", "w+sel"])
@pytest.mark.parametrize("K", (1, 3, 17, 33, 64))
@pytest.mark.parametrize("d", (1, 17, 33, 64))
def test_grad_equals_twin(d, K, rows):
    for n, blocks in NS:
        X, y, w, live, C = _case(d, K, n, 1000 * d + 10 * K + n, rows != "plain")
        wt, st = (None, None) if rows == "plain" else (torch.from_numpy(w), torch.from_numpy(live))
        want = L.logreg_pass_host(X, y, wt, st, C, L.GRAD).numpy()
        bound = _bound(X, y, w if wt is not None else np.ones(n), live, C)
        for dtype in (torch.float32, torch.float64):
            got = device.logreg_pass(torch.from_numpy(X).to(dtype).cuda(), torch.from_numpy(y).cuda(),
                                     None if wt is None else wt.to(dtype).cuda(), None if st is None else st.cuda(),
                                     C, L.GRAD, blocks).cpu().numpy()
            err = np.abs(got - want)
            assert (err <= bound).all(), (n, dtype, err.max())
            assert got[-2] == live.sum() and got[-1] == 0


@pytest.mark.parametrize("K", (1, 5))
def test_large_margins_and_bad_labels(K):
    d, n = 9, 333
    X, y, w, live, C = _case(d, K, n, 5 + K, True, big=True)
    M = C[:, :d] @ np.where(live, X, 0.0) + C[:, d:]
    assert np.abs(M).max() > 800
    y[1], y[2], y[3], live[1:4] = -1.0, 1.5, max(K, 2), True  # three bad labels on live rows
    X[:, 1:4], w[1:4] = 0.25, 1.0
    want = L.logreg_pass_host(X, y, w, live, C, L.GRAD).numpy()
    got = device.logreg_pass(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(),
                             torch.from_numpy(live).cuda(), C, L.GRAD).cpu().numpy()
    ok = live.copy()
    ok[1:4] = False
    assert np.isfinite(got).all() and got[-1] == want[-1] == 3 and got[-2] == live.sum()
    assert (np.abs(got - want) <= _bound(X, y, w, ok, C)).all()


@pytest.mark.parametrize("d,K", [(1, 1), (33, 1), (17, 3), (64, 17), (33, 64)])
def test_predict_equals_twin(d, K):
    for n, blocks in ((65, None), (1061, 2)):
        X, _, _, live, C = _case(d, K, n, 77 * d + K + n, True)
        Xz = np.where(live, X, 0.0)
        wr, wp, wpred = (t.numpy() for t in L.logreg_pass_host(X, None, None, live, C, L.PREDICT))
        rb = 1e-12 * (np.abs(C[:, :d]) @ np.abs(Xz) + np.abs(C[:, d:]))  # per (class, row): sum of |terms|
        rb = np.concatenate([rb, rb]) if K == 1 else rb
        top = np.sort(np.where(live, wr, 0.0), axis=0)
        assert ((top[-1] - top[-2])[live] > 2 * rb.max()).all()  # every live row's winner is clear
        assert (np.abs(wp[1] - 0.5)[live] > 1e-9).all() if K == 1 else True
        for dtype in (torch.float32, torch.float64):
            raw, prob, pred = (t.cpu().numpy() for t in device.logreg_pass(
                torch.from_numpy(X).to(dtype).cuda(), None, None, torch.from_numpy(live).cuda(), C, L.PREDICT, blocks))
            assert np.isnan(raw[:, ~live]).all() and np.isnan(prob[:, ~live]).all()
            assert (np.abs(raw - wr)[:, live] <= rb[:, live]).all()
            assert (np.abs(prob - wp)[:, live] <= 1e-12).all()
            np.testing.assert_array_equal(pred, wpred)


def test_two_runs_are_bit_identical():
    X, y, w, live, C = _case(33, 17, 20000, 5, False)
    args = (torch.from_numpy(X).float().cuda(), torch.from_numpy(y).cuda(), None, None, C, L.GRAD)
    assert torch.equal(device.logreg_pass(*args), device.logreg_pass(*args).clone())


def test_kmeans_statistics_unchanged_by_shared_slab_sum():
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.integers(-8, 9, (17, 64 * 4 * 3 + 7)).astype(np.float64))
    C = rng.integers(-8, 9, (5, 17)).astype(np.float64)
    want = kernels.kmeans_pass(X, None, C, KM.STEP)
    assert torch.equal(device.kmeans_pass(X.cuda(), None, C, KM.STEP, 3).cpu(), want)


def test_validation_errors():
    X, y = torch.zeros(4, 10).cuda(), torch.zeros(10, dtype=torch.float64).cuda()
    with pytest.raises(ValueError, match="d <= 64"):
        device.logreg_pass(torch.zeros(65, 10).cuda(), y, None, None, np.zeros((2, 66)), L.GRAD)
    with pytest.raises(ValueError, match="K <= 64"):
        device.logreg_pass(X, y, None, None, np.zeros((65, 5)), L.GRAD)
    with pytest.raises(ValueError, match="f32 / f64"):
        device.logreg_pass(X.to(torch.bfloat16), y, None, None, np.zeros((2, 5)), L.GRAD)
    with pytest.raises(ValueError, match="coef"):
        device.logreg_pass(X, y, None, None, np.zeros((2, 6)), L.GRAD)
    with pytest.raises(ValueError, match="mode"):
        device.logreg_pass(X, y, None, None, np.zeros((2, 5)), 2)
