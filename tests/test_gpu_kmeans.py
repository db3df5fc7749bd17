"""The fused k-means pass (csrc/hip/kmeans.hip) against its fp64 twin (ops/kmeans.py).

Real-valued cases: assignments and counts equal the twin's exactly -- the inputs are asserted to have
every live row's two smallest squared distances further apart than 1e-12 (|x|^2 + max |c|^2) -- and
sums and cost lie within 1e-12 S, S the fp64 sum of the absolute per-row terms (the project's bound
for f64 row reductions, tests/test_gpu_rowops.py).  Integer cases are exact: everything bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, kmeans as K  # noqa: E402

DS, KS = (1, 16, 17, 33, 64), (2, 16, 17, 64)
NS = ((1, None), (63, None), (64, None), (65, None), (333, None), (64 * 4 * 3 + 7, 1), (64 * 4 * 3 + 7, 3))


def _dev(X, dtype, pad=0):
    """Feature-major device matrix of ``dtype`` with ``pad`` extra columns behind the rows (ld > n)."""
    t = torch.from_numpy(X).to(dtype)
    if pad:
        t = torch.cat([t, torch.full((t.shape[0], pad), float("nan"), dtype=dtype)], dim=1)
    return t.cuda()[:, :X.shape[1]]


def _stats_bound(Xz, live, C, a):
    k, d = C.shape
    S = np.zeros(K.stats_size(k, d))
    for c in range(k):
        S[c * d:(c + 1) * d] = np.abs(Xz[:, live & (a == c)]).sum(axis=1)
    S[k * d + k] = ((Xz * Xz).sum(axis=0) + (C * C).sum(axis=1)[a])[live].sum()
    return 1e-12 * S


@pytest.mark.parametrize("with_sel", [False, True], ids=["all", "sel"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
def test_pass_equals_twin(d, k, with_sel):
    for n, blocks in NS:
        rng = np.random.default_rng(1000 * d + 10 * k + n)
        X = rng.uniform(-1, 1, (d, n)).astype(np.float32).astype(np.float64)
        C = rng.uniform(-1, 1, (k, d))
        live = rng.random(n) < 0.8 if with_sel else np.ones(n, dtype=bool)
        live[0] = True
        d2 = np.sort(((X.T[:, None, :] - C[None, :, :]) ** 2).sum(axis=2), axis=1)
        gap = (d2[:, 1] - d2[:, 0]) / ((X * X).sum(axis=0) + (C * C).sum(axis=1).max())
        assert gap[live].min() > 1e-12
        Xn = np.where(live[None, :], X, np.nan)  # dead rows hold NaN
        sel = torch.from_numpy(live) if with_sel else None
        want = K.lloyd_pass_host(torch.from_numpy(Xn), sel, C, K.STEP).numpy()
        wa, wc = (t.numpy() for t in K.lloyd_pass_host(torch.from_numpy(Xn), sel, C, K.ASSIGN))
        bound = _stats_bound(X, live, C, wa)
        for dtype in (torch.float32, torch.float64):
            Xd = _dev(Xn, dtype, pad=11 if n == 333 else 0)  # ld = 344: aligned, so this view is what is staged
            seld = None if sel is None else sel.cuda()
            got = device.kmeans_pass(Xd, seld, C, K.STEP, blocks).cpu().numpy()
            np.testing.assert_array_equal(got[k * d:k * d + k], want[k * d:k * d + k])
            assert got[-1] == want[-1] == live.sum()
            assert (np.abs(got - want) <= bound).all(), (n, dtype, np.abs(got - want).max())
            ga, gc = device.kmeans_pass(Xd, seld, C, K.ASSIGN, blocks)
            np.testing.assert_array_equal(ga.cpu().numpy(), wa)
            assert (np.abs(gc.cpu().numpy() - wc) <= 1e-12 * ((X * X).sum(axis=0) + (C * C).sum(axis=1).max())).all()


@pytest.mark.parametrize("d,k", [(1, 2), (17, 17), (33, 16), (64, 64)])
def test_integer_case_is_bit_exact(d, k):
    rng = np.random.default_rng(7 * d + k)
    n = 64 * 4 * 3 + 7
    C = rng.integers(-8, 9, (k, d)).astype(np.float64)
    C[1] = C[0]                      # a duplicated centre: the lower index wins
    C[k - 1] = 1000.0                # attracts no row
    X = rng.integers(-8, 9, (d, n)).astype(np.float64)
    X[:, :8] = ((C[0] + C[2 % k]) / 2.0)[:, None] if k > 2 else C[0][:, None]  # (half-integers are exact too)
    live = rng.random(n) < 0.9
    want = K.lloyd_pass_host(torch.from_numpy(X), torch.from_numpy(live), C, K.STEP).numpy()
    wa, wc = K.lloyd_pass_host(torch.from_numpy(X), torch.from_numpy(live), C, K.ASSIGN)
    assert want[k * d + 1] == 0 and want[k * d + k - 1] == 0
    for dtype in (torch.float32, torch.float64):
        Xd, seld = _dev(X, dtype), torch.from_numpy(live).cuda()
        for blocks in (1, 3):
            np.testing.assert_array_equal(device.kmeans_pass(Xd, seld, C, K.STEP, blocks).cpu().numpy(), want)
        ga, gc = device.kmeans_pass(Xd, seld, C, K.ASSIGN)
        assert torch.equal(ga.cpu(), wa) and torch.equal(gc.cpu(), wc)


def test_update_keeps_empty_centre_and_stops_when_done():
    k, d, tol = 3, 2, 0.5
    C = np.array([[0.0, 0.0], [4.0, 4.0], [9.0, 9.0]])
    stats = np.array([1.0, 1.0, 8.4, 8.6, 0.0, 0.0, 4.0, 2.0, 0.0, 12.5, 6.0])
    new = np.array([[0.25, 0.25], [4.2, 4.3], [9.0, 9.0]])  # sum / count; the empty centre stays
    moved = ((new - C) ** 2).sum(axis=1)
    cen = torch.from_numpy(np.concatenate([C.reshape(-1), 0.5 * (C * C).sum(axis=1)])).cuda()
    state = torch.zeros(4, dtype=torch.float64).cuda()
    device.kmeans_update(torch.from_numpy(stats).cuda(), k, d, tol, cen, state)
    got = cen.cpu().numpy()
    np.testing.assert_array_equal(got[:k * d].reshape(k, d), new)
    np.testing.assert_allclose(got[k * d:], 0.5 * (new * new).sum(axis=1), rtol=1e-15)
    st = state.cpu().numpy()
    assert st[0] == 1 and st[1] == float((moved <= tol * tol).all()) == 1.0 and st[2] == 12.5
    np.testing.assert_allclose(st[3], moved.max(), rtol=1e-15)
    before = cen.clone()
    device.kmeans_update(torch.from_numpy(stats * 2).cuda(), k, d, tol, cen, state)  # done: a no-op
    assert torch.equal(cen, before) and torch.equal(state.cpu(), torch.from_numpy(st))
    state.zero_()
    fresh = torch.from_numpy(np.concatenate([C.reshape(-1), 0.5 * (C * C).sum(axis=1)])).cuda()
    device.kmeans_update(torch.from_numpy(stats).cuda(), k, d, 1e-3, fresh, state)
    assert state.cpu().numpy()[1] == 0.0  # centre 0 moved 0.125 > tol^2


def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.normal(size=(33, 20000)).astype(np.float32)).cuda()
    C = rng.normal(size=(17, 33))
    assert torch.equal(device.kmeans_pass(X, None, C, K.STEP), device.kmeans_pass(X, None, C, K.STEP))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_device_fit_equals_host_loop(dtype):
    rng = np.random.default_rng(11)
    k, d, n = 5, 9, 3001
    X = (rng.normal(size=(k, d))[rng.integers(0, k, n)] * 4 + rng.normal(size=(n, d))).T.astype(np.float32)
    C0 = X[:, :k].T.astype(np.float64)
    Xh = torch.from_numpy(X).to(dtype)
    want = K.lloyd(Xh, None, C0, 20, 1e-4, "host")
    got = device.kmeans_fit(Xh.cuda(), None, C0, 20, 1e-4, K.DEVICE_BATCH)
    assert got["iterations"] == want.iterations and got["done"] == want.converged
    wa, _ = K.lloyd_pass_host(Xh, None, want.centers, K.ASSIGN)
    ga, _ = device.kmeans_pass(Xh.cuda(), None, got["centers"], K.ASSIGN)
    assert torch.equal(ga.cpu(), wa)
    S = np.stack([np.abs(X[:, wa.numpy() == c]).astype(np.float64).sum(axis=1) for c in range(k)])
    assert (np.abs(got["centers"] - want.centers) <= 1e-12 * S).all()


def test_validation_errors():
    X = torch.zeros(4, 10).cuda()
    with pytest.raises(ValueError, match="d <= 64"):
        device.kmeans_pass(torch.zeros(65, 10).cuda(), None, np.zeros((2, 65)), K.STEP)
    with pytest.raises(ValueError, match="k <= 64"):
        device.kmeans_pass(X, None, np.zeros((65, 4)), K.STEP)
    with pytest.raises(ValueError):
        device.kmeans_pass(X, None, np.zeros((1, 4)), K.STEP)
    with pytest.raises(ValueError, match="f32 / f64"):
        device.kmeans_pass(X.to(torch.bfloat16), None, np.zeros((2, 4)), K.STEP)
    with pytest.raises(ValueError, match="centers"):
        device.kmeans_pass(X, None, np.zeros((2, 5)), K.STEP)
