"""The decision-tree kernels (csrc/hip/tree.hip) against their fp64 twins (ops/tree.py).

Bins, histogram words and routing are integers: bit for bit, for any grid.  The split search: the
test asserts through the twin that the two largest gains of every node differ by more than 1e-9 of
the parent impurity, then the chosen (feature, split), the counts and the leaf flags are equal and
gain, impurities and predictions lie within 1e-12 of the parent's sum y^2 / n (of 1 for gini /
entropy), the project's bound for f64 row reductions (tests/test_gpu_rowops.py).  Integer labels
under variance and gini are bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, tree as T  # noqa: E402

TRIPS = 256 * 3 + 7
NS = ((1, None), (63, None), (64, None), (65, None), (TRIPS, 1), (TRIPS, 3))
NSPLIT = 256 * 40 + 7  # the split search is checked here: enough rows that no bin of a node is empty at the top
# (kind, impurity, d, bins, open nodes): the last two regression shapes hold 7 nodes per LDS group
LEVELS = [(T.REG, T.VARIANCE, 1, 2, 1), (T.REG, T.VARIANCE, 5, 32, 3), (T.REG, T.VARIANCE, 1, 256, 3),
          (T.REG, T.VARIANCE, 64, 2, 3), (T.REG, T.VARIANCE, 64, 2, 17), (T.CLS, T.GINI, 1, 2, 1),
          (T.CLS, T.ENTROPY, 5, 32, 3), (T.CLS, T.GINI, 64, 32, 3), (T.CLS, T.ENTROPY, 5, 256, 1), (T.CLS, T.GINI, 64, 32, 9)]


def _case(d, bins, n, seed, integer=False):
    """Features (dead rows hold NaN), selection, thresholds with ``bins - 1`` splits in feature 0."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-40, 41, (d, n)).astype(np.float64) if integer else rng.uniform(-1, 1, (d, n)).astype(np.float32).astype(np.float64)
    live = rng.random(n) < 0.85
    live[0] = True
    k = [bins - 1 - (f % 3 if bins > 4 else 0) for f in range(d)]  # feature 0 has every split, others up to two fewer
    cuts = [np.sort(rng.choice(np.arange(-39, 40) + 0.5, k[f], replace=False)) if integer
            else np.linspace(-1, 1, k[f] + 2)[1:-1] + rng.uniform(-1e-3, 1e-3) for f in range(d)]
    thr, ns = T.pack_splits(cuts)
    return np.where(live[None, :], X, np.nan), live, thr, ns


def _dev(X, dtype, pad):
    t = torch.from_numpy(X).to(dtype)
    if pad:
        t = torch.cat([t, torch.full((t.shape[0], pad), float("nan"), dtype=dtype)], dim=1)
    return t.cuda()[:, :X.shape[1]]


@pytest.mark.parametrize("bins", [2, 32, 256])
@pytest.mark.parametrize("d", [1, 5, 64])
def test_bins_equal_twin(d, bins):
    for n, blocks in NS:
        Xn, live, thr, ns = _case(d, bins, n, 100 * d + bins + n)
        Xn[:, live] = np.where(np.arange(live.sum())[None, :] % 7 == 0, thr[:, :1], Xn[:, live])  # x == t goes left
        want, flag = T.bin_host(torch.from_numpy(Xn), torch.from_numpy(live), thr, ns)
        assert not bool(flag)
        for dtype in (torch.float32, torch.float64):
            w = want if dtype == torch.float64 else T.bin_host(torch.from_numpy(Xn).to(dtype), torch.from_numpy(live), thr, ns)[0]
            got, gflag = device.tree_bin(_dev(Xn, dtype, 11 if n == 65 else 0), torch.from_numpy(live).cuda(), thr, ns, blocks)
            assert torch.equal(got.cpu(), w) and int(gflag) == 0
    Xn[3 % d, 0] = np.nan  # a NaN in a live row
    assert int(device.tree_bin(torch.from_numpy(Xn).cuda(), torch.from_numpy(live).cuda(), thr, ns)[1]) != 0


def _check_split(got, want, gains, kind, scale):
    top = np.sort(gains.reshape(gains.shape[0], -1), axis=1)[:, -2:]
    assert (~np.isfinite(top[:, 0]) | (top[:, 1] - top[:, 0] > 1e-9 * want[:, 3])).all()  # the input: no near-ties
    for cols in ((0, 1, 4, 6, 7, 10, 11, 12), tuple(range(16, 64))):
        np.testing.assert_array_equal(got[:, cols], want[:, cols])
    real = (2, 3, 5, 8, 9, 13, 14)
    assert (np.abs(got[:, real] - want[:, real]) <= 1e-12 * scale[:, None]).all(), np.abs(got - want).max()


@pytest.mark.parametrize("kind,impurity,d,bins,nodes", LEVELS)
def test_level_equals_twin(kind, impurity, d, bins, nodes):
    for n, blocks in NS + ((NSPLIT, None),):
        rng = np.random.default_rng(7 * d + bins + n + nodes)
        Xn, live, thr, ns = _case(d, bins, n, 3 * d + bins + n)
        classes = 5 if kind == T.CLS else 0
        y = rng.integers(0, 5, n).astype(np.float64) if kind == T.CLS else rng.normal(size=n) * 3.0 + 1.0
        e = int(np.frexp(np.abs(y).max())[1])
        node = np.where(live, rng.integers(-1, nodes, n), -1).astype(np.int32)
        nb = int(ns.max()) + 1
        for dtype in (torch.float32, torch.float64):
            B = device.tree_bin(_dev(Xn, dtype, 0), torch.from_numpy(live).cuda(), thr, ns)[0]
            yd, nd = torch.from_numpy(y).to(dtype).cuda(), torch.from_numpy(node).cuda()
            want = T.hist_host(B.cpu(), node, yd.cpu(), kind, nodes, d, nb, classes, e)
            H = device.tree_hist(B, nd, yd, kind, nodes, d, nb, classes, e, blocks)
            assert torch.equal(H.cpu(), want)
            for again in (blocks, 3 if blocks == 1 else 1):  # the same grid once more, and another grid
                assert torch.equal(device.tree_hist(B, nd, yd, kind, nodes, d, nb, classes, e, again), H)
            if n == NSPLIT:
                wrec, gains = T.split_stats(want.numpy(), ns, kind, impurity, e, 2, 0.0, False, False, with_gains=True)
                scale = np.ones(nodes) if kind == T.CLS else np.array(
                    [(yd.cpu().double().numpy()[node == s] ** 2).mean() for s in range(nodes)])
                _check_split(device.tree_split(H, ns, kind, impurity, e, 2, 0.0, False, False).cpu().numpy(), wrec, gains, kind, scale)
            tab = np.stack([rng.integers(-1, d, nodes), rng.integers(0, nb, nodes), rng.integers(-1, 2 * nodes, nodes),
                            rng.integers(-1, 2 * nodes, nodes)], axis=1).astype(np.int32)
            assert torch.equal(device.tree_route(B, nd.clone(), tab, blocks).cpu(), T.route_host(B.cpu(), torch.from_numpy(node), tab))


@pytest.mark.parametrize("kind,impurity", [(T.REG, T.VARIANCE), (T.CLS, T.GINI)])
def test_integer_case_is_bit_exact(kind, impurity):
    d, bins, nodes, n = 17, 32, 3, TRIPS
    rng = np.random.default_rng(11)
    Xn, live, thr, ns = _case(d, bins, n, 5, integer=True)
    y = rng.integers(0, 9, n).astype(np.float64)
    node = np.where(live, rng.integers(0, nodes, n), -1).astype(np.int32)
    B = device.tree_bin(torch.from_numpy(Xn).cuda(), torch.from_numpy(live).cuda(), thr, ns)[0]
    H = device.tree_hist(B, torch.from_numpy(node).cuda(), torch.from_numpy(y).cuda(), kind, nodes, d, int(ns.max()) + 1, 9, 4)
    want = T.split_host(H.cpu(), ns, kind, impurity, 4, 1, 0.0, False, False)
    np.testing.assert_array_equal(device.tree_split(H, ns, kind, impurity, 4, 1, 0.0, False, False).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_predict_walk_equals_twin(dtype):
    rng = np.random.default_rng(3)
    Xn, live, _, _ = _case(5, 4, TRIPS, 9)
    feat, left, right = np.array([2, 0, -1, -1, 4, -1, -1]), np.array([1, 2, -1, -1, 5, -1, -1]), np.array([4, 3, -1, -1, 6, -1, -1])
    thr = rng.uniform(-0.5, 0.5, 7)
    Xn[:, live] = np.where(np.arange(live.sum())[None, :] % 5 == 0, thr[0], Xn[:, live])
    Xd = _dev(Xn, dtype, 9)
    want = T.predict_host(Xd.cpu(), torch.from_numpy(live), feat, thr, left, right)
    assert torch.equal(device.tree_predict(Xd, torch.from_numpy(live).cuda(), feat, thr, left, right, 3).cpu(), want)
    assert set(want.tolist()) == {-1, 2, 3, 5, 6}
