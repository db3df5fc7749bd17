"""The random-forest kernels (csrc/hip/forest.hip, and tree.hip's split search over feature subsets)
against their twins (ops/forest.py).

Bag words, histogram words and routing are integers, the prediction sums are added in the twin's
order: bit for bit, for any grid and any slot group.  The split search has test_gpu_tree.py's
precondition and bounds: the twin shows that the two largest gains of every slot differ by more than
1e-9 of the parent impurity, then the integer fields are equal and the real ones lie within 1e-12 of
the parent's sum y^2 / n (of 1 for gini / entropy); integer labels are bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, forest as F, tree as T  # noqa: E402

TRIPS = 256 * 3 + 7
NS = ((1, 1), (65, 1), (TRIPS, 1), (TRIPS, 3))  # (rows, blocks)
NSPLIT = 256 * 40 + 7
# (kind, d, m, bins, trees, slots per tree, group cap): m = 1; m = d = 64 with a group boundary inside
# tree 1; d = 5 with m = 2 at 256 bins, one group spanning three trees; 20 roots in one launch
LEVELS = [(T.CLS, 1, 1, 2, 1, 1, None), (T.REG, 64, 64, 2, 3, 2, 3), (T.CLS, 5, 2, 256, 3, 1, None),
          (T.CLS, 9, 3, 32, 20, 1, None), (T.REG, 5, 2, 32, 3, 3, 2)]


def _level(kind, d, m, bins, trees, spt, n, seed, rate=1.0, integer=False):
    """Bins (dead rows: zero bins, NaN label), bagged words spread over ``spt`` slots per tree (some
    rows in a leaf), labels, the slots' features."""
    rng = np.random.default_rng(seed)
    live = rng.random(n) < 0.85
    live[0] = True
    B = np.zeros((n, (d + 3) // 4 * 4), dtype=np.uint8)
    B[:, :d] = rng.integers(0, bins, (n, d)) * live[:, None]
    y = rng.integers(0, 5, n).astype(np.float64) if kind == T.CLS or integer else rng.normal(size=n) * 3.0 + 1.0
    e = int(np.frexp(np.abs(y).max())[1])
    y = np.where(live, y, np.nan)
    node = F.bag_host(n, 1000, torch.from_numpy(live), F.tree_seeds(seed, trees), F.bag_thresholds(max(trees, 2), rate)).numpy()
    slot = spt * (node & F.SLOT_MASK) + rng.integers(0, spt, node.shape)
    node = np.where((node >= 0) & (rng.random(node.shape) < 0.9), (node & ~F.SLOT_MASK) | slot, -1).astype(np.int32)
    feats = np.stack([F.node_subset(seed, t, 1 + s, d, m) for t in range(trees) for s in range(spt)])
    return B, node, y, e, feats, np.repeat(np.arange(trees), spt)


@pytest.mark.parametrize("trees,rate", [(1, 1.0), (3, 1.0), (20, 1.0), (1, 0.3), (20, 0.3)])
def test_bag_equals_twin(trees, rate):
    for n, blocks in NS:
        live = np.random.default_rng(n + trees).random(n) < 0.85
        seeds, thr = F.tree_seeds(9, trees), F.bag_thresholds(trees, rate)
        want = F.bag_host(n, 12345, torch.from_numpy(live), seeds, thr)
        got = device.forest_bag(n, 12345, torch.from_numpy(live).cuda(), seeds, thr, "cuda", blocks)
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("kind,d,m,bins,trees,spt,group", LEVELS)
def test_hist_and_route_equal_twin(kind, d, m, bins, trees, spt, group):
    classes = 5 if kind == T.CLS else 0
    for n, blocks in NS:
        B, node, y, e, feats, slot_tree = _level(kind, d, m, bins, trees, spt, n, 7 * d + bins + n + trees)
        masks = [F._mask(f) for f in feats]
        if n == TRIPS:
            assert (node >> F.COUNT_SHIFT).max() >= 3 or trees == 1
        Bd, nd = torch.from_numpy(B).cuda(), torch.from_numpy(node).cuda()
        for dtype in (torch.float32, torch.float64):
            yd = torch.from_numpy(y).to(dtype).cuda()
            want = F.hist_host(B, node, yd.cpu(), kind, d, m, bins, classes, e, masks)
            H = device.forest_hist(Bd, nd, yd, kind, d, m, bins, classes, e, masks, slot_tree, blocks, group)
            assert torch.equal(H.cpu(), want)
            other = device.forest_hist(Bd, nd, yd, kind, d, m, bins, classes, e, masks, slot_tree, 3 if blocks == 1 else 1, 1)
            assert torch.equal(other, H)  # another grid, and one slot per group
        rng = np.random.default_rng(n)
        k = len(masks)
        tab = np.stack([rng.integers(-1, d, k), rng.integers(0, bins, k), rng.integers(-1, 2 * k, k),
                        rng.integers(-1, 2 * k, k)], axis=1).astype(np.int32)
        got = device.forest_route(Bd, nd.clone(), tab, blocks).cpu()
        want = F.route_host(torch.from_numpy(B), torch.from_numpy(node), tab)
        assert torch.equal(got, want) and ((want >= 0) <= (want >> F.COUNT_SHIFT == torch.from_numpy(node) >> F.COUNT_SHIFT)).all()


@pytest.mark.parametrize("kind", [T.REG, T.CLS])
def test_full_masks_give_the_tree_words(kind):
    d, bins, n = 7, 32, TRIPS
    B, node, y, e, feats, slot_tree = _level(kind, d, d, bins, 1, 3, n, 4)
    node = np.where(node >= 0, (1 << F.COUNT_SHIFT) | (node & F.SLOT_MASK), -1).astype(np.int32)  # c = 1
    Bd, yd = torch.from_numpy(B).cuda(), torch.from_numpy(y).cuda()
    H = device.forest_hist(Bd, torch.from_numpy(node).cuda(), yd, kind, d, d, bins, 5, e, [F._mask(f) for f in feats], slot_tree)
    slots = torch.from_numpy(np.where(node[0] >= 0, node[0] & F.SLOT_MASK, -1).astype(np.int32)).cuda()
    assert torch.equal(H, device.tree_hist(Bd, slots, yd, kind, 3, d, bins, 5, e))


def _split_case(kind, integer):
    d, m, bins, trees, spt = 9, 3, 32, 2, 2
    B, node, y, e, feats, _ = _level(kind, d, m, bins, trees, spt, NSPLIT, 21 + kind, integer=integer)
    if not integer:
        y = y + 0.5 * B[:, 4] * (kind == T.REG)  # a signal, so that gains are not all noise
    nsplit = np.array([bins - 1 - f % 3 for f in range(d)], dtype=np.int32)
    H = F.hist_host(B, node, y, kind, d, m, bins, 5, e + 3, [F._mask(f) for f in feats])
    scale = np.ones(trees * spt) if kind == T.CLS else np.array(
        [np.repeat(y, np.where((node[s // spt] >= 0) & ((node[s // spt] & F.SLOT_MASK) == s), node[s // spt] >> F.COUNT_SHIFT, 0)).__pow__(2).mean()
         for s in range(trees * spt)])
    return H, feats, nsplit, e + 3, scale


@pytest.mark.parametrize("kind,impurity", [(T.REG, T.VARIANCE), (T.CLS, T.GINI), (T.CLS, T.ENTROPY)])
def test_split_over_subsets_equals_twin(kind, impurity):
    H, feats, nsplit, e, scale = _split_case(kind, False)
    want, gains = F.split_host(H, feats, nsplit, kind, impurity, e, 2, 0.0, False, False, with_gains=True)
    top = np.sort(gains.reshape(gains.shape[0], -1), axis=1)[:, -2:]
    assert (np.isfinite(top[:, 0]) & (top[:, 1] - top[:, 0] > 1e-9 * want[:, 3])).all()  # the input: no near-ties
    got = device.forest_split(H.cuda(), feats, nsplit, kind, impurity, e, 2, 0.0, False, False).cpu().numpy()
    assert all(r[0] in fs for r, fs in zip(got, feats))
    for cols in ((0, 1, 4, 6, 7, 10, 11, 12), tuple(range(16, 64))):
        np.testing.assert_array_equal(got[:, cols], want[:, cols])
    real = (2, 3, 5, 8, 9, 13, 14)
    assert (np.abs(got[:, real] - want[:, real]) <= 1e-12 * scale[:, None]).all(), np.abs(got - want).max()


@pytest.mark.parametrize("kind,impurity", [(T.REG, T.VARIANCE), (T.CLS, T.GINI)])
def test_split_of_integer_labels_is_bit_exact(kind, impurity):
    H, feats, nsplit, e, _ = _split_case(kind, True)
    want = F.split_host(H, feats, nsplit, kind, impurity, e, 1, 0.0, False, False)
    np.testing.assert_array_equal(device.forest_split(H.cuda(), feats, nsplit, kind, impurity, e, 1, 0.0, False, False).cpu().numpy(), want)


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_predict_sums_equal_twin(dtype, C):
    rng = np.random.default_rng(3 + C)
    n, d = TRIPS, 5
    live = rng.random(n) < 0.85
    X = torch.from_numpy(np.where(live[None, :], rng.uniform(-1, 1, (d, n)), np.nan)).to(dtype)
    Xd = torch.cat([X, torch.full((d, 9), float("nan"), dtype=dtype)], dim=1).cuda()[:, :n]  # a padded ld
    feat, left, right = np.array([2, 0, -1, -1, 4, -1, -1]), np.array([1, 2, -1, -1, 5, -1, -1]), np.array([4, 3, -1, -1, 6, -1, -1])
    trees = 3  # the same shape three times over, each with its own thresholds and values
    tabs = (np.tile(feat, trees), rng.uniform(-0.5, 0.5, 7 * trees),
            np.concatenate([np.where(left >= 0, left + 7 * t, -1) for t in range(trees)]),
            np.concatenate([np.where(right >= 0, right + 7 * t, -1) for t in range(trees)]), np.arange(trees) * 7,
            rng.uniform(0, 1, (7 * trees, C)) * 10.0 ** rng.integers(-9, 3, (7 * trees, 1)))
    want = F.predict_host(X, torch.from_numpy(live), *tabs)
    got = device.forest_predict(Xd, torch.from_numpy(live).cuda(), *tabs, 3).cpu()
    assert got.shape == (C, n) and torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want[:, ~live]).all())
    assert torch.equal(got[:, live], want[:, live])
