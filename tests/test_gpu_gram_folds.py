"""The one-pass fold-partitioned Gram kernel (``gram_folds.hip``) and ``fold_ids_kernel`` against
the host implementations (``ops.kernels``: fp64 torch statistics over the numpy fold ids)."""
import functools

import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import kernels

pytestmark = pytest.mark.gpu

N = 2373  # 37 whole granules and a 5-row tail granule
DEAD = 100  # the dead row that carries NaN features (with a selection)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _host_data(n, d, xdt):
    g = torch.Generator().manual_seed(1000 * d + n % 997)
    X = (torch.randn(d, n, generator=g, dtype=torch.float64) * 2 + 0.5).to(xdt)
    y = torch.randn(n, generator=g, dtype=torch.float64) * 3 - 1
    sel = torch.rand(n, generator=g) > 0.3
    if n > DEAD:
        sel[DEAD] = False
    return X, y, sel


@functools.lru_cache(maxsize=None)
def _oracle(n, d, xdt, k, with_sel, seed=42):
    X, y, sel = _host_data(n, d, xdt)
    return kernels.gram_stats_folds(X, y, sel if with_sel else None, k, seed, 64)


def _check(out, ref):
    assert out.shape == ref.shape and out.dtype == torch.float64
    out = out.cpu()
    assert not torch.isnan(out).any()
    for f in range(ref.shape[0]):
        assert float(out[f, 0]) == float(ref[f, 0])  # count: exact
        if float(ref[f, 0]) == 0:
            assert float(out[f].abs().max()) == 0.0
        else:
            assert _rel(out[f], ref[f]) < 1e-12


@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("xdt", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [1, 9, 16, 17, 33, 64])
def test_onepass_matches_oracle(d, xdt, k, with_sel):
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    X, y, sel = _host_data(N, d, xdt)
    Xg = X.cuda()
    if with_sel:
        Xg[:, DEAD] = float("nan")  # a dead row's features never enter a product
    out = device.gram_stats_folds(Xg, y.cuda(), sel.cuda() if with_sel else None, k, 42, 64, "fp64", route="onepass")
    _check(out, _oracle(N, d, xdt, k, with_sel))


@pytest.mark.parametrize("n", [63, 64])
def test_single_granule(n):
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    X, y, _ = _host_data(n, 17, torch.float32)
    out = device.gram_stats_folds(X.cuda(), y.cuda(), None, 3, 42, 64, "fp64", route="onepass").cpu()
    ref = _oracle(n, 17, torch.float32, 3, False)
    _check(out, ref)
    # granule 0 under seed 42 falls in fold 2: the other folds' vectors are exactly zero
    assert float(out[2, 0]) == n
    assert float(out[0].abs().max()) == 0.0 and float(out[1].abs().max()) == 0.0


@pytest.mark.parametrize("blocks", [3, 2048])
def test_blocks_below_and_above_granule_count(blocks):
    """262_337 rows = 4099 granules: 3 blocks give every wave a long range; 2048 blocks (8192
    waves) leave one granule to some waves and none to most blocks, so whole slabs are zeros."""
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    n, d, k = 262_337, 17, 5
    X, y, sel = _host_data(n, d, torch.float32)
    out = device.gram_stats_folds(X.cuda(), y.cuda(), sel.cuda(), k, -7, 64, "fp64", route="onepass", blocks=blocks)
    _check(out, _oracle(n, d, torch.float32, k, True, seed=-7))


@pytest.mark.parametrize("d", [9, 40])
def test_consistency_with_plain_and_masked(d):
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    X, y, sel = (t.cuda() for t in _host_data(20_011, d, torch.float32))
    one = device.gram_stats_folds(X, y, sel, 5, 42, 64, "fp64", route="onepass")
    again = device.gram_stats_folds(X, y, sel, 5, 42, 64, "fp64", route="onepass")
    assert torch.equal(one, again)  # no atomics: bit-identical
    plain = device.gram_stats(X, y, None, sel, "fp64")
    assert float(one[:, 0].sum()) == float(plain[0])
    assert _rel(one.sum(0), plain) < 1e-12
    masked = device.gram_stats_folds(X, y, sel, 5, 42, 64, "fp64", route="masked")
    assert torch.equal(one[:, 0], masked[:, 0])
    for f in range(5):
        assert _rel(one[f], masked[f]) < 1e-12
    auto = device.gram_stats_folds(X, y, sel, 5, 42, 64, "fp64")
    want = one if device.ONEPASS_MIN_D <= d <= device.ONEPASS_MAX_D else masked
    assert torch.equal(auto, want)
    assert kernels.folds_route(X, 64, "fp64") == ("onepass" if want is one else "masked")
    assert kernels.folds_route(X, 1, "fp64") == "masked" and kernels.folds_route(X, 64, "bf16") == "masked"


def test_weighted_classes_onepass():
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    X, y, sel = _host_data(20_011, 33, torch.float64)
    out = device.gram_stats_folds(X.cuda(), y.cuda(), sel.cuda(), [0.75, 0.25], 11, 64, "fp64", route="onepass")
    _check(out, kernels.gram_stats_folds(X, y, sel, [0.75, 0.25], 11, 64))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("granule", [1, 64])
def test_fold_ids_kernel(n, granule):
    for classes, seed in ((3, 42), (16, -7), ([3, 1], 42), ([1, 1, 2], (1 << 63) + 12345)):
        dev = kernels.fold_ids(n, classes, seed, granule, "cuda")
        assert dev.is_cuda and dev.dtype == torch.uint8
        host = kernels.fold_ids(n, classes, seed, granule)
        assert np.array_equal(dev.cpu().numpy(), host.numpy())
