"""The fold rule (ops/kernels.py: fold_hash / fold_thresholds / fold_ids) and the host
fold-partitioned statistics, the oracle of the gram_folds kernel tests."""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import kernels

# S = 42, granules 0..7 (numpy uint64 evaluation of the rule written in docs/DESIGN.md)
PINNED_U = [0xBDD73226, 0x28EFE333, 0x47526757, 0x581CE1FF, 0x09BC585A, 0xDE4431FA, 0x37E9671C, 0xCCF635EE]
PINNED_FOLDS_K3 = [2, 0, 0, 1, 0, 2, 0, 2]


def test_pinned_hash_vector():
    u = kernels.fold_hash(42, np.arange(8, dtype=np.uint64))
    assert u.dtype == np.uint32
    assert [int(v) for v in u] == PINNED_U


def test_equal_fold_thresholds():
    assert [int(t) for t in kernels.fold_thresholds(3)] == [1431655765, 2863311530]
    assert kernels.fold_thresholds(1).size == 0
    assert [int(t) for t in kernels.fold_thresholds(16)] == [(j << 32) // 16 for j in range(1, 16)]
    with pytest.raises(ValueError):
        kernels.fold_thresholds(17)


def test_weight_thresholds():
    t = kernels.fold_thresholds([3, 1])
    assert [int(v) for v in t] == [3 << 30]
    t = kernels.fold_thresholds([0.75, 0.25])
    assert [int(v) for v in t] == [3 << 30]
    assert [int(v) for v in kernels.fold_thresholds([1, 1, 2])] == [1 << 30, 1 << 31]
    with pytest.raises(ValueError):
        kernels.fold_thresholds([1, -1])
    with pytest.raises(ValueError):
        kernels.fold_thresholds([0, 0])


def test_pinned_folds_granule_1_and_64():
    ids = kernels.fold_ids(8, 3, 42, 1)
    assert ids.dtype == torch.uint8 and ids.tolist() == PINNED_FOLDS_K3
    n = 8 * 64 - 5  # a 59-row tail granule
    ids64 = kernels.fold_ids(n, 3, 42, 64)
    assert ids64.shape == (n,)
    want = np.repeat(np.array(PINNED_FOLDS_K3, dtype=np.uint8), 64)[:n]
    assert np.array_equal(ids64.numpy(), want)


def test_negative_seed_is_its_value_mod_2_64():
    assert kernels.fold_seed(-1, rank=0) == (1 << 64) - 1
    assert kernels.fold_seed(-7, rank=0) == (1 << 64) - 7
    a = kernels.fold_ids_host(1000, 5, kernels.fold_seed(-7, rank=0), 1)
    b = kernels.fold_ids_host(1000, 5, (1 << 64) - 7, 1)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, kernels.fold_ids_host(1000, 5, 7, 1))


def test_rank_mixes_the_seed():
    assert kernels.fold_seed(42, rank=0) == 42
    assert kernels.fold_seed(42, rank=1) == 42 ^ 0xD1B54A32D192ED03
    assert kernels.fold_seed(42, rank=3) == 42 ^ ((3 * 0xD1B54A32D192ED03) % (1 << 64))


def test_fold_ids_cover_every_class_evenly():
    ids = kernels.fold_ids(200_000, 5, 1, 1).numpy()
    cnt = np.bincount(ids, minlength=5)
    assert cnt.sum() == 200_000 and np.all(np.abs(cnt - 40_000) < 5 * np.sqrt(40_000 * 0.8))
    w = kernels.fold_ids(200_000, [3, 1], 1, 1).numpy()
    assert abs(int((w == 0).sum()) - 150_000) < 5 * np.sqrt(200_000 * 0.75 * 0.25)
    assert set(np.unique(w)) == {0, 1}


def _data(n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(d, n, generator=g, dtype=torch.float64)
    y = torch.linspace(-1, 1, d, dtype=torch.float64) @ X + 5.0 + torch.randn(n, generator=g, dtype=torch.float64)
    return X, y


@pytest.mark.parametrize("granule", [1, 64])
@pytest.mark.parametrize("with_sel", [False, True])
def test_host_fold_statistics(granule, with_sel):
    n, d, k = 2373, 12, 3
    X, y = _data(n, d)
    sel = None
    if with_sel:
        sel = torch.rand(n, generator=torch.Generator().manual_seed(1)) < 0.8
        dead = int(torch.nonzero(~sel)[0])
        X[:, dead] = float("nan")  # a dead row's features never enter a product
    S = kernels.gram_stats_folds(X, y, sel, k, 42, granule)
    assert S.shape == (k, kernels.gram_layout_size(d)) and S.dtype == torch.float64
    assert not torch.isnan(S).any()
    Xz = X if sel is None else torch.where(sel.unsqueeze(0), X, torch.zeros_like(X))
    total = kernels.gram_stats(Xz, y, None, sel)
    np.testing.assert_allclose(S.sum(0).numpy(), total.numpy(), rtol=1e-12, atol=0)
    ids = kernels.fold_ids(n, k, 42, granule)
    for f in range(k):
        m = ids == f
        if sel is not None:
            m = m & sel
        ref = kernels.gram_stats(Xz, y, None, m)
        assert float(S[f, 0]) == float(m.sum())
        np.testing.assert_allclose(S[f].numpy(), ref.numpy(), rtol=1e-12, atol=0)
