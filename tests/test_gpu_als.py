"""The fused ALS half-step (csrc/hip/als.hip) against extended-precision normal equations and its
fp64 twin: every band width, both storages, the one-chunk and the slab path, a 2-block grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import als as A, kernels  # noqa: E402
from test_als_host import C, residual_ratio, table  # noqa: E402

# 1, 10, 62, 64 and both sides of every band edge: the band [y | r | 1] has rank + 2 columns, so a
# 16-wide tile is added at ranks 15, 31, 47 and 63
RANKS = (1, 10, 14, 15, 30, 31, 46, 47, 62, 63, 64)


def cuda(*ts):
    return tuple(t.cuda() for t in ts)


@pytest.mark.parametrize("reg", (0.1, 1e-6))
@pytest.mark.parametrize("rank", RANKS)
def test_half_step_meets_the_bound(rank, reg):
    off, src, rating, Y = table(rank)  # segments of 0, 1, 3, 4, 5, C - 1, C, C + 1 and 3 C + 7 ratings
    d = cuda(off, src, rating)
    X64, status = kernels.als_half_step(*d, Y.double().cuda(), reg)
    ratio = residual_ratio(off, src, rating, Y, reg, X64.cpu().numpy()) / 1e-12
    twin, _ = A.als_half_step_host(off, src, rating, Y, reg, np.float64)
    print("device residual / bound", rank, reg, ratio, "device - twin", np.abs(X64.cpu().numpy() - twin).max())
    assert status.tolist() == [0, 0] and ratio <= 1.0
    # f32 storage: the same arithmetic, each solution rounded once at its store
    X32, status = kernels.als_half_step(*d, Y.cuda(), reg)
    assert status.tolist() == [0, 0] and X32.dtype == torch.float32 and torch.equal(X32, X64.float())
    # any grid, any run: the same bits
    for blocks in (2, None):
        again, _ = kernels.als_half_step(*d, Y.double().cuda(), reg, blocks=blocks)
        assert torch.equal(again, X64)


@pytest.mark.parametrize("rank", (3, 15, 64))
def test_slab_path_equals_the_one_chunk_path(rank):
    """Dyadic factors and integer ratings: every pre-solve sum is exact, whatever its order."""
    rng = np.random.default_rng(rank)
    lengths = (200, 0, 192, 193, 3 * C + 7, 300)  # each of far more than 64 distinct sources: full rank
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    src = torch.from_numpy(rng.integers(0, 400, int(off[-1])).astype(np.int32))
    rating = torch.from_numpy(rng.integers(1, 6, int(off[-1])).astype(np.float64))
    Y = torch.from_numpy(rng.integers(-8, 9, (400, rank)) / 8.0)
    _, _, want = A.als_half_step_host(off, src, rating, Y, 0.0, np.float64, presolve=True)
    d = cuda(off, src, rating, Y)
    Xs, ss, slab = kernels.als_half_step(*d, 0.0, chunk=64, presolve=True)       # 3 to 97 chunks per segment
    Xo, so, one = kernels.als_half_step(*d, 0.0, chunk=8192, presolve=True)      # one chunk each
    assert torch.equal(slab, one) and np.array_equal(one.cpu().numpy(), want)
    assert ss.tolist() == so.tolist() == [0, 0] and torch.equal(Xs, Xo) and not Xs[1].any()


def test_rank_deficient_segment_is_counted_and_poisons_nothing_else():
    off, src, rating, Y = table(3, lengths=(40, 1, 40), dtype=np.float64)
    Y[int(src[40])] = torch.tensor([0.5, 0.25, 1.0])  # y y^T: the second pivot is exactly 0
    X, status = kernels.als_half_step(*cuda(off, src, rating, Y), 0.0)
    X = X.cpu().numpy()
    assert status.tolist() == [1, 0] and np.isnan(X[1]).all() and np.isfinite(X[[0, 2]]).all()
    one = torch.tensor([0, 40])
    assert residual_ratio(one, src, rating, Y, 0.0, X[:1]) <= 1e-12
    assert residual_ratio(one, src[41:], rating[41:], Y, 0.0, X[2:]) <= 1e-12


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_predict(dtype):
    rng = np.random.default_rng(5)
    U, V = (torch.from_numpy(rng.normal(size=(n, 33))).to(dtype) for n in (40, 50))
    u = torch.from_numpy(rng.integers(-1, 40, 1000).astype(np.int32))
    v = torch.from_numpy(rng.integers(-1, 50, 1000).astype(np.int32))
    sel = torch.from_numpy(rng.random(1000) < 0.9)
    got = kernels.als_predict(*cuda(u, v, sel, U, V)).cpu()
    want = kernels.als_predict(u, v, sel, U, V)
    dead = (u < 0) | (v < 0) | ~sel
    assert torch.equal(torch.isnan(got), dead) and torch.equal(torch.isnan(want), dead)
    scale = (U.double()[u.long().clamp(min=0)] * V.double()[v.long().clamp(min=0)]).abs().sum(1)
    assert ((got - want).abs()[~dead] <= 1e-12 * scale[~dead]).all()


def test_validation_errors():
    off, src, rating, Y = cuda(*table(4, lengths=(3, 5)))
    bad = [((off, src, rating, torch.zeros(300, 65).cuda(), 0.1), {}), ((off, src, rating, Y, 0.1), dict(chunk=100)),
           ((off, src, rating, Y, -1.0), {}), ((off, src, rating, Y, 0.1), dict(blocks=0)),
           ((off, src + 300, rating, Y, 0.1), {}), ((off.flip(0), src, rating, Y, 0.1), {}),
           ((off, src.long(), rating, Y, 0.1), {}), ((off, src, rating.float(), Y, 0.1), {}),
           ((off, src, rating, Y.cpu().cuda().half(), 0.1), {}), ((off, src.cpu(), rating, Y, 0.1), {})]
    for args, kw in bad:
        with pytest.raises((ValueError, TypeError)):
            kernels.als_half_step(*args, **kw)
    with pytest.raises(ValueError):
        kernels.als_predict(src[:2], src[:2] + 1000, None, Y, Y)
    with pytest.raises(ValueError, match="rank"):
        A.route(Y, 65)
    assert A.route(Y, 64) == "fused" and A.route(Y.cpu(), 65) == "host"
