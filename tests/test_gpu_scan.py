"""The device prefix scans of ``scan.h``: the row walker under every operator it runs with
(``scan_rows``), the block-count scan (``scan_counts``), and its two largest users past one walker
trip (``compact_indices``, ``sort_permutation``).  Every comparison is integer or bit equality."""
import numpy as np
import pytest
import torch

import _sort_cases as sc
from net.jgp.labs.sparkdq4ml_amd.ops import device, kernels, native
from net.jgp.labs.sparkdq4ml_amd.ops.window import _seg_cummin

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = 3
# the wave edge, the block edge (256 threads), the block edge at 4 entries per thread, several trips
LENS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
I64_ADD, U32_ADD4, BND_FWD, BND_BWD, SEG = range(5)


def _scan_rows(kind, a: np.ndarray, length: int) -> np.ndarray:
    """``a``: the ``[ROWS][...]`` array in its device layout, any 4- or 8-byte integer dtype."""
    t = torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).to(DEV)
    native.hip().scan_rows(kind, t.data_ptr(), ROWS, length, torch.cuda.current_stream().cuda_stream)
    return t.cpu().numpy().view(a.dtype)


def _exclusive(inclusive: np.ndarray, identity) -> np.ndarray:
    """The inclusive scan along axis 1 shifted by one position, the identity in front."""
    out = np.empty_like(inclusive)
    out[:, :1] = identity
    out[:, 1:] = inclusive[:, :-1]
    return out


@pytest.mark.parametrize("length", LENS)
def test_rows_i64_add_wraps(length):
    rng = np.random.default_rng(length)
    a = rng.integers(1 << 61, 1 << 62, (ROWS, length), dtype=np.int64) * rng.choice(np.array([-1, 1, 1]), (ROWS, length))
    want = _exclusive(np.cumsum(a, axis=1, dtype=np.int64), 0)  # (int64 sums wrap)
    if length >= 63:
        assert (np.abs(np.cumsum(a.astype(np.float64), axis=1)) > 2.0 ** 63).any(), "the sums were meant to wrap"
    assert np.array_equal(_scan_rows(I64_ADD, a, length), want)


@pytest.mark.parametrize("length", LENS)
def test_rows_u32_add_four_per_thread(length):
    rng = np.random.default_rng(100 + length)
    pitch = (length + 3) // 4 * 4
    a = rng.integers(0, 1 << 32, (ROWS, pitch), dtype=np.uint64).astype(np.uint32)  # the padding holds anything
    want = _exclusive(np.cumsum(a[:, :length], axis=1, dtype=np.uint32), 0)
    assert np.array_equal(_scan_rows(U32_ADD4, a, length)[:, :length], want)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("length", LENS)
def test_rows_bounds(length, backward):
    rng = np.random.default_rng(200 + length)
    x = rng.integers(0, 1 << 32, (ROWS, length, 4), dtype=np.uint64).astype(np.uint32)
    x[..., 3] = 0
    got = _scan_rows(BND_BWD if backward else BND_FWD, x, length)
    if backward:
        assert np.array_equal(got[..., 0], _exclusive(np.minimum.accumulate(x[..., 0], axis=1), 0xFFFFFFFF))
        assert np.array_equal(got[..., 1], _exclusive(np.minimum.accumulate(x[..., 1], axis=1), 0xFFFFFFFF))
        assert not got[..., 2].any()  # the backward triple carries no count
    else:
        assert np.array_equal(got[..., 0], _exclusive(np.maximum.accumulate(x[..., 0], axis=1), 0))
        assert np.array_equal(got[..., 1], _exclusive(np.maximum.accumulate(x[..., 1], axis=1), 0))
        assert np.array_equal(got[..., 2], _exclusive(np.cumsum(x[..., 2], axis=1, dtype=np.uint32), 0))
    assert not got[..., 3].any()


@pytest.mark.parametrize("length", LENS)
def test_rows_segmented_min(length):
    rng = np.random.default_rng(300 + length)
    key = rng.integers(0, 1 << 64, (ROWS, length), dtype=np.uint64)
    key[:, ::3] >>= np.uint64(50)  # small keys too, so that a restart shows
    flag = np.stack([rng.random(length) < 0.05, np.zeros(length, dtype=bool), np.ones(length, dtype=bool)])
    x = np.stack([key, flag.astype(np.uint64)], axis=2)  # (u64 key, u32 flag, u32 0)
    got = _scan_rows(SEG, x, length)
    if length:
        incl = np.stack([_seg_cummin(key[r], flag[r]) for r in range(ROWS)])
        assert np.array_equal(got[..., 0], _exclusive(incl, np.uint64(0xFFFFFFFFFFFFFFFF)))
        assert np.array_equal(got[..., 1], _exclusive((np.cumsum(flag, axis=1) > 0).astype(np.uint64), 0))


@pytest.mark.parametrize("nb", [0, 1, 4095, 4096, 4097, 3 * 4096 + 5])
def test_scan_counts(nb):
    rng = np.random.default_rng(400 + nb)
    c = rng.integers(0, 16384, nb + 1, dtype=np.int64, endpoint=True)  # ([nb] holds anything)
    got = device.scan_counts(torch.from_numpy(c).to(DEV)).cpu().numpy()
    incl = np.cumsum(c[:nb])
    assert np.array_equal(got[:nb], incl - c[:nb])
    assert got[nb] == (incl[-1] if nb else 0)


def test_compact_indices_past_one_trip_of_blocks():
    n = 4097 * 4096  # 4097 block counts: one more than a trip of the counts scan
    g = torch.Generator(device=DEV).manual_seed(5)
    sel = torch.rand(n, generator=g, device=DEV) > 0.5
    got = device.compact_indices(sel)
    assert np.array_equal(got.cpu().numpy(), np.nonzero(sel.cpu().numpy())[0])


def test_sort_past_one_trip_of_tiles():
    m = (4 * sc.THREADS + 1) * sc.TILE + 3  # live rows: one tile more than a trip of the tile-count scan
    rng = np.random.default_rng(6)
    n = m + m // 8
    sel = np.zeros(n, dtype=bool)
    sel[rng.permutation(n)[:m]] = True
    frame = ([sc.pattern_column("random64", n, "i32", 6)], [torch.from_numpy(rng.random(n) >= 0.1)], torch.from_numpy(sel))
    want = sc.run(frame)  # the host engine
    got = sc.run(sc.to_device(frame, DEV))
    assert got.is_cuda and int(got.numel()) == m
    assert torch.equal(got.cpu(), want)
