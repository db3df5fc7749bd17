"""The ``sort.hip`` kernels against the numpy twin and against the plain-Python oracle: the same
permutation, for every ``blocks`` override (a stable sort has one right answer, so every check is
``torch.equal``)."""
import pytest
import torch

import _sort_cases as sc
from net.jgp.labs.sparkdq4ml_amd.ops import kernels, native

pytestmark = pytest.mark.gpu

T = sc.TILE
DEV = "cuda"
BLOCKS = (None, 1, 8)  # one block walks every tile; eight leave blocks without a tile


def test_limits_are_the_extensions():
    assert tuple(native.hip().sort_limits()) == tuple(kernels.sort_limits())
    threads, run, tile, bits = kernels.sort_limits()
    assert tile == threads * run and threads % 64 == 0 and 64 % bits == 0


def check(tag, frame, ascending, nulls_first, want_live=None):
    want = sc.cached_oracle(tag, frame, ascending, nulls_first)
    stats = []
    twin = sc.run(frame, ascending, nulls_first, stats=stats)
    assert torch.equal(twin, want), f"{tag}: twin"
    d = sc.to_device(frame, DEV)
    for blocks in BLOCKS:
        dstats = []
        got = sc.run(d, ascending, nulls_first, blocks=blocks, stats=dstats)
        assert got.is_cuda and got.dtype == torch.int64
        assert torch.equal(got.cpu(), want), f"{tag}: blocks={blocks}"
        assert dstats == stats, f"{tag}: the device ran other passes than the twin"
    if want_live is not None:
        assert [s["live"] for s in stats] == want_live
    return want


# a partial wave, an exact tile and one row over, a block that walks several tiles, idle blocks
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 77])
def test_sizes_and_blocks(n):
    frame = sc.make_frame(n, [("random64", "i64")], nulls=True, selection=False, seed=n)
    check(("size", n), frame, True, None)
    frame = sc.make_frame(n, [("floats", "f64")], nulls=True, selection=True, seed=n)
    check(("size-sel", n), frame, False, True)


@pytest.mark.parametrize("dtype", list(sc.DTYPES))
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_patterns_dtypes_orders(pattern, dtype):
    n = 2 * T + 1
    plain = sc.make_frame(n, [(pattern, dtype)], nulls=False, selection=True, seed=1)
    for asc in (True, False):
        check(("plain", pattern, dtype), plain, asc, None)
    nulls = sc.make_frame(n, [(pattern, dtype)], nulls=True, selection=True, seed=2)
    for asc, nf in sc.PLACEMENTS:
        check(("nulls", pattern, dtype), nulls, asc, nf)


@pytest.mark.parametrize("name", list(sc.MULTI))
def test_multi_key(name):
    keys, asc, nf = sc.MULTI[name]
    frame = sc.make_frame(2 * T + 1, keys, nulls=True, selection=True, seed=5)
    check(("multi", name), frame, asc, nf)


def test_every_pass_skipped_is_the_identity():
    n = 2 * T + 1
    frame = sc.make_frame(n, [("equal", "i64")], selection=True, seed=3)
    want = check(("equal-id",), frame, True, None, want_live=[[]])
    assert torch.equal(want, torch.nonzero(frame[2]).flatten())


def test_all_eight_byte_passes_live():
    frame = sc.make_frame(2 * T + 1, [("random64", "i64")], seed=4)
    check(("all-live",), frame, True, None, want_live=[list(range(8))])


def test_only_the_null_digit_is_live():
    n = 2 * T + 1
    frame = sc.make_frame(n, [("equal", "f64")], nulls=True, selection=True, seed=6)
    for asc, nf in sc.PLACEMENTS:
        check(("null-only",), frame, asc, nf, want_live=[[8]])


def test_every_row_dead():
    n = T + 5
    cols, valids, _ = sc.make_frame(n, [("random64", "i32")], nulls=True, seed=7)
    frame = (cols, valids, torch.zeros(n, dtype=torch.bool))
    got = sc.run(sc.to_device(frame, DEV))
    assert got.is_cuda and got.numel() == 0 and got.dtype == torch.int64
    assert sc.run(frame).numel() == 0


def test_bad_arguments_raise():
    h = native.hip()
    x = torch.zeros(8, dtype=torch.float16, device=DEV)
    with pytest.raises(TypeError):
        kernels.sort_permutation([x])
    buf = torch.zeros(9 * 256, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="2\\^31"):  # std::invalid_argument
        h.sort_keys(buf.data_ptr(), 4, 0, 0, 1 << 31, 1 << 31, False, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0)
    with pytest.raises(ValueError, match="f64, f32, i32, i64 or u8"):
        h.sort_keys(buf.data_ptr(), 2, 0, 0, 8, 8, False, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0)
