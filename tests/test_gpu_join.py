"""The ``join.hip`` kernels against the numpy twin and against the plain-Python oracle: the same
pairs in the same order, for every ``blocks`` override (the pair order is defined, so every check
is ``torch.equal``), and the same ``stats``."""
import numpy as np
import pytest
import torch

import _join_cases as jc
from net.jgp.labs.sparkdq4ml_amd.ops import device, groupby, kernels, native
from net.jgp.labs.sparkdq4ml_amd.ops.join import join_capacity

pytestmark = pytest.mark.gpu

T = jc.TRIP
DEV = "cuda"
BLOCKS = (None, 1, 8)  # one block walks every trip; eight leave blocks idle
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 77]


def test_limits_are_the_extensions():
    assert tuple(native.hip().join_limits()) == tuple(kernels.join_limits())
    trip, tile, lds_rows, max_cap = kernels.join_limits()
    assert trip % 256 == 0 and tile % 256 == 0 and lds_rows >= tile and max_cap == 1 << 30


def check(tag, case, hows=jc.HOWS + ("mask",), capacity=None, unique=None):
    d = jc.to_device(case, DEV)
    for how in hows:
        want = jc.cached_oracle(tag, case, how)
        stats = []
        if how == "mask":
            twin = jc.run_mask(case, stats=stats)
            assert torch.equal(twin, want), f"{tag}: twin mask"
            pairs = int(want.sum())
        else:
            twin = jc.run(case, how, stats=stats)
            assert torch.equal(twin[0], want[0]) and torch.equal(twin[1], want[1]), f"{tag}: twin {how}"
            pairs = int(want[0].numel())
        assert jc.core(stats[0]) == jc.oracle_stats(case, pairs), f"{tag}: twin stats {how}"
        if unique is not None:
            assert stats[0]["unique_build"] is unique
        for blocks in BLOCKS:
            dstats = []
            if how == "mask":
                got = jc.run_mask(d, capacity=capacity, blocks=blocks, stats=dstats)
                assert got.is_cuda and got.dtype == torch.bool
                assert torch.equal(got.cpu(), want), f"{tag}: mask blocks={blocks}"
            else:
                li, ri = jc.run(d, how, capacity=capacity, blocks=blocks, stats=dstats)
                assert li.is_cuda and ri.is_cuda and li.dtype == torch.int64 and ri.dtype == torch.int64
                assert torch.equal(li.cpu(), want[0]) and torch.equal(ri.cpu(), want[1]), f"{tag}: {how} blocks={blocks}"
            assert jc.core(dstats[0]) == jc.core(stats[0]), f"{tag}: device stats {how} blocks={blocks}"
            assert dstats[0]["capacity"] == (capacity or join_capacity(int(case[1].numel())))


# a partial wave, an exact trip and one row over, a block that walks several trips, idle blocks
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_blocks(n):
    m = 2 * T + 1
    check(("left-size", n), jc.make_case(n, m, span=400, seed=n))
    check(("right-size", n), jc.make_case(m, n, span=400, seed=n + 1))


def _distinct(n, seed, lo=-5):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.permutation(np.arange(lo, lo + n, dtype=np.int64)))


def test_unique_right_keys_take_the_fast_path_without_a_sort(monkeypatch):
    nl, nr = 2 * T + 1, T + 1
    rkey = _distinct(nr, 1)
    lkey = jc.key_column(nl, "i64", 2 * nr, 3, specials=False)
    case = jc.case_of(lkey, rkey)
    for how in jc.HOWS:
        jc.cached_oracle(("unique",), case, how)

    def no_sort(*a, **k):
        raise AssertionError("the unique-key path sorted")

    monkeypatch.setattr(device, "sort_permutation", no_sort)
    check(("unique",), case, hows=jc.HOWS, unique=True)


def test_one_duplicated_right_key_takes_the_general_path():
    nl, nr = 2 * T + 1, T + 1
    rkey = _distinct(nr, 1)
    rkey[nr - 1] = rkey[3]
    lkey = jc.key_column(nl, "i64", 2 * nr, 3, specials=False)
    case = jc.case_of(lkey, rkey)
    check(("one-dup",), case, unique=False)
    stats = []
    jc.run(jc.to_device(case, DEV), stats=stats)
    assert stats[0]["distinct"] == nr - 1


def test_all_equal_keys_300_by_300():
    case = jc.case_of(torch.full((300,), 7, dtype=torch.int32), torch.full((300,), 7, dtype=torch.int64))
    check(("all-equal",), case)
    assert jc.cached_oracle(("all-equal",), case, "inner")[0].numel() == 90_000


def test_one_hot_key_among_zero_match_rows():
    """5000 right rows of one key against 40 left rows of it among 2T others: expansion tiles that
    start and end inside one left row, and tiles that span many zero-match rows."""
    rng = np.random.default_rng(5)
    rkey = torch.cat([torch.full((5000,), 77, dtype=torch.int64), _distinct(500, 2, lo=1000)])
    rkey = rkey[torch.from_numpy(rng.permutation(5500))]
    lkey = torch.from_numpy(rng.integers(2000, 3000, 2 * T + 40))  # no match ...
    lkey[torch.from_numpy(rng.choice(2 * T + 40, 40, replace=False))] = 77  # ... but for the hot key
    lkey[5] = 1003
    check(("hot",), jc.case_of(lkey, rkey))


def test_a_tile_spanning_more_left_rows_than_the_lds_budget():
    """Three matching left rows, each after more zero-match rows than a tile stages in LDS: the
    lanes search the global offsets."""
    gap = jc.LDS_ROWS + 9
    lkey = torch.arange(1000, 1000 + 3 * gap + 3, dtype=torch.int64)
    for i in range(3):
        lkey[(i + 1) * gap + i] = 5
    rkey = torch.tensor([5, 9, 5, 5, 8], dtype=torch.int64)
    check(("wide-tile",), jc.case_of(lkey, rkey), hows=("inner", "mask"))


def test_no_overlap_at_all():
    check(("disjoint",), jc.case_of(_distinct(T + 3, 1, lo=0), _distinct(T + 9, 2, lo=10_000)))


def test_every_left_row_dead_and_every_right_row_dead_or_null():
    lkey, rkey, lvalid, rvalid, lsel, rsel = jc.make_case(T + 5, T + 7, span=60, seed=9)
    check(("left-dead",), (lkey, rkey, lvalid, rvalid, torch.zeros(T + 5, dtype=torch.bool), rsel))
    half = torch.arange(T + 7) % 2 == 0
    check(("right-gone",), (lkey, rkey, lvalid, ~half, lsel, half))  # a live right row has a null key


def _colliding(capacity: int, home: int, count: int, start: int = 1):
    out, k = [], start
    while len(out) < count:
        if groupby.hash_home(k, capacity) == home:
            out.append(k)
        k += 1
    return out


def test_colliding_keys_wrap_around_a_small_table():
    cap = 16
    run_keys = _colliding(cap, cap - 1, 5)  # one home slot, the last: the probe wraps to slots 0, 1, ...
    absent = _colliding(cap, cap - 1, 1, start=run_keys[-1] + 1) + _colliding(cap, 1, 1)  # hash into the run, not there
    others = _colliding(cap, 7, 2)
    rkey = torch.tensor(run_keys + others + run_keys[:2], dtype=torch.int64)
    lkey = torch.tensor(run_keys[::-1] + absent + others + absent + run_keys[:1], dtype=torch.int64)
    check(("collide",), jc.case_of(lkey, rkey), capacity=cap)
    check(("collide-default",), jc.case_of(lkey, rkey))


def test_a_capacity_too_small_raises():
    d = jc.to_device(jc.case_of(_distinct(40, 1), _distinct(40, 2)), DEV)
    for cap in (16, 32):  # fewer slots than distinct keys
        with pytest.raises(RuntimeError, match="cannot hold"):
            jc.run(d, capacity=cap)
    d16 = jc.to_device(jc.case_of(_distinct(40, 1), _distinct(16, 2)), DEV)
    with pytest.raises(RuntimeError, match="cannot hold"):  # the distinct keys fit, the one empty slot does not
        jc.run_mask(d16, capacity=16)
    jc.run(d16, capacity=32)
    with pytest.raises(ValueError, match="power of two"):
        jc.run(d16, capacity=24)


@pytest.mark.parametrize("where", ["left", "right", "both", "neither"])
def test_the_out_of_band_int64_max_key(where):
    lkey = jc.key_column(T + 3, "i64", 40, 1, specials=False)
    rkey = jc.key_column(2 * T + 1, "i64", 40, 2, specials=False)
    if where in ("left", "both"):
        lkey[::7] = jc.I64_MAX
    if where in ("right", "both"):
        rkey[::5] = jc.I64_MAX
    check(("top", where), jc.case_of(lkey, rkey))


@pytest.mark.parametrize("ldt,rdt", jc.DTYPE_PAIRS)
def test_every_kernel_dtype_pair(ldt, rdt):
    check(("dtypes", ldt, rdt), jc.make_case(T + 65, T + 1, ldt, rdt, span=300, seed=4))


def test_bad_arguments_raise():
    h = native.hip()
    x = torch.zeros(8, dtype=torch.float16, device=DEV)
    with pytest.raises(TypeError):
        kernels.join_pairs(x, x)
    with pytest.raises(ValueError, match="how must be one of"):
        kernels.join_pairs(x.to(torch.float32), x.to(torch.float32), how="cross")
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    with pytest.raises(ValueError, match="2\\^31 rows"):  # std::invalid_argument
        h.join_build(p, 4, 0, 0, 1 << 31, p, 16, p, p, p, p, 1, 0)
    with pytest.raises(ValueError, match="f64, f32, i32, i64 or u8"):
        h.join_build(p, 2, 0, 0, 8, p, 16, p, p, p, p, 1, 0)
    with pytest.raises(ValueError, match="power of two"):
        h.join_build(p, 4, 0, 0, 8, p, 24, p, p, p, p, 1, 0)
    with pytest.raises(ValueError, match="blocks must be >= 1"):
        h.join_probe(p, 4, 0, 0, 8, p, 16, p, 0, p, p, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="unknown probe mode"):
        h.join_probe(p, 4, 0, 0, 8, p, 16, p, 9, p, p, 0, 0, 1, 0)
    with pytest.raises(ValueError, match="null buffer"):
        h.join_probe(p, 4, 0, 0, 8, p, 16, p, 2, p, p, 0, 0, 1, 0)  # a full outer probe without `matched`
    with pytest.raises(ValueError, match="2\\^31 pairs"):
        h.join_expand(p, 8, 1 << 31, p, 0, 0, 0, p, 16, p, p, 1, 0)
    with pytest.raises(ValueError, match="come together"):
        h.join_expand(p, 8, 8, p, p, 0, 0, p, 16, p, p, 1, 0)
