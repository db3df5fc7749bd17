"""The ``window.hip`` kernels against the numpy twin (``torch.equal`` on every raw integer output)
and against the plain-Python oracle, for every ``blocks`` override."""
import pytest
import torch

import _window_cases as wc
from net.jgp.labs.sparkdq4ml_amd.ops import kernels, native
from net.jgp.labs.sparkdq4ml_amd.ops import window as wn

pytestmark = pytest.mark.gpu

T = wc.T
DEV = "cuda"
BLOCKS = (None, 1, 8)  # one block walks every tile; eight leave blocks without a tile


def test_limits_are_the_extensions():
    assert tuple(native.hip().window_limits()) == tuple(kernels.window_limits())
    threads, run, tile, keys, words = kernels.window_limits()
    assert tile == threads * run and threads % 64 == 0 and words >= wn.SUM_WORDS


def same_raw(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g = got[k]
        assert g.is_cuda and g.dtype == want[k].dtype and g.shape == want[k].shape, f"{what}: {k}"
        assert torch.equal(g.cpu(), want[k]), f"{what}: {k}"


def check(m, layout, **kw):
    case, twin, order, want = wc.reference(m, layout, **kw)
    assert twin["perm"].tolist() == order
    wc.same_results(wc.finalize(case, twin), want)
    d = wc.to_device(case, DEV)
    for blocks in BLOCKS:
        got = wc.run_raw(d, blocks=blocks)
        same_raw(got, twin, f"{layout} m={m} blocks={blocks}")
    wc.same_results(wc.finalize(case, got), want)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
@pytest.mark.parametrize("m", wc.SIZES)
def test_sizes_layouts_frames(m, layout):
    check(m, layout)


def test_heads_layout_puts_heads_at_64_and_tile():
    _, twin, _, _ = wc.reference(2 * T + 1, "heads")
    h = twin["heads"]
    assert torch.nonzero(h & 1).flatten().tolist() == [0, 64, T]


def test_second_trip_of_the_totals_scan():
    """257 * T + 1 positions in one partition: 258 tile totals, one more than a trip of the
    one-block scan holds.  Twin only."""
    m = 257 * T + 1
    case = wc.cached(("trip", m), lambda: wc.make_case(m, "one", seed=3))
    frames = {"running": wc.FRAMES["running"], "rest": wc.FRAMES["rest"]}
    twin = wc.cached(("trip-twin", m), lambda: wc.run_raw(case, frames=frames))
    got = wc.run_raw(wc.to_device(case, DEV), frames=frames)
    same_raw(got, twin, "second trip")


@pytest.mark.parametrize("dtype", list(wc.DTYPES))
def test_key_dtypes(dtype):
    check(2 * T + 1, "sel", part_dtype=dtype, order_dtype=dtype)


def test_two_partition_and_two_order_columns_mixed_directions():
    check(2 * T + 1, "nulls", two_by_two=True)


def test_more_key_columns_than_a_launch_takes():
    """Nine key columns: the launcher chunks them and ORs the heads."""
    case, twin, _, _ = wc.reference(T + 1, "sel")
    d = wc.to_device(case, DEV)
    pc, pv = case["parts"][0]
    oc, ov = case["orders"][0][:2]
    cols, dcols = [pc] * 4 + [oc] * 5, [d["parts"][0][0]] * 4 + [d["orders"][0][0]] * 5
    want = kernels.window_heads(cols[:4], [None] * 4, cols[4:], [None] * 5, twin["perm"], case["n"])
    assert torch.equal(want, twin["heads"])
    got = kernels.window_heads(dcols[:4], [None] * 4, dcols[4:], [None] * 5, twin["perm"].to(DEV), case["n"])
    assert torch.equal(got.cpu(), want)


def test_groupby_identity_on_the_device(gpu_session):
    """sum / avg / min / max / count over partitionBy(k) equal groupBy(k) joined back, bit for bit."""
    import _window_api_cases as ac

    ac.groupby_identity(gpu_session)
