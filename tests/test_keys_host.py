"""``ops/keys.py``, the numpy / torch statement of ``keys.h``: the key rule, the side preamble and
the mixed-radix combiner that the groupby, sort and join twins share."""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb
from net.jgp.labs.sparkdq4ml_amd.ops import keys, kernels


def test_order_keys_fold_and_round_trip():
    nan2 = np.array([0xFFF0000000000123], dtype=np.uint64).view(np.float64)[0]
    x = np.array([-np.inf, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, np.inf, np.nan, nan2])
    k = keys.skeys_np(x, True)
    assert k[3] == k[4] == 0 and k[8] == k[9]  # -0.0 folds, every NaN is one key
    assert np.all(np.diff(np.delete(k, [3, 9])) > 0)  # numeric order, NaN above +inf
    unfolded = keys.skeys_np(x, False)
    assert unfolded[3] < unfolded[4]  # MIN / MAX keep -0.0 below +0.0
    back = keys.keys_to_values(torch.from_numpy(k[:8]), torch.float64).numpy()
    assert np.array_equal(back, np.where(x[:8] == 0, 0.0, x[:8])) and not np.signbit(back[3])
    i = np.array([keys.I64_MIN, -1, 0, keys.I64_MAX], dtype=np.int64)
    assert np.array_equal(keys.skeys_np(i, True), i)  # an integer's signed key is the value
    assert gb.hash_home is keys.hash_home and gb.keys_to_values is keys.keys_to_values  # the re-exports


def test_side_reads_uint8_as_zero_or_not():
    col = torch.tensor([0, 1, 2, 255, 7], dtype=torch.uint8)
    k, live, ok = keys.side_np(col, torch.tensor([1, 1, 1, 0, 1], dtype=torch.uint8), torch.tensor([1, 1, 1, 1, 0]).bool())
    assert k.tolist() == [0, 1, 1, 1, 1] and live.tolist() == [1, 1, 1, 1, 0] and ok.tolist() == [1, 1, 1, 0, 0]


def test_uint8_groups_and_aggregates_follow_the_kernel_loaders():
    """The loaders of keys.h read a uint8 column as 0 / non-zero; so does the host engine."""
    x = torch.tensor([0, 1, 2, 255, 0, 2], dtype=torch.uint8)
    for mode in (None, "hash"):
        enc = kernels.group_encode(x, mode=mode)
        assert enc.keys[1:].tolist() == [0, 1] and enc.gid.tolist() == [1, 2, 2, 2, 1, 2]
    acc, off = kernels.group_agg(None, 1, [(gb.MIN, x, None), (gb.MAX, x, None), (gb.SUM_I, x, None)])
    lo, hi, s = (int(acc[0, w]) for w in off)
    assert (lo ^ keys.I64_MIN, hi ^ keys.I64_MIN, s) == (0, 1, 4)


def test_mixed_radix_first_column_most_significant():
    a, b = torch.tensor([0, 1, 2, 1]), torch.tensor([3, 0, 4, 4])
    code, strides = keys.mixed_radix([a, b], [3, 5], "group_encode")
    assert code.dtype == torch.int64 and code.tolist() == [3, 5, 14, 9] and strides == [5, 1]
    with pytest.raises(ValueError, match="join: the product of the key columns' cardinalities"):
        keys.mixed_radix([a, b], [1 << 40, 1 << 40], "join")
