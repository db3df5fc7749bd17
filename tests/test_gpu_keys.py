"""The four consumers of the one key reader of ``keys.h`` (group_encode, sort_permutation,
join_pairs, quantiles) see the same key of the same column: each is checked against
``ops.keys.skeys_np``, the numpy statement of the rule.  Every check is integer or bit equality."""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb
from net.jgp.labs.sparkdq4ml_amd.ops import keys, kernels

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 2 * 1024 + 3  # two block trips and a ragged run of 3
I64_MIN, I64_MAX = keys.I64_MIN, keys.I64_MAX


def _nan(sign: int, payload: int) -> float:
    return float(np.array([(sign << 63) | 0x7FF0000000000000 | payload], dtype=np.uint64).view(np.float64)[0])


F64_SPECIALS = [0.0, -0.0, np.inf, -np.inf, _nan(0, 1 << 51), _nan(1, 1 << 51), _nan(0, 0x123), _nan(1, 0x123),
                np.finfo(np.float64).max, -np.finfo(np.float64).max, np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny,
                5e-324, -5e-324, 1.5, 1.5, -2.25]
SPECIALS = {
    "f64": F64_SPECIALS,
    # (the f64 extremes cast to +-inf and 0: add f32's own largest, smallest and denormal values)
    "f32": [np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1e-45, -1e-45],
    "i64": [I64_MIN, I64_MAX, -1, 0, (1 << 53) + 1, -(1 << 53) - 1, I64_MAX - 1, I64_MIN + 1],
    "i32": [-(1 << 31), (1 << 31) - 1, -1, 0],
}
NP_DTYPE = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32}


def _frame():
    """The f64 column and its f32 / i64 / i32 casts (each with its own extremes written over a few
    rows), a validity mask and a selection of about 80 %.  The first row of every special value is
    live and valid."""
    rng = np.random.default_rng(20261020)
    base = rng.integers(-40, 40, N).astype(np.float64) * 0.5  # repeats, and +0.0 among them
    where = rng.permutation(N)
    valid, sel = rng.random(N) < 0.8, rng.random(N) < 0.8
    k = len(F64_SPECIALS)
    for rep in range(3):  # every special three times: ties across trips
        base[where[rep * k:(rep + 1) * k]] = F64_SPECIALS
    valid[where[:k]] = sel[where[:k]] = True
    cols = {"f64": base}
    with np.errstate(over="ignore", invalid="ignore"):
        cols["f32"] = base.astype(np.float32)
    finite = np.where(np.isfinite(base), np.clip(base, -1e6, 1e6), 0.0)
    cols["i64"], cols["i32"] = finite.astype(np.int64), finite.astype(np.int32)
    for name in ("f32", "i64", "i32"):
        own = where[3 * k:3 * k + len(SPECIALS[name])]
        cols[name][own] = np.array(SPECIALS[name], dtype=NP_DTYPE[name])
        valid[own] = sel[own] = True
    return cols, valid, sel


COLS, VALID, SEL = _frame()
REF = {}


def _ref(name):
    """(keys, live, ok) by the numpy statement, once per dtype."""
    if name not in REF:
        REF[name] = keys.side_np(torch.from_numpy(COLS[name]), torch.from_numpy(VALID), torch.from_numpy(SEL))
    return REF[name]


def _device(x: np.ndarray, off: int) -> torch.Tensor:
    """x on the device as a view `off` elements past a fresh allocation: off = 1 leaves the 16-byte
    grid (the scalar path of every loader), off = 0 stays on it (16-byte loads and the ragged tail)."""
    t = torch.from_numpy(x)
    buf = torch.empty(x.size + off, dtype=t.dtype, device=DEV)
    out = buf[off:]
    out.copy_(t)
    assert out.data_ptr() % 16 == (off * x.itemsize) % 16
    return out


@pytest.fixture(scope="module", params=[1, 0], ids=["off-grid", "on-grid"])
def off(request):
    return request.param


@pytest.fixture(scope="module")
def masks(off):
    return _device(VALID.view(np.uint8), off), _device(SEL.view(np.uint8), off)


@pytest.mark.parametrize("name", ["f64", "f32", "i64", "i32"])
def test_group_sort_join_see_one_key(name, off, masks):
    ks, live, ok = _ref(name)
    col = _device(COLS[name], off)
    valid, sel = masks
    rows = np.arange(N)

    # (a) the groups are the distinct keys, and every row gets the rank of its own
    enc = kernels.group_encode(col, valid, sel, mode="hash")
    uniq = np.unique(ks[ok])
    assert np.array_equal(enc.keys[1:].cpu().numpy(), uniq)
    want_gid = np.where(~live, -1, np.where(~ok, 0, np.searchsorted(uniq, ks) + 1))
    assert np.array_equal(enc.gid.cpu().numpy(), want_gid)

    # (b) along the permutation: the live rows, nulls first, then keys non-decreasing, ties in row order
    perm = kernels.sort_permutation([col], [valid], sel).cpu().numpy()
    assert np.array_equal(np.sort(perm), rows[live])
    nulls = int((live & ~ok).sum())
    assert np.array_equal(perm[:nulls], rows[live & ~ok])
    tail = perm[nulls:]
    assert np.array_equal(tail, rows[ok][np.argsort(ks[ok], kind="stable")])
    seq = ks[tail]
    assert np.all((seq[1:] > seq[:-1]) | ((seq[1:] == seq[:-1]) & (tail[1:] > tail[:-1])))

    # a self-join pairs exactly the rows of equal key: left rows in order, their matches in order
    li, ri = kernels.join_pairs(col, col, valid, valid, sel, sel)
    eq = (ks[:, None] == ks[None, :]) & ok[:, None] & ok[None, :]
    wl, wr = np.nonzero(eq)
    assert np.array_equal(li.cpu().numpy(), wl) and np.array_equal(ri.cpu().numpy(), wr)


@pytest.mark.parametrize("name", ["f64", "f32", "i64", "i32"])
def test_quantile_extremes_are_the_extreme_keys(name, off, masks):
    """(c) p = 0 / p = 1 are the values behind the smallest / largest non-NaN key of the column
    cast to double (an i64 rounds to the nearest double first)."""
    _, _, ok = _ref(name)
    valid, sel = masks
    with np.errstate(invalid="ignore"):
        x = COLS[name].astype(np.float64)
    m = ok & ~np.isnan(x)
    kd = keys.skeys_np(x[m], True)
    want = keys.keys_to_values(torch.tensor([int(kd.min()), int(kd.max())]), torch.float64)
    values, counts = kernels.quantiles([_device(COLS[name], off)], [valid], sel, [0.0, 1.0])
    assert int(counts[0]) == int(m.sum())
    assert torch.equal(values[0].cpu().view(torch.int64), want.view(torch.int64))


def test_uint8_reads_as_zero_or_not_on_both_engines():
    """A uint8 column of {0, 1, 2, 255} is 0 / non-zero to the loaders of keys.h, so to both engines:
    the same groups, and the same MIN / MAX / SUM_I accumulators."""
    rng = np.random.default_rng(7)
    x = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), N)
    g = rng.integers(0, 5, N).astype(np.int32)
    host = dict(col=torch.from_numpy(x), valid=torch.from_numpy(VALID), sel=torch.from_numpy(SEL), gid=torch.from_numpy(g))
    dev = {k: _device(v.numpy().view(np.uint8) if v.dtype == torch.bool else v.numpy(), 1) for k, v in host.items()}
    for mode in (None, "hash"):
        eh = kernels.group_encode(host["col"], host["valid"], host["sel"], mode=mode)
        ed = kernels.group_encode(dev["col"], dev["valid"], dev["sel"], mode=mode)
        assert (eh.G, eh.mode) == (ed.G, ed.mode)
        assert torch.equal(eh.gid, ed.gid.cpu()) and torch.equal(eh.keys, ed.keys.cpu())
        assert set(eh.keys[1:].tolist()) <= {0, 1}
    slots = lambda d: [(op, d["col"], d["valid"]) for op in (gb.MIN, gb.MAX, gb.SUM_I)]  # noqa: E731
    ah, offh = kernels.group_agg(host["gid"], 5, slots(host), host["sel"])
    ad, offd = kernels.group_agg(dev["gid"], 5, slots(dev), dev["sel"])
    assert offh == offd and torch.equal(ah, ad.cpu())
    ok = VALID & SEL
    want = np.array([int((x[ok & (g == i)] != 0).sum()) for i in range(5)])
    assert np.array_equal(ah[:, offh[2]].numpy(), want)  # SUM_I counts the non-zero bytes
