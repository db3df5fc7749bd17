"""The exact Gram cases on the host: what ``test_gpu_gram_exact.py`` feeds the kernels is what
``_gram_exact_cases.py`` says it is.  For every generated case: the stated bound, the
representability claims (bf16, fp8 e4m3, the split-bf16 cut), the shifts ``ops/shift.py`` picks, and
the host engine ``kernels.gram_stats(..., "fp64")`` equal to the integer oracle under
``np.array_equal``.  And the gap the exact tests close, in one assertion: one dropped row at
n = 70 001 passes the suite's relative measure and fails ``array_equal``."""
import numpy as np
import pytest
import torch

import _gram_exact_cases as gx
from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.ops.shift import column_shift

CASES = gx.all_cases()
IDS = [c.name for c in CASES]


def _rel(out, ref):
    """The measure of test_gpu_kernels.py / test_gpu_wide.py / test_gpu_syrk.py."""
    return float(np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-300))


def _rt(t, dtype):
    return t.to(dtype).to(torch.float64)


def test_case_list_is_distinct():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_claims(case):
    X, y, w = case.X.double(), case.y.double(), case.w
    d, n = case.d, case.n
    # the stated bound: every f32 accumulator holds a multiple of 1/2 below 2^24 of them
    assert case.bound < gx.LIMIT, case.bound
    # row 0 is live in every combination; integers everywhere; weights in {0, 1/2, 1, 2}
    assert bool(case.sel[0]) and float(w[0]) == 1.0
    assert torch.equal(X, X.round()) and torch.equal(y, y.round()) and float(y.abs().max()) <= 7
    assert set(w.unique().tolist()) <= {0.0, 0.5, 1.0, 2.0}
    if n >= 1000 and not case.shift_free:
        assert 0.2 < float((~case.sel).double().mean()) < 0.4 and float((w == 0).double().mean()) > 0.05
    # the shift ops/shift.py picks from all rows (the dead ones' draws included)
    sh = column_shift([case.X])
    s = torch.zeros(d, dtype=torch.float64) if sh is None else torch.from_numpy(sh.host)
    if case.shift_free or n < 256 or not case.off_cols:
        assert sh is None
    else:
        want = torch.zeros(d, dtype=torch.float64)
        want[case.off_cols] = 100.0 if "hundred" in case.name else 5.0
        assert torch.equal(s, want)
    lo, hi = X.amin(dim=1), X.amax(dim=1)
    assert bool(((s == 0) | ((lo <= s) & (s <= hi))).all())  # inside the column's own range: the bound covers it
    for v in (y, y * w):
        assert torch.equal(_rt(v, torch.bfloat16), v)
    if case.shift_free:
        # Family B: 11-bit integers split exactly into two bf16 terms, with a non-zero mid term
        live = case.X[:, case.sel].numpy()
        hi16, mid, low = gx.split_bf16(live)
        assert np.array_equal(hi16.astype(np.float64) + mid.astype(np.float64), live.astype(np.float64))
        assert not low.any() and np.count_nonzero(mid) > mid.size // 2
        assert float(np.abs(live).max()) == 1023.0 and np.count_nonzero(live % 2) > 0.9 * live.size
        assert case.sel.nonzero().flatten().tolist() == list(gx.B_LIVE)
        assert torch.equal(case.sel, w != 0)
    else:
        # bf16 round trips of x, x - s and w * (x - s) are the identity
        for v in (X, X - s[:, None], (X - s[:, None]) * w):
            assert torch.equal(_rt(v, torch.bfloat16), v)
        # Family A value ranges; zeros in the zero column; fp8: (x - s) * 64 survives e4m3, and every
        # column's largest live |x - s| is exactly 7 where the fp8 path runs (no small off-centre columns)
        Xs = X - (s if "hundred" not in case.name else torch.where(hi > 50, 100.0, 0.0).double())[:, None]
        cen = [j for j in range(d) if j not in case.off_cols]
        assert float(Xs[cen].abs().max()) == 7.0
        if n > 1:
            assert bool((X[case.zero_col] == 0).any())
        if "small" not in case.name:
            q = Xs * 64.0
            assert torch.equal(_rt(q.float(), torch.float8_e4m3fn), q)
            for weighted, masked in ((False, False), (False, True)):
                livem = ~case.dead(weighted, masked)
                assert bool((Xs[:, livem].abs().amax(dim=1) == 7.0).all())
        if "zero_sum" in case.name:
            for livem in (torch.ones(n, dtype=torch.bool), case.sel):
                assert float(y[livem].sum()) == 0.0 and float(y[livem].max()) == 7.0 and float(y[livem].min()) >= -7.0
            assert torch.equal(_rt((y * 64.0).float(), torch.float8_e4m3fn), y * 64.0)
        if "rare" in case.name:
            # what the patched companion asks for: zeros only at zero_rows of the zero column,
            # shifted or not
            for v in (X, X - s[:, None]):
                z = (v == 0).nonzero()
                assert z[:, 0].unique().tolist() == [case.zero_col] and z[:, 1].tolist() == gx.zero_rows(n)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_engine_equals_integer_oracle(case):
    combos = case.combos if case.n * case.d * case.d <= 20_000_000 else ((True, True),)
    for weighted, masked in combos:
        w, sel = case.rows(weighted, masked)
        got = kernels.gram_stats(case.X.double(), case.y.double(), w, sel, "fp64")
        assert np.array_equal(got.numpy(), case.oracle(weighted, masked).numpy()), (case.name, weighted, masked)


def test_oracle_ignores_dead_rows_whatever_they_hold():
    case = gx.family_a(1025, 9)
    for weighted, masked in ((False, True), (True, False), (True, True)):
        w, sel = case.rows(weighted, masked)
        Xp, yp = case.poisoned(weighted, masked)
        assert bool(torch.isnan(Xp).any()) and bool(torch.isinf(Xp).any()) and bool(torch.isnan(yp).any())
        got = gx.oracle(Xp.numpy(), yp.numpy(), None if w is None else w.numpy(), None if sel is None else sel.numpy())
        assert np.array_equal(got, case.oracle(weighted, masked).numpy())
        Xz = case.zero_dead(weighted, masked)
        assert np.array_equal(gx.oracle(Xz.numpy(), case.y.numpy(), None if w is None else w.numpy(),
                                        None if sel is None else sel.numpy()), case.oracle(weighted, masked).numpy())


def test_oracle_layout_by_hand():
    X = np.array([[1.0, 2.0, 3.0], [4.0, -5.0, 6.0]])
    y = np.array([1.0, -2.0, 7.0])
    w = np.array([0.5, 2.0, 1.0])
    sel = np.array([True, True, False])
    got = gx.oracle(X, y, w, sel)
    #        count  Σw   Σw²   Σwy   Σwy²  Σwx0 Σwx1  Σwx0y Σwx1y  G00   G01    G11
    want = [2.0, 2.5, 4.25, -3.5, 8.5, 4.5, -8.0, -7.5, 22.0, 8.5, -18.0, 58.0]
    assert got.tolist() == want
    # a zero weight: nothing in any sum; counted like every selected row, or not (the SYRK launcher)
    w0 = np.array([0.5, 0.0, 1.0])
    assert gx.oracle(X, y, w0, None).tolist() == [3.0, 1.5, 1.25, 7.5, 49.5, 3.5, 8.0, 21.5, 44.0, 9.5, 20.0, 44.0]
    assert gx.oracle(X, y, w0, None, count_zero_weight=False)[0] == 2.0


@pytest.mark.parametrize("d", gx.ONE_ROW_D)
def test_one_row_variant_exemption_share(d):
    c = gx.one_row(d)
    gram, sx = c.shares()
    assert gram >= 0.5 and sx == 1.0 and bool(c.exact[:5].all())
    assert not c.exact.all()  # the 24-bit x 24-bit products are there, and are not representable
    assert int(c.sel.sum()) == 1 and bool(c.sel[c.live])
    assert column_shift([c.X]) is None
    # every even column: 24 significant bits; every odd one: a power of two
    x = c.X[:, c.live].double().numpy()
    m, _ = np.frexp(x)
    assert np.all(np.abs(m[1::2]) == 0.5) and np.all((np.abs(m[0::2]) * (1 << 24)) % 2 == 1)
    got = kernels.gram_stats(c.X.double(), c.y.double(), None, c.sel, "fp64")
    assert np.array_equal(got.numpy(), c.ref)


def test_one_dropped_row_passes_the_relative_measure():
    """The gap: at n = 70 001 a kernel that drops one live row (the last: +-1 in every column, so
    every entry changes by at most 1) stays far inside the suite's ``_rel(out, ref) < 2e-5``, and
    fails ``array_equal``.  (A row of the largest values, 7 * 7 = 49 against a diagonal of about
    18.7 n, sits at 3.7e-5: the measure sees it at this n and no longer at the n = 250 000 and
    300 001 of the tolerance tests.)"""
    case = gx.family_a(70_001, 64, off="none")
    assert float(case.X[:, -1].abs().max()) == 1.0
    for weighted, masked in case.combos:
        w, sel = case.rows(weighted, masked)
        host = kernels.gram_stats(case.X.double(), case.y.double(), w, sel, "fp64").numpy()
        assert np.array_equal(case.oracle(weighted, masked).numpy(), host)
        cut = slice(0, case.n - 1)
        dropped = gx.oracle(case.X.numpy()[:, cut], case.y.numpy()[cut], None if w is None else w.numpy()[cut],
                            None if sel is None else sel.numpy()[cut])
        assert _rel(dropped, host) < 2e-5
        assert not np.array_equal(dropped, host)
        assert int((dropped != host).sum()) > 2000  # nearly every one of the 2213 entries is off, by at most 1
