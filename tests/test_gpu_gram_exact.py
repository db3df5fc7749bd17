"""Every low-precision Gram path against an integer oracle, bit for bit.

The inputs (``_gram_exact_cases.py``; their claims are checked on the host by
``test_gram_exact_cases.py``) make every product and every partial sum of every path exactly
representable, so each path has ONE right answer and the comparison is ``torch.equal`` on all
``5 + 2d + d(d+1)/2`` doubles: a row dropped or counted twice at a range boundary, a tail lane read,
a dead row leaking or a wrong packed index changes an entry by at least 1/2 and fails, at any n.
Every case first asserts the path it takes -- the launcher entry point and the arguments the C++
dispatch keys on, read off a recording proxy of the native module (``_Spy``) -- so none passes by
falling back.

Entries left under a tolerance, and why:

* fp8 wide path, labels whose live mean is not 0: the label entries Σwy, Σwy², Σw·x·y keep
  test_gpu_wide.py's 1e-2.  By design: ``wide_label_scales_kernel`` (csrc/hip/gram_wide.hip, "t = sy
  / fmax(sw, 1.0)") centres the label on its live mean before the two-digit e4m3 split, and y - t is
  no multiple of the digit step.  The count, Σw, Σw², Σw·x and Σw·x·xᵀ are ``==`` for every label,
  and the whole vector is with the zero-sum, max-7 label (t = 0, scale 2^-6, low digit 0).
  (Columns stored under a shift of 100 hold the 1e-2 on Σw·x·y only because the label un-shift
  takes the centred label's sum as the 0 it is: the summed digit rounding, about 3 at n = 20 011,
  times the shift had put them at 1.14e-2.)
* the one-live-row variant of Family B (arbitrary 24-bit mantissas) on the f32-class paths: only
  the entries whose exact product is f32-representable are ``==``; a 24 x 24-bit product is rounded
  to f32 by the exact-f32 MFMA and by the split-bf16 sum, so the others keep today's 2e-6 (stream
  kernels) and 2e-5 (SYRK).

The count of the d > 64 SYRK launcher leaves out the rows of zero weight, the d <= 64 kernels and
the host engine count every selected row (``_gram_exact_cases.oracle``); each is compared with its
own count.
"""
import numpy as np
import pytest
import torch

import _gram_exact_cases as gx

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, native  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops.layout import PackedTiles, PatchedTiles  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops.shift import Shift  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DT_NAME = {0: "f64", 1: "f32", 2: "bf16"}
MODE_NAME = {v: k for k, v in device.GRAM_MODES.items()}


@pytest.fixture(scope="module", autouse=True)
def _hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    native.hip()


class _Spy:
    """The native module with every call recorded as ``(name, args)``."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v):
            return v

        def call(*args):
            self.calls.append((name, args))
            return v(*args)

        return call

    def only(self, name):
        got = [a for k, a in self.calls if k == name]
        assert len(got) == 1, (name, [k for k, _ in self.calls])
        return got[0]

    def names(self):
        return {k for k, _ in self.calls}


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(native.hip())
    monkeypatch.setattr(native, "hip", lambda: s)
    return s


def _tall_path(args):
    """The kernel family one ``gram_tall`` call resolves to, and what tells its instantiations
    apart: the dispatch of csrc/hip/gram.hip ``gram_tall`` / ``with_kernel`` and
    gram_stream.hip ``gram_stream_ok``, restated on the recorded arguments."""
    mode, X, ld, d, n, xdt, tiled, xshift, xpack, xdir, xrec, xovf, y, ydt, w, wdt, sel, xmode = args[:18]
    xs = 8 if xdt == 0 else 4
    stream_ok = (not tiled and 1 <= d <= 64 and n >= 1 and xdt in (0, 1) and (mode == 0 or xdt == 1)
                 and X % 16 == 0 and (d == 1 or (ld * xs) % 16 == 0) and ydt in (0, 1) and y % 16 == 0
                 and (w == 0 or (wdt in (0, 1) and w % 16 == 0)) and (sel == 0 or sel % 4 == 0))
    if xshift:
        assert stream_ok and mode in (1, 2, 4)
        return "stream", MODE_NAME[mode], "shifted"
    if mode == 0 and not tiled and d <= 8 and xdt in (0, 1):
        return "skinny", "fp64", DT_NAME[xdt]
    if (mode in (0, 1, 4) or (mode == 2 and xdt == 1)) and stream_ok:
        return "stream", MODE_NAME[mode], DT_NAME[xdt]
    assert mode == 2, "the fp64 and f32 modes have no other kernel: the f64 fallback is gone, gram_tall refuses"
    assert xdt != 1, "bf16 mode on f32 storage has no kernel but the stream kernel: gram_tall refuses"
    comp = "patched" if xrec else ("mixed" if xdir else None)
    assert (xpack != 0) == (comp is not None)
    return "tall_bf16", ("tiled" if tiled else DT_NAME[xdt]), comp, xmode


def _entry(k, d):
    if k < 5:
        return ("count", "Σw", "Σw²", "Σwy", "Σwy²")[k]
    if k < 5 + d:
        return f"Σw·x[{k - 5}]"
    if k < 5 + 2 * d:
        return f"Σw·x·y[{k - 5 - d}]"
    e = k - 5 - 2 * d
    j = int((np.sqrt(8 * e + 1) - 1) // 2)
    while j * (j + 1) // 2 > e:
        j -= 1
    while (j + 1) * (j + 2) // 2 <= e:
        j += 1
    return f"Σw·x·xᵀ[{e - j * (j + 1) // 2}, {j}]"


def _same(out, ref, d, note, where=None):
    """``torch.equal`` (on the entries ``where``), with the first differing entries in the message."""
    got = out.detach().cpu()
    assert got.dtype == torch.float64 and got.shape == ref.shape, (note, got.dtype, got.shape)
    if where is not None:
        keep = torch.as_tensor(where)
        if torch.equal(got[keep], ref[keep]):
            return
        bad = ((got != ref) & keep).nonzero().flatten()
    else:
        if torch.equal(got, ref):
            return
        bad = (got != ref).nonzero().flatten()
    rows = [f"  {_entry(int(k), d)}: got {float(got[k])!r}, want {float(ref[k])!r}" for k in bad[:10]]
    raise AssertionError(f"{note}: {bad.numel()} of {ref.numel()} entries differ\n" + "\n".join(rows))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _rows(case, weighted, masked, wdt=F64):
    w, sel = case.rows(weighted, masked)
    return (None if w is None else w.to(wdt).cuda()), (None if sel is None else sel.cuda())


def _grids(n):
    return (None, 1, 2) if n in gx.MID_N else (None,)


# ------------------------------------------------------------------------------------------------
# path 1: device.gram_stats on dense storage, d <= 64
# ------------------------------------------------------------------------------------------------
def _expect_dense(mode, xdt, d, shifted, weighted):
    if mode == "fp64" or (mode in ("fp32", "fp32split") and d <= 8):
        return ("skinny", "fp64", DT_NAME[device.dtype_code(torch.empty(0, dtype=xdt))]) if d <= 8 else \
            ("stream", "fp64", "f64" if xdt == F64 else "f32")
    if mode in ("fp32", "fp32split"):
        return "stream", mode, "shifted" if shifted else "f32"
    if xdt == F32:
        return "stream", "bf16", "shifted" if shifted else "f32"
    if shifted:  # other storage is tiled shifted once; with weights it rides the stream kernel as f32
        return ("stream", "bf16", "shifted") if weighted else ("tall_bf16", "tiled")
    return "tall_bf16", "bf16" if xdt == BF16 else "f64"


DENSE = [("bf16", BF16), ("bf16", F32), ("bf16", F64), ("fp32", F32), ("fp32split", F32), ("fp64", F32), ("fp64", F64)]


@pytest.mark.parametrize("mode,xdt", DENSE, ids=[f"{m}-{str(t)[6:]}" for m, t in DENSE])
@pytest.mark.parametrize("d", gx.TALL_D)
@pytest.mark.parametrize("n", gx.TALL_N)
def test_dense_gram_stats_exact(spy, mode, xdt, d, n):
    """Family A through ``device.gram_stats``: no mask and no weights, ``sel``, ``w`` (f32), ``w``
    (f64) with ``sel``; f32 and f64 labels; ``blocks`` 1 and 2 at the mid sizes.  The weighted bf16
    operand w * (x - s) is bf16-exact (w in {1/2, 1, 2}), so the weighted call is ``==`` too.  The
    f64 skinny kernel promises not to read the rows the selection drops: they hold NaN / inf."""
    case = gx.family_a(n, d)
    shifted = n >= 256 and bool(case.off_cols) and mode != "fp64" and not (mode != "bf16" and d <= 8)
    X = case.X.to(xdt).cuda()
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked, F32 if not masked else F64)
        y = case.y.cuda() if not weighted else case.y.double().cuda()
        Xin = X
        want = _expect_dense(mode, xdt, d, shifted, weighted)
        if want[0] == "skinny" and masked:
            Xp, yp = case.poisoned(False, True)
            Xin, y = Xp.to(xdt).cuda(), yp.to(y.dtype).cuda()
        for blocks in _grids(n):
            spy.calls.clear()
            out = device.gram_stats(Xin, y, w, sel, mode, blocks=blocks)
            note = f"{case.name} {mode} {xdt} w={weighted} sel={masked} blocks={blocks}"
            path = _tall_path(spy.only("gram_tall"))
            assert path[:len(want)] == want, (note, path)
            if path[0] == "tall_bf16":
                assert path[2] is None and ("tile_bf16" in spy.names()) == (path[1] == "tiled")
            _same(out, case.oracle(weighted, masked), d, note)


@pytest.mark.parametrize("mode", ["fp32", "fp32split"])
@pytest.mark.parametrize("d", gx.B_TALL_D)
def test_dense_family_b_exact(spy, mode, d):
    """Family B (4 live rows, 11-bit odd integers: hi + mid of the split) on the exact-f32 and the
    split-bf16 stream kernels, unshifted."""
    case = gx.family_b(d)
    X = case.X.cuda()
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked)
        for blocks in (None, 1, 2):
            spy.calls.clear()
            out = device.gram_stats(X, case.y.cuda(), w, sel, mode, blocks=blocks)
            note = f"{case.name} {mode} w={weighted} sel={masked} blocks={blocks}"
            assert _tall_path(spy.only("gram_tall")) == ("stream", mode, "f32"), note
            _same(out, case.oracle(weighted, masked), d, note)


@pytest.mark.parametrize("mode", ["fp32", "fp32split"])
@pytest.mark.parametrize("d", [d for d in gx.ONE_ROW_D if d <= 64])
def test_dense_one_live_row(spy, mode, d):
    """One live row of arbitrary 24-bit mantissas and powers of two: ``==`` wherever the exact
    product is f32-representable (at least half of the Gram entries and all of Σx: the host test
    asserts the share), today's 2e-6 on the rest."""
    c = gx.one_row(d)
    spy.calls.clear()
    out = device.gram_stats(c.X.cuda(), c.y.cuda(), None, c.sel.cuda(), mode)
    assert _tall_path(spy.only("gram_tall")) == ("stream", mode, "f32")
    ref = torch.from_numpy(c.ref)
    _same(out, ref, d, f"{c.name} {mode}", where=c.exact)
    assert _rel(out, ref) < 2e-6


# ------------------------------------------------------------------------------------------------
# path 2: TiledBF16 and its companions
# ------------------------------------------------------------------------------------------------
def _explicit_shift(case):
    """An integer shift that is not the sampled one: the first and the last off-centre column only."""
    s = np.zeros(case.d)
    s[[case.off_cols[0], case.off_cols[-1]]] = 5.0
    return Shift(s, "cuda")


def _xmode(w, sel, zero_dead=False):
    return 2 if w is not None else (1 if sel is not None and not zero_dead else 0)


@pytest.mark.parametrize("pack", [False, True, "patched"], ids=["raw", "mixed", "patched"])
@pytest.mark.parametrize("shift", [None, "auto", "explicit"])
@pytest.mark.parametrize("d", gx.PATCH_D)
@pytest.mark.parametrize("n", gx.PATCH_N)
def test_tiled_companions_exact(spy, pack, shift, d, n):
    """``tile_bf16(X, shift, pack)`` on the rare-zero form of Family A (the table the patched
    companion takes; its zeros are the exceptions): the raw, the mixed and the patched launch each
    against the oracle, not against one another.  The patched kernel takes the f32 label without a
    mask; every other call on that table must read the raw tiles and still be exact."""
    case = gx.family_a(n, d, zeros="rare")
    X = case.X.cuda()
    sh = _explicit_shift(case) if shift == "explicit" else shift
    T = device.tile_bf16(X, shift=sh, pack=pack)
    if shift is None or (shift == "auto" and n < 256):
        assert T.shift is None
    else:
        want = np.zeros(d)
        want[case.off_cols if shift == "auto" else [case.off_cols[0], case.off_cols[-1]]] = 5.0
        assert np.array_equal(T.shift.host, want)
    assert torch.equal(T.to_dense().float(), X)
    entries = (n // 64) * (d // 32)
    zeros = len([r for r in gx.zero_rows(n) if r < 64 * (n // 64)])
    if pack is False:
        assert T.packed is None
    elif pack is True:
        # the entries that hold a zero stay raw (more than 15 binades), as does the ragged superstep
        assert isinstance(T.packed, PackedTiles) and T.packed.npacked == entries - zeros
    else:
        assert isinstance(T.packed, PatchedTiles) and T.packed.nexc == zeros > 0 and T.packed.npacked == entries
    kind = {False: None, True: "mixed", "patched": "patched"}[pack]
    y32, y64 = case.y.cuda(), case.y.double().cuda()
    runs = [(False, False, y32, kind), (False, False, y64, None if kind == "patched" else kind)]
    runs += [(wt, mk, y32, None if kind == "patched" else kind) for wt, mk in case.combos[1:]]
    for weighted, masked, y, want in runs:
        w, sel = _rows(case, weighted, masked)
        assert device._tiled_pre(T, y, w, sel, _xmode(w, sel))[0] == want
        for blocks in _grids(n):
            spy.calls.clear()
            out = device.gram_stats(T, y, w, sel, "bf16", blocks=blocks)
            note = f"{case.name} shift={shift} pack={pack} {y.dtype} w={weighted} sel={masked} blocks={blocks}"
            assert _tall_path(spy.only("gram_tall")) == ("tall_bf16", "tiled", want, _xmode(w, sel)), note
            _same(out, case.oracle(weighted, masked), d, note)


@pytest.mark.parametrize("shift", [None, "auto"])
@pytest.mark.parametrize("d", [7, 33])
@pytest.mark.parametrize("n", gx.TALL_N)
def test_tiled_ragged_widths_exact(spy, shift, d, n):
    """Tile widths with padding features (d = 7, 33), no companion; the off-centre columns go in
    unshifted too (integers in [0, 10] are bf16-exact, and 0 is inside their range: the bound holds)."""
    case = gx.family_a(n, d)
    T = device.tile_bf16(case.X.cuda(), shift=shift, pack=False)
    assert (T.shift is not None) == (shift == "auto" and n >= 256) and T.packed is None
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked)
        for blocks in _grids(n):
            spy.calls.clear()
            out = device.gram_stats(T, case.y.cuda(), w, sel, "bf16", blocks=blocks)
            note = f"{case.name} shift={shift} w={weighted} sel={masked} blocks={blocks}"
            assert _tall_path(spy.only("gram_tall")) == ("tall_bf16", "tiled", None, _xmode(w, sel)), note
            _same(out, case.oracle(weighted, masked), d, note)


def _mixed_columns(case, X=None):
    """The case's columns as separate source tensors: int32, f32, f64 in turn, and (from three
    columns on) one f32 view that starts 4 bytes off a 16-byte boundary."""
    X = case.X if X is None else X
    dts = (torch.int32, F32, F64)
    cols = [X[j].to(dts[j % 3]).cuda() for j in range(case.d)]
    if case.d >= 2:
        j = 1  # an f32 column
        buf = torch.empty(case.n + 1, dtype=F32, device="cuda")
        buf[1:] = X[j].cuda()
        cols[j] = buf[1:]
        assert cols[j].data_ptr() % 16 == 4
    return cols


@pytest.mark.parametrize("d", [7, 32, 33, 64])
@pytest.mark.parametrize("n", gx.TALL_N)
def test_pack_tiled_zero_dead_exact(spy, d, n):
    """``pack_tiled(cols, sel)``: zero-dead storage of x - s from mixed source columns, read with
    ``x_zero_dead=True`` (row mode 0 with a selection)."""
    case = gx.family_a(n, d)
    sel = case.sel.cuda()
    T = device.pack_tiled(_mixed_columns(case), sel)
    assert (T.shift is not None) == (n >= 256)
    s = torch.zeros(d, 1, device="cuda") if T.shift is None else T.shift.dev.unsqueeze(1)
    assert torch.equal(T.to_dense().float(), torch.where(sel, case.X.cuda(), s.expand(d, n)))  # stored x' = 0 on the dead rows
    for blocks in _grids(n):
        spy.calls.clear()
        out = device.gram_stats(T, case.y.cuda(), None, sel, "bf16", x_zero_dead=True, blocks=blocks)
        assert _tall_path(spy.only("gram_tall")) == ("tall_bf16", "tiled", None, 0)
        _same(out, case.oracle(False, True), d, f"{case.name} blocks={blocks}")


# ------------------------------------------------------------------------------------------------
# path 3: the source-column kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", gx.COLS_D)
@pytest.mark.parametrize("n", gx.TALL_N)
def test_gram_cols_typed_loads_exact(spy, d, n):
    """``gram_cols`` over int32 / f32 / f64 columns with one unaligned view: the typed-load kernel."""
    case = gx.family_a(n, d)
    cols = _mixed_columns(case)
    for masked in (False, True):
        _, sel = _rows(case, False, masked)
        for blocks in _grids(n):
            spy.calls.clear()
            out = device.gram_cols(cols, case.y.cuda() if masked else case.y.double().cuda(), sel, blocks=blocks)
            note = f"{case.name} sel={masked} blocks={blocks}"
            assert spy.only("gram_cols")[1] == -1, note  # sdt: per-element typed loads
            assert "gram_stream_cols" not in spy.names()
            _same(out, case.oracle(False, masked), d, note)


def _f32_columns(case, dtype=F32):
    return [case.X[j].to(dtype).cuda() for j in range(case.d)]  # separate allocations: 16-byte aligned


@pytest.mark.parametrize("d", [9, 33, 64])
@pytest.mark.parametrize("n", gx.TALL_N)
def test_gram_cols_stream_exact(spy, d, n):
    """``gram_cols`` over aligned all-f32 columns: the LDS-DMA stream kernel in bf16 mode."""
    case = gx.family_a(n, d)
    cols = _f32_columns(case)
    for masked in (False, True):
        _, sel = _rows(case, False, masked)
        spy.calls.clear()
        out = device.gram_cols(cols, case.y.cuda(), sel)
        call = spy.only("gram_stream_cols")
        assert call[0] == 2 and call[4] == 1 and "gram_cols" not in spy.names()
        assert (call[-1] != 0) == (n >= 256)  # the sampled shift, subtracted in-kernel
        _same(out, case.oracle(False, masked), d, f"{case.name} sel={masked}")


@pytest.mark.parametrize("compute,xdt", [("fp64", F64), ("fp64", F32), ("fp32", F32)])
@pytest.mark.parametrize("d", [9, 33, 64])
@pytest.mark.parametrize("n", gx.TALL_N)
def test_gram_stream_cols_exact(spy, compute, xdt, d, n):
    case = gx.family_a(n, d)
    cols = _f32_columns(case, xdt)
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked, F32 if masked else F64)
        spy.calls.clear()
        out = device.gram_stream_cols(cols, case.y.double().cuda(), w, sel, compute)
        assert out is not None
        call = spy.only("gram_stream_cols")
        assert call[0] == device.GRAM_MODES[compute] and call[4] == (0 if xdt == F64 else 1)
        _same(out, case.oracle(weighted, masked), d, f"{case.name} {compute} {xdt} w={weighted} sel={masked}")


@pytest.mark.parametrize("d", [1, 4, 8])
@pytest.mark.parametrize("n", gx.TALL_N)
def test_gram_skinny_cols_exact(spy, d, n):
    case = gx.family_a(n, d)
    cols = _mixed_columns(case)
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked)
        for blocks in _grids(n):
            spy.calls.clear()
            out = device.gram_skinny_cols(cols, case.y.cuda(), w, sel, blocks=blocks)
            assert len(spy.only("gram_skinny_cols")[0]) == d
            _same(out, case.oracle(weighted, masked), d, f"{case.name} w={weighted} sel={masked} blocks={blocks}")


# ------------------------------------------------------------------------------------------------
# path 4: the wide fragment path
# ------------------------------------------------------------------------------------------------
def _wide_runs():
    runs = []
    for d, n in gx.WIDE_SHAPES:
        nsup = (n + 63) // 64
        scheds = ["grid"]
        if nsup >= 8 * 3:
            scheds.append("gang3" if d == 1100 else "gang")  # d = 1100, S = 3: 45 units on 32 blocks, a partial last round
        if nsup >= 8 * 16:
            scheds.append("queue")
        runs += [(d, n, s) for s in scheds]
    return runs


WIDE_KERNEL = {"gang": "gram_wide_gang", "queue": "gram_wide_queue", "grid": "gram_wide"}


@pytest.mark.parametrize("eb", [16, 8])
@pytest.mark.parametrize("off", ["none", "hundred"], ids=["unshifted", "shift100"])
@pytest.mark.parametrize("d,n,sched", _wide_runs())
def test_wide_exact(spy, monkeypatch, eb, off, d, n, sched):
    """``pack_wide(..., eb, sel, shift)`` then the fragment SYRK under each schedule.  ``off="none"``:
    every column centred, ``shift=None``; ``"hundred"``: columns 100 + k under an explicit integer
    Shift of 100.  First the storage: ``to_dense()`` gives the integers back and every fp8 scale is
    2^-6.  bf16: the whole vector is ``==``.  fp8: count, Σw, Σw², Σw·x and Σw·x·xᵀ are ``==`` for
    every label, and the whole vector with the zero-sum, max-7 label; a label of non-zero live mean
    keeps 1e-2 on Σwy, Σwy² and Σw·x·y (by design: see the module docstring)."""
    monkeypatch.setenv("DQ4ML_WIDE_SCHED", sched[:4] if sched.startswith("gang") else sched)
    monkeypatch.setenv("DQ4ML_WIDE_GANG_S", "3" if sched.endswith("3") else "2")
    monkeypatch.setenv("DQ4ML_WIDE_H", "1")
    mode = "bf16" if eb == 16 else "fp8"
    for label in ("plain", "zero_sum"):
        case = gx.family_a(n, d, off=off, label=label)
        X, y = case.X.cuda(), case.y.double().cuda()
        shift = None
        s = torch.zeros(d, 1, device="cuda")
        if off == "hundred":
            shift = Shift(np.where(np.isin(np.arange(d), case.off_cols), 100.0, 0.0), "cuda")
            s = shift.dev.unsqueeze(1)
        for how in ("all", "packed_sel", "masked_after"):
            sel = None if how == "all" else case.sel.cuda()
            T = device.pack_wide([X], eb, sel if how == "packed_sel" else None, shift=shift)
            dense = X if how != "packed_sel" else torch.where(sel, X, s.expand(d, n))
            assert torch.equal(T.to_dense().float(), dense)
            if eb == 8:
                assert torch.equal(T.scales, torch.full((d,), 2.0 ** -6, device="cuda"))
            spy.calls.clear()
            out = device.gram_stats(T, y, None, sel, mode, x_zero_dead=how == "packed_sel")
            note = f"{case.name} eb={eb} {sched} {how}"
            kern = WIDE_KERNEL[sched[:4] if sched.startswith("gang") else sched]
            assert kern in spy.names() and not (set(WIDE_KERNEL.values()) - {kern}) & spy.names(), (note, spy.names())
            assert ("wide_mask_rows" in spy.names()) == (how == "masked_after") and "gram_syrk" not in spy.names()
            ref = case.oracle(False, sel is not None)
            if eb == 16 or label == "zero_sum":
                _same(out, ref, d, note)
            else:
                lab = torch.zeros(ref.numel(), dtype=torch.bool)
                lab[3:5] = True
                lab[5 + d:5 + 2 * d] = True
                _same(out, ref, d, note, where=~lab)
                got = out.cpu()
                assert _rel(got[3:5], ref[3:5]) < 1e-2 and _rel(got[5 + d:5 + 2 * d], ref[5 + d:5 + 2 * d]) < 1e-2, note
                # Σwy = t * W with t = Σy / W in doubles (two roundings), not the folded digits' sum
                assert abs(float(got[3] - ref[3])) <= 2 * np.finfo(np.float64).eps * abs(float(ref[3])), note


# ------------------------------------------------------------------------------------------------
# path 5: the exact-f32 and f64 SYRK (d > 64)
# ------------------------------------------------------------------------------------------------
SYRK = [("fp32", F32), ("bf16", BF16), ("fp64", F32), ("fp64", F64)]


@pytest.mark.parametrize("mode,xdt", SYRK, ids=[f"{m}-{str(t)[6:]}" for m, t in SYRK])
@pytest.mark.parametrize("d,n", gx.SYRK_SHAPES)
def test_syrk_exact(spy, mode, xdt, d, n):
    """Family A on the SYRK: the fp32 request, the weighted bf16 request (served by the exact-f32
    kernel) and fp64, with and without ``w`` and ``sel``; every dead row of the combination (dropped
    by the selection or of zero weight) holds NaN / inf, features and label.  The launcher's count
    leaves out the rows of zero weight."""
    case = gx.family_a(n, d)
    for weighted, masked in case.combos:
        if mode == "bf16" and not weighted:
            continue  # (unweighted bf16 is the fragment path: test_wide_exact)
        w, sel = _rows(case, weighted, masked)
        Xp, yp = case.poisoned(weighted, masked) if (weighted or masked) else (case.X, case.y)
        spy.calls.clear()
        out = device.gram_stats(Xp.to(xdt).cuda(), yp.cuda(), w, sel, mode)
        note = f"{case.name} {mode} {xdt} w={weighted} sel={masked}"
        assert spy.only("gram_syrk")[0] == (1 if mode == "fp64" else 0), note
        _same(out, case.oracle(weighted, masked, count_zero_weight=False), d, note)


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("d", gx.B_SYRK_D)
def test_syrk_family_b_exact(spy, mode, d):
    case = gx.family_b(d)
    for weighted, masked in case.combos:
        w, sel = _rows(case, weighted, masked)
        Xp, yp = case.poisoned(weighted, masked)
        spy.calls.clear()
        out = device.gram_stats(Xp.cuda(), yp.cuda(), w, sel, mode)
        note = f"{case.name} {mode} w={weighted} sel={masked}"
        assert spy.only("gram_syrk")[0] == (1 if mode == "fp64" else 0), note
        _same(out, case.oracle(weighted, masked, count_zero_weight=False), d, note)


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_syrk_one_live_row(spy, mode):
    """fp64: 24 x 24-bit products are exact in a double, the whole vector is ``==``.  fp32: ``==``
    on the f32-representable entries, today's 2e-5 on the rest."""
    c = gx.one_row(66)
    out = device.gram_stats(c.X.cuda(), c.y.cuda(), None, c.sel.cuda(), mode)
    assert spy.only("gram_syrk")[0] == (1 if mode == "fp64" else 0)
    ref = torch.from_numpy(c.ref)
    _same(out, ref, c.d, f"{c.name} {mode}", where=None if mode == "fp64" else c.exact)
    assert _rel(out, ref) < 2e-5
