"""The one launch path of the tiled bf16 Gram pass: ``gram_stats`` on a tiled table,
``TiledGramPlan.launch`` and the deferred launch give the same bits on raw, mixed and patched
tables for every set of row operands, the companion each launch reads is the documented one, and
the unified ``gram_tall`` binding refuses every inconsistent companion before it launches.

Shapes (blocks=1: 8 waves, wave w takes supersteps w, w + 8, ...): 29 supersteps + 7 rows gives
waves 0..4 four supersteps and waves 5..7 three -- even and odd trip counts of the pair loops --
plus the ragged tail; 3 supersteps give fewer supersteps than waves and no tail."""
import functools

import pytest
import torch

from patched_cases import with_exceptions

pytestmark = pytest.mark.gpu

SHAPES = [64 * 29 + 7, 64 * 3]
ROWS = ["none", "sel", "w", "w+sel"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device():
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    return device


def _plan(n, NT):
    """Exceptions per entry (s, t), at most one per entry of the table on average (PATCH_SHARE).
    29 supersteps: every superstep of wave 0 (s = 0, 8, 16, 24) and of wave 5 (5, 13, 21: an odd
    trip count, the left-over compute), the last full superstep and storage neighbours; counts
    1..3 stay inline, larger ones go to the overflow table.  3 supersteps: the first and the last,
    and at d = 64 (six entries) an overflow entry between them."""
    if n // 64 == 3:
        return {(0, 0): 1, (2, 0): 2} if NT == 1 else {(0, 0): 1, (1, 1): 4, (2, 0): 1}
    return {(0, 0): 1, (1, NT - 1): 4, (8, NT - 1): 4, (16, 0): 3, (24, NT - 1): 5, (5, 0): 2, (13, NT - 1): 1,
            (21, 0): 4, (28, 0): 1, (27, NT - 1): 2}


@functools.lru_cache(maxsize=None)
def _tables(d, n):
    """The three ingests of one matrix whose exceptions are known: inline and overflow records in
    the patched form, raw entries in the mixed form."""
    from net.jgp.labs.sparkdq4ml_amd.ops.layout import RAW_ENTRY

    device = _device()
    X, want = with_exceptions(d, n, 3 * d + n, _plan(n, d // 32))
    T = {pack: device.tile_bf16(X.cuda(), shift=None, pack=pack) for pack in (False, True, "patched")}
    assert T[False].packed is None
    m, p = T[True].packed, T["patched"].packed
    nraw = int((m.dir == RAW_ENTRY).sum())
    ragged = d // 32 if n % 64 else 0  # (the zero-padded last superstep: zeros beside values, raw)
    assert m.kind == "mixed" and nraw == len(want) + ragged and m.npacked == m.dir.numel() - nraw > 0
    assert p.kind == "patched" and p.nexc == sum(len(r) for r in want.values())
    novf = sum(len(r) for r in want.values() if len(r) > 3)
    assert p.ovf.numel() == novf and (novf > 0 or p.counts.numel() == 3)
    assert int(((p.counts > 0) & (p.counts <= 3)).sum()) == sum(1 for r in want.values() if len(r) <= 3) > 0
    return T


def _operands(n, rows, ydt):
    g = torch.Generator(device="cuda").manual_seed(n + len(rows))
    y = torch.randn(n, device="cuda", generator=g).to(ydt)
    w = (torch.rand(n, device="cuda", generator=g) + 0.5).to(ydt) if "w" in rows else None
    sel = (torch.arange(n, device="cuda") % 3 != 0) if "sel" in rows else None
    return y, w, sel


@pytest.mark.parametrize("ydt", [torch.float32, torch.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("d", [32, 64])
def test_three_launchers_three_tables(d, n, rows, ydt):
    from net.jgp.labs.sparkdq4ml_amd.ops import native

    device, h = _device(), native.hip()
    y, w, sel = _operands(n, rows, ydt)
    xmode = 2 if w is not None else (1 if sel is not None else 0)
    plain = ydt == torch.float32 and w is None and sel is None
    st = torch.cuda.current_stream().cuda_stream
    ref = None
    for pack, T in _tables(d, n).items():
        kind = "mixed" if pack is True else ("patched" if pack == "patched" and plain else None)
        assert device._tiled_pre(T, y, w, sel, xmode)[0] == kind
        plan = device.TiledGramPlan(h, T, y, w, sel, False, blocks=1)
        assert plan.kind == kind and plan.nb == 1 and plan.packed == (pack is not False)
        a = device.gram_stats(T, y, w, sel, "bf16", blocks=1)
        b = plan.launch(st, False)
        c = plan.launch(st, True)
        assert isinstance(c, device.DeferredGram)
        c = c.finish()
        assert torch.equal(a, b) and torch.equal(a, c)
        if ref is None:
            ref = a  # the pack=False table
            assert bool(torch.isfinite(ref).all()) and float(ref[0]) == (n if sel is None else int(sel.sum()))
        assert torch.equal(a, ref)


def _args(T, y, n=None, **over):
    """``gram_tall``'s positional arguments for the tiled table ``T`` with its companion; ``over``
    replaces single ones."""
    p = T.packed
    a = dict(mode=2, X=T.buf.data_ptr(), ld=0, d=T.d, n=T.n if n is None else n, xdt=2, tiled=1, xshift=0,
             xpack=p.a.data_ptr(), xdir=0, xrec=0, xovf=0, y=y.data_ptr(), ydt=1, w=0, wdt=0, sel=0, xmode=0)
    if p.kind == "patched":
        a.update(xrec=p.dir.data_ptr(), xovf=p.ovf.data_ptr())
    else:
        a.update(xdir=p.dir.data_ptr())
    assert set(over) <= set(a)
    a.update(over)
    return tuple(a.values())


def test_gram_tall_rejects_bad_companions():
    """Every refusal is raised on the host before a launch (the arguments of a case that also
    shifts a pointer cover one superstep less, so they would stay in bounds anyway).  The last
    lines run the same argument builder unchanged: the order of the arguments is the binding's."""
    from net.jgp.labs.sparkdq4ml_amd.ops import native

    device, h = _device(), native.hip()
    d, n = 32, SHAPES[0]
    T = _tables(d, n)
    Tm, Tp = T[True], T["patched"]
    y = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    w = torch.ones(n, device="cuda")
    sel = torch.ones(n, dtype=torch.bool, device="cuda")
    P = int(h.gram_partial_stride(2, d))
    partials = torch.empty(P, dtype=torch.float64, device="cuda")
    out = torch.empty(device.gram_layout_size(d), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch(args):
        h.gram_tall(*args, partials.data_ptr(), 1, out.data_ptr(), st, True)

    short = n - 64
    bad = {
        "patched, xmode 1": _args(Tp, y, sel=sel.data_ptr(), xmode=1),
        "patched, selection": _args(Tp, y, sel=sel.data_ptr()),
        "patched, weights": _args(Tp, y, w=w.data_ptr(), wdt=1, xmode=2),
        "patched, f64 label": _args(Tp, y, ydt=0),
        "patched, d % 32": _args(Tp, y, d=16),
        "patched, no full superstep": _args(Tp, y, n=63),
        "patched, no overflow table": _args(Tp, y, xovf=0),
        "patched, records not 16-byte aligned": _args(Tp, y, short, xrec=Tp.packed.dir.data_ptr() + 4),
        "patched, slots not 16-byte aligned": _args(Tp, y, short, xpack=Tp.packed.a.data_ptr() + 4),
        "patched, f32 storage": _args(Tp, y, xdt=1),
        "patched records without slots": _args(Tp, y, xpack=0),
        "directory without slots": _args(Tm, y, xpack=0),
        "slots without a directory": _args(Tm, y, xdir=0),
        "two directories": _args(Tm, y, xrec=Tp.packed.dir.data_ptr(), xovf=Tp.packed.ovf.data_ptr()),
        "mixed, not tiled": _args(Tm, y, tiled=0),
        "mixed, f64 mode": _args(Tm, y, mode=0),
        "mixed, weights without xmode 2": _args(Tm, y, w=w.data_ptr(), wdt=1, xmode=0),
        "mixed, bf16 label": _args(Tm, y, ydt=2),
        "mixed, directory not word aligned": _args(Tm, y, short, xdir=Tm.packed.dir.data_ptr() + 1),
        "mixed, slots not 16-byte aligned": _args(Tm, y, short, xpack=Tm.packed.a.data_ptr() + 4),
    }
    for what, args in bad.items():
        with pytest.raises(ValueError):
            launch(args)
            pytest.fail(f"gram_tall accepted: {what}")
    for Tc in (Tm, Tp):
        launch(_args(Tc, y))
        assert torch.equal(out, device.gram_stats(Tc, y, None, None, "bf16", blocks=1))


def _dense_args(mode, feats, n, label, select, **over):
    """``gram_tall``'s positional arguments for a dense feature-major ``feats[:, :n]`` (row stride:
    the buffer's) with a selection; ``over`` replaces single ones."""
    device = _device()
    a = dict(mode=mode, X=feats.data_ptr(), ld=feats.stride(0), d=feats.shape[0], n=n, xdt=device.dtype_code(feats),
             tiled=0, xshift=0, xpack=0, xdir=0, xrec=0, xovf=0, y=label.data_ptr(), ydt=device.dtype_code(label), w=0,
             wdt=0, sel=select.data_ptr(), xmode=1)
    assert set(over) <= set(a)
    a.update(over)
    return tuple(a.values())


def test_gram_tall_rejects_unstreamable_dense_operands():
    """fp64 mode above the skinny kernel's d and bf16 mode on f32 storage have one kernel, the
    stream kernel: operands that it cannot take (16-byte alignment, f32 / f64 dtypes) are refused
    on the host before a launch, where a fallback kernel used to take them.  Every buffer is longer
    than the rows used (labels and selection by two elements, each feature row by four, which
    keeps f32 and f64 rows 16-byte aligned), so an accepted call would still read in bounds.  The
    last lines run the same argument builder unchanged with the aligned operands."""
    from net.jgp.labs.sparkdq4ml_amd.ops import native

    device, h = _device(), native.hip()
    n = 128
    g = torch.Generator(device="cuda").manual_seed(7)
    sel = torch.arange(n + 2, device="cuda") % 3 != 0
    st = torch.cuda.current_stream().cuda_stream
    ops = {}
    for name, mode, d, xdt, ydt in (("fp64", 0, 16, torch.float64, torch.float64), ("bf16", 2, 32, torch.float32, torch.float32)):
        X = torch.randn(d, n + 4, device="cuda", generator=g).to(xdt)
        y = torch.randn(n + 2, device="cuda", generator=g).to(ydt)
        ops[name] = (mode, X, y)
    (m64, X64, y64), (m16, X32, y32) = ops["fp64"], ops["bf16"]
    bad = {
        "fp64, label not 16-byte aligned": (X64, _dense_args(m64, X64, n, y64, sel, y=y64.data_ptr() + 8)),
        "fp64, feature rows not 16-byte aligned": (X64, _dense_args(m64, X64, n, y64, sel, ld=n + 1)),
        "fp64, selection not word aligned": (X64, _dense_args(m64, X64, n, y64, sel, sel=sel.data_ptr() + 1)),
        "bf16 on f32 storage, label not 16-byte aligned": (X32, _dense_args(m16, X32, n, y32, sel, y=y32.data_ptr() + 4)),
    }

    def launch(X, args):
        mode, d = args[0], X.shape[0]
        partials = torch.empty(int(h.gram_partial_stride(mode, d)), dtype=torch.float64, device="cuda")
        out = torch.empty(device.gram_layout_size(d), dtype=torch.float64, device="cuda")
        h.gram_tall(*args, partials.data_ptr(), 1, out.data_ptr(), st, True)
        return out

    for what, (X, args) in bad.items():
        with pytest.raises(ValueError):
            launch(X, args)
            pytest.fail(f"gram_tall accepted: {what}")
    for name, (mode, X, y) in ops.items():
        out = launch(X, _dense_args(mode, X, n, y, sel))
        assert torch.equal(out, device.gram_stats(X[:, :n], y[:n], None, sel[:n], name, blocks=1))
