"""The row-pass kernels of ``ops/csrc/hip/rowops.hip`` -- the Huber loss/gradient pass (host- and
device-steered), dense / tiled predict and regression metrics, column pack and compaction -- each
against the CPU engine's plain fp64 implementation (``ops/kernels.py``).

Oracle.  Always fp64 on the CPU, computed from the values the kernel reads, so storage rounding is
not part of the error: ``X.double()`` for dense storage; for tiled / wide storage the stored
elements widened to f64, times the fp8 scale, plus the shift (``_dense64``).  ``to_dense()`` itself
forms ``q * scale`` and ``x' + s`` in f32, a 2^-24 rounding the kernels do not make, so it is not
used for scaled or shifted storage.  ``kernels.huber_pass`` multiplies a dead row's features by a
zero multiplier (NaN * 0 = NaN); the oracle therefore gets a copy whose dead rows are zeroed, the
kernel the copy whose dead rows hold NaN.

Bound.  For every f64 sum ``|got_k - ref_k| <= 1e-12 * S_k`` with ``S_k`` the fp64 sum of the
absolute per-row terms of component k (for Σ m_r x_rj: Σ |m_r x_rj|), so cancelling components
cannot fail falsely.  1e-12 is the project's bound for f64 row reductions
(``test_gpu_kernels.py::test_predict_and_metrics``): the kernels make about 40 roundings per sum
(<= 2 serial rows per thread up to 2.1e6 rows, a 64-lane tree, 4 wave totals, the slab sum) on top
of (d + 3) * 2^-53 per term, i.e. ~5e-15 * S, while one dropped or duplicated row in 1e6 moves a
component by ~1e-6 * S.  Every test prints its largest ``|Δ| / S`` before it asserts.

Huber inputs.  Labels are margin + N(0, 2.6²) noise and σ ε = 1.3 * 1.35, the median of |noise|, so
about half the rows fall in each branch; each test asserts from the oracle alone that both
branches hold >= 20 % of the live rows whenever there are at least 20 live rows (one row cannot
be in both)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, kernels, native  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops.layout import TiledBF16, TiledWide  # noqa: E402
from net.jgp.labs.sparkdq4ml_amd.ops.shift import Shift  # noqa: E402

TOL = 1e-12
CAP_N = 4096 * 256 + 257       # the 4096 x 256 grids make a second grid-stride trip
PACK_CAP_N = 2048 * 256 + 300  # pack_kernel's 2048 x 256 grid
SIGMA, EPS = 1.3, 1.35
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    native.hip()


def _gen(*key):
    s = 0x9E3779B1
    for k in key:
        s = (s * 1000003 + int(k) + 12345) % (2 ** 61 - 1)
    return torch.Generator().manual_seed(s)


def _ceil64(n):
    return (n + 63) // 64 * 64


def _padded(X, fill):
    """``X`` as the ``[:, :n]`` view of a (d, ceil64(n) + 64) buffer whose padding holds ``fill``."""
    d, n = X.shape
    buf = torch.full((d, _ceil64(n) + 64), fill, dtype=X.dtype, device=X.device)
    buf[:, :n] = X
    return buf[:, :n]


def _dense64(T):
    """fp64 [d, n] on the CPU of exactly what the kernels read from ``T``."""
    if torch.is_tensor(T):
        return T.detach().cpu().to(torch.float64)
    d, n = T.shape
    if isinstance(T, TiledBF16):
        raw = TiledBF16(T.buf, d, n, None).to_dense().to(torch.float64)
    elif T.eb == 16:
        raw = TiledWide(T.buf, d, n, 16, None, None).to_dense().to(torch.float64)
    else:
        one = torch.ones(d, dtype=torch.float32, device=T.buf.device)
        raw = TiledWide(T.buf, d, n, 8, one, None).to_dense().to(torch.float64)
        raw = raw * T.scales.to(torch.float64).unsqueeze(1)  # (fp8 value) * (f32 scale): exact in f64
    if T.shift is not None:
        raw = raw + T.shift.dev64.to(raw.device).unsqueeze(1)
    return raw.cpu()


def _off_centre(d, n, g):
    """The columns of tests/test_gpu_centering.py: 1000 + N(0, 1), U(20, 200), 10 +- 0.5."""
    X = torch.randn(d, n, generator=g)
    X[0::3] += 1000.0
    X[1::3] = torch.rand(len(range(1, d, 3)), n, generator=g) * 180.0 + 20.0
    X[2::3] = X[2::3] * 0.5 + 10.0
    return X


def _rows(n, mode, g):
    """(w, sel, dead) of a row mode: weights f32 / f64 with exact zeros, a random selection."""
    w = sel = None
    if mode in ("w32sel", "w64"):
        w = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
        w[torch.rand(n, generator=g) < 0.15] = 0.0
        w = w.to(torch.float32 if mode == "w32sel" else torch.float64)
    if mode in ("w32sel", "sel"):
        sel = torch.rand(n, generator=g) < 0.75
    dead = torch.zeros(n, dtype=torch.bool)
    if w is not None:
        dead |= w == 0
    if sel is not None:
        dead |= ~sel
    return w, sel, dead


def _cuda(t):
    return None if t is None else t.cuda()


_YDT = {"plain": torch.float64, "w32sel": torch.float32, "w64": torch.float64, "sel": torch.float32}


# ------------------------------------------------------------------------------------------
# storage builders: (kind, ...) -> what the device ops take.  ``Xc`` is clean CPU data, ``dead`` the
# rows whose features may be poisoned (dense float storage only).
# ------------------------------------------------------------------------------------------
def _store(kind, Xc, dead):
    name = kind[0]
    if name == "dense":
        _, dt, layout = kind
        X = Xc.to(dt)
        if dead is not None and dead.any() and dt.is_floating_point:
            X[:, dead] = NAN
        X = X.cuda()
        if layout == "padded":
            X = _padded(X, NAN if dt.is_floating_point else 7_777_777)
        return X
    if name == "tall":
        return device.tile_bf16(Xc.cuda(), shift=None)
    if name == "tall_shift":
        sh = Shift(Xc.double().mean(1).numpy() if Xc.shape[1] else np.zeros(Xc.shape[0]), "cuda")
        return device.tile_bf16(Xc.cuda(), shift=sh)
    if name == "wide":
        return device.pack_wide([Xc.cuda()], kind[1], None, shift=None)
    if name == "wide_shift":
        sh = Shift(Xc.double().mean(1).numpy(), "cuda", uniform=True)
        return device.pack_wide([Xc.cuda()], kind[1], None, shift=sh)
    raise AssertionError(kind)


def _kind_id(kind):
    return "-".join(str(k).replace("torch.", "") for k in kind)


# ------------------------------------------------------------------------------------------
# A / B: the Huber pass
# ------------------------------------------------------------------------------------------
class _Huber:
    """One Huber problem: device inputs (poisoned dead rows) and the oracle's clean copies."""

    def __init__(self, kind, d, n, mode, seed):
        g = _gen(seed, d, n, len(mode), ord(mode[0]))
        self.d, self.n = d, n
        self.w, self.sel, dead = _rows(n, mode, g)
        shifted = kind[0].endswith("_shift")
        Xc = _off_centre(d, n, g) if shifted else torch.randn(d, n, generator=g) + 0.25
        if kind[0] == "dense" and kind[1] == torch.float64:
            Xc = Xc.double() + 1e-9 * torch.randn(d, n, generator=g, dtype=torch.float64)  # (all 53 bits in use)
        self.X = _store(kind, Xc, dead)
        D = _dense64(self.X)
        self.D = torch.where(dead.unsqueeze(0), torch.zeros_like(D), D)
        cs = (0.05 if shifted else 1.0) / math.sqrt(d)
        ctrue = torch.randn(d, generator=g, dtype=torch.float64) * cs
        y = ctrue @ self.D + 0.4 + 2.6 * torch.randn(n, generator=g, dtype=torch.float64)
        self.y = y.to(_YDT[mode])                      # as stored; the oracle reads the same values
        self.y_dev = self.y.clone()
        self.y_dev[dead] = NAN
        self.y_dev = self.y_dev.cuda()
        self.y = torch.where(dead, torch.zeros_like(self.y), self.y)
        # evaluated off the generating coefficients (by little on off-centre columns: |x| ~ 1000)
        pert = (0.003 if shifted else 0.1) * cs
        self.ceff = (ctrue + pert * torch.randn(d, generator=g, dtype=torch.float64)).numpy()
        self.icpt = 0.6
        self.live = ~dead

    def run(self):
        return device.huber_pass(self.X, self.y_dev, _cuda(self.w), _cuda(self.sel), self.ceff, self.icpt, SIGMA,
                                 EPS).cpu()

    def oracle(self):
        """(ref, S): kernels.huber_pass and the sums of the absolute per-row terms; asserts the
        branch condition."""
        ref = kernels.huber_pass(self.D, self.y, self.w, self.sel, self.ceff, self.icpt, SIGMA, EPS)
        wt = torch.ones(self.n, dtype=torch.float64) if self.w is None else self.w.to(torch.float64)
        wt = torch.where(self.live, wt, torch.zeros_like(wt))
        lin = self.y.to(torch.float64) - (torch.as_tensor(self.ceff) @ self.D + self.icpt)
        inside = lin.abs() <= SIGMA * EPS
        q = lin / SIGMA
        loss = torch.where(inside, 0.5 * wt * (SIGMA + lin * lin / SIGMA),
                           0.5 * wt * (SIGMA + 2.0 * EPS * lin.abs() - SIGMA * EPS * EPS))
        m = torch.where(inside, -wt * q, wt * torch.where(lin >= 0, -torch.ones_like(lin), torch.ones_like(lin)) * EPS)
        gs = torch.where(inside, 0.5 * wt * (1.0 - q * q), 0.5 * wt * (1.0 - EPS * EPS))
        S = torch.cat([torch.stack([loss.abs().sum(), wt.abs().sum(), m.abs().sum(), gs.abs().sum()]),
                       self.D.abs() @ m.abs()])
        nlive = int(self.live.sum())
        if nlive >= 20:
            fin = float((inside & self.live).sum()) / nlive
            assert 0.2 <= fin <= 0.8, f"Huber branch split {fin:.2f} of {nlive} live rows"
        return ref, S


def _check_sums(family, got, ref, S):
    assert got.shape == ref.shape
    assert torch.isfinite(got).all(), got
    err = (got - ref).abs()
    ratio = float(torch.where(S > 0, err / S.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
    print(f"ROWOPS {family} max|d|/S = {ratio:.3e}")
    bad = err > TOL * S
    assert not bad.any(), (family, ratio, bad.nonzero().flatten().tolist())


_HN = [1, 63, 64, 257, 20_011]
_MODES = ["plain", "w32sel", "w64", "sel"]

_FUSED = ([(("dense", dt, lay), d) for dt in (torch.float64, torch.float32) for d in (1, 5, 16)
           for lay in ("contig", "padded")]
          + [(("dense", torch.bfloat16, lay), d) for d in (3, 16) for lay in ("contig", "padded")]
          + [(("tall",), 7), (("tall",), 16), (("tall_shift",), 7), (("tall_shift",), 16),
             (("wide", 16), 16), (("wide", 8), 16)])
_XT_SMALL = ([(("dense", dt, lay), d) for dt in (torch.float32, torch.float64) for d in (17, 40)
              for lay in ("contig", "padded")] + [(("tall",), 33), (("tall_shift",), 33)])
_XT_WIDE = [(("wide", 16), 300), (("wide", 8), 300), (("wide_shift", 8), 300)]


def _family(kind, d):
    if d > 16:
        return "huber-xt"
    return "huber-dense" if kind[0] == "dense" and kind[1] != torch.bfloat16 else "huber-generic"


def _huber_case(kind, d, n, mode):
    p = _Huber(kind, d, n, mode, 1)
    ref, S = p.oracle()
    _check_sums(_family(kind, d), p.run(), ref, S)


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("n", _HN)
@pytest.mark.parametrize("kind,d", _FUSED, ids=[f"{_kind_id(k)}-d{d}" for k, d in _FUSED])
def test_huber_pass_fused(kind, d, n, mode):
    """d <= 16: the dense f32 / f64 pipelined kernel (contiguous, padded ld, d = 1) and the generic
    fused kernel (dense bf16, tall tiled plain and shifted, wide bf16 / fp8)."""
    _huber_case(kind, d, n, mode)


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("n", _HN + [70_001])
@pytest.mark.parametrize("kind,d", _XT_SMALL, ids=[f"{_kind_id(k)}-d{d}" for k, d in _XT_SMALL])
def test_huber_pass_xt(kind, d, n, mode):
    """d > 16: margin pass + Xᵀm over xt_chunks(n, d) row chunks (70 001 rows: two chunks)."""
    _huber_case(kind, d, n, mode)


@pytest.mark.parametrize("n,mode", [(1, "plain"), (63, "w32sel"), (64, "sel"), (257, "w64"), (20_011, "w32sel"),
                                    (20_011, "plain"), (70_001, "plain"), (70_001, "w32sel")])
@pytest.mark.parametrize("kind,d", _XT_WIDE, ids=[f"{_kind_id(k)}-d{d}" for k, d in _XT_WIDE])
def test_huber_pass_xt_wide(kind, d, n, mode):
    _huber_case(kind, d, n, mode)


def test_huber_pass_xt_chunks_capped():
    """d = 1025, n = 65 537: ceil(n / 65536) = 2 chunks capped to 2048 / d = 1."""
    _huber_case(("dense", torch.bfloat16, "contig"), 1025, 65_537, "w32sel")


@pytest.mark.parametrize("kind,d,mode", [(("dense", torch.float32, "contig"), 16, "w32sel"),
                                         (("dense", torch.float32, "contig"), 16, "plain"),
                                         (("dense", torch.float64, "padded"), 5, "plain"),
                                         (("dense", torch.float32, "contig"), 17, "plain"),
                                         (("tall",), 16, "sel"), (("tall",), 16, "plain")],
                         ids=["dense-f32-d16-w32sel", "dense-f32-d16", "dense-f64-padded-d5", "dense-f32-d17",
                              "tall-d16-sel", "tall-d16"])
def test_huber_pass_crosses_grid_cap(kind, d, mode):
    """n = 4096 * 256 + 257: the first 257 threads make a second grid-stride trip (the dense
    kernel's software pipeline carries a row between trips only here)."""
    _huber_case(kind, d, CAP_N, mode)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32, torch.bfloat16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("d", [1, 5, 16, 17, 40])
def test_huber_pass_no_rows(d, dt):
    """n = 0 (an action whose filter keeps no row): all zeros, no error.  For d > 16 the single Xᵀm
    chunk is empty."""
    X = torch.empty(d, 0, dtype=dt, device="cuda")
    y = torch.empty(0, dtype=torch.float64, device="cuda")
    for XX in (X, _padded(X, NAN)):
        out = device.huber_pass(XX, y, None, None, np.ones(d), 0.5, SIGMA, EPS)
        assert out.shape == (4 + d,) and torch.equal(out.cpu(), torch.zeros(4 + d, dtype=torch.float64))
    w = torch.empty(0, dtype=torch.float32, device="cuda")
    sel = torch.empty(0, dtype=torch.bool, device="cuda")
    out = device.huber_pass(X, y, w, sel, np.ones(d), 0.5, SIGMA, EPS)
    assert torch.equal(out.cpu(), torch.zeros(4 + d, dtype=torch.float64))


# ---- B: the device-steered entry, through the binding (device.huber_fit_dp's argument packing) ----
def _pass_dev(p, act_value, fill=7.0):
    h = native.hip()
    X, d, n = p.X, p.d, p.n
    Xb, xdt, ld, tiled = device._x_args(X)
    y, w, sel = device._prep_rows(p.y_dev, _cuda(p.w), _cuda(p.sel), n)
    fp8 = isinstance(X, TiledWide) and X.eb == 8
    scale = X.scales.to(torch.float64).contiguous() if fp8 else None
    sh = getattr(X, "shift", None)
    shift = None if sh is None else sh.dev64.contiguous()
    c = torch.as_tensor(p.ceff, device="cuda")
    if fp8:
        c = c * scale
    tail = torch.tensor([device._icpt(X, p.ceff, p.icpt), SIGMA], dtype=torch.float64, device="cuda")
    trial = torch.cat([c, tail]).contiguous()
    act = torch.tensor([act_value], dtype=torch.int32, device="cuda")
    mult = torch.full((max(n, 1) if d > 16 else 1,), fill, dtype=torch.float64, device="cuda")
    partials = torch.full((int(h.huber_partials(n, d)),), fill, dtype=torch.float64, device="cuda")
    out = torch.full((4 + d,), fill, dtype=torch.float64, device="cuda")
    h.huber_pass_dev(Xb.data_ptr(), xdt, int(ld), d, n, tiled, y.data_ptr(), device.dtype_code(y), device._ptr(w),
                     device.dtype_code(w) if w is not None else 0, device._ptr(sel), trial.data_ptr(),
                     act.data_ptr(), float(EPS), device._ptr(scale), device._ptr(shift), mult.data_ptr(),
                     partials.data_ptr(), out.data_ptr(), device._stream())
    torch.cuda.synchronize()
    return out.cpu(), partials.cpu(), mult.cpu()


_DEV_PLAIN = [(("dense", torch.float32, "contig"), 16), (("dense", torch.float64, "padded"), 17), (("tall",), 16)]
_DEV_EPI = [(("wide", 8), 16), (("wide_shift", 8), 16), (("wide_shift", 8), 300), (("tall_shift",), 16),
            (("tall_shift",), 33), (("wide_shift", 16), 300)]
_DEV_ALL = _DEV_PLAIN + _DEV_EPI
_DEV_IDS = [f"{_kind_id(k)}-d{d}" for k, d in _DEV_ALL]


@pytest.mark.parametrize("mode", ["plain", "w32sel"])
@pytest.mark.parametrize("kind,d", _DEV_ALL, ids=_DEV_IDS)
def test_huber_pass_dev_bit_identical_to_host_steered(kind, d, mode):
    """act = HUBER_EVAL, trial = [ceff | icpt | sigma]: the same kernels in the same order as
    device.huber_pass, and the in-kernel scale / shift epilogue makes the same two roundings as
    the host-steered torch expressions -> the same bits (and so the oracle's sums)."""
    p = _Huber(kind, d, 20_011, mode, 2)
    out, _, _ = _pass_dev(p, int(native.hip().HUBER_EVAL))
    host = p.run()
    assert torch.equal(out, host), (out - host).abs().max()
    ref, S = p.oracle()
    _check_sums(_family(kind, d) + "-dev", out, ref, S)


@pytest.mark.parametrize("kind,d", _DEV_ALL, ids=_DEV_IDS)
def test_huber_pass_dev_done_touches_nothing(kind, d):
    """act = HUBER_DONE: every kernel of the pass (and the epilogue) returns before its first
    store -- out, partials and mult keep their fill."""
    p = _Huber(kind, d, 20_011, "w32sel", 3)
    for t in _pass_dev(p, int(native.hip().HUBER_DONE)):
        assert torch.equal(t, torch.full_like(t, 7.0))


# ------------------------------------------------------------------------------------------
# C: predict and regression metrics
# ------------------------------------------------------------------------------------------
def _features(kind, d, n, g):
    if kind[0] == "dense" and kind[1] == torch.int32:
        return torch.randint(-50, 50, (d, n), generator=g).to(torch.float32)
    X = torch.randn(d, n, generator=g) + 0.25
    if kind[0] == "dense" and kind[1] == torch.float64:
        X = X.double() + 1e-9 * torch.randn(d, n, generator=g, dtype=torch.float64)
    return X


_PDT = [torch.float64, torch.float32, torch.bfloat16, torch.int32]


def _predict_case(kind, d, n):
    g = _gen(11, d, n)
    X = _store(kind, _features(kind, d, n, g), None)
    coef = (torch.randn(d, generator=g, dtype=torch.float64) / math.sqrt(d)).numpy()
    b = 0.25
    got = device.predict(X, coef, b).cpu()
    D = _dense64(X)
    ref = kernels.predict(D, coef, b)
    S = abs(b) + torch.as_tensor(coef).abs() @ D.abs()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got - ref).abs()
    print(f"ROWOPS predict max|d|/S = {float((err / S).max()) if n else 0.0:.3e}")
    assert bool((err <= TOL * S).all()), float((err / S).max())


@pytest.mark.parametrize("layout", ["contig", "padded"])
@pytest.mark.parametrize("n", [1, 255, 256, 10_007])
@pytest.mark.parametrize("d", [1, 7, 65])
@pytest.mark.parametrize("dt", _PDT, ids=["f64", "f32", "bf16", "i32"])
def test_predict_dense(dt, d, n, layout):
    _predict_case(("dense", dt, layout), d, n)


def test_predict_crosses_grid_cap():
    _predict_case(("dense", torch.float32, "contig"), 7, CAP_N)


def test_predict_no_rows():
    out = device.predict(torch.empty(3, 0, dtype=torch.float32, device="cuda"), np.ones(3), 1.0)
    assert out.shape == (0,) and out.dtype == torch.float64


_LDT = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64}
_MSTORE = [(("dense", torch.float64, "contig"), 7, 10_007), (("dense", torch.float32, "padded"), 65, 4_099),
           (("dense", torch.int32, "padded"), 1, 10_007), (("tall",), 7, 10_007), (("tall",), 40, 4_099),
           (("tall_shift",), 7, 4_099), (("wide", 16), 300, 4_099), (("wide", 8), 300, 4_099)]


def _metrics_case(kind, d, n, ldt, selkind):
    g = _gen(13, d, n, len(selkind), ord(ldt[1]))
    sel = {"none": None, "random": torch.rand(n, generator=g) < 0.7, "allfalse": torch.zeros(n, dtype=torch.bool),
           "alltrue": torch.ones(n, dtype=torch.bool)}[selkind]
    dead = torch.zeros(n, dtype=torch.bool) if sel is None else ~sel
    Xc = _off_centre(d, n, g) if kind[0] == "tall_shift" else _features(kind, d, n, g)
    X = _store(kind, Xc, dead)
    D = _dense64(X)
    D = torch.where(dead.unsqueeze(0), torch.zeros_like(D), D)
    cs = (0.05 if kind[0] == "tall_shift" else 1.0) / math.sqrt(d)
    coef = (torch.randn(d, generator=g, dtype=torch.float64) * cs).numpy()
    b = 0.25
    yt = _LDT[ldt]
    y = torch.as_tensor(coef) @ D + 3.0 + 2.0 * torch.randn(n, generator=g, dtype=torch.float64)
    y = (y.round() if not yt.is_floating_point else y).to(yt)
    y_dev = y.clone()
    y_dev[dead] = NAN if yt.is_floating_point else 2_000_000_000  # garbage where a float label holds NaN
    live = ~dead
    p = kernels.predict(D, coef, b)
    for shift in (0.0, float(y.double()[live].mean()) if live.any() else 2.5):
        got = device.regression_metrics(X, y_dev.cuda(), coef, b, _cuda(sel), shift).cpu()
        ref = kernels.regression_metrics(D, y, coef, b, sel, shift)
        yd, pl = y.double()[live], p[live]
        ys, ps, res = yd - shift, pl - shift, yd - pl
        S = torch.stack([torch.tensor(float(yd.numel()), dtype=torch.float64), ys.abs().sum(), (ys * ys).sum(),
                         res.abs().sum(), (res * res).sum(), res.abs().sum(), ps.abs().sum(), (ps * ps).sum()])
        assert float(got[0]) == float(ref[0]) == float(live.sum())  # the live-row count, exactly
        _check_sums("metrics-dense" if kind[0] == "dense" else "metrics-tiled", got, ref, S)
        if not live.any():
            assert torch.equal(got, torch.zeros(8, dtype=torch.float64))


@pytest.mark.parametrize("selkind", ["none", "random", "allfalse", "alltrue"])
@pytest.mark.parametrize("ldt", list(_LDT))
@pytest.mark.parametrize("kind,d,n", _MSTORE, ids=[f"{_kind_id(k)}-d{d}" for k, d, _ in _MSTORE])
def test_regression_metrics(kind, d, n, ldt, selkind):
    """Dense (metrics_kernel, any label dtype code), tall tiled (tiled_rows_kernel<1, f64 | f32 | -1, 1>)
    and wide storage; dead rows hold NaN features (dense float storage) and a NaN / garbage label."""
    _metrics_case(kind, d, n, ldt, selkind)


@pytest.mark.parametrize("kind,d,ldt", [(("dense", torch.float32, "contig"), 7, "f32"), (("tall",), 7, "i32")],
                         ids=["dense-f32", "tall-i32"])
def test_regression_metrics_crosses_grid_cap(kind, d, ldt):
    _metrics_case(kind, d, CAP_N, ldt, "random")


@pytest.mark.parametrize("ldt", list(_LDT))
def test_regression_metrics_no_rows(ldt):
    X = torch.empty(4, 0, dtype=torch.float64, device="cuda")
    y = torch.empty(0, dtype=_LDT[ldt], device="cuda")
    for sel in (None, torch.empty(0, dtype=torch.bool, device="cuda")):
        out = device.regression_metrics(X, y, np.ones(4), 0.5, sel, 1.0)
        assert torch.equal(out.cpu(), torch.zeros(8, dtype=torch.float64))


# ------------------------------------------------------------------------------------------
# D: pack and compaction edges
# ------------------------------------------------------------------------------------------
def _pack_sources(n, g):
    """(device parts, their CPU f64 values [10, n], bad): the f32 and f64 sources hold NaN in `bad` rows."""
    bad = torch.rand(n, generator=g) < 0.2
    f32 = torch.randn(n, generator=g)
    f64 = torch.randn(n, generator=g, dtype=torch.float64)
    f32[bad] = NAN
    f64[bad] = NAN
    rowmajor = torch.randn(n, 2, generator=g)  # its column 1 is a row view of element stride 2
    cpu = [torch.randint(-(1 << 24), 1 << 24, (n,), generator=g, dtype=torch.int32),
           torch.randint(-(1 << 24), (1 << 24) + 1, (n,), generator=g, dtype=torch.int64),
           torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8),
           torch.rand(n, generator=g) < 0.5,
           f32, f64,
           (torch.randn(n, generator=g) * 3).to(torch.bfloat16),
           rowmajor[:, 1],
           torch.randn(2, n, generator=g, dtype=torch.float64)]
    parts = [c.cuda() for c in cpu]
    parts[7] = rowmajor.cuda()[:, 1]
    assert not parts[7].is_contiguous() or n == 1
    vals = torch.cat([c.reshape(-1, n).to(torch.float64) for c in cpu])
    return parts, vals, bad


def _rne_bf16(v64):
    """f64 -> the nearest bf16, ties to even, in ONE rounding (normal range only).  torch's
    ``.to(bfloat16)`` rounds an f64 to f32 first; when that lands exactly between two bf16 values
    the second rounding can go the other way (about 1 f64 value in 2^17).  The kernel stores the
    correctly rounded value."""
    drop = 52 - 7
    bits = v64.contiguous().view(torch.int64)
    r = (bits + ((1 << (drop - 1)) - 1) + ((bits >> drop) & 1)) & ~((1 << drop) - 1)
    r = torch.where(torch.isnan(v64), bits, r)
    return r.view(torch.float64).to(torch.bfloat16)  # (exactly representable now)


def _nan_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.to(torch.float64), b.to(torch.float64)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("odt", [torch.float64, torch.float32, torch.bfloat16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, PACK_CAP_N])
def test_pack_columns_exact(n, odt):
    """Every source dtype, a non-contiguous row view and a 2-D part, to every output dtype: equal
    to the source value rounded once to the output type, dead rows exactly 0 even where the source
    holds NaN, and the padding [n, ceil64(n)) zero.  n = 2048 * 256 + 300: second grid-stride trip
    (and enough f64 values for a few to round to f32 onto a bf16 tie, see _rne_bf16)."""
    g = _gen(17, n)
    parts, vals, bad = _pack_sources(n, g)

    def expect(v64):  # the source value, rounded once to the output type
        return _rne_bf16(v64) if odt == torch.bfloat16 else v64.to(odt)

    def padding_is_zero(out):
        base = out._base
        assert base is not None and base.shape == (vals.shape[0], _ceil64(n))
        return not base[:, n:].cpu().to(torch.float64).any()

    for s in (~bad & (torch.rand(n, generator=g) < 0.8), ~bad):  # every NaN row is dead
        out = device.pack_columns(parts, odt, s.cuda())
        ref = expect(torch.where(s.unsqueeze(0), vals, torch.zeros_like(vals)))
        assert out.shape == ref.shape == (10, n) and out.dtype == odt
        assert torch.equal(out.cpu(), ref)
        assert padding_is_zero(out)
    out = device.pack_columns(parts, odt)  # no selection: NaN passes through, all else exact
    assert _nan_equal(out.cpu(), expect(vals))
    assert padding_is_zero(out)


@pytest.mark.parametrize("n", [1, 4096, 4096 * 3, 4096 * 3 + 1])
@pytest.mark.parametrize("selkind", ["alltrue", "allfalse", "random"])
def test_compact_indices_edges(n, selkind):
    g = _gen(19, n)
    sel = {"alltrue": torch.ones(n, dtype=torch.bool), "allfalse": torch.zeros(n, dtype=torch.bool),
           "random": torch.rand(n, generator=g) < 0.5}[selkind]
    full = torch.nonzero(sel).flatten()
    live = int(full.numel())
    for limit in (None, 0, 1, live, live + 5, n + 100):
        got = device.compact_indices(sel.cuda(), limit)
        ref = full if limit is None else full[:limit]
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref), (limit, live)
