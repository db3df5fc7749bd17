"""The patched (all-packed) companion of the tiled bf16 storage on the GPU: the device packer
against the torch reference bit for bit, and the tall Gram pass reading patched tiles against the
same pass on the raw tiles under ``torch.equal`` -- on inputs whose exceptions are known, with
the companion's kind, its counts and the kernel the launch resolves to asserted first, so no case
passes by falling back."""
import pytest
import torch

from packed_cases import clamped_gaussian
from patched_cases import check_records, with_exceptions

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device():
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    return device


def _plan(n, NT):
    """Exceptions for a blocks=2 grid (16 waves, wave w takes supersteps w, w + 16, w + 32):
    wave 0's first, second and (at 40 supersteps) last superstep -- both loop buffers and the
    left-over compute after the loop; wave 9's pair; two neighbours in storage; overflow entries
    in either buffer and in a wave's last superstep.  Only full supersteps."""
    full = n // 64
    plan = {(0, 0): 1, (16, NT - 1): 4, (32, 0): 3, (9, NT - 1): 1, (25, 0): 1, (3, 0): 1, (4, NT - 1): 2,
            (39, 0): 5, (23, NT - 1): 3, (38, 0): 1}
    return {k: v for k, v in plan.items() if k[0] < full}


def _ingest(X, d, n, want):
    """Patched and raw ingests of X; the device packer equals the reference bit for bit and holds
    the injected records."""
    from net.jgp.labs.sparkdq4ml_amd.ops.layout import PatchedTiles, patch_reference

    device = _device()
    Tp = device.tile_bf16(X.cuda(), shift=None, pack="patched")
    Tr = device.tile_bf16(X.cuda(), shift=None, pack=False)
    assert isinstance(Tp.packed, PatchedTiles) and Tp.packed.kind == "patched"
    assert Tr.packed is None and torch.equal(Tp.buf, Tr.buf)
    ref = patch_reference(Tp.buf.cpu(), d, n)
    assert torch.equal(Tp.packed.dir.cpu(), ref.dir)
    assert torch.equal(Tp.packed.a.cpu(), ref.a)
    assert torch.equal(Tp.packed.ovf.cpu(), ref.ovf)
    assert Tp.packed.nexc == ref.nexc == sum(len(r) for r in want.values())
    check_records(Tp.packed, d // 32, want)
    return Tp, Tr


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("n", [64, 64 * 40, 64 * 40 + 5])
def test_gram_patched_equals_raw(d, n):
    device = _device()
    X, want = with_exceptions(d, n, 11 * d + n, _plan(n, d // 32))
    Tp, Tr = _ingest(X, d, n, want)
    if n >= 64 * 40:
        assert Tp.packed.ovf.numel() == 9 and int((Tp.packed.counts > 0).sum()) == 10
    y = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n + d))
    assert device._tiled_pre(Tp, y, None, None, 0)[0] == "patched"
    a = device.gram_stats(Tp, y, None, None, "bf16", blocks=2)
    b = device.gram_stats(Tr, y, None, None, "bf16", blocks=2)
    assert torch.equal(a, b)
    # calls the patched kernel does not take read the raw tiles: same statistics as without a companion
    sel = torch.arange(n, device="cuda") % 3 != 0
    assert device._tiled_pre(Tp, y, None, sel, 1)[0] is None
    assert torch.equal(device.gram_stats(Tp, y, None, sel, "bf16", blocks=2),
                       device.gram_stats(Tr, y, None, sel, "bf16", blocks=2))
    assert torch.equal(device.gram_stats(Tp, y.double(), None, None, "bf16", blocks=2),
                       device.gram_stats(Tr, y.double(), None, None, "bf16", blocks=2))


def test_gram_patched_planned_grid():
    """The planned grid at 64 * 4096 rows: exceptions in the grid's first and last supersteps, in
    storage neighbours, in one wave's consecutive supersteps (1024 waves: s and s + 1024), on a
    stretch of every other superstep, and overflow entries."""
    device = _device()
    d, n = 32, 64 * 4096
    plan = {(s, 0): 1 for s in range(1000, 1400, 2)}
    plan.update({(0, 0): 3, (1, 0): 1, (2, 0): 4, (77, 0): 6, (1024, 0): 2, (1101, 0): 1, (3077, 0): 4, (4095, 0): 5})
    X, want = with_exceptions(d, n, 5, plan)
    Tp, Tr = _ingest(X, d, n, want)
    assert Tp.packed.npacked == 4096 and Tp.packed.ovf.numel() == 19
    y = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    assert device._tiled_pre(Tp, y, None, None, 0)[0] == "patched"
    assert torch.equal(device.gram_stats(Tp, y, None, None, "bf16"), device.gram_stats(Tr, y, None, None, "bf16"))


def test_packer_gaussian_and_rejects():
    """Unclamped N(0, 1) data (its own exceptions) against the reference, and the tables the
    device packer must refuse: one exception over the cap, d = 31, no full superstep."""
    from net.jgp.labs.sparkdq4ml_amd.ops.layout import PATCH_CAP, patch_reference

    device = _device()
    d, n = 64, 64 * 200 + 17
    X = torch.randn(d, n, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    T = device.tile_bf16(X.cuda(), shift=None, pack="patched")
    ref = patch_reference(T.buf.cpu(), d, n)
    assert T.packed.nexc == ref.nexc > 0
    assert torch.equal(T.packed.dir.cpu(), ref.dir) and torch.equal(T.packed.a.cpu(), ref.a)
    assert torch.equal(T.packed.ovf.cpu(), ref.ovf)
    n = 64 * 40
    X, _ = with_exceptions(32, n, 7, {(6, 0): PATCH_CAP})
    assert device.tile_bf16(X.cuda(), shift=None, pack="patched").packed.nexc == PATCH_CAP
    X, _ = with_exceptions(32, n, 7, {(6, 0): PATCH_CAP + 1})
    assert device.tile_bf16(X.cuda(), shift=None, pack="patched").packed is None
    assert device.tile_bf16(clamped_gaussian(31, n, 1).cuda(), shift=None, pack="patched").packed is None
    assert device.tile_bf16(clamped_gaussian(32, 63, 1).cuda(), shift=None, pack="patched").packed is None


def test_fit_replay_bitwise(gpu_session):
    """Two asynchronous fits of one DataFrame (the second replays the recorded launch): patched
    and raw ingests give the same coefficients and intercept bit for bit."""
    from net.jgp.labs.sparkdq4ml_amd import LinearRegression

    device = _device()
    gpu_session.conf.set("dq4ml.fit.async", "true")
    d, n = 32, 64 * 600 + 9
    X, _ = with_exceptions(d, n, 9, {(0, 0): 1, (1, 0): 4, (300, 0): 2, (599, 0): 5})
    X = X.cuda()
    y = (torch.linspace(-1, 1, d, device="cuda") @ X.float() + 0.3).float()
    got = {}
    for pack in ("patched", False):
        T = device.tile_bf16(X, pack=pack)
        if pack:
            assert T.packed.kind == "patched" and T.packed.nexc > 0 and T.packed.ovf.numel() > 0
        else:
            assert T.packed is None
        df = gpu_session.createDataFrame({"features": T, "label": y})
        lr = LinearRegression(solver="normal", gramDtype="bf16")
        ms = [lr.fit(df) for _ in range(2)]
        (replay,) = df.__dict__["_fit_replays"].values()  # the second fit found the recorded launch
        assert replay.plan.kind == (pack or None)
        got[pack] = [(m.coefficients.toArray().copy(), float(m.intercept)) for m in ms]
    for (ca, ia), (cb, ib) in zip(got["patched"], got[False]):
        assert (ca == cb).all() and ia == ib
    assert (got["patched"][0][0] == got["patched"][1][0]).all() and got["patched"][0][1] == got["patched"][1][1]


def _same_companion(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.kind == b.kind and torch.equal(a.dir, b.dir) and torch.equal(a.a, b.a)


def test_auto_policy(monkeypatch):
    from net.jgp.labs.sparkdq4ml_amd.ops.layout import PATCH_CAP

    device = _device()
    monkeypatch.setattr(device, "PACK_MIN_ROWS", 64 * 64)
    n = 64 * 128

    def auto(X, knob):
        if knob is None:
            monkeypatch.delenv("DQ4ML_TILE_PACK", raising=False)
        else:
            monkeypatch.setenv("DQ4ML_TILE_PACK", knob)
        return device.tile_bf16(X, shift=None).packed

    X = torch.randn(32, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(21)).to(torch.bfloat16)
    p = auto(X, None)
    assert p.kind == "patched" and p.npacked == 128 and 0 < p.nexc <= 128
    assert auto(X[:, :64 * 63], None) is None  # below the row threshold
    m = auto(X, "mixed")  # the knob's A/B value: today's mixed companion
    assert m.kind == "mixed" and _same_companion(m, device.tile_bf16(X, shift=None, pack=True).packed)
    assert auto(X, "0") is None
    # tables that do not take the patched form get exactly what the mixed-only policy gives them
    Z = X.clone()
    Z[:, torch.arange(n, device="cuda") % 64 < 48] = 0  # zero-heavy
    Z[:, :64 * 16] = clamped_gaussian(32, 64 * 16, 3).cuda()
    assert auto(Z, None) is None and auto(Z, "mixed") is None
    C, _ = with_exceptions(32, n, 8, {(5, 0): PATCH_CAP + 1})  # one entry over the cap: mixed, 127 packed
    got = auto(C.cuda(), None)
    assert got.kind == "mixed" and got.npacked == 127 and _same_companion(got, auto(C.cuda(), "mixed"))
    D31 = clamped_gaussian(31, n, 4).cuda()
    assert _same_companion(auto(D31, None), auto(D31, "mixed"))
    assert auto(D31, None) is None  # (padding feature: every entry holds zeros)
