"""The 12-bit packed companion of the tiled bf16 storage on the GPU: the device packer against the
torch reference bit for bit, and the tall Gram pass reading packed tiles against the same pass on
the raw tiles under ``torch.equal`` -- on inputs whose packed / raw mix is known and asserted first,
so no case passes by silently going raw."""
import pytest
import torch

from packed_cases import all_patterns, clamped_gaussian, expected_dir, inject, raw_patterns, specials

pytestmark = pytest.mark.gpu

RAW = 0xFF


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device():
    from net.jgp.labs.sparkdq4ml_amd.ops import device

    return device


def _mix(d, n, seed):
    X = clamped_gaussian(d, n, seed)
    return inject(X, raw_patterns(n))


def _check_packer(X):
    """Device ``pack_tiles`` == ``pack_reference``: the directory everywhere, the slots of packed
    entries, and zero-filled slots elsewhere."""
    from net.jgp.labs.sparkdq4ml_amd.ops.layout import SLOT_DWORDS, pack_reference

    device = _device()
    T = device.tile_bf16(X.cuda(), shift=None, pack=True)
    ref = pack_reference(T.buf.cpu())
    assert torch.equal(T.packed.dir.cpu(), ref.dir)
    assert torch.equal(T.packed.dir.cpu(), expected_dir(X))
    assert torch.equal(T.packed.a.cpu().view(-1, SLOT_DWORDS), ref.a.view(-1, SLOT_DWORDS))
    assert T.packed.npacked == ref.npacked
    return T


def test_packer_all_patterns():
    T = _check_packer(all_patterns(shuffle=False))
    assert T.packed.dir.cpu().tolist() == [16 * (s // 2) for s in range(32)]
    T = _check_packer(all_patterns(shuffle=True))
    assert T.packed.npacked == 0


def test_packer_specials():
    T = _check_packer(specials())
    assert T.packed.dir.cpu().tolist() == [0, 240, RAW, RAW]


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64])
def test_packer_shapes(d):
    for n in (1, 63, 64, 65, 64 * 7 + 17):
        _check_packer(_mix(d, n, seed=100 * d + n))


def _assert_mix(T, d, n):
    """The directory is the constructed mix: whole entries pack unless injected, the rest is raw."""
    NT, full = (d + 31) // 32, n // 64
    dirs = T.packed.dir.cpu().view(-1, NT)
    raw = set(raw_patterns(n))
    for s in range(dirs.shape[0]):
        for t in range(NT):
            packs = s < full and 32 * (t + 1) <= d and s not in raw
            assert (int(dirs[s, t]) != RAW) == packs, (s, t)
    return dirs


@pytest.mark.parametrize("d", [1, 5, 32, 33, 64])
@pytest.mark.parametrize("n", [1, 64, 65, 64 * 40 + 5])
def test_gram_packed_equals_raw(d, n):
    device = _device()
    X = _mix(d, n, seed=7 * d + n).cuda()
    g = torch.Generator(device="cuda").manual_seed(n + d)
    y = torch.randn(n, generator=g, device="cuda")
    sel = torch.rand(n, generator=g, device="cuda") > 0.3
    w = torch.rand(n, generator=g, device="cuda") + 0.5
    Tp = device.tile_bf16(X, shift=None, pack=True)
    Tr = device.tile_bf16(X, shift=None, pack=False)
    dirs = _assert_mix(Tp, d, n)
    if d in (32, 64) and n >= 64 * 40:
        assert (dirs != RAW).any() and (dirs == RAW).any()
    assert Tr.packed is None and torch.equal(Tp.buf, Tr.buf)
    for ww, ss in ((None, None), (None, sel), (w, None), (w, sel)):
        a = device.gram_stats(Tp, y, ww, ss, "bf16", blocks=2)
        b = device.gram_stats(Tr, y, ww, ss, "bf16", blocks=2)
        assert torch.equal(a, b), (d, n, ww is not None, ss is not None)


@pytest.mark.parametrize("d", [32, 64])
def test_gram_packed_equals_raw_shifted(d):
    """Shifted storage: an f32 column with mean 1000 is stored as x - 1000, so its tile still packs
    (a tiny value in that column is stored as -1000 beside values below 8: raw all the same)."""
    import numpy as np

    from net.jgp.labs.sparkdq4ml_amd.ops.shift import Shift

    device = _device()
    n = 64 * 40 + 5
    X = clamped_gaussian(d, n, seed=d).float()
    X[3] += 1000.0
    X = inject(X, raw_patterns(n)).cuda()
    s = np.zeros(d)
    s[3] = 1000.0
    y = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    Tp = device.tile_bf16(X, shift=Shift(s, X.device), pack=True)
    Tr = device.tile_bf16(X, shift=Shift(s, X.device), pack=False)
    assert Tp.shift is not None and torch.equal(Tp.buf, Tr.buf)
    _assert_mix(Tp, d, n)
    assert Tp.packed.npacked > 0 and (Tp.packed.dir == RAW).any()
    for ss in (None, torch.arange(n, device="cuda") % 3 != 0):
        assert torch.equal(device.gram_stats(Tp, y, None, ss, "bf16", blocks=2),
                           device.gram_stats(Tr, y, None, ss, "bf16", blocks=2))


def test_gram_packed_planned_grid():
    device = _device()
    d, n = 32, 64 * 4096
    X = inject(clamped_gaussian(d, n, 5), [0, 1, 2, 77, 4095] + list(range(1000, 1400, 2))).cuda()
    y = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    Tp = device.tile_bf16(X, shift=None, pack=True)
    Tr = device.tile_bf16(X, shift=None, pack=False)
    assert Tp.packed.npacked == 4096 - 205
    assert torch.equal(device.gram_stats(Tp, y, None, None, "bf16"), device.gram_stats(Tr, y, None, None, "bf16"))


def test_fit_replay_bitwise(gpu_session):
    """Two asynchronous fits of one DataFrame (the second replays the recorded launch): packed and
    raw ingests give the same coefficients and intercept bit for bit."""
    from net.jgp.labs.sparkdq4ml_amd import LinearRegression

    device = _device()
    gpu_session.conf.set("dq4ml.fit.async", "true")
    d, n = 32, 64 * 600 + 9
    X = _mix(d, n, seed=9).cuda()
    y = (torch.linspace(-1, 1, d, device="cuda") @ X.float() + 0.3).float()
    got = {}
    for pack in (True, False):
        T = device.tile_bf16(X, pack=pack)
        assert (T.packed is not None) == pack
        df = gpu_session.createDataFrame({"features": T, "label": y})
        lr = LinearRegression(solver="normal", gramDtype="bf16")
        ms = [lr.fit(df) for _ in range(2)]
        (replay,) = df.__dict__["_fit_replays"].values()  # the second fit found the recorded launch
        assert replay.plan.packed == pack
        got[pack] = [(m.coefficients.toArray().copy(), float(m.intercept)) for m in ms]
    for (ca, ia), (cb, ib) in zip(got[True], got[False]):
        assert (ca == cb).all() and ia == ib
    assert (got[True][0][0] == got[True][1][0]).all() and got[True][0][1] == got[True][1][1]


def test_auto_policy(monkeypatch):
    device = _device()
    monkeypatch.setattr(device, "PACK_MIN_ROWS", 64 * 64)
    monkeypatch.delenv("DQ4ML_TILE_PACK", raising=False)
    n = 64 * 128
    X = clamped_gaussian(32, n, 21).cuda()
    T = device.tile_bf16(X, shift=None)
    assert T.packed is not None and T.packed.npacked == 128
    assert device.tile_bf16(X[:, :64 * 63], shift=None).packed is None  # below the row threshold
    Z = X.clone()
    Z[:, torch.arange(n, device="cuda") % 64 < 48] = 0  # zero-heavy: every entry spans to exponent 0
    Z[:, :64 * 16] = X[:, :64 * 16]  # an eighth still packs: fewer than half, the companion is dropped
    assert device.tile_bf16(Z, shift=None).packed is None
    assert device.tile_bf16(Z, shift=None, pack=True).packed.npacked == 16
    monkeypatch.setenv("DQ4ML_TILE_PACK", "0")
    assert device.tile_bf16(X, shift=None).packed is None
