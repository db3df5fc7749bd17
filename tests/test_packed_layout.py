"""The 12-bit packed tile layout (ops/layout.py ``pack_reference`` / ``unpack_reference``) on the
CPU: the decode is the identity on every bf16 bit pattern, and the directory is exactly what the
packability rule says for inputs whose packed / raw mix is known by construction."""
import pytest
import torch

from packed_cases import (all_patterns, bits_of, clamped_gaussian, expected_dir, inject, raw_patterns, specials,
                          tile_cpu)

from net.jgp.labs.sparkdq4ml_amd.ops.layout import RAW_ENTRY, SLOT_DWORDS, pack_reference, unpack_reference


def _roundtrip(X):
    buf = tile_cpu(X)
    P = pack_reference(buf)
    back = unpack_reference(P, buf)
    assert torch.equal(back.view(torch.int16), buf.view(torch.int16))
    # the decode must not lean on the raw buffer where an entry packed: hide those entries
    hidden = buf.view(torch.int16).clone().view(-1, 2048)
    hidden[P.dir != RAW_ENTRY] = 0x5555
    back = unpack_reference(P, hidden.view(-1).view(torch.bfloat16))
    assert torch.equal(back.view(torch.int16), buf.view(torch.int16))
    assert P.a.numel() == P.dir.numel() * SLOT_DWORDS
    assert not P.a.view(-1, SLOT_DWORDS)[P.dir == RAW_ENTRY].any(), "raw slots are zero-filled"
    assert P.npacked == int((P.dir != RAW_ENTRY).sum())
    return P


def test_every_pattern_packs_and_decodes():
    X = all_patterns(shuffle=False)
    assert torch.equal(bits_of(X).reshape(-1).sort().values, torch.arange(65536, dtype=torch.int32))
    P = _roundtrip(X)
    want = torch.tensor([16 * (s // 2) for s in range(32)], dtype=torch.uint8)
    assert torch.equal(P.dir, want)
    assert P.npacked == 32


def test_shuffled_patterns_stay_raw():
    P = _roundtrip(all_patterns(shuffle=True))
    assert torch.equal(P.dir, torch.full((32,), RAW_ENTRY, dtype=torch.uint8))
    assert P.npacked == 0


def test_zeros_denormals_infinities_nans():
    P = _roundtrip(specials())
    assert P.dir.tolist() == [0, 240, RAW_ENTRY, RAW_ENTRY]


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 7 + 17])
def test_shapes_and_directory(d, n):
    X = clamped_gaussian(d, n, seed=100 * d + n)
    raw = raw_patterns(n)
    inject(X, raw)
    P = _roundtrip(X)
    NT, full = (d + 31) // 32, n // 64
    dirs = P.dir.view(-1, NT)
    assert torch.equal(P.dir, expected_dir(X))
    emin = ((bits_of(X) >> 7) & 0xFF)
    for s in range(dirs.shape[0]):
        for t in range(NT):
            whole = s < full and 32 * (t + 1) <= d
            if whole and s not in raw:  # packable: carries its emin
                assert int(dirs[s, t]) == int(emin[32 * t:32 * t + 32, 64 * s:64 * s + 64].min())
                assert int(dirs[s, t]) >= 117
            else:  # an injected 2^-30, the padded tail rows or padding features (stored zeros)
                assert int(dirs[s, t]) == RAW_ENTRY
