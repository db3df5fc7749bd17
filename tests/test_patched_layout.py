"""The patched (all-packed) companion of the tiled bf16 storage on the CPU: the torch reference
packer and un-packer (ops/layout.py ``patch_reference`` / ``unpatch_reference``) round-trip to the
tiled buffer bit for bit, the records are the ones injected, and the table-level rule rejects
what it should."""
import pytest
import torch

from packed_cases import bits_of, clamped_gaussian, from_bits, tile_cpu
from patched_cases import CORNERS, PAYLOADS, check_records, with_exceptions

from net.jgp.labs.sparkdq4ml_amd.ops.layout import (PATCH_CAP, PATCH_SHARE, pack_reference, patch_reference,
                                                    patched_entries, unpatch_reference)


def _roundtrip(X, d, n, **kw):
    buf = tile_cpu(X)
    p = patch_reference(buf, d, n, **kw)
    assert p is not None
    ne = patched_entries(d, n)
    assert p.npacked == ne == p.dir.shape[0]
    assert torch.equal(bits_of(unpatch_reference(p)), bits_of(buf)[: ne * 2048])
    return buf, p


@pytest.mark.parametrize("d", [32, 64])
def test_exception_counts(d):
    """0, 1, 3 and 4 exceptions per entry (4 takes the overflow table), both tile columns, a
    ragged tail that the companion does not cover."""
    NT, n = d // 32, 64 * 20 + 5
    plan = {(1, 0): 1, (2, NT - 1): 3, (3, 0): 4, (4, NT - 1): 4, (5, 0): 2, (8, NT - 1): 1}
    X, want = with_exceptions(d, n, 3 + d, plan)
    buf, p = _roundtrip(X, d, n)
    check_records(p, NT, want)
    assert p.ovf.numel() == 8 and p.nexc == 15
    # an entry without exceptions keeps the mixed format's slot and base bit for bit
    mixed = pack_reference(buf)
    clean = [e for e in range(p.npacked) if (e // NT, e % NT) not in plan]
    assert torch.equal(p.a.view(-1, 768)[clean], mixed.a.view(-1, 768)[clean])
    assert torch.equal((p.dir[clean, 0] & 0xFF).to(torch.uint8), mixed.dir[clean])


def test_corners_and_payloads():
    """Lane 0 and 63, dwords 0 / 3 / 12 / 15, both halfwords; zero, denormal and negative
    payloads: each record names its halfword and carries its bits."""
    assert {(l, w) for l, w, _ in CORNERS[:8]} == {(l, w) for l in (0, 63) for w in (0, 3, 12, 15)}
    assert {h for _, _, h in CORNERS[:8]} == {0, 1} and {0x0000, 0x8000, 0x0001, 0x807F, 0xB080} <= set(PAYLOADS)
    X, want = with_exceptions(32, 64 * 24, 5, {(0, 0): 8, (2, 0): 8, (23, 0): 6})
    _, p = _roundtrip(X, 32, 64 * 24)
    check_records(p, 1, want)
    seen = {r & 0xFFFF for recs in want.values() for r in recs}
    assert seen == set(PAYLOADS)


def test_cap_and_share():
    n = 64 * 40
    X, want = with_exceptions(32, n, 7, {(6, 0): PATCH_CAP})
    _, p = _roundtrip(X, 32, n)
    check_records(p, 1, want)
    X, _ = with_exceptions(32, n, 7, {(6, 0): PATCH_CAP + 1})
    assert patch_reference(tile_cpu(X), 32, n) is None
    # the share: 40 entries x 2048 values allow 40 exceptions in all
    assert PATCH_SHARE == 2048
    X, _ = with_exceptions(32, n, 7, {(s, 0): 1 for s in range(40)})
    assert patch_reference(tile_cpu(X), 32, n) is not None
    X, _ = with_exceptions(32, n, 7, {(s, 0): 2 if s == 0 else 1 for s in range(40)})
    assert patch_reference(tile_cpu(X), 32, n) is None
    assert patch_reference(tile_cpu(X), 32, n, share=1024) is not None


def test_shapes_that_do_not_patch():
    X = clamped_gaussian(31, 64 * 4, 1)
    assert patch_reference(tile_cpu(X), 31, 64 * 4) is None  # d not a multiple of 32
    X = clamped_gaussian(32, 63, 1)
    assert patch_reference(tile_cpu(X), 32, 63) is None  # no full superstep
    Z = clamped_gaussian(32, 64 * 4, 1)
    Z[:, torch.arange(64 * 4) % 64 < 48] = 0  # zero-heavy: hundreds of exceptions per entry
    assert patch_reference(tile_cpu(Z), 32, 64 * 4) is None


def test_tiny_entry_and_gaussian():
    """An entry whose largest exponent field is below 15 (base = emin, nothing below it), and
    unclamped N(0, 1) data (exceptions occur on their own; cap and share hold with room)."""
    g = torch.Generator().manual_seed(13)
    b = (torch.randint(0, 2, (32, 64), generator=g) << 15) | (torch.randint(0, 15, (32, 64), generator=g) << 7) | \
        torch.randint(0, 128, (32, 64), generator=g)
    X = torch.cat([from_bits(b), clamped_gaussian(32, 64, 2)], dim=1)
    _, p = _roundtrip(X, 32, 128)
    assert p.counts.tolist() == [0, 0] and int(p.dir[0, 0]) == int(((b >> 7) & 0xFF).min())
    d, n = 32, 64 * 300
    X = torch.randn(d, n, generator=g).to(torch.bfloat16)
    _, p = _roundtrip(X, d, n)
    assert 0 < p.nexc * PATCH_SHARE * 4 < 300 * 2048 and int(p.counts.max()) <= 6
