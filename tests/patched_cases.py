"""Inputs with known exceptions for the patched tile tests (ops/layout.py ``PatchedTiles``), shared
by test_patched_layout.py (CPU) and test_gpu_patched_tiles.py.  Built on the clamped Gaussians of
packed_cases.py: every entry packs with exponent fields 117..130, so a value set to ``TINY`` (or
zero, or a denormal) is exactly one exception and nothing else in the entry changes."""
import torch

from packed_cases import TINY, bits_of, clamped_gaussian, from_bits

# (lane, dword, halfword) slots of an entry: the corners of the record's fields
CORNERS = [(0, 0, 0), (0, 3, 1), (0, 12, 0), (0, 15, 1), (63, 0, 1), (63, 3, 0), (63, 12, 1), (63, 15, 0),
           (31, 5, 0), (32, 10, 1), (17, 7, 1), (46, 8, 0), (5, 1, 1), (58, 14, 0), (20, 2, 0), (40, 13, 1),
           (9, 9, 0)]
# payload bit patterns: tiny, exact +0 and -0, denormals of both signs, a negative tiny normal
PAYLOADS = [int(bits_of(torch.tensor([TINY], dtype=torch.bfloat16))[0]), 0x0000, 0x8000, 0x0001, 0x807F, 0xB080]


def position(s: int, t: int, lane: int, dword: int, half: int):
    """(feature, row) of the value that entry (s, t) keeps at (lane, dword, halfword)."""
    h, f = lane >> 5, lane & 31
    i, j = dword >> 2, dword & 3
    return 32 * t + f, 64 * s + 32 * h + 8 * i + 2 * j + half


def record(lane: int, dword: int, half: int, bits: int) -> int:
    return lane << 21 | dword << 17 | half << 16 | bits


def with_exceptions(d: int, n: int, seed: int, plan):
    """Clamped Gaussians with ``plan[(s, t)]`` = number of exceptions injected into that entry,
    at the first slots of ``CORNERS`` with the payloads in turn.  Returns the matrix and, per
    entry, its expected records in directory order."""
    X = clamped_gaussian(d, n, seed)
    b = bits_of(X)
    want = {}
    for (s, t), k in plan.items():
        recs = []
        for q, (lane, dword, half) in enumerate(CORNERS[:k]):
            bits = PAYLOADS[(q + s + t) % len(PAYLOADS)]
            f, r = position(s, t, lane, dword, half)
            b[f, r] = bits
            recs.append(record(lane, dword, half, bits))
        want[(s, t)] = sorted(recs, key=lambda rec: rec >> 16)
    return from_bits(b), want


def check_records(p, NT: int, want) -> None:
    """The directory and overflow table of ``p`` hold exactly the expected records (and none
    elsewhere)."""
    cnt = p.counts.cpu().tolist()
    dirw, ovf = p.dir.cpu().tolist(), p.ovf.cpu().tolist()
    off = 0
    for e, c in enumerate(cnt):
        recs = want.get((e // NT, e % NT), [])
        assert c == len(recs), (e, c)
        if c <= 3:
            assert dirw[e][1:] == recs + [0] * (3 - c), e
        else:
            assert dirw[e][1:] == [off, 0, 0] and ovf[off:off + c] == recs, e
            off += c
    assert off == len(ovf) and p.nexc == sum(cnt)
