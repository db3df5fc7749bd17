"""Inputs with a known packed / raw mix for the 12-bit packed tile tests (ops/layout.py
``PackedTiles``), shared by test_packed_layout.py (CPU) and test_gpu_packed_tiles.py."""
import torch

from net.jgp.labs.sparkdq4ml_amd.ops.layout import tiled_offsets

TINY = 2.0 ** -30  # exponent field 97: more than 15 binades below the clamped Gaussians (>= 117)


def bits_of(X: torch.Tensor) -> torch.Tensor:
    """bf16 tensor -> its 16-bit patterns as int32 in 0..65535."""
    return X.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits(b: torch.Tensor) -> torch.Tensor:
    return (((b.to(torch.int32) + 0x8000) & 0xFFFF) - 0x8000).to(torch.int16).view(torch.bfloat16)


def tile_cpu(X: torch.Tensor) -> torch.Tensor:
    """Dense bf16 ``[d, n]`` -> the tiled buffer (zero padded), by the layout's own offsets."""
    d, n = X.shape
    NT, nsup = (d + 31) // 32, (n + 63) // 64
    buf = torch.zeros(nsup * NT * 2048, dtype=torch.int16)
    f = torch.arange(d, dtype=torch.int64).unsqueeze(1)
    r = torch.arange(n, dtype=torch.int64).unsqueeze(0)
    buf[tiled_offsets(f, r, d)] = X.contiguous().view(torch.int16)
    return buf.view(torch.bfloat16)


def clamped_gaussian(d: int, n: int, seed: int) -> torch.Tensor:
    """N(0, 1) with the magnitude clamped to [2^-10, 8): exponent fields 117..130, so every full
    superstep of a full 32-feature tile packs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(d, n, generator=g)
    sign = torch.where(x < 0, -1.0, 1.0)
    return (sign * x.abs().clamp(2.0 ** -10, 7.9)).to(torch.bfloat16)


def inject(X: torch.Tensor, supersteps) -> torch.Tensor:
    """One tiny value in every feature tile of the given supersteps: those entries go raw."""
    d, n = X.shape
    for s in supersteps:
        for f0 in range(0, d, 32):
            X[f0 + (s % min(32, d - f0)), 64 * s + (7 * s + 3) % 64] = TINY
    return X


def raw_patterns(n: int):
    """The raw supersteps of the mix cases: the first, the last full one, two consecutive ones and
    every other one of a stretch (deduplicated, only full supersteps)."""
    full = n // 64
    if full == 0:
        return []
    want = {0, full - 1, 3, 4} | set(range(8, min(full, 20), 2))
    return sorted(s for s in want if s < full)


def expected_dir(X: torch.Tensor) -> torch.Tensor:
    """The directory by the rule, from the dense matrix: exponent span of each zero-padded
    64-row x 32-feature block."""
    d, n = X.shape
    NT, nsup = (d + 31) // 32, (n + 63) // 64
    e = torch.zeros(NT * 32, nsup * 64, dtype=torch.int32)
    e[:d, :n] = (bits_of(X) >> 7) & 0xFF
    e = e.view(NT, 32, nsup, 64).permute(2, 0, 1, 3).reshape(nsup * NT, -1)
    lo, hi = e.amin(dim=1), e.amax(dim=1)
    ok = (hi - lo <= 15) & (lo <= 254)
    return torch.where(ok, lo, torch.full_like(lo, 0xFF)).to(torch.uint8)


def all_patterns(shuffle: bool) -> torch.Tensor:
    """All 65536 bf16 bit patterns as a d = 32 matrix of 32 supersteps.  Ordered: superstep s holds
    the 16-binade window ``16 * (s // 2) .. + 15`` (both signs, every mantissa; the two supersteps
    of a window split the mantissas by parity), so each packs with base ``16 * (s // 2)`` and every
    (sign, exponent offset, mantissa) code occurs.  Shuffled: every superstep spans far more."""
    sg, w, eo, m = torch.meshgrid(torch.arange(2), torch.arange(16), torch.arange(16), torch.arange(128), indexing="ij")
    bits = (sg << 15) | ((16 * w + eo) << 7) | m
    # order: window, mantissa parity, then the rest -> 32 groups of 2048
    bits = bits.permute(1, 3, 0, 2).reshape(16, 64, 2, 2, 16).permute(0, 2, 1, 3, 4).reshape(32, 2048)
    if shuffle:
        g = torch.Generator().manual_seed(7)
        bits = bits.reshape(-1)[torch.randperm(65536, generator=g)].reshape(32, 2048)
    # superstep s -> dense block [32 features, 64 rows]
    X = bits.view(32, 32, 64).permute(1, 0, 2).reshape(32, 32 * 64)
    return from_bits(X)


def specials() -> torch.Tensor:
    """d = 32, four supersteps: (0) +-0, denormals and tiny normals, exponents 0..15 -> base 0;
    (1) exponents 240..255 with +-inf and NaN payloads -> base 240; (2) zeros beside ones -> raw;
    (3) nothing but +-inf / NaN, emin = 255 -> raw (a base of 0xFF cannot be told from raw)."""
    g = torch.Generator().manual_seed(11)
    r = lambda lo, hi: torch.randint(lo, hi, (32, 64), generator=g)  # noqa: E731
    s0 = (r(0, 2) << 15) | (r(0, 16) << 7) | r(0, 128)
    s0[0, :4] = torch.tensor([0x0000, 0x8000, 0x0001, 0x807F])
    s1 = (r(0, 2) << 15) | (r(240, 256) << 7) | r(0, 128)
    s1[0, :6] = torch.tensor([0x7F80, 0xFF80, 0x7FC0, 0xFFFF, 0x7F81, 0x7800])
    s2 = torch.where(r(0, 2) == 0, torch.tensor(0x0000), torch.tensor(0x3F80))
    s3 = (r(0, 2) << 15) | (255 << 7) | r(0, 128)
    return from_bits(torch.cat([s0, s1, s2, s3], dim=1))
