"""Physical layouts of assembled feature matrices.

``TiledBF16`` is the MI355X-native storage of a bf16 ``vector`` column: the MFMA-fragment order
of ``v_mfma_f32_32x32x16_bf16`` (csrc/hip/gram.h).  For superstep ``s`` (64 rows), 32-feature tile
``t`` and k-step ``i``, the 64 lanes' 16-byte fragments are contiguous, so the Gram kernel's
every wave load is one contiguous KiB and the pass runs at HBM speed (measured 6.25 TB/s vs
3.06 TB/s for the same kernel on plain feature-major storage, scripts/gram_ab.py).  Rows are
zero padded to whole supersteps, features to whole tiles.

Everything that needs individual rows (show/collect/compaction) gathers them with
:meth:`gather_rows`; the hot consumers (Gram, predict, metrics) read the tiles directly.

Both layouts may store the features SHIFTED: ``shift`` (an ``ops.shift.Shift`` or None) holds a
per-feature value ``s`` that was subtracted before the low-precision cast (``x' = x - s`` is
what the tiles hold; dead and padding rows are exactly 0).  Consumers correct for it: the Gram
un-shifts its statistics in f64, predictions add ``s . coef`` to the intercept, and
:meth:`gather_rows` returns ``x' + s`` (f32).
"""
from __future__ import annotations

import torch

__all__ = ["TiledBF16", "tiled_offsets", "PackedTiles", "pack_reference", "unpack_reference"]


def tiled_offsets(feats: torch.Tensor, rows: torch.Tensor, d: int) -> torch.Tensor:
    """Element offsets of (feature, row) pairs (broadcast) in the tiled layout."""
    NT = (d + 31) // 32
    s = rows >> 6
    h = (rows >> 5) & 1
    i = (rows >> 3) & 3
    j = rows & 7
    t = feats >> 5
    lane = 32 * h + (feats & 31)
    return ((((s * NT + t) * 4 + i) * 64 + lane) << 3) + j


def _unshift_rows(vals: torch.Tensor, shift) -> torch.Tensor:
    if shift is None:
        return vals
    return vals.to(torch.float32) + shift.dev.to(vals.device).unsqueeze(1)


RAW_ENTRY = 0xFF  # directory byte of an entry that stays raw
SLOT_DWORDS = 768  # one packed entry: 3 pieces x 64 lanes x 4 dwords = 3 KiB


class PackedTiles:
    """Lossless 12-bit companion of a ``TiledBF16`` buffer, read by the tall Gram pass in place of
    the raw tiles wherever an entry packed (csrc/hip/gram.h ``pack_tiles``).

    An entry is one (superstep ``s``, 32-feature tile ``t``): 2048 stored bf16 values, 4 KiB.  It is
    packable iff the 8-bit exponent fields of all 2048 values span at most 15 binades
    (``emax - emin <= 15`` and ``emin <= 254``).  Then ``dir[s * NT + t] = emin`` and every value
    ``v`` (sign ``sg``, exponent ``e``, mantissa ``m``) has the 12-bit code
    ``p = sg << 11 | (e - emin) << 7 | m``; its halfword decodes as
    ``((p & 0x800) << 4 | (p & 0x7FF)) + (emin << 7)``.  Otherwise ``dir = 0xFF`` and the entry is
    read from ``TiledBF16.buf``.  Zeros, denormals, infinities and NaN payloads are not special:
    the code is a bit-exact function of the 16 stored bits, or the entry is raw.  Padding rows and
    features are stored zeros (exponent 0), so ragged entries are raw unless all values are tiny.

    Slot ``s * NT + t`` of ``a`` (int32, ``SLOT_DWORDS`` each, zero for raw entries) is three
    pieces of 64 lanes x 4 dwords: piece ``k`` holds, for lane ``l`` and k-step ``i`` = 0..3, the
    dword ``D_k``.  With the lane's raw fragment of k-step ``i`` being dwords ``R0..R3`` (two
    values each, low halfword first), each halfword of ``D_k`` has the sign of ``R_k``'s at bit 15
    and its ``p & 0x7FF`` at bits 10..0; bits 14..11 carry the code of ``R3``'s halfword: D0 its
    ``p`` bits 3..0, D1 bits 7..4, D2 bits 10..8 with the sign on top.

    Memory: +75 % of the tiled buffer plus one byte per entry (n/64 bytes per tile column) --
    +4.8 GB beside the 6.4 GB of a 1e8 x 32 table.  ``npacked``: entries that packed."""

    def __init__(self, dir: torch.Tensor, a: torch.Tensor, npacked: int):
        assert dir.dtype == torch.uint8 and a.dtype == torch.int32 and a.numel() == dir.numel() * SLOT_DWORDS
        self.dir, self.a, self.npacked = dir, a, int(npacked)

    @property
    def fraction(self) -> float:
        return self.npacked / max(1, self.dir.numel())


def _halfwords(buf: torch.Tensor) -> torch.Tensor:
    """Tiled buffer -> its stored 16-bit patterns as int32 ``[entries, k-step, lane, 8]``."""
    return (buf.view(torch.int16).to(torch.int32) & 0xFFFF).view(-1, 4, 64, 8)


def _to_i16(hw: torch.Tensor) -> torch.Tensor:
    return (((hw + 0x8000) & 0xFFFF) - 0x8000).to(torch.int16)


def pack_reference(buf: torch.Tensor) -> PackedTiles:
    """The :class:`PackedTiles` of a tiled bf16 buffer in plain torch (CPU or GPU): the
    specification of the layout and the oracle of the device packer."""
    v = _halfwords(buf)
    e = (v >> 7) & 0xFF
    emin, emax = e.amin(dim=(1, 2, 3)), e.amax(dim=(1, 2, 3))
    ok = ((emax - emin) <= 15) & (emin <= 254)
    base = torch.where(ok, emin, torch.zeros_like(emin)).view(-1, 1, 1, 1)
    p = (v & 0x7FFF) - (base << 7)  # 11-bit codes (sign apart) wherever the entry packs
    sg = v & 0x8000
    p3, s3 = p[..., 6:8], sg[..., 6:8]
    nib = torch.stack([p3 & 0xF, (p3 >> 4) & 0xF, ((p3 >> 8) & 0x7) | (s3 >> 12)], dim=-2)  # [e, i, lane, k, half]
    hw = (sg[..., :6] | p[..., :6]).reshape(-1, 4, 64, 3, 2) | (nib << 11)
    hw = hw.permute(0, 3, 2, 1, 4)  # -> [entry, piece k, lane, k-step i, half]
    hw = torch.where(ok.view(-1, 1, 1, 1, 1), hw, torch.zeros_like(hw))
    a = _to_i16(hw).contiguous().view(-1).view(torch.int32)
    d8 = torch.where(ok, emin, torch.full_like(emin, RAW_ENTRY)).to(torch.uint8)
    return PackedTiles(d8, a, int(ok.sum()))


def unpack_reference(packed: PackedTiles, buf: torch.Tensor) -> torch.Tensor:
    """The tiled buffer that a reader of ``packed`` sees: packed entries decoded from their slots,
    raw entries taken from ``buf``.  Equals ``buf`` bit for bit."""
    ne = packed.dir.numel()
    hw = (packed.a.view(torch.int16).to(torch.int32) & 0xFFFF).view(ne, 3, 64, 4, 2).permute(0, 3, 2, 1, 4)
    base = packed.dir.to(torch.int32).view(-1, 1, 1, 1, 1) << 7  # [entry, i, lane, k, half]
    main = (hw & 0x87FF) + base
    nib = (hw >> 11) & 0xF
    p3 = nib[..., 0, :] | (nib[..., 1, :] << 4) | ((nib[..., 2, :] & 0x7) << 8)
    r3 = (p3 | ((nib[..., 2, :] & 0x8) << 12)) + base[..., 0, :]
    dec = torch.cat([main.reshape(ne, 4, 64, 6), r3], dim=-1)
    raw = _halfwords(buf)
    out = torch.where((packed.dir != RAW_ENTRY).view(-1, 1, 1, 1), dec, raw)
    return _to_i16(out).view(-1).view(torch.bfloat16)


class TiledBF16:
    def __init__(self, buf: torch.Tensor, d: int, n: int, shift=None, packed: "PackedTiles" = None):
        assert buf.dtype == torch.bfloat16 and buf.dim() == 1
        self.buf, self.d, self.n = buf, int(d), int(n)
        self.shift = shift
        self.packed = packed  # optional 12-bit companion (only the tall Gram pass reads it)

    @property
    def shape(self):
        return (self.d, self.n)

    @property
    def device(self):
        return self.buf.device

    @property
    def dtype(self):
        return torch.bfloat16

    @property
    def is_cuda(self):
        return self.buf.is_cuda

    def dim(self):
        return 2

    def gather_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """Dense ``[d, k]`` of the given rows: bf16, or f32 ``x' + s`` for shifted storage."""
        rows = rows.to(self.buf.device, torch.int64)
        f = torch.arange(self.d, device=self.buf.device, dtype=torch.int64).unsqueeze(1)
        return _unshift_rows(self.buf[tiled_offsets(f, rows.unsqueeze(0), self.d)], self.shift)

    def to_dense(self) -> torch.Tensor:
        return self.gather_rows(torch.arange(self.n, device=self.buf.device))

    def slice_rows(self, start: int, stop: int) -> torch.Tensor:
        return self.gather_rows(torch.arange(start, stop, device=self.buf.device))

    def __repr__(self):
        return f"TiledBF16(d={self.d}, n={self.n}, device={self.buf.device})"


def wide_offsets(feats: torch.Tensor, rows: torch.Tensor, d: int, eb: int = 16) -> torch.Tensor:
    """Element offsets in the wide (d > 64) fragment layout, tiles padded to whole 256-feature
    panels (csrc/hip/gram_wide.hip).  Per (superstep s = 64 rows, 32-feature tile t) one chunk of
    512 elements: bf16 ``[k-step][64 lanes][8]``; fp8 ``[half][64 lanes][16]`` where a lane's 32
    bytes are its 4 k-steps (half = k-step >> 1) — one K=64 block-scaled MFMA operand."""
    NT = ((d + 255) // 256) * 8
    s = rows >> 6
    ki = (rows >> 4) & 3
    h = (rows >> 3) & 1
    j = rows & 7
    t = feats >> 5
    lane = 32 * h + (feats & 31)
    if eb == 8:
        return (s * NT + t) * 2048 + (((ki >> 1) * 64 + lane) << 4) + ((ki & 1) << 3) + j
    return ((((s * NT + t) * 4 + ki) * 64 + lane) << 3) + j


class TiledWide:
    """Wide MFMA-fragment storage: bf16 (eb=16) or fp8 e4m3 OCP with per-feature scales (eb=8)."""

    def __init__(self, buf: torch.Tensor, d: int, n: int, eb: int, scales=None, shift=None):
        self.buf, self.d, self.n, self.eb = buf, int(d), int(n), int(eb)
        self.scales = scales  # f32 [d] (fp8 only): x = q * scale (+ shift)
        self.shift = shift

    @property
    def nt(self):
        return ((self.d + 255) // 256) * 8

    @property
    def shape(self):
        return (self.d, self.n)

    @property
    def device(self):
        return self.buf.device

    @property
    def dtype(self):
        return torch.bfloat16 if self.eb == 16 else torch.float8_e4m3fn

    @property
    def is_cuda(self):
        return self.buf.is_cuda

    def dim(self):
        return 2

    def gather_rows(self, rows: torch.Tensor) -> torch.Tensor:
        rows = rows.to(self.buf.device, torch.int64)
        f = torch.arange(self.d, device=self.buf.device, dtype=torch.int64).unsqueeze(1)
        off = wide_offsets(f, rows.unsqueeze(0), self.d, self.eb)
        if self.eb == 16:
            return _unshift_rows(self.buf.view(torch.bfloat16)[off], self.shift)
        q = self.buf.view(torch.float8_e4m3fn)[off].to(torch.float32)
        return _unshift_rows(q * self.scales.unsqueeze(1), self.shift)

    def to_dense(self) -> torch.Tensor:
        return self.gather_rows(torch.arange(self.n, device=self.buf.device))

    def slice_rows(self, start: int, stop: int) -> torch.Tensor:
        return self.gather_rows(torch.arange(start, stop, device=self.buf.device))

    def __repr__(self):
        return f"TiledWide(d={self.d}, n={self.n}, eb={self.eb}, device={self.buf.device})"
