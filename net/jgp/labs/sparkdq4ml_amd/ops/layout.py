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

__all__ = ["TiledBF16", "tiled_offsets", "tall_tiles", "wide_tiles", "wide_bytes", "PackedTiles", "pack_reference", "unpack_reference",
           "PatchedTiles", "patch_reference", "unpatch_reference", "patched_entries", "gram_layout_size"]


def gram_layout_size(d: int) -> int:
    """Length of the flat WLS statistics of d features: count, Σw, Σw², Σwy, Σwy², Σw·x (d),
    Σw·x·y (d), packed upper Σw·x·xᵀ."""
    return 5 + 2 * d + d * (d + 1) // 2


def tall_tiles(d: int) -> int:
    """32-feature tiles of a superstep in the tall layout (``TiledBF16``): the live ones."""
    return (d + 31) // 32


def wide_tiles(d: int) -> int:
    """32-feature tiles of a superstep in the wide layouts (``TiledWide``): whole 256-feature panels."""
    return ((d + 255) // 256) * 8


def wide_bytes(nt: int, n: int, eb: int) -> int:
    """Bytes of a wide tiled buffer of ``n`` rows and tile stride ``nt``: 64 x 32 elements per
    (superstep, tile) chunk, ``eb // 8`` bytes each."""
    return ((n + 63) // 64) * nt * 2048 * (eb // 8)


def tiled_offsets(feats: torch.Tensor, rows: torch.Tensor, d: int) -> torch.Tensor:
    """Element offsets of (feature, row) pairs (broadcast) in the tiled layout.  This function and
    :func:`wide_offsets` are the specification of the formats; csrc/host/tile_layout.h is the
    native twin that every kernel-side user takes them from, tested against these."""
    NT = tall_tiles(d)
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

    kind = "mixed"

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
    hw = _encode_slots(v, torch.where(ok, emin, torch.zeros_like(emin)))
    hw = torch.where(ok.view(-1, 1, 1, 1, 1), hw, torch.zeros_like(hw))
    a = _to_i16(hw).contiguous().view(-1).view(torch.int32)
    d8 = torch.where(ok, emin, torch.full_like(emin, RAW_ENTRY)).to(torch.uint8)
    return PackedTiles(d8, a, int(ok.sum()))


def unpack_reference(packed: PackedTiles, buf: torch.Tensor) -> torch.Tensor:
    """The tiled buffer that a reader of ``packed`` sees: packed entries decoded from their slots,
    raw entries taken from ``buf``.  Equals ``buf`` bit for bit."""
    dec = _decode_slots(packed.a, packed.dir)
    raw = _halfwords(buf)
    out = torch.where((packed.dir != RAW_ENTRY).view(-1, 1, 1, 1), dec, raw)
    return _to_i16(out).view(-1).view(torch.bfloat16)


PATCH_INLINE = 3  # exception records that fit the 16-byte directory record itself
# A table takes the patched form only if no entry has more than PATCH_CAP exceptions and the
# exceptions are at most one value in PATCH_SHARE.  N(0, 1) data has 0.113 per 2048-value entry
# (one value in 18000) and 1e8 x 32 of it would meet a 6-exception entry once in ~250 tables, so
# it passes ninefold in the share and with ten more records in the cap; an entry with a zero in
# every 64th value (32 exceptions) or a table with one zero per 2000 values fails, and takes
# today's mixed companion or none.  The cap also bounds the reader's overflow loop and fits the
# record's 8-bit count.
PATCH_CAP = 16
PATCH_SHARE = 2048


class PatchedTiles:
    """The all-packed companion of a ``TiledBF16`` buffer with ``d`` a multiple of 32
    (csrc/hip/gram.h ``patch_tiles``): every entry of the FULL supersteps has a 12-bit slot, so
    the tall Gram pass reads 3 KiB per entry, always, in a loop without a conditional load.  The
    zero-padded ragged superstep is not covered (the pass reads it from the raw tiles).

    Entry base: ``emin`` where ``emax - emin <= 15`` (slot bits as in :class:`PackedTiles`), else
    ``emax - 15``.  A value whose exponent field is below the base is an *exception*: its slot
    code is the filler 0 (decoding to ``base << 7``) and its 16 stored bits travel in a record
    ``lane << 21 | dword << 17 | halfword << 16 | bits`` -- ``record >> 16`` is the value's index
    in the entry taken lane-major (``lane * 32 + k-step * 8 + element``), and an entry's records
    are sorted by it.  ``dir`` (int32 ``[entries, 4]``) holds per entry ``base | count << 8`` and
    then, for ``count <= PATCH_INLINE``, the records themselves (unused words 0); for more, word 1
    is the index of the entry's first record in ``ovf`` (int32), where all of them sit in order.

    Memory: +75 % of the tiled buffer plus 16 bytes per entry (+0.4 % of it) and the overflow
    table (a few hundred bytes for Gaussian data).  ``nexc``: exceptions in all."""

    kind = "patched"

    def __init__(self, dir: torch.Tensor, a: torch.Tensor, ovf: torch.Tensor, nexc: int):
        assert dir.dtype == torch.int32 and a.dtype == torch.int32 and ovf.dtype == torch.int32
        assert dir.dim() == 2 and dir.shape[1] == 4 and a.numel() == dir.shape[0] * SLOT_DWORDS
        self.dir, self.a, self.ovf, self.nexc = dir, a, ovf, int(nexc)

    @property
    def npacked(self) -> int:
        return self.dir.shape[0]

    @property
    def fraction(self) -> float:
        return 1.0

    @property
    def counts(self) -> torch.Tensor:
        return (self.dir[:, 0] >> 8) & 0xFF


def _encode_slots(v: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """Halfwords ``[entries, 4, 64, 8]`` inside their entry's window -> slot halfwords
    ``[entry, piece, lane, k-step, half]`` (the arithmetic of :func:`pack_reference`)."""
    p = (v & 0x7FFF) - (base.view(-1, 1, 1, 1) << 7)
    sg = v & 0x8000
    p3, s3 = p[..., 6:8], sg[..., 6:8]
    nib = torch.stack([p3 & 0xF, (p3 >> 4) & 0xF, ((p3 >> 8) & 0x7) | (s3 >> 12)], dim=-2)
    hw = (sg[..., :6] | p[..., :6]).reshape(-1, 4, 64, 3, 2) | (nib << 11)
    return hw.permute(0, 3, 2, 1, 4)


def _decode_slots(a: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """Slots + bases -> halfwords ``[entries, 4, 64, 8]`` (the arithmetic of :func:`unpack_reference`)."""
    ne = base.numel()
    hw = (a.view(torch.int16).to(torch.int32) & 0xFFFF).view(ne, 3, 64, 4, 2).permute(0, 3, 2, 1, 4)
    b7 = base.to(torch.int32).view(-1, 1, 1, 1, 1) << 7
    main = (hw & 0x87FF) + b7
    nib = (hw >> 11) & 0xF
    p3 = nib[..., 0, :] | (nib[..., 1, :] << 4) | ((nib[..., 2, :] & 0x7) << 8)
    r3 = (p3 | ((nib[..., 2, :] & 0x8) << 12)) + b7[..., 0, :]
    return torch.cat([main.reshape(ne, 4, 64, 6), r3], dim=-1)


def patched_entries(d: int, n: int) -> int:
    """Entries the patched companion covers: the full supersteps of a ``d % 32 == 0`` table."""
    return (n // 64) * (d // 32) if d % 32 == 0 and d > 0 else 0


def patch_reference(buf: torch.Tensor, d: int, n: int, cap: int = PATCH_CAP, share: int = PATCH_SHARE):
    """The :class:`PatchedTiles` of a tiled bf16 buffer in plain torch (CPU or GPU), or None where
    the table does not take the patched form (``d`` not a multiple of 32, no full superstep, an
    entry with more than ``cap`` exceptions, or more than one exception per ``share`` values):
    the specification of the layout and the oracle of the device packer."""
    ne = patched_entries(d, n)
    if ne == 0:
        return None
    v = _halfwords(buf[: ne * 2048])
    e = (v >> 7) & 0xFF
    emin, emax = e.amin(dim=(1, 2, 3)), e.amax(dim=(1, 2, 3))
    base = torch.where(emax - emin <= 15, emin, emax - 15)
    exc = (e < base.view(-1, 1, 1, 1)).permute(0, 2, 1, 3).reshape(ne, 2048)  # lane-major
    cnt = exc.sum(dim=1)
    nexc = int(cnt.sum())
    if int(cnt.max()) > cap or nexc * share > ne * 2048:
        return None
    slots = _encode_slots(torch.where(e < base.view(-1, 1, 1, 1), base.view(-1, 1, 1, 1) << 7, v), base)
    a = _to_i16(slots).contiguous().view(-1).view(torch.int32)
    # records in (entry, lane-major index) order: nonzero() is row-major
    ent, pos = exc.nonzero(as_tuple=True)
    bits = v.permute(0, 2, 1, 3).reshape(ne, 2048)[ent, pos]
    rec = ((pos << 16) | bits).to(torch.int32)
    start = torch.cumsum(cnt, 0) - cnt
    rank = torch.arange(ent.numel(), device=buf.device) - start[ent]
    big = cnt > PATCH_INLINE
    ovcnt = torch.where(big, cnt, torch.zeros_like(cnt))
    ovoff = torch.cumsum(ovcnt, 0) - ovcnt
    dirw = torch.zeros(ne, 4, dtype=torch.int32, device=buf.device)
    dirw[:, 0] = (base | (cnt << 8)).to(torch.int32)
    dirw[:, 1] = torch.where(big, ovoff, torch.zeros_like(ovoff)).to(torch.int32)
    inl = ~big[ent]
    dirw[ent[inl], 1 + rank[inl]] = rec[inl]
    ovf = torch.zeros(int(ovcnt.sum()), dtype=torch.int32, device=buf.device)
    ovf[ovoff[ent[~inl]] + rank[~inl]] = rec[~inl]
    return PatchedTiles(dirw, a, ovf, nexc)


def unpatch_reference(p: PatchedTiles) -> torch.Tensor:
    """The tiled buffer of the full supersteps as a reader of ``p`` sees it: slots decoded, then
    every exception record written over its halfword.  Equals that part of the raw tiles bit for
    bit."""
    ne = p.dir.shape[0]
    hw = _decode_slots(p.a, p.dir[:, 0] & 0xFF).permute(0, 2, 1, 3).reshape(ne, 2048).clone()  # lane-major
    cnt = p.counts.tolist()
    for e in (i for i, c in enumerate(cnt) if c):
        w = p.dir[e].tolist()
        recs = w[1 : 1 + cnt[e]] if cnt[e] <= PATCH_INLINE else p.ovf[w[1] : w[1] + cnt[e]].tolist()
        for r in recs:
            hw[e, r >> 16] = r & 0xFFFF
    return _to_i16(hw.view(ne, 64, 4, 8).permute(0, 2, 1, 3).contiguous()).view(-1).view(torch.bfloat16)


class TiledBF16:
    def __init__(self, buf: torch.Tensor, d: int, n: int, shift=None, packed=None):
        assert buf.dtype == torch.bfloat16 and buf.dim() == 1
        self.buf, self.d, self.n = buf, int(d), int(n)
        self.shift = shift
        # optional 12-bit companion, a PackedTiles (mixed) or a PatchedTiles (only the tall Gram pass reads it)
        self.packed = packed

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
    NT = wide_tiles(d)
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
        return wide_tiles(self.d)

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
