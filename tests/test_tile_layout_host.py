"""csrc/host/tile_layout.h, the one native owner of the MFMA-fragment tile formats, against their
specification ops/layout.py (``tiled_offsets``, ``wide_offsets``) -- on the CPU, through the host
module, which compiles the same header the kernels do.

Shapes: d = 33 tall (2 tiles, the second ragged), d = 257 wide bf16 and wide fp8 (2 panels, 9 live
tiles of 16), n = 130 (3 supersteps, the last ragged): the smallest with more than one tile, a
padded panel and a ragged superstep.  Everything is integer arithmetic: the comparisons are exact.
"""
import numpy as np
import pytest
import torch

from net.jgp.labs.sparkdq4ml_amd.ops import layout, native

TALL, WIDE, WIDE_FP8 = 1, 2, 3
N = 130
# (layout code, d, bytes per element)
CASES = [pytest.param(TALL, 33, 2, id="tall"), pytest.param(WIDE, 257, 2, id="wide-bf16"),
         pytest.param(WIDE_FP8, 257, 1, id="wide-fp8")]


@pytest.fixture(scope="module")
def h():
    return native.host()


def spec_offsets(code, feats, rows, d):
    f, r = torch.from_numpy(feats), torch.from_numpy(rows)
    if code == TALL:
        return layout.tiled_offsets(f, r, d).numpy()
    return layout.wide_offsets(f, r, d, eb=16 if code == WIDE else 8).numpy()


@pytest.mark.parametrize("code,d,esize", CASES)
def test_offsets_match_the_python_specification(h, code, d, esize):
    feats = np.arange(d, dtype=np.int64)[:, None]
    rows = np.arange(N, dtype=np.int64)[None, :]
    got = h.tile_elem_offsets(code, feats, rows, h.tile_tiles(code, d))
    assert got.shape == (d, N)
    np.testing.assert_array_equal(got, spec_offsets(code, feats, rows, d))


@pytest.mark.parametrize("code,d,esize", CASES)
def test_offsets_are_a_bijection_onto_the_buffer(h, code, d, esize):
    nt = h.tile_tiles(code, d)
    nsup = (N + 63) // 64
    feats = np.arange(nt * 32, dtype=np.int64)[:, None]
    rows = np.arange(nsup * 64, dtype=np.int64)[None, :]
    got = h.tile_elem_offsets(code, feats, rows, nt).ravel()
    nelem = h.tile_bytes(code, d, N) // esize
    assert got.size == nelem
    np.testing.assert_array_equal(np.sort(got), np.arange(nelem, dtype=np.int64))


@pytest.mark.parametrize("code,d,esize", CASES)
def test_frag_row_inverts_the_fragment_address(h, code, d, esize):
    """The element at the address the lsq passes read -- chunk base + (sub * 64 + lane) * 16 + e,
    written out here -- is the element of row frag_row(s, sub, h, e) of that lane's feature."""
    nt = h.tile_tiles(code, d)
    nsup = (N + 63) // 64
    chunk_bytes = 64 * 32 * esize
    ups, fe = chunk_bytes // (64 * 16), 16 // esize  # 16-byte fragments of 64 lanes per chunk
    s, sub, hh, e, t, fl = np.meshgrid(np.arange(nsup), np.arange(ups), np.arange(2), np.arange(fe), np.arange(nt),
                                       np.arange(32), indexing="ij")
    at = (s * nt + t) * chunk_bytes + (sub * 64 + 32 * hh + fl) * 16 + e * esize
    assert (at % esize == 0).all()
    rows = h.tile_frag_rows(code, s, sub, hh, e)
    assert rows.min() == 0 and rows.max() == nsup * 64 - 1
    np.testing.assert_array_equal(at // esize, h.tile_elem_offsets(code, t * 32 + fl, rows, nt))


@pytest.mark.parametrize("d", [1, 32, 33, 64, 65, 256, 257, 4096])
def test_sizes_match_the_closed_forms(h, d):
    tall, wide = -(-d // 32), -(-d // 256) * 8
    assert layout.tall_tiles(d) == tall and layout.wide_tiles(d) == wide
    assert h.tile_tiles(TALL, d) == tall
    assert h.tile_tiles(WIDE, d) == wide and h.tile_tiles(WIDE_FP8, d) == wide
    for n in (0, 1, 64, 65, N):
        nsup = -(-n // 64)
        assert h.tile_bytes(TALL, d, n) == nsup * tall * 64 * 32 * 2
        assert h.tile_bytes(WIDE, d, n) == nsup * wide * 64 * 32 * 2
        assert h.tile_bytes(WIDE_FP8, d, n) == nsup * wide * 64 * 32
