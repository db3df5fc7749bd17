"""The ``groupby.hip`` kernels against their numpy twins (raw accumulators and group ids bit for
bit, for every ``blocks`` override) and against the plain-Python oracle."""
import math

import numpy as np
import pytest
import torch

import _groupby_cases as gc
from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb
from net.jgp.labs.sparkdq4ml_amd.ops import kernels, native

pytestmark = pytest.mark.gpu

NAN, INF = gc.NAN, gc.INF
TRIP, LDS_WORDS, MAX_SLOTS, CAPACITY, DIRECT_CAP = kernels.group_limits()
DEV = "cuda"
BLOCKS = (None, 1, 8)  # one block takes two and three trips; eight leave blocks without rows


def test_limits_are_the_extensions():
    assert tuple(native.hip().group_limits()) == tuple(kernels.group_limits())
    assert 3 * TRIP + 77 <= 5000


_HOST = {}


def host_run(n, pattern):
    """The twin's result of the standard frame, computed once and shared."""
    if (n, pattern) not in _HOST:
        f = gc.make_frame(n, pattern)
        _HOST[(n, pattern)] = (f, gc.run_frame(f), gc.run_frame(f, mode="hash"))
    return _HOST[(n, pattern)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1, 3 * TRIP + 77])
def test_sizes_and_blocks_bit_identical(n):
    f, (enc, acc, off, slots), (enc_h, acc_h, _, _) = host_run(n, "mixed")
    d = gc.to_device(f, DEV)
    for blocks in BLOCKS:
        e2, a2, _, s2 = gc.run_frame(d, blocks=blocks)
        assert e2.mode == "direct" and e2.G == enc.G and torch.equal(e2.gid.cpu(), enc.gid)
        assert [s[3] for s in s2] == [s[3] for s in slots]  # the ABSMAX pre-pass: the same exponents
        assert torch.equal(a2.cpu(), acc), f"blocks={blocks}"
        e3, a3, _, _ = gc.run_frame(d, blocks=blocks, mode="hash")
        assert e3.mode == "hash" and torch.equal(e3.gid.cpu(), enc_h.gid) and torch.equal(e3.keys.cpu(), enc_h.keys)
        assert torch.equal(a3.cpu(), acc_h), f"blocks={blocks} (hash)"
    cells = gc.null_by(gc.finalise(a2, off, slots), slots, gc.FRAME_COUNTS)
    gc.assert_cells(cells, gc.frame_oracle(f))


@pytest.mark.parametrize("pattern", ["one", "wave64", "alt", "holes"])
def test_group_shapes(pattern):
    # one group: every lane shares a gid; wave64: no lane does; alt: two rounds cover a wave;
    # holes: direct slots that no row reaches
    n = 2 * TRIP + 1
    f, (enc, acc, off, slots), _ = host_run(n, pattern)
    d = gc.to_device(f, DEV)
    for blocks in BLOCKS:
        e2, a2, _, _ = gc.run_frame(d, blocks=blocks)
        assert torch.equal(e2.gid.cpu(), enc.gid) and torch.equal(a2.cpu(), acc), f"blocks={blocks}"
    if pattern == "holes":
        assert enc.G == 1002 and int((acc[:, 0] > 0).sum()) == 4  # null, -500, -495, 500
    cells = gc.null_by(gc.finalise(a2, off, slots), slots, gc.FRAME_COUNTS)
    gc.assert_cells(cells, gc.frame_oracle(f))


@pytest.mark.parametrize("words", [1, 7])
def test_lds_budget_and_one_past_it(words):
    # G * words at the LDS budget accumulates on chip, one group more goes to HBM atomics
    n = 5000
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.integers(-1000, 1000, n) * 0.25)
    valid = torch.from_numpy(rng.random(n) < 0.9)
    sel = torch.from_numpy(rng.random(n) < 0.8)
    for G in (LDS_WORDS // words, LDS_WORDS // words + 1):
        assert (G * words <= LDS_WORDS) == (G == LDS_WORDS // words)
        gid = torch.from_numpy((rng.permutation(n) % G).astype(np.int32))
        slots = [] if words == 1 else [(gb.COUNT, None, valid, 0), (gb.SUM_F, x, valid, 10)]
        want, _ = gb.group_agg(gid, G, slots, sel)
        assert want.shape == (G, words)
        dslots = [(op, None if c is None else c.to(DEV), v.to(DEV), e) for op, c, v, e in slots]
        for blocks in BLOCKS:
            got, _ = gb.group_agg(gid.to(DEV), G, dslots, sel.to(DEV), blocks=blocks)
            assert torch.equal(got.cpu(), want), f"G={G} blocks={blocks}"


def both(col, valid=None, sel=None, **kw):
    """group_encode on both engines: equal gid, keys and slot count; returns the device one."""
    h = gb.group_encode(col, valid, sel, **kw)
    d = gb.group_encode(col.to(DEV), None if valid is None else valid.to(DEV), None if sel is None else sel.to(DEV), **kw)
    assert (d.G, d.mode) == (h.G, h.mode) and torch.equal(d.gid.cpu(), h.gid)
    if h.mode == "hash":
        assert torch.equal(d.keys.cpu(), h.keys)
    return d


def test_float_keys_zero_nan_inf_null():
    nan2 = np.array([0x7FF0000000000001, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)
    k = torch.from_numpy(np.concatenate([[0.0, -0.0, NAN], nan2, [INF, -INF, 1.5, 7.0, -2.5]]))  # (payloads kept)
    valid = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=torch.bool)
    enc = both(k, valid)
    # null first, then -inf, -2.5, 0 (both zeros), 1.5, +inf, NaN (every payload and sign) last
    assert enc.G == 7 and enc.gid.tolist() == [3, 3, 6, 6, 6, 5, 1, 4, 0, 2]
    vals = gb.keys_to_values(enc.keys, torch.float64).tolist()[1:]
    assert vals[:5] == [-INF, -2.5, 0.0, 1.5, INF] and math.isnan(vals[5]) and math.copysign(1.0, vals[2]) == 1.0
    enc32 = both(k.to(torch.float32), valid)
    assert enc32.gid.tolist() == enc.gid.tolist()
    # MIN / MAX: -0.0 < +0.0, NaN the largest
    acc, off = gb.group_agg(None, 1, [(gb.MIN, k[:2].to(DEV), None), (gb.MAX, k[:2].to(DEV), None)])
    acc2, off2 = gb.group_agg(None, 1, [(gb.MAX, k.to(DEV), None)])
    lo, hi = (gb.keys_to_values(acc[:, w] ^ gc.I64_MIN, torch.float64).item() for w in off)
    top = gb.keys_to_values(acc2[:, off2[0]] ^ gc.I64_MIN, torch.float64).item()
    assert (math.copysign(1.0, lo), math.copysign(1.0, hi)) == (-1.0, 1.0) and lo == 0.0 == hi and math.isnan(top)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.int32, torch.int64, torch.uint8, torch.bool])
def test_every_key_dtype(dtype):
    rng = np.random.default_rng(8)
    n = TRIP + 13
    raw = rng.integers(0, 2, n) if dtype in (torch.bool, torch.uint8) else rng.integers(-9, 9, n)
    col = torch.from_numpy(raw).to(dtype)
    valid, sel = torch.from_numpy(rng.random(n) < 0.9), torch.from_numpy(rng.random(n) < 0.7)
    enc = both(col, valid, sel)
    assert enc.mode == ("hash" if dtype in (torch.float64, torch.float32) else "direct")
    keys = [(v if ok else None,) for v, ok in zip(col.to(torch.float64).tolist(), valid.tolist())]
    groups = gc.oracle_groups(keys, sel.tolist())
    acc, _ = gb.group_agg(enc.gid, enc.G, [], sel.to(DEV))
    assert acc[acc[:, 0] > 0, 0].tolist() == [len(r) for r in groups.values()]


def test_int64_extremes_and_two_column_keys():
    k = torch.tensor([gc.I64_MAX, gc.I64_MIN, 0, gc.I64_MAX, gc.I64_MIN, -1], dtype=torch.int64)
    enc = both(k)
    # INT64_MAX's key is the table's empty word: it is kept out of band and still ordered last
    assert enc.mode == "hash" and enc.gid.tolist() == [4, 1, 3, 4, 1, 2]
    assert enc.keys.tolist()[1:] == [gc.I64_MIN, -1, 0, gc.I64_MAX]
    a = torch.tensor([2, 1, 2, 1, 1] * 300, dtype=torch.int32)
    c = torch.tensor([0.5, NAN, 0.5, -0.0, 0.0] * 300, dtype=torch.float64)
    va = torch.tensor([1, 1, 1, 0, 1] * 300, dtype=torch.bool)
    gh, Gh, _ = gb.group_encode_columns([a, c], [va, None])
    gid, G, kv = gb.group_encode_columns([a.to(DEV), c.to(DEV)], [va.to(DEV), None])
    assert G == Gh and torch.equal(gid.cpu(), gh)
    acc, _ = gb.group_agg(gid, G, [])
    keep = acc[:, 0] > 0
    rows = [(x if ox else None, y if oy else None) for (x, ox, y, oy) in
            zip(kv[0][0][keep].tolist(), kv[0][1][keep].tolist(), kv[1][0][keep].tolist(), kv[1][1][keep].tolist())]
    assert repr(rows) == repr([(None, 0.0), (1, 0.0), (1, NAN), (2, 0.5)]) and acc[keep, 0].tolist() == [300, 300, 300, 600]


def test_hash_table_growth_wraparound_and_half_full():
    rng = np.random.default_rng(12)
    # capacity 4 against 100 distinct keys: the table overflows and grows 8x until it fits
    k = torch.from_numpy(rng.integers(0, 100, 3000) * 1.5)
    enc = both(k, capacity=4)
    assert enc.G == 101 and enc.capacity == 256
    # three keys whose home is the last slot of 8: probing wraps past the table's end
    last = [v for v in range(1, 4000) if gb.hash_home(v, 8) == 7][:3]
    assert len(last) == 3
    k = torch.tensor(last * 50, dtype=torch.int64)
    enc = both(k, capacity=8, mode="hash")
    assert enc.capacity == 8 and enc.G == 4 and enc.gid.tolist()[:3] == [1 + sorted(last).index(v) for v in last]
    # exactly half full is no overflow; one key more is
    k = torch.tensor([10, 20, 30, 40] * 64, dtype=torch.int64)
    assert both(k, capacity=8, mode="hash").capacity == 8
    k = torch.tensor([10, 20, 30, 40, 50] * 64, dtype=torch.int64)
    enc = both(k, capacity=8, mode="hash")
    assert enc.capacity == 64 and enc.G == 6


def test_flags_nulls_cancellation_wraparound_and_f32():
    g, x = [], []
    for combo in range(8):  # every combination of NaN (1), +inf (2), -inf (4) next to a finite value
        vals = [1.25] + [v for bit, v in ((1, NAN), (2, INF), (4, -INF)) if combo & bit]
        g += [combo] * len(vals)
        x += vals
    g += [8, 8, 9, 9, 9]  # 8: only nulls; 9: x, -x cancellation next to a small term
    x += [5.0, 6.0, 1e16, -1e16, 0.125]
    valid = [True] * (len(g) - 5) + [False, False, True, True, True]
    g, x, valid = g * 40, x * 40, valid * 40  # several waves, groups shared across lanes
    sel = [r % 7 != 3 for r in range(len(g))]
    xd = [v if s else NAN for v, s in zip(x, sel)]  # dead rows hold NaN
    gid = torch.tensor(g, dtype=torch.int32)
    xs, v, st = torch.tensor(xd, dtype=torch.float64), torch.tensor(valid), torch.tensor(sel)
    x32 = [float(np.float32(t)) for t in x]
    ops = [(gb.COUNT, None, valid), (gb.SUM_F, x, valid), (gb.MIN, x, valid), (gb.MAX, x, valid), (gb.SUM_F, x32, valid)]
    want = gc.oracle_cells(gc.oracle_groups([(k,) for k in g], sel), ops)
    for dev in ("cpu", DEV):
        s32 = xs.to(torch.float32).to(dev)
        slots = gc.scales([(gb.COUNT, None, v.to(dev), 0), (gb.SUM_F, xs.to(dev), v.to(dev), None), (gb.MIN, xs.to(dev), v.to(dev), 0),
                           (gb.MAX, xs.to(dev), v.to(dev), 0), (gb.SUM_F, s32, v.to(dev), None)], st.to(dev))
        acc, off = gb.group_agg(gid.to(dev), 10, slots, st.to(dev))
        if dev == "cpu":
            ref = acc
        else:
            assert torch.equal(acc.cpu(), ref)
        cells = gc.null_by(gc.finalise(acc, off, slots), slots, [None, 1, 1, 1, 1])
        gc.assert_cells(cells, want)
        assert cells[8][1:] == [0, None, None, None, None]
    # Java wraparound of long sums; int sums widen to long
    l = torch.tensor([gc.I64_MAX, 1, gc.I64_MIN, -1], dtype=torch.int64).to(DEV)
    acc, off = gb.group_agg(torch.tensor([0, 0, 1, 1], dtype=torch.int32).to(DEV), 2, [(gb.SUM_I, l, None)])
    assert acc[:, off[0]].tolist() == [gc.I64_MIN, gc.I64_MAX]
    i = torch.full((5,), 2 ** 31 - 1, dtype=torch.int32).to(DEV)
    acc, off = gb.group_agg(None, 1, [(gb.SUM_I, i, None)])
    assert acc[0, off[0]].item() == 5 * (2 ** 31 - 1)


def test_shards_add_up_and_first_honours_row_offset():
    n, cut = 3 * TRIP + 77, 1337  # an uneven split that is no multiple of the run
    f, (enc, acc, off, slots), _ = host_run(n, "mixed")
    d = gc.to_device(f, DEV)
    gid = enc.gid.to(DEV)
    dslots = [(op, None if c is None else c.to(DEV), None if v is None else v.to(DEV), e) for op, c, v, e in slots]
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        sl = [(op, None if c is None else c[lo:hi], None if v is None else v[lo:hi], e) for op, c, v, e in dslots]
        a, _ = gb.group_agg(gid[lo:hi], enc.G, sl, d["sel"][lo:hi], row_offset=lo)
        parts.append(a.cpu())
    out = parts[0].clone()
    for w, k in enumerate([gb.K_ADD] + gb.word_kinds([s[0] for s in slots])):
        a, b = parts[0][:, w], parts[1][:, w]
        if k == gb.K_ADD:
            out[:, w] = a + b
        elif k == gb.K_OR:
            out[:, w] = a | b
        else:  # unsigned max / min through the sign-flipped words
            a, b = a ^ gc.I64_MIN, b ^ gc.I64_MIN
            out[:, w] = (torch.maximum(a, b) if k == gb.K_MAX else torch.minimum(a, b)) ^ gc.I64_MIN
    assert torch.equal(out, acc)
    w = off[-1]  # FIRST: the second shard alone reports global row indices
    second = parts[1][:, w][parts[1][:, 0] > 0]
    assert int(second.min()) >= cut
