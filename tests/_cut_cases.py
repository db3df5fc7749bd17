"""Shared by the CSV cutter's field and converter tests: the Python model of the numeric fast path,
the field and file generators, and the oracles.  Pure Python and numpy, no GPU import.

The fast path's accepted set (``csv_field_fast`` in ``ops/csrc/hip/csv_parse_dev.h``) is
``[+-]?`` then digits with at most one dot, 1 to 9 digits counted with leading zeros.  For an
accepted field ``m = int(digits)``, ``fr`` = the digits after the dot, and the value is Python's
``float(text)``, which is correctly rounded (``-0`` gives ``-0.0``).

Files are rows joined from a small pool of pre-rendered rows; pool row 0 is the shortest row the
shape can hold (every field one byte) and pool row 1 the longest (every field 11 bytes, 10 in an
int32 column), and every file holds both, so all files of a shape share their line-length facts
and with them one compiled kernel.

Family A values are integer multiples of 2^-6 below 2^10 in magnitude: every product is a multiple
of 2^-12 below 2^20, so any sum of up to 2^20 of them is exact in f64 in any order, with or
without fma, and the oracle is integer arithmetic scaled by 2^12.  Family B values are arbitrary
mantissas of at most 9 digits with 0 to 9 fractional digits; its oracle is exact integer
arithmetic on the ``float(text)`` values scaled by 2^SCALE_B."""
import re
import struct

import numpy as np

WINDOW = 16384
_FAST = re.compile(rb"([+-]?)(\d*)(\.?)(\d*)")


def fast_model(field: bytes):
    """``(m, fr, neg, dot, value)`` of a field the fast path accepts, else None."""
    mt = _FAST.fullmatch(field)
    if mt is None:
        return None
    sg, ip, dt, fp = mt.groups()
    nd = len(ip) + len(fp)
    if nd < 1 or nd > 9:
        return None
    return int(ip + fp), len(fp), sg == b"-", bool(dt), float(field.decode("ascii"))


def f64_bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---- the converter unit test's fields -----------------------------------------------------------
def quotient_miss_mantissas(per_fr=64, seed=11):
    """For fr = 1..9: mantissas m < 10^9 whose one-multiply quotient ``m * RN(10^-fr)`` is not the
    correctly rounded ``m / 10^fr`` (the converter's fma correction has to act), found by a numpy
    loop over random mantissas.  Returns ({fr: [m, ...]}, {fr: misses among the candidates tried},
    candidates tried per fr)."""
    rng = np.random.default_rng(seed)
    tried = 20000
    out, counts = {}, {}
    for fr in range(1, 10):
        m = rng.integers(1, 10 ** 9, tried).astype(np.float64)
        miss = np.nonzero(m * float(f"1e-{fr}") != m / float(10 ** fr))[0]
        counts[fr] = int(miss.size)
        out[fr] = [int(m[i]) for i in miss[:per_fr]]
    return out, counts, tried


def _with_fr(m: int, fr: int) -> bytes:
    s = str(m).zfill(fr)
    return (s[:len(s) - fr] + ("." + s[len(s) - fr:] if fr else "")).encode()


def convert_valid_fields(seed=3):
    """Field texts around the accepted set: every length 1..16, every dot position (first and last
    included), the three sign variants, leading zeros up to 9 digits, 9-digit mantissas, each fr
    with quotient-miss mantissas, and the classic rejects (two dots, a lone sign, a lone dot, a
    sign in mid-field, 10 digits; ``0.000000001`` is one of those, ``.000000001`` is valid).  Most
    are valid; ``fast_model`` decides."""
    rng = np.random.default_rng(seed)
    out = []
    for ln in range(1, 17):
        for sg in (b"", b"+", b"-"):
            n = ln - len(sg)
            if n < 1:
                out.append(sg)  # a lone sign
                continue
            for dp in [None] + list(range(n)):
                nd = n - (0 if dp is None else 1)
                variants = ["".join(str(x) for x in rng.integers(0, 10, nd)) for _ in range(2)]
                variants += ["9" * nd, "0" * nd, "0" * (nd - 1) + "7" if nd else "",
                             "1" + "0" * (nd - 1) if nd else ""]
                for dg in dict.fromkeys(variants):
                    body = dg if dp is None else dg[:dp] + "." + dg[dp:]
                    out.append(sg + body.encode())
    miss, _, _ = quotient_miss_mantissas()
    for fr, ms in miss.items():
        for i, m in enumerate(ms):
            t = _with_fr(m, fr)
            if len(str(m).zfill(fr)) <= 9:
                out.append((b"", b"-", b"+")[i % 3] + t)
    for m in rng.integers(0, 10 ** 9, 16):  # fr = 0: the quotient is the mantissa itself
        out.append(str(int(m)).encode())
    out += [b"999999999", b"0.000000001", b".000000001", b"-999999999.", b"+.999999999", b"000000000", b"-0", b"+0",
            b"-0.0", b".5", b"5.", b"-.5", b"+5.", b"1..2", b"..", b".", b"+", b"-", b"+.", b"-.", b"1.2.3", b"1-2",
            b"12+", b"+-5", b"--5", b"1234567890", b"0000000000", b"12345.67890", b"1e5", b"1 2", b" 12", b"12 "]
    return list(dict.fromkeys(out))


def convert_invalid_fields():
    """Otherwise valid fields of each length with every byte value 0..255 substituted at each
    position (lengths 12..16 cannot be valid: their bases hold 10 digits or more)."""
    bases = []
    for ln in range(1, 17):
        dg = "".join(str((3 * i + 1) % 10) for i in range(ln))
        bases.append(dg.encode())
        if ln >= 2:
            bases.append(b"-" + dg[:ln - 1].encode())
        if ln >= 3:
            k = (ln - 1) // 2
            bases.append(b"+" + (dg[:k] + "." + dg[k:ln - 2]).encode())
    out = []
    for b in bases:
        for pos in range(len(b)):
            for v in range(256):
                out.append(b[:pos] + bytes([v]) + b[pos + 1:])
    return list(dict.fromkeys(out))


SLOT = 32                      # bytes per field slot of the converter harness
CONTEXTS = (0x37, 0x2E, 0x2D, 0xFF, 0x22, 0x2B, 0x2C)  # the slot's other bytes: 7 . - 0xFF " + ,


def convert_layout(seed=5):
    """The converter harness's input: ``(buf uint8 [N * SLOT], end int32 [N], length int32 [N],
    uid int32 [N], texts)``.  Field i is ``buf[end[i] - length[i] : end[i]]`` inside slot i; every
    other byte of the slot (the bytes right before and after the field, which the right-aligned
    frames read) is one of ``CONTEXTS``.  Valid-family texts sit at 8 end offsets (all four
    ``end mod 4``, ``end mod 16`` from 4 to 11) in every context; substituted texts at all four
    ``end mod 4`` with the context and the ``end mod 16`` rotating."""
    valid, invalid = convert_valid_fields(), convert_invalid_fields()
    texts = list(dict.fromkeys(valid + invalid))
    index = {t: i for i, t in enumerate(texts)}
    uid, off, ctx = [], [], []
    for t in valid:
        for k in range(8):
            for c in CONTEXTS:
                uid.append(index[t])
                off.append(20 + k)
                ctx.append(c)
    for j, t in enumerate(invalid):
        for k in range(4):
            uid.append(index[t])
            off.append(20 + k + 4 * ((j >> 1) & 1))
            ctx.append(CONTEXTS[(j + k) % len(CONTEXTS)])
    uid, off, ctx = np.asarray(uid, np.int32), np.asarray(off, np.int32), np.asarray(ctx, np.uint8)
    n = uid.size
    lens = np.asarray([len(t) for t in texts], np.int32)
    right = np.zeros((len(texts), 16), np.uint8)  # the texts right-aligned
    for i, t in enumerate(texts):
        right[i, 16 - len(t):] = np.frombuffer(t, np.uint8)
    buf = np.repeat(ctx[:, None], SLOT, axis=1)
    ln = lens[uid]
    rows = np.arange(n)
    for j in range(16):  # byte j from the field's end
        msk = ln > j
        buf[rows[msk], off[msk] - 1 - j] = right[uid[msk], 15 - j]
    end = (rows * SLOT + off).astype(np.int32)
    return buf.reshape(-1), end, ln.astype(np.int32), uid, texts


def convert_expected(texts):
    """Per text: ``ok uint8, m int64, fr, neg, dot, bits uint64`` of ``fast_model``."""
    n = len(texts)
    ok = np.zeros(n, bool)
    m = np.zeros(n, np.int64)
    fr = np.zeros(n, np.int32)
    neg = np.zeros(n, bool)
    dot = np.zeros(n, bool)
    bits = np.zeros(n, np.uint64)
    for i, t in enumerate(texts):
        r = fast_model(t)
        if r is not None:
            ok[i], m[i], fr[i], neg[i], dot[i], bits[i] = True, r[0], r[1], r[2], r[3], f64_bits(r[4])
    return ok, m, fr, neg, dot, bits


# ---- spellings ----------------------------------------------------------------------------------
def _render(neg, ipd, frac, rng, allow_dot):
    """One legal spelling of sign / integer digits / fraction digits: leading zeros, zeros after
    the value, a dropped ``0`` before the dot, a ``+``, a trailing dot; at most 9 digits."""
    drop = allow_dot and ipd == "0" and frac != "" and rng.random() < 0.4
    if drop:
        ipd = ""
    free = 9 - len(ipd) - len(frac)
    mode = int(rng.integers(0, 14))  # (6 and up: the shortest spelling)
    lead = trail = 0
    if mode == 1 and not drop:
        lead = int(rng.integers(0, free + 1))
    elif mode == 2 and allow_dot:
        trail = int(rng.integers(0, free + 1))
    elif mode == 3 and not drop:
        lead = free
    elif mode == 4 and allow_dot:
        trail = free
    elif mode == 5 and allow_dot and not drop:
        lead = int(rng.integers(0, free + 1))
        trail = int(rng.integers(0, free - lead + 1))
    if ipd == "" and frac == "" and trail == 0:
        ipd = "0"
    dot = "." if (frac or trail) else ("." if allow_dot and rng.random() < 0.15 else "")
    sign = "-" if neg else ("+" if rng.random() < 0.15 else "")
    return (sign + "0" * lead + ipd + dot + frac + "0" * trail).encode()


def spell_a(k: int, rng, int_only=False) -> bytes:
    """A legal spelling of k / 64 (|k| < 2^16; k even from 1000 up, so 9 digits suffice)."""
    a = abs(k)
    ip, fp = a >> 6, a & 63
    frac = ("%06d" % (fp * 15625)).rstrip("0") if fp else ""
    assert not (int_only and frac) and len(str(ip)) + len(frac) <= 9
    return _render(k < 0, str(ip), frac, rng, not int_only)


def spell_b(rng, int_only=False) -> bytes:
    """A general decimal: a mantissa of 1..9 digits with 0..9 fractional digits (none in an
    int32 column)."""
    nd = int(rng.integers(1, 10))
    m = int(rng.integers(0, 10 ** nd))
    fr = 0 if int_only else int(rng.integers(0, 10))
    s = str(m).zfill(fr)
    ipd, frac = s[:len(s) - fr], s[len(s) - fr:] if fr else ""
    if ipd == "" and len(frac) < 9:
        ipd = "0"
    return _render(rng.random() < 0.4, ipd, frac, rng, not int_only)


class Vocab:
    """Distinct field texts with their values; ``short`` / ``long`` index the 1-byte and the
    longest entries (pool rows 0 and 1 are drawn from them)."""

    def __init__(self, texts, values, longest):
        self.texts, self.values = texts, values
        ln = np.asarray([len(t) for t in texts])
        self.short = np.nonzero(ln == 1)[0]
        self.long = np.nonzero(ln == longest)[0]
        assert self.short.size and self.long.size and ln.max() == longest


def vocab_a(rng, size, kind, lo=-65535, hi=65535):
    """Family A fields of a double (``kind`` 'd') or int32 ('i') column: (text, k), value k / 64."""
    seen = {}
    fixed = [(b"-0", 0), (b"0", 0), (b"7", 448), (b"+7", 448), (b"007", 448), (b"-000000012", -768), (b"+000000150", 9600)]
    if kind == "d":
        fixed += [(b"0.015625", 1), (b"12.500000", 800), (b"000012.5", 800), (b".500000000", 32), (b"7.", 448),
                  (b"-.5", -32), (b"3.50", 224), (b"-0.0", 0), (b"-000012.500", -800), (b"+0001.12500", 72),
                  (b"-.015625000", -1)]
    for t, k in fixed:
        seen[t] = k
    for dgt in range(1, 10):
        seen[str(dgt).encode()] = 64 * dgt
    while len(seen) < size:
        k = int(rng.integers(lo, hi + 1))
        if rng.random() < 0.15:
            k = int(rng.integers(-63, 64))  # below 1 in magnitude: spellings with no integer digit
        if kind == "i" or rng.random() < 0.3:
            k = (abs(k) >> 6 << 6) * (-1 if k < 0 else 1)  # an integer value (a double column holds those too)
        if abs(k) >= 64000:
            k = (abs(k) & ~1) * (-1 if k < 0 else 1)
        seen.setdefault(spell_a(k, rng, kind == "i" or (k & 63 == 0 and rng.random() < 0.5)), k)
    texts = list(seen)
    return Vocab(texts, np.asarray([seen[t] for t in texts], np.int64), 10 if kind == "i" else 11)


def vocab_b(rng, size, lo=None, hi=None, kind="d"):
    """Family B fields of a double or an int32 column: (text, float(text)), optionally with
    lo <= value <= hi (the 1-byte and the longest entries stay whatever their value)."""
    seen = {}
    for dgt in range(10):
        seen[str(dgt).encode()] = float(dgt)
    longest = 11 if kind == "d" else 10
    for t in ((b"-999999999.", b"+.000000001", b"-00012.5000", b"+123456.789", b"999999999", b".000000001")
              if kind == "d" else (b"-999999999", b"+000000120", b"999999999", b"-0")):
        seen[t] = float(t.decode())
    while len(seen) < size:
        t = spell_b(rng, kind == "i")
        seen.setdefault(t, float(t.decode()))
    if lo is not None:
        seen = {t: v for t, v in seen.items() if lo <= v <= hi or len(t) in (1, longest)}
    texts = list(seen)
    return Vocab(texts, np.asarray([seen[t] for t in texts], np.float64), longest)


# ---- shapes, pools and files --------------------------------------------------------------------
class Shape:
    """One CSV layout and fit: ``kinds`` per column ('d' double, 'i' int32), the assembler's
    feature columns in order, the label column, the row terminator."""

    def __init__(self, name, ncols, feats, label, term, ints=()):
        self.name, self.C, self.feats, self.label, self.term = name, ncols, list(feats), label, term
        self.kinds = ["i" if c in set(ints) else "d" for c in range(ncols)]
        self.d = len(self.feats)
        assert label not in self.feats and len(set(self.feats)) == self.d


_SUB12 = [29, 3, 36, 11, 22, 0, 38, 8, 25, 14, 33, 6]           # scrambled, not contiguous
_SUB9 = [173, 5, 88, 199, 41, 120, 7, 150, 64]
SHAPES = {
    "d32": Shape("d32", 33, range(32), 32, b"\r"),                                   # yfirst + strip
    "d32crlf": Shape("d32crlf", 33, range(32), 32, b"\r\n"),
    "sub12": Shape("sub12", 40, _SUB12, 17, b"\r", ints=(3, 19, 38)),               # non-yfirst MFMA
    "sub12i": Shape("sub12i", 40, _SUB12, 17, b"\r", ints=(1, 3, 5, 8, 12, 17, 19, 22, 27, 31, 36, 38)),
    "d3of40": Shape("d3of40", 40, [31, 4, 18], 39, b"\n", ints=(4, 20)),            # register sums
    "d9of200": Shape("d9of200", 200, _SUB9, 101, b"\r", ints=(5, 60, 150)),         # H = 4096, HG = 2
    "d80": Shape("d80", 81, range(80), 80, b"\n"),                                   # VALU Gram, a block per thread
    "d100": Shape("d100", 101, range(100), 100, b"\r\n"),                            # VALU Gram, 2 and 3 blocks per thread
    "d128": Shape("d128", 129, range(128), 128, b"\r\n"),
    "d32c": Shape("d32c", 33, range(32), 32, b"\r", ints=(32,)),                    # family C: an int32 label
    "d100c": Shape("d100c", 101, range(100), 100, b"\r\n", ints=(100,)),
    "ones": Shape("ones", 33, range(32), 32, b"\r", ints=range(33)),                 # every field 1 byte
}


class Pool:
    """Pre-rendered rows (no terminator) and their values [P, C]; row 0 shortest, row 1 longest."""

    def __init__(self, shape, rows, values):
        self.shape, self.rows, self.values = shape, rows, values
        self.lens = np.asarray([len(r) for r in rows], np.int64)


def _pool(shape, vocabs, rng, size, ones=False):
    C = shape.C
    idx = np.empty((size, C), np.int64)
    for c in range(C):
        v = vocabs[c]
        idx[:, c] = v.short[rng.integers(0, v.short.size, size)] if ones else rng.integers(0, len(v.texts), size)
        idx[0, c] = v.short[rng.integers(0, v.short.size)]
        if not ones:
            idx[1, c] = v.long[rng.integers(0, v.long.size)]
    rows = [b",".join(vocabs[c].texts[idx[r, c]] for c in range(C)) for r in range(size)]
    values = np.stack([vocabs[c].values[idx[:, c]] for c in range(C)], axis=1)
    return Pool(shape, rows, values)


def pool_a(shape, seed=0, size=None):
    """Family A pool: int64 k values (value k / 64); the label column draws from [-30, 300]."""
    rng = np.random.default_rng(seed + 1000 * shape.C)
    size = size or max(256, min(2048, 120000 // shape.C))
    vd, vi = vocab_a(rng, 1500, "d"), vocab_a(rng, 500, "i")
    yk = shape.kinds[shape.label]
    vy = vocab_a(rng, 600, yk, -1920, 19200)
    vocabs = [vy if c == shape.label else (vi if k == "i" else vd) for c, k in enumerate(shape.kinds)]
    return _pool(shape, vocabs, rng, size, ones=shape.name == "ones")


def pool_b(shape, seed=0, size=1000, label=None):
    """Family B pool: f64 values; the label column holds general decimals in [-50, 300], or, with
    ``label`` = (live text, dead text), the dead text everywhere (family C sets its live row)."""
    rng = np.random.default_rng(seed + 77 + 1000 * shape.C)
    vd, vi = vocab_b(rng, 3000), vocab_b(rng, 1000, kind="i")
    vocabs = [vi if k == "i" else vd for k in shape.kinds]
    if label is None:
        vocabs[shape.label] = vocab_b(rng, 4000, -50.0, 300.0, shape.kinds[shape.label])
        return _pool(shape, vocabs, rng, size)
    p = _pool(shape, vocabs, rng, size)
    dead = label[1]
    for r in range(size):
        f = p.rows[r].split(b",")
        f[shape.label] = dead
        p.rows[r] = b",".join(f)
    p.values[:, shape.label] = float(dead.decode())
    p.lens = np.asarray([len(r) for r in p.rows], np.int64)
    return p


def join_rows(rows, term: bytes, final: bool) -> bytes:
    return term.join(rows) + (term if final else b"")


def pick(pool, n, rng):
    """n pool row indices holding rows 0 and 1 (the shortest and the longest) at random places,
    neither of them last (a last line without a terminator then never sets a line-length fact)."""
    sel = rng.integers(2, len(pool.rows), n)
    a, b = rng.choice(n - 1, 2, replace=False)
    sel[a], sel[b] = 0, 1
    return sel


def rows_for_bytes(pool, nbytes, rng):
    """Row indices (rows 0 and 1 among them) whose file is just over ``nbytes`` long."""
    tl = len(pool.shape.term)
    n = int(nbytes / (pool.lens.mean() + tl) * 1.02) + 8
    while True:
        sel = pick(pool, n, rng)
        if int(pool.lens[sel].sum()) + tl * n > nbytes:
            return sel
        n += max(8, n // 50)


# ---- oracles ------------------------------------------------------------------------------------
LO, HI = 0.0, 150.0  # RangeRule(0, 150) then ``> 0``: a row lives when 0 < y <= 150


def stats_index(d):
    """(i, j) of the packed-upper Σxx slots, column-major (the gram_stats layout)."""
    return [(i, j) for j in range(d) for i in range(j + 1)]


def oracle_a(shape, K, weights=None):
    """gram_stats vector [n, n, n, Σy, Σy², Σx, Σxy, packed-upper Σxx] of rows with int64 k values
    ``K`` [R, C] (value k / 64), each row counted ``weights`` times: integers scaled by 2^12."""
    K = np.asarray(K, np.int64)
    w = np.ones(K.shape[0], np.int64) if weights is None else np.asarray(weights, np.int64)
    y = K[:, shape.label]
    w = w * ((y > 0) & (y <= int(HI) * 64))
    X = K[:, shape.feats]
    n = int(w.sum())
    Xw = X * w[:, None]
    G = Xw.T @ X
    out = [n * 4096] * 3 + [int((w * y).sum()) * 64, int((w * y * y).sum())]
    out += [int(v) * 64 for v in Xw.sum(0)] + [int(v) for v in Xw.T @ y]
    out += [int(G[i, j]) for i, j in stats_index(shape.d)]
    assert max(abs(v) for v in out) < 2 ** 53
    return np.asarray([v / 4096.0 for v in out], np.float64)


SCALE_B = 96  # every |float(text)| here is 0 or at least 1e-9 > 2^-30: a multiple of 2^-83


def _scaled(v: float) -> int:
    p, q = float(v).as_integer_ratio()
    assert (1 << SCALE_B) % q == 0
    return p * ((1 << SCALE_B) // q)


def oracle_b(shape, V):
    """Exact sums of the live rows of f64 values ``V`` [R, C] as integers scaled by 2^(2 SCALE_B):
    ``(ref, absref, n_live)`` in the gram_stats order, ``absref`` the sums of |terms|."""
    V = np.asarray(V, np.float64)
    y = V[:, shape.label]
    live = (y > LO) & (y <= HI)
    one = 1 << SCALE_B
    Xo = np.array([[_scaled(v) for v in row] for row in V[live][:, shape.feats]], dtype=object).reshape(-1, shape.d)
    yo = np.array([_scaled(v) for v in y[live]], dtype=object)
    n = int(live.sum())

    def sums(X, yy):
        G = X.T.dot(X) if n else np.zeros((shape.d, shape.d), dtype=object)
        sx = [int(v) * one for v in X.sum(0)] if n else [0] * shape.d
        sxy = [int(v) for v in X.T.dot(yy)] if n else [0] * shape.d
        return ([n * one * one] * 3 + [int(yy.sum()) * one if n else 0, int((yy * yy).sum()) if n else 0] + sx + sxy
                + [int(G[i, j]) for i, j in stats_index(shape.d)])

    return sums(Xo, yo), sums(abs(Xo), abs(yo)), n


def within_b(got, ref, absref, n):
    """Per entry ``|got - ref| <= (n + 2) 2^-53 Σ|terms|``, in exact integer arithmetic: the
    worst case of n rounded products summed in any order.  Returns the failing indices."""
    bad = []
    for i, g in enumerate(np.asarray(got, np.float64)):
        if not np.isfinite(g):
            bad.append(i)
            continue
        p, q = float(g).as_integer_ratio()
        if (1 << (2 * SCALE_B)) % q:  # finer than any sum of these products can be
            bad.append(i)
            continue
        gi = p * ((1 << (2 * SCALE_B)) // q)
        if abs(gi - ref[i]) << 53 > (n + 2) * absref[i]:
            bad.append(i)
    return bad


def oracle_c(shape, row_values):
    """Family C: one live row.  Every statistic is one value or one rounded product (plus exact
    zeros): Σx_i = x_i, Σx_i y = x_i * y, Σx_i x_j = x_i * x_j, bit for bit."""
    v = np.asarray(row_values, np.float64)
    x, y = v[shape.feats], float(v[shape.label])
    return np.asarray([1.0, 1.0, 1.0, y, y * y] + list(x) + [xi * y for xi in x]
                      + [x[i] * x[j] for i, j in stats_index(shape.d)], np.float64)


# ---- the boundary sweep -------------------------------------------------------------------------
def padded_first_row(shape, shift):
    """A first row of one-digit fields with ``shift`` zeros of padding in all, at most 8 per
    field, the first field first: (text, k values).  Every field stays a legal <= 9-digit spelling."""
    assert 0 <= shift <= 8 * shape.C
    fields, ks = [], []
    for c in range(shape.C):
        z = min(8, shift)
        shift -= z
        dgt = 1 + c % 9
        fields.append(b"0" * z + str(dgt).encode())
        ks.append(64 * dgt)
    return b",".join(fields), np.asarray(ks, np.int64)


def sweep_rows(pool, nwin, rng, target):
    """Row indices for the boundary sweep: ``[second row] + body`` such that, behind an unpadded
    first row, some row's terminator (its first byte) sits at a file offset t with
    ``target - (8 C - 40) <= t <= target`` (the first row's padding then carries it to the target
    and 36 bytes on); returns (sel, t).  The body spans ``nwin`` windows and holds
    pool rows 0 and 1."""
    sh = pool.shape
    tl = len(sh.term)
    body = rows_for_bytes(pool, nwin * WINDOW, rng)
    first_len = 2 * sh.C - 1
    for j in range(len(pool.rows)):
        sel = np.concatenate([[j], body])
        ends = np.concatenate([[first_len], first_len + np.cumsum(pool.lens[sel] + tl)])  # terminator offsets
        hit = ends[(ends >= target - (8 * sh.C - 40)) & (ends <= target)]
        if hit.size:
            return sel, int(hit[0])
    raise AssertionError("no second row aligns the sweep")
