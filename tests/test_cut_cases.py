"""CPU checks of the cutter tests' own generators and oracles (tests/_cut_cases.py), so that a
failure of tests/test_gpu_scancut_fields.py or tests/test_gpu_csv_convert.py points at the device
code: the generators emit only fast-path fields, family A's integer oracle is the exact sum of
the texts, and the host engine (``master("cpu")``), running the same DataFrame chain on one small
file per family, agrees with the oracles (family A and C exactly, family B within its bound)."""
from fractions import Fraction

import numpy as np
import pytest

import _cut_cases as cc


def _fields(pool):
    for row in pool.rows:
        f = row.split(b",")
        assert len(f) == pool.shape.C
        yield f


@pytest.mark.parametrize("name", ["d32", "sub12i", "d3of40", "ones", "d100"])
def test_family_a_pool_is_fast_path_and_exact(name):
    shape = cc.SHAPES[name]
    pool = cc.pool_a(shape, size=96)
    lens = set()
    for r, f in enumerate(_fields(pool)):
        for c, t in enumerate(f):
            m = cc.fast_model(t)
            assert m is not None, t
            assert not (shape.kinds[c] == "i" and m[3]), (c, t)  # an int32 column: integer spellings only
            assert Fraction(t.decode()) == Fraction(int(pool.values[r, c]), 64), t
            assert abs(int(pool.values[r, c])) < 2 ** 16
            lens.add(len(t))
    assert min(pool.lens) == pool.lens[0] == 2 * shape.C - 1  # row 0: every field one byte
    if name != "ones":
        assert max(pool.lens) == pool.lens[1] and lens == set(range(1, 12))  # 1- to 11-byte fields
        for c, k in enumerate(shape.kinds):  # row 1 keeps a double column double: a dot in each
            assert (b"." in pool.rows[1].split(b",")[c]) == (k == "d")


def test_family_a_spellings_cover_the_issue_list():
    v = cc.vocab_a(np.random.default_rng(0), 1500, "d")
    texts = set(v.texts)
    assert {b"0.015625", b"12.500000", b"000012.5", b".500000000", b"+7", b"7.", b"007", b"-.5", b"3.50", b"-0"} <= texts
    import re

    for pat in (rb"\+\d+", rb"\d+\.", rb"0\d+", rb"-\.\d+", rb"\.\d{9}", rb"[+-]?\d{9}", rb"\d+\.\d*0", rb"\d"):
        assert sum(1 for t in texts if re.fullmatch(pat, t)) >= 3, pat
    vi = cc.vocab_a(np.random.default_rng(0), 500, "i")
    assert all(b"." not in t for t in vi.texts) and all(k % 64 == 0 for k in vi.values)


@pytest.mark.parametrize("name", ["d32", "sub12"])
def test_family_b_pool_is_fast_path(name):
    shape = cc.SHAPES[name]
    pool = cc.pool_b(shape, size=64)
    frs, nds = set(), set()
    for r, f in enumerate(_fields(pool)):
        for c, t in enumerate(f):
            m = cc.fast_model(t)
            assert m is not None and m[4] == pool.values[r, c], t
            assert not (shape.kinds[c] == "i" and m[3]), (c, t)
            frs.add(m[1])
            nds.add(len(str(m[0])))
    assert frs == set(range(10)) and nds == set(range(1, 10))


@pytest.mark.parametrize("name", ["sub12", "d3of40"])
def test_family_a_oracle_is_the_fraction_sum_of_the_texts(name):
    shape = cc.SHAPES[name]
    pool = cc.pool_a(shape, size=64)
    sel = cc.pick(pool, 90, np.random.default_rng(2))
    ref = cc.oracle_a(shape, pool.values, np.bincount(sel, minlength=64))
    rows = [[Fraction(t.decode()) for t in pool.rows[i].split(b",")] for i in sel]
    live = [r for r in rows if 0 < r[shape.label] <= 150]
    X = [[r[c] for c in shape.feats] for r in live]
    y = [r[shape.label] for r in live]
    n = len(live)
    want = [n, n, n, sum(y), sum(v * v for v in y)] + [sum(x[i] for x in X) for i in range(shape.d)]
    want += [sum(x[i] * v for x, v in zip(X, y)) for i in range(shape.d)]
    want += [sum(x[i] * x[j] for x in X) for i, j in cc.stats_index(shape.d)]
    assert 0 < n < 90 and [Fraction(float(v)) for v in ref] == want


def _host_rows(spark, path, shape):
    from net.jgp.labs.sparkdq4ml_amd import VectorAssembler, callUDF, col
    from net.jgp.labs.sparkdq4ml_amd.dq.rules import RangeRule
    from net.jgp.labs.sparkdq4ml_amd.sql.types import DataTypes

    spark.udf().register("rangeRule", RangeRule(cc.LO, cc.HI, name="rangeRule"), DataTypes.DoubleType)
    df = spark.read().format("csv").option("inferSchema", "true").load(path)
    kinds = ["i" if type(f.dataType).__name__ == "IntegerType" else "d" for f in df.schema.fields]
    assert kinds == shape.kinds  # the inference the cutter's facts come from
    df = df.withColumn("y_ok", callUDF("rangeRule", col(f"_c{shape.label}"))).filter(col("y_ok") > 0)
    df = df.withColumn("label", col("y_ok"))
    df = VectorAssembler().setInputCols([f"_c{i}" for i in shape.feats]).setOutputCol("features").transform(df)
    rows = df.select("features", "label").collect()
    return np.array([r[0].toArray() for r in rows], np.float64).reshape(-1, shape.d), np.array([r[1] for r in rows])


def _stats(X, y):
    n = float(len(y))
    G = X.T @ X
    return np.concatenate([[n, n, n, y.sum(), (y * y).sum()], X.sum(0), X.T @ y,
                           [G[i, j] for i, j in cc.stats_index(X.shape[1])]])


def _write(tmp_path, rows, shape, final=True):
    p = str(tmp_path / "f.csv")
    with open(p, "wb") as f:
        f.write(cc.join_rows(rows, shape.term, final))
    return p


@pytest.mark.parametrize("name", ["sub12", "d32"])
def test_host_engine_agrees_with_family_a_oracle(cpu_session, tmp_path, name):
    shape = cc.SHAPES[name]
    pool = cc.pool_a(shape, size=64)
    sel = cc.pick(pool, 80, np.random.default_rng(3))
    X, y = _host_rows(cpu_session, _write(tmp_path, [pool.rows[i] for i in sel], shape), shape)
    ref = cc.oracle_a(shape, pool.values, np.bincount(sel, minlength=64))
    assert np.array_equal(_stats(X, y), ref)  # every sum exact: any order, any engine


def test_host_engine_agrees_with_family_b_oracle(cpu_session, tmp_path):
    shape = cc.SHAPES["sub12"]
    pool = cc.pool_b(shape, size=120)
    sel = np.random.default_rng(4).permutation(120)
    X, y = _host_rows(cpu_session, _write(tmp_path, [pool.rows[i] for i in sel], shape), shape)
    V = pool.values[sel]
    live = (V[:, shape.label] > cc.LO) & (V[:, shape.label] <= cc.HI)
    assert np.array_equal(X, V[live][:, shape.feats]) and np.array_equal(y, V[live, shape.label])  # float(text), bit for bit
    ref, absref, n = cc.oracle_b(shape, V)
    assert n == len(y) > 10
    assert cc.within_b(_stats(X, y), ref, absref, n) == []
    worse = _stats(X, y)
    worse[7] += 2.0 ** -40 * absref[7] / float(1 << cc.SCALE_B) ** 2  # an error the bound must catch
    assert cc.within_b(worse, ref, absref, n) == [7]


def test_host_engine_agrees_with_family_c_oracle(cpu_session, tmp_path):
    shape = cc.SHAPES["d32c"]
    pool = cc.pool_b(shape, size=40, label=(b"001", b"200"))
    rows = list(pool.rows)
    f = rows[17].split(b",")
    f[shape.label] = b"001"
    rows[17] = b",".join(f)
    X, y = _host_rows(cpu_session, _write(tmp_path, rows, shape, final=False), shape)
    v = pool.values[17].copy()
    v[shape.label] = 1.0
    assert len(y) == 1 and np.array_equal(_stats(X, y), cc.oracle_c(shape, v))


def test_converter_case_model():
    """The converter test's reference on hand-checked fields, and its layout."""
    for t, want in ((b"-0", (0, 0, True, False, -0.0)), (b".5", (5, 1, False, True, 0.5)), (b"5.", (5, 0, False, True, 5.0)),
                    (b"+007", (7, 0, False, False, 7.0)), (b"-.5", (5, 1, True, True, -0.5)),
                    (b".000000001", (1, 9, False, True, 1e-9)), (b"999999999", (999999999, 0, False, False, 999999999.0))):
        got = cc.fast_model(t)
        assert got == want and cc.f64_bits(got[4]) == cc.f64_bits(want[4]), t
    for t in (b"", b".", b"+", b"-", b"1..2", b"1-2", b"1234567890", b"0.000000001", b"1e5", b"1 ", b"\xb1", b"1\n", b"1,2"):
        assert cc.fast_model(t) is None, t
    miss, counts, tried = cc.quotient_miss_mantissas()
    assert all(len(miss[fr]) == 64 for fr in range(1, 10))
    for fr, ms in miss.items():
        for m in ms:
            assert float(m) * float(f"1e-{fr}") != float(Fraction(m, 10 ** fr))  # (Fraction -> float rounds correctly)
    buf, end, ln, uid, texts = cc.convert_layout()
    for i in np.random.default_rng(0).integers(0, end.size, 500):
        e, n = int(end[i]), int(ln[i])
        assert bytes(buf[e - n:e].tobytes()) == texts[uid[i]] and buf[e] == buf[e - n - 1]
        assert e // cc.SLOT == i and e % cc.SLOT >= 20 and e % cc.SLOT + 4 <= cc.SLOT  # its reads stay in its slot
