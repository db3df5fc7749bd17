"""Joins on the CPU engine: the numpy twin of the join kernels against the plain-Python oracle
(equal pairs in the contract's order), then ``DataFrame.join`` and SQL ``JOIN ... USING`` against a
row-level oracle, the schema rules, the errors, and a gloo world of two ranks."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

import _join_cases as jc
from net.jgp.labs.sparkdq4ml_amd.ops import kernels
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F
from net.jgp.labs.sparkdq4ml_amd.sql.expressions import AnalysisException
from net.jgp.labs.sparkdq4ml_amd.sql.joins import HOW_SPELLINGS

NAN, INF = jc.NAN, jc.INF
CANON_HOWS = tuple(HOW_SPELLINGS)


# ---- the twin --------------------------------------------------------------------------------------
def check(tag, case):
    for how in jc.HOWS:
        want = jc.cached_oracle(tag, case, how)
        stats = []
        li, ri = jc.run(case, how, stats=stats)
        assert li.dtype == torch.int64 and ri.dtype == torch.int64
        assert torch.equal(li, want[0]) and torch.equal(ri, want[1]), f"{tag}: {how}"
        assert stats == [jc.oracle_stats(case, int(want[0].numel()))]
    want = jc.cached_oracle(tag, case, "mask")
    assert torch.equal(jc.run_mask(case), want)


@pytest.mark.parametrize("ldt,rdt", jc.DTYPE_PAIRS)
def test_twin_equals_oracle(ldt, rdt):
    check(("host", ldt, rdt), jc.make_case(300, 200, ldt, rdt, span=120, seed=3))
    check(("host-plain", ldt, rdt), jc.make_case(200, 300, ldt, rdt, span=500, seed=4, nulls=False, selection=False))


@pytest.mark.parametrize("nl,nr", [(0, 0), (0, 7), (7, 0), (1, 1), (65, 3)])
def test_small_and_empty_sides(nl, nr):
    check(("small", nl, nr), jc.make_case(nl, nr, span=4, seed=nl + nr, nulls=nl > 1, selection=False))


def test_float_and_extreme_keys_literally():
    neg_nan = torch.tensor([-1], dtype=torch.int64).view(torch.float64)[0].item()  # a NaN of another payload and sign
    lkey = torch.tensor([0.0, NAN, -0.0, 1.5, INF, 2.0], dtype=torch.float64)
    rkey = torch.tensor([-0.0, neg_nan, 1.5, 0.0, -INF, NAN], dtype=torch.float32)
    lvalid = torch.tensor([True, True, True, True, True, False])
    li, ri = kernels.join_pairs(lkey, rkey, lvalid=lvalid, how="full_outer")
    # -0.0 joins 0.0, every NaN joins every NaN, a null key matches nothing; then the unmatched right rows
    assert list(zip(li.tolist(), ri.tolist())) == [(0, 0), (0, 3), (1, 1), (1, 5), (2, 0), (2, 3), (3, 2), (4, -1), (5, -1),
                                                   (-1, 4)]
    top = torch.tensor([jc.I64_MAX, 5, jc.I64_MIN, jc.I64_MAX], dtype=torch.int64)
    li, ri = kernels.join_pairs(top, torch.tensor([jc.I64_MIN, jc.I64_MAX, jc.I64_MAX - 1], dtype=torch.int64), how="left_outer")
    assert list(zip(li.tolist(), ri.tolist())) == [(0, 1), (1, -1), (2, 0), (3, 1)]
    li, ri = kernels.join_pairs(torch.tensor([7, 8], dtype=torch.int32), torch.tensor([8, 7, 8], dtype=torch.int64))
    assert list(zip(li.tolist(), ri.tolist())) == [(0, 1), (1, 0), (1, 2)]


def test_two_to_the_31_pairs_raise_from_the_count_alone():
    lkey = torch.zeros(32768, dtype=torch.int32)
    rkey = torch.zeros(65536, dtype=torch.int32)
    with pytest.raises(ValueError, match="2147483648 pairs"):
        kernels.join_pairs(lkey, rkey)
    li, _ = kernels.join_pairs(lkey[:3], rkey[:5])
    assert li.numel() == 15


def test_key_columns_of_several_columns():
    rng = torch.Generator().manual_seed(5)
    nl, nr = 400, 300
    mk = lambda n, hi, dt: torch.randint(0, hi, (n,), generator=rng).to(dt)  # noqa: E731
    lcols = [mk(nl, 4, torch.int64), mk(nl, 3, torch.float64) * 0.5, mk(nl, 2, torch.bool)]
    rcols = [mk(nr, 4, torch.int64), mk(nr, 3, torch.float64) * 0.5, mk(nr, 2, torch.bool)]
    lcols[1][::9] = NAN
    rcols[1][::7] = NAN
    lvalids = [None, torch.rand(nl, generator=rng) > 0.1, None]
    rvalids = [torch.rand(nr, generator=rng) > 0.1, None, None]
    lsel = torch.rand(nl, generator=rng) > 0.2
    for k in (2, 3):
        lkey, lvalid, rkey, rvalid = kernels.join_key_columns(lcols[:k], rcols[:k], lvalids[:k], rvalids[:k], lsel, None)
        assert lkey.dtype == torch.int64 and lvalid.dtype == torch.bool and lkey.numel() == nl and rkey.numel() == nr
        li, ri = kernels.join_pairs(lkey, rkey, lvalid, rvalid, lsel, None, how="left_outer")

        def key(cols, valids, i):
            if any(v is not None and not bool(v[i]) for v in valids[:k]):
                return None
            return tuple(jc.canon(c[i].item()) for c in cols[:k])

        rows = {}
        for r in range(nr):
            if key(rcols, rvalids, r) is not None:
                rows.setdefault(key(rcols, rvalids, r), []).append(r)
        want = []
        for l in range(nl):
            if lsel[l]:
                hit = rows.get(key(lcols, lvalids, l)) if key(lcols, lvalids, l) is not None else None
                want += [(l, r) for r in hit] if hit else [(l, -1)]
        assert list(zip(li.tolist(), ri.tolist())) == want
    with pytest.raises(TypeError, match="share a dtype"):
        kernels.join_key_columns([lcols[0], lcols[1]], [rcols[0], rcols[0]])


def test_limits_and_bad_arguments():
    trip, tile, lds_rows, max_cap = kernels.join_limits()
    assert (trip, tile) == (1024, 2048) and lds_rows >= tile and max_cap == 1 << 30
    x = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="how must be one of"):
        kernels.join_pairs(x, x, how="left_semi")
    with pytest.raises(TypeError, match="unsupported key dtype"):
        kernels.join_pairs(x.to(torch.float16), x)
    with pytest.raises(ValueError, match="one entry per row"):
        kernels.join_pairs(x, x, lvalid=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="power of two"):
        kernels.join_pairs(x, x, capacity=12)
    with pytest.raises(ValueError, match="blocks"):
        kernels.join_mask(x, x, blocks=0)


# ---- the API ---------------------------------------------------------------------------------------
L_ROWS = [(1, "a", 1.5, True), (2, "b", NAN, False), (2, "a", -0.0, None), (None, "c", 2.0, True), (4, None, 0.0, False),
          (5, "b", None, True), (1, "c", 3.0, None), (7, "a", INF, False)]
L_SCHEMA = "k int, s string, x double, b boolean"
R_ROWS = [(2, "b", 0.0, True, 10), (2, "a", NAN, False, 20), (3, "c", 1.5, None, 30), (None, "a", 2.0, True, 40),
          (1, None, -INF, False, 50), (4, "zz", NAN, True, 60), (2, "b", 5.0, True, 70)]
R_SCHEMA = "k long, t string, y double, c boolean, w int"


def frames(spark):
    return spark.createDataFrame(L_ROWS, L_SCHEMA), spark.createDataFrame(R_ROWS, R_SCHEMA)


def _ck(v, as_float):
    if v is None:
        return None
    if isinstance(v, (bool, str)):
        return v
    if as_float:
        return "nan" if v != v else float(v) + 0.0
    return v


def py_join(lrows, rrows, lk, rk, how, using=True):
    """The rows of the join of ``lrows`` and ``rrows`` on the column index pairs ``lk`` / ``rk``,
    in the contract's order and Spark's column order (plain Python, nested loops)."""
    as_float = [any(isinstance(row[i], float) for row in rows if row[i] is not None)
                for pair in zip(lk, rk) for rows, i in ((lrows, pair[0]), (rrows, pair[1]))]
    as_float = [as_float[2 * j] or as_float[2 * j + 1] for j in range(len(lk))]

    def key(row, idx):
        k = tuple(_ck(row[i], f) for i, f in zip(idx, as_float))
        return None if any(v is None for v in k) else k

    if how == "right_outer":
        pairs = _py_pairs(rrows, lrows, lambda r: key(r, rk), lambda r: key(r, lk), "left_outer")
        pairs = [(l, r) for r, l in pairs]
    elif how in ("left_semi", "left_anti"):
        hits = {l for l, r in _py_pairs(lrows, rrows, lambda r: key(r, lk), lambda r: key(r, rk), "inner")}
        return [row for l, row in enumerate(lrows) if (l in hits) == (how == "left_semi")]
    else:
        pairs = _py_pairs(lrows, rrows, lambda r: key(r, lk), lambda r: key(r, rk), how)
    nl, nr = len(lrows[0]), len(rrows[0])
    out = []
    for l, r in pairs:
        lrow = lrows[l] if l >= 0 else (None,) * nl
        rrow = rrows[r] if r >= 0 else (None,) * nr
        if not using:
            out.append(tuple(lrow) + tuple(rrow))
            continue
        if how == "right_outer":
            keys = [rrow[i] for i in rk]
        elif how == "full_outer":
            keys = [lrow[i] if l >= 0 else rrow[j] for i, j in zip(lk, rk)]
            keys = [float(v) if f and v is not None else v for v, f in zip(keys, as_float)]
        else:
            keys = [lrow[i] for i in lk]
        out.append(tuple(keys) + tuple(v for i, v in enumerate(lrow) if i not in lk)
                   + tuple(v for i, v in enumerate(rrow) if i not in rk))
    return out


def _py_pairs(lrows, rrows, lkey, rkey, how):
    rows = {}
    for r, row in enumerate(rrows):
        if rkey(row) is not None:
            rows.setdefault(rkey(row), []).append(r)
    pairs, met = [], set()
    for l, row in enumerate(lrows):
        hit = rows.get(lkey(row)) if lkey(row) is not None else None
        if hit:
            met.add(lkey(row))
            pairs += [(l, r) for r in hit]
        elif how != "inner":
            pairs.append((l, -1))
    if how == "full_outer":
        pairs += [(-1, r) for r, row in enumerate(rrows) if not (rkey(row) is not None and rkey(row) in met)]
    return pairs


SQL_TYPES = {"inner": "INNER JOIN", "left_outer": "LEFT OUTER JOIN", "right_outer": "RIGHT JOIN", "full_outer": "FULL OUTER JOIN",
             "left_semi": "LEFT SEMI JOIN", "left_anti": "LEFT ANTI JOIN"}


def api_results(spark):
    """Every API / SQL case as plain tuples (one list per case), for the host checks and the
    engine-to-engine comparison."""
    out = {}
    rows = lambda df: [tuple(r) for r in df.collect()]  # noqa: E731
    L, R = frames(spark)
    R2 = R.withColumnRenamed("t", "s").withColumnRenamed("c", "b")
    R4 = R.withColumnRenamed("k", "rk")  # (the condition form keeps both sides' columns: no name twice)
    for how in CANON_HOWS:
        out["k_" + how] = rows(L.join(R, "k", how))
        out["xy_" + how] = rows(L.join(R4, L.x == R4.y, how))
        out["ky_" + how] = rows(L.join(R4, F.col("k") == F.col("y"), how))  # int against double
        out["s_" + how] = rows(L.join(R2.drop("k", "b"), "s", how))
        out["b_" + how] = rows(L.join(R2.drop("k", "s"), ["b"], how))
        out["ks_" + how] = rows(L.join(R2.drop("b"), ["k", "s"], how))
        out["ksb_" + how] = rows(L.join(R2, ["k", "s", "b"], how))
    out["two_conds"] = rows(L.join(R4, (L.k == R4.w) & (R4.t == L.s), "left"))
    out["filtered"] = rows(L.filter("x < 100").join(R.filter("w > 10"), "k", "full"))
    agg = L.groupBy("k").agg(F.count("*").alias("n"), F.sum("x").alias("sx"))
    out["agg_back"] = rows(L.join(agg, "k", "left"))
    out["agg_semi"] = rows(L.join(agg.filter("n > 1"), "k", "semi"))
    out["then_group"] = rows(L.join(R, "k").groupBy("s").agg(F.sum("w").alias("sw")).orderBy("s"))
    L.createOrReplaceTempView("lt")
    R.createOrReplaceTempView("rt")
    agg.createOrReplaceTempView("ag")
    for how, words in SQL_TYPES.items():
        out["sql_" + how] = rows(spark.sql(f"SELECT * FROM lt {words} rt USING (k)"))
    out["sql_plain"] = rows(spark.sql("SELECT lt.s, r.w, k FROM lt l JOIN rt AS r USING (k) WHERE r.w > 10 ORDER BY w DESC, s"))
    text = "SELECT k, s, w, n FROM lt JOIN rt USING (k) LEFT JOIN ag USING (k) ORDER BY w, s"
    out["sql_chain"] = rows(spark.sql(text))
    out["sql_chain_again"] = rows(spark.sql(text))
    out["sql_group"] = rows(spark.sql("SELECT s, count(*) c, sum(w) sw FROM lt LEFT JOIN rt USING (k) GROUP BY s ORDER BY s"))
    return out


def test_api_rows_equal_the_row_oracle(cpu_session):
    got = api_results(cpu_session)
    rep = repr  # (NaN cells compare by their text)
    R2 = [(k, t, y, c, w) for k, t, y, c, w in R_ROWS]
    for how in CANON_HOWS:
        assert rep(got["k_" + how]) == rep(py_join(L_ROWS, R_ROWS, [0], [0], how)), how
        assert rep(got["xy_" + how]) == rep(py_join(L_ROWS, R_ROWS, [2], [2], how, using=False)), how
        assert rep(got["ky_" + how]) == rep(py_join(L_ROWS, R_ROWS, [0], [2], how, using=False)), how
        assert rep(got["s_" + how]) == rep(py_join(L_ROWS, [r[1:3] + r[4:] for r in R2], [1], [0], how)), how
        assert rep(got["b_" + how]) == rep(py_join(L_ROWS, [r[2:] for r in R2], [3], [1], how)), how
        assert rep(got["ks_" + how]) == rep(py_join(L_ROWS, [r[:3] + r[4:] for r in R2], [0, 1], [0, 1], how)), how
        assert rep(got["ksb_" + how]) == rep(py_join(L_ROWS, R2, [0, 1, 3], [0, 1, 3], how)), how
        assert rep(got["sql_" + how]) == rep(got["k_" + how]), how
    assert rep(got["two_conds"]) == rep(py_join(L_ROWS, R_ROWS, [0, 1], [4, 1], "left_outer", using=False))
    lf = [r for r in L_ROWS if r[2] is not None and r[2] < 100]  # (NaN is above everything)
    assert rep(got["filtered"]) == rep(py_join(lf, [r for r in R_ROWS if r[4] > 10], [0], [0], "full_outer"))
    n = {}
    for r in L_ROWS:
        n[r[0]] = n.get(r[0], 0) + 1
    assert [(r[0], r[4]) for r in got["agg_back"]] == [(r[0], n[r[0]] if r[0] is not None else None) for r in L_ROWS]
    assert rep(got["agg_semi"]) == rep([r for r in L_ROWS if r[0] in (1, 2)])
    inner = py_join(L_ROWS, R_ROWS, [0], [0], "inner")
    assert got["sql_plain"] == sorted([(r[1], r[7], r[0]) for r in inner if r[7] > 10], key=lambda r: (-r[1], r[0]))
    assert got["sql_chain"] == sorted([(r[0], r[1], r[7], n[r[0]]) for r in inner], key=lambda r: (r[2], r[1]))
    assert got["sql_chain_again"] == got["sql_chain"]
    sw = {}
    for r in inner:
        sw[r[1]] = sw.get(r[1], 0) + r[7]
    assert got["then_group"] == sorted(sw.items(), key=lambda kv: (kv[0] is not None, kv[0]))


def test_schema_column_order_and_nullability(cpu_session):
    s = cpu_session
    L = s.createDataFrame([(1, 2.0)], "k int, x double")
    R = s.createDataFrame([(1, 3)], "k long, w int")
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import LocalRelation
    from net.jgp.labs.sparkdq4ml_amd.sql.types import StructField, StructType

    def strict(df):  # the same frame with non-nullable fields
        t = df._table()
        sch = StructType([StructField(f.name, f.dataType, False) for f in t.schema.fields])
        return type(df)(LocalRelation(type(t)(sch, t.columns, t.nrows, None, t.device)), s)

    L, R = strict(L), strict(R)
    desc = lambda df: [(f.name, f.dataType.simpleString(), f.nullable) for f in df.schema.fields]  # noqa: E731
    assert desc(L.join(R, "k")) == [("k", "int", False), ("x", "double", False), ("w", "int", False)]
    assert desc(L.join(R, "k", "left")) == [("k", "int", False), ("x", "double", False), ("w", "int", True)]
    assert desc(L.join(R, "k", "right")) == [("k", "bigint", False), ("x", "double", True), ("w", "int", False)]
    assert desc(L.join(R, "k", "full")) == [("k", "bigint", True), ("x", "double", True), ("w", "int", True)]
    assert desc(L.join(R, "k", "semi")) == desc(L) and desc(L.join(R, "k", "anti")) == desc(L)
    R3 = R.withColumnRenamed("k", "kk")
    assert [n for n, _, _ in desc(L.join(R3, L.k == R3.kk, "left"))] == ["k", "x", "kk", "w"]
    D = strict(s.createDataFrame([(1.0, 5)], "k double, v int"))
    assert desc(L.join(D, "k", "outer"))[0] == ("k", "double", True)
    assert desc(L.join(D, "k"))[0] == ("k", "int", False)


def test_every_spelling_of_how(cpu_session):
    L, R = frames(cpu_session)
    for canon, spellings in HOW_SPELLINGS.items():
        want = repr(L.join(R, "k", canon).collect())
        for sp in spellings:
            for variant in (sp, sp.upper(), sp.replace("_", "").capitalize()):
                assert repr(L.join(R, "k", variant).collect()) == want, variant
    with pytest.raises(ValueError, match="left_outer.*full_outer.*left_semi.*left_anti"):
        L.join(R, "k", "sideways")


def test_semi_and_anti_narrow_the_selection_and_move_no_row(cpu_session):
    L, R = frames(cpu_session)
    base = L._table()
    for how, keep in (("semi", [0, 1, 2, 4, 6]), ("anti", [3, 5, 7])):
        t = L.join(R, "k", how)._table()
        assert t.nrows == base.nrows and torch.nonzero(t.sel).flatten().tolist() == keep
        assert all(a is b for a, b in zip(t.columns, base.columns))
    f = L.filter("x > 0")
    ft = f._table()
    t = f.join(R, "k", "anti")._table()
    assert torch.equal(t.sel, ft.sel & ~torch.tensor([True, True, True, False, True, False, True, False]))


def test_explain_and_plan(cpu_session, capsys):
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import Join, prune_columns

    L, R = frames(cpu_session)
    j = L.join(R, "k", "left")
    assert isinstance(j._plan, Join) and j._plan.children() == [L._plan, R._plan] and j._plan.skey() is not None
    assert j._plan.skey() == L.join(R, "k", "leftouter")._plan.skey() != L.join(R, "k")._plan.skey()
    assert prune_columns(j._plan, {"k"}) is j._plan
    j.explain()
    assert "Join left_outer [k]" in capsys.readouterr().out


def test_errors(cpu_session):
    s = cpu_session
    L, R = frames(s)
    with pytest.raises(AnalysisException, match="ambiguous"):
        L.join(R, L.k == R.k)
    with pytest.raises(AnalysisException, match="withColumnRenamed"):  # s, x, b on both sides, not keys
        L.join(L.withColumnRenamed("k", "kk"), F.col("k") == F.col("kk"))
    with pytest.raises(AnalysisException, match="withColumnRenamed"):
        L.join(L, "k")
    with pytest.raises(AnalysisException, match="cross joins are not implemented"):
        L.join(R)
    with pytest.raises(AnalysisException, match="cross joins are not implemented"):
        L.crossJoin(R)
    with pytest.raises(AnalysisException, match="cross joins are not implemented"):
        L.join(R, "k", "cross")
    with pytest.raises(AnalysisException, match="cannot be resolved on the right"):
        L.join(R, "s")
    with pytest.raises(AnalysisException, match="is not implemented"):
        L.join(R, L.k < R.w)
    with pytest.raises(AnalysisException, match="no common type"):  # a string against an int
        L.join(R, L.s == R.w)
    with pytest.raises(AnalysisException, match="no common type"):
        L.join(R, L.b == R.w)
    from net.jgp.labs.sparkdq4ml_amd import VectorAssembler

    V = VectorAssembler().setInputCols(["x"]).setOutputCol("v").transform(L.na.drop(subset=["x"]))
    with pytest.raises(AnalysisException, match="vector column cannot be a join key"):
        V.select("v", "k").join(V.select("v", "s"), "v")
    L.createOrReplaceTempView("lt")
    R.createOrReplaceTempView("rt")
    with pytest.raises(AnalysisException, match="JOIN ... ON is not implemented; use USING"):
        s.sql("SELECT * FROM lt JOIN rt ON lt.k = rt.k")
    with pytest.raises(AnalysisException, match="cross joins are not implemented"):
        s.sql("SELECT * FROM lt CROSS JOIN rt")
    with pytest.raises(AnalysisException, match="not found: nope"):
        s.sql("SELECT * FROM lt JOIN nope USING (k)")


# ---- two ranks (gloo) ------------------------------------------------------------------------------
def _dp_rows():
    return [(j % 9 if j % 5 else None, float((j * 37) % 11) - 5.0, f"s{j % 3}") for j in range(80)]


_DP_SCHEMA = "k int, x double, s string"
_DP_SPLIT = 33
_DIM_ROWS = [(k, f"name{k}", k * 10) for k in (0, 2, 3, 3, 5, 8, 11)]
_DIM_SCHEMA = "k long, name string, w int"


def _replicated(spark, rows, schema):
    """A frame every rank holds whole."""
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import LocalRelation

    df = spark.createDataFrame(rows, schema)
    return type(df)(LocalRelation(df._table(), sharded=False), spark)


def _dp_results(spark, rows):
    df = spark.createDataFrame(rows, _DP_SCHEMA)
    dim = _replicated(spark, _DIM_ROWS, _DIM_SCHEMA)
    t = lambda d: [tuple(r) for r in d.collect()]  # noqa: E731
    agg = df.groupBy("k").agg(F.count("*").alias("n"), F.sum("x").alias("sx"))
    return (t(df.join(dim, "k")), t(df.join(dim, "k", "left")), t(df.join(dim, "k", "semi")), t(df.join(dim, "k", "anti")),
            t(df.join(agg, "k", "left")), df.join(dim, "k", "left").count())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DQ4ML_DEVICE="cpu")
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm
    from net.jgp.labs.sparkdq4ml_amd.sql.plan import is_sharded

    comm.init(backend="gloo")
    rows = _dp_rows()
    mine = rows[:_DP_SPLIT] if rank == 0 else rows[_DP_SPLIT:]
    spark = SparkSession.builder().master("cpu").getOrCreate()
    res = _dp_results(spark, mine)
    df = spark.createDataFrame(mine, _DP_SCHEMA)
    dim = _replicated(spark, _DIM_ROWS, _DIM_SCHEMA)
    raised = []
    for left, right, how in ((df, dim, "full"), (df, dim, "right"), (dim, df, "inner"), (df, df.withColumnRenamed("x", "x2")
                                                                                         .withColumnRenamed("s", "s2"), "inner"),
                             (dim, df, "semi")):
        try:
            left.join(right, "k", how)
            raised.append("")
        except AnalysisException as e:
            raised.append(str(e))
    sharded = (is_sharded(df.join(dim, "k")._plan), is_sharded(dim.join(dim.withColumnRenamed("w", "w2")
                                                                        .withColumnRenamed("name", "n2"), "k")._plan))
    q.put((rank, res, raised, sharded))
    comm.barrier()
    comm.shutdown()


def test_two_ranks_join_a_sharded_left_with_a_replicated_right(cpu_session):
    want = _dp_results(cpu_session, _dp_rows())
    assert len(want[0]) > 20 and want[5] == len(want[1]) > len(want[0]) and len(want[2]) + len(want[3]) == 80
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, got, raised, sharded in res:
        assert repr(got) == repr(want)  # the ranks' rows in rank order are the single-process rows
        assert all("shuffle join across ranks is not implemented" in r for r in raised), raised
        assert sharded == (True, False)
