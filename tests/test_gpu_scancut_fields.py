"""The byte-parallel CSV cutter (``ops/scancut.py``) end to end with sharp oracles: field spellings,
kernel shapes and window edges the synthetic-CSV tests (tests/test_gpu_scancut.py) never reach.

Family A (values k / 64, |value| < 2^10, every legal spelling): every sum is exact in f64, the
oracle is integer arithmetic, the whole statistics vector is compared with ``np.array_equal``.
Family B (general decimals of at most 9 digits): per entry ``|got - ref| <= (n + 2) 2^-53 Σ|terms|``
against exact integer sums of the ``float(text)`` values.  Family C (one live row): every
statistic is one value or one rounded product, compared with ``==`` (a sum of -0.0 and exact
zeros is +0.0, which ``==`` takes as equal).

Every case checks that the cutter ran (``scancut.STATS``) and that its deferred fact checks
pass, so a silent reroute cannot pass.  Files of one shape share their facts (the pools hold a
shortest and a longest row, ``_cut_cases``) and with them one hipRTC build: 9 family A shapes (the
sweeps and the large files reuse them), 2 family B, 2 family C."""
import os

import numpy as np
import pytest
import torch

import _cut_cases as cc

pytestmark = pytest.mark.gpu
W = cc.WINDOW


@pytest.fixture
def spark():
    from net.jgp.labs.sparkdq4ml_amd import SparkSession
    from net.jgp.labs.sparkdq4ml_amd.runtime import filecache

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    filecache.clear()
    s = SparkSession.builder().master("mi355x[*]").config("dq4ml.csv.deviceThresholdBytes", "0").getOrCreate()
    old = os.environ.get("DQ4ML_CUT_MIN_LINE")
    os.environ["DQ4ML_CUT_MIN_LINE"] = "0"  # the cutter for d <= 8 too
    yield s
    if old is None:
        os.environ.pop("DQ4ML_CUT_MIN_LINE", None)
    else:
        os.environ["DQ4ML_CUT_MIN_LINE"] = old
    s.stop()


_POOLS = {}


def _pool(kind, shape, **kw):
    key = (kind, shape.name)
    if key not in _POOLS:
        _POOLS[key] = (cc.pool_a if kind == "a" else cc.pool_b)(shape, **kw)
    return _POOLS[key]


class Cut:
    """One action through the cutter: the statistics, the compiled plan, the relation's facts."""

    def __init__(self, spark, path, shape, nrows):
        from net.jgp.labs.sparkdq4ml_amd import LinearRegression, VectorAssembler, callUDF, col
        from net.jgp.labs.sparkdq4ml_amd.dq.rules import RangeRule
        from net.jgp.labs.sparkdq4ml_amd.models import regression
        from net.jgp.labs.sparkdq4ml_amd.ops import scancut
        from net.jgp.labs.sparkdq4ml_amd.runtime.checks import verify
        from net.jgp.labs.sparkdq4ml_amd.sql.types import DataTypes

        def load():
            return spark.read().format("csv").option("inferSchema", "true").load(path)

        assert load().count() == nrows  # the eager scan: the facts
        spark.udf().register("rangeRule", RangeRule(cc.LO, cc.HI, name="rangeRule"), DataTypes.DoubleType)
        df = load()
        self.facts = df._plan.fused
        df = df.withColumn("y_ok", callUDF("rangeRule", col(f"_c{shape.label}"))).filter(col("y_ok") > 0)
        df = df.withColumn("label", col("y_ok"))
        df = VectorAssembler().setInputCols([f"_c{i}" for i in shape.feats]).setOutputCol("features").transform(df)
        before = scancut.STATS["cut_grams"]
        plans, launch_cut = [], scancut.launch_cut

        def spy(cp, rel, d):
            plans.append(cp)
            return launch_cut(cp, rel, d)

        scancut.launch_cut = spy  # (the compiled plan this action launches)
        try:
            fused = regression._fused_scan_stats(LinearRegression(solver="normal", regParam=1e-3), df)
        finally:
            scancut.launch_cut = launch_cut
        assert fused is not None and scancut.STATS["cut_grams"] == before + 1 and len(plans) == 1, "the cutter did not run"
        verify(fused.checks)
        self.stats = fused.flat.cpu().numpy()
        self.cp = plans[0]
        self.kinds = [int(k) for k in self.facts["kinds"]]
        assert self.kinds == [1 if k == "i" else 0 for k in shape.kinds], "inferred column kinds"


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _run_a(spark, tmp_path, shape, pool, sel, final=True, name="a.csv"):
    data = cc.join_rows([pool.rows[i] for i in sel], shape.term, final)
    cut = Cut(spark, _write(tmp_path, name, data), shape, len(sel))
    ref = cc.oracle_a(shape, pool.values, np.bincount(sel, minlength=len(pool.rows)))
    assert ref[0] > 0
    return cut, ref, len(data)


# what tells each shape's code path apart, checked on the compiled plan
def _path_a(shape, cp):
    sh, src = cp.sh, cp.src
    n = shape.name
    if n in ("d32", "ones"):
        assert sh.yfirst and sh.mfma and sh.vstrip and "gt[q_ga] = dv;" in src
    if n in ("sub12", "sub12i"):
        assert sh.mfma and not sh.yfirst and not sh.vstrip and "gt[q_ga] = dv;" not in src
        assert "*(fs >= 0 ? gt + q_gb + fs" in src and "ctab[2 * c + 1]" in src  # one store, table lookups
        assert ("csv_conforms(dot ?" in src) == (n == "sub12i")
    if n == "d3of40":
        assert not sh.blocked
    if n == "d9of200":
        assert sh.H == 4096 and sh.HG == 2 and "const bool hfast = false;" in src
    if n in ("d80", "d100", "d128"):
        assert sh.blocked and not sh.mfma and "DQ_TIDX" not in src and "DQ_GIDX" in src
        assert (sh.U > 256) == (n != "d80")  # more 4 x 4 blocks than threads: several per thread
    if n == "ones":
        assert sh.DCAP == (sh.H + W) // 2 + 64  # sized by the delimiter density, not by the row count


A_SHAPES = ["d32", "sub12", "sub12i", "d3of40", "d9of200", "d80", "d100", "d128", "ones"]


@pytest.mark.parametrize("name", A_SHAPES)
def test_exact_sums_are_bitwise(spark, tmp_path, name):
    """Family A over 3 to 5 windows of every kernel shape."""
    from net.jgp.labs.sparkdq4ml_amd.ops import scancut

    shape = cc.SHAPES[name]
    pool = _pool("a", shape)
    rng = np.random.default_rng(17)
    sel = cc.rows_for_bytes(pool, int(3.4 * W), rng)
    cut, ref, nbytes = _run_a(spark, tmp_path, shape, pool, sel)
    _path_a(shape, cut.cp)
    assert 3 <= scancut.n_windows(0, nbytes) <= 6
    print(f"{name}: {nbytes} bytes, {len(sel)} rows, {int(ref[0])} live")
    assert np.array_equal(cut.stats, ref), np.nonzero(cut.stats != ref)[0][:10]


@pytest.mark.parametrize("name", ["d32", "d9of200"])
def test_exact_sums_with_carried_row_starts(spark, tmp_path, name):
    """A file large enough that every block owns at least 2 consecutive windows: the row start of
    a block's second window is carried from the cut of its first."""
    from net.jgp.labs.sparkdq4ml_amd.ops import native, scancut

    shape = cc.SHAPES[name]
    pool = _pool("a", shape)
    h = native.hip()
    cus = int(h.device_info()["multiProcessorCount"])
    sel = cc.rows_for_bytes(pool, 2 * W * 4 * cus + W, np.random.default_rng(23))
    assert len(sel) < 2 ** 20
    cut, ref, nbytes = _run_a(spark, tmp_path, shape, pool, sel)
    assert nbytes > 2 * W * 4 * cus
    nwin = scancut.n_windows(cut.facts["buf"].data_ptr(), int(cut.facts["n"]))
    assert nwin >= 2 * scancut._grid(h, cut.cp.per_cu, nwin)
    print(f"{name}: {nbytes} bytes, {len(sel)} rows, {nwin} windows, {cus} CUs")
    assert np.array_equal(cut.stats, ref), np.nonzero(cut.stats != ref)[0][:10]


@pytest.mark.parametrize("name", ["d32", "d100"])
def test_row_boundaries_slide_across_a_window_boundary(spark, tmp_path, name):
    """36 files: zero-padding in the first row moves every later row boundary one byte at a time,
    so that one row's terminator goes from 18 bytes before the second window to 17 bytes into
    it (for CR LF: also the CR as the window's last byte and the LF as the next one's first).
    Then file lengths n = -1, 0, +1 (mod 16384), each with and without a final terminator (with
    none at n = 0 the virtual terminator alone fills an extra window)."""
    from net.jgp.labs.sparkdq4ml_amd.ops import scancut

    shape = cc.SHAPES[name]
    pool = _pool("a", shape)
    tl = len(shape.term)
    sel, t0 = cc.sweep_rows(pool, 2.3, np.random.default_rng(31), W - 18)
    body = [pool.rows[i] for i in sel]
    srcs = set()

    def run(shift, final, rows, ks, tag):
        first, k0 = cc.padded_first_row(shape, shift)
        data = cc.join_rows([first] + rows, shape.term, final)
        cut = Cut(spark, _write(tmp_path, f"s{tag}.csv", data), shape, len(rows) + 1)
        ref = cc.oracle_a(shape, np.vstack([k0[None, :], ks]))
        srcs.add(cut.cp.src)
        assert np.array_equal(cut.stats, ref), (tag, shift, final, len(data), np.nonzero(cut.stats != ref)[0][:10])
        return data

    s0 = W - 18 - t0
    seen = set()
    for s in range(s0, s0 + 36):
        data = run(s, True, body, pool.values[sel], f"w{s}")
        assert data[t0 + s:t0 + s + tl] == shape.term
        seen.add(t0 + s - W)
    assert seen == set(range(-18, 18))  # (-1: the terminator's first byte is the window's last)
    base = len(cc.join_rows([cc.padded_first_row(shape, 0)[0]] + body, shape.term, False))
    for final in (False, True):
        for r in (-1, 0, 1):
            s = (r - base - (tl if final else 0)) % W
            # more rows at the end until the first row's padding can make up the rest
            rows, idx = list(body), list(sel)
            j = 2
            while s > 8 * shape.C:
                while pool.lens[j] + tl > s:
                    j += 1
                s -= int(pool.lens[j]) + tl
                rows.append(pool.rows[j])
                idx.append(j)
                j += 1
            data = run(s, final, rows, pool.values[idx], f"n{r}{int(final)}")
            assert (len(data) - r) % W == 0
            assert scancut.n_windows(0, len(data)) == len(data) // W + 1
    assert len(srcs) == 1  # one compiled kernel for the whole sweep


@pytest.mark.parametrize("name", ["d32", "sub12"])
def test_general_decimals_within_the_rounding_bound(spark, tmp_path, name):
    """Family B: 1 000 rows of arbitrary <= 9-digit decimals."""
    shape = cc.SHAPES[name]
    pool = _pool("b", shape, size=1000)
    sel = np.random.default_rng(5).permutation(1000)
    data = cc.join_rows([pool.rows[i] for i in sel], shape.term, True)
    cut = Cut(spark, _write(tmp_path, "b.csv", data), shape, 1000)
    ref, absref, n = cc.oracle_b(shape, pool.values[sel])
    assert 100 < n <= 1000 and cut.stats[0] == n
    one2 = float(1 << cc.SCALE_B) ** 2
    rel = max(abs(float(g) - r / one2) / max(a / one2, 1e-300) for g, r, a in zip(cut.stats, ref, absref))
    print(f"{name}: {n} live rows, max |got - ref| / sum|terms| = {rel:.3e} (bound {(n + 2) * 2.0 ** -53:.3e})")
    bad = cc.within_b(cut.stats, ref, absref, n)
    assert not bad, (bad[:10], [(float(cut.stats[i]), ref[i] / one2) for i in bad[:5]])


@pytest.mark.parametrize("name", ["d32c", "d100c"])
def test_single_live_row_is_bitwise(spark, tmp_path, name):
    """Family C: general decimals, the label ``001`` in one row and ``200`` elsewhere (equal
    lengths: same facts, same kernel); RangeRule(0, 150) keeps that row alone."""
    shape = cc.SHAPES[name]
    pool = _pool("c", shape, size=600, label=(b"001", b"200"))
    tl = len(shape.term)
    rng = np.random.default_rng(41)
    sel = cc.rows_for_bytes(pool, int(2.6 * W), rng)
    n = len(sel)
    starts = np.concatenate([[0], np.cumsum(pool.lens[sel] + tl)])  # row r spans [starts[r], starts[r + 1])
    srcs = set()

    def run(live, final, tag):
        rows = [pool.rows[i] for i in sel]
        f = rows[live].split(b",")
        f[shape.label] = b"001"
        rows[live] = b",".join(f)
        cut = Cut(spark, _write(tmp_path, f"c{tag}.csv", cc.join_rows(rows, shape.term, final)), shape, n)
        v = pool.values[sel[live]].copy()
        v[shape.label] = 1.0
        ref = cc.oracle_c(shape, v)
        srcs.add(cut.cp.src)
        assert np.array_equal(cut.stats, ref), (tag, live, np.nonzero(cut.stats != ref)[0][:10])
        return cut

    RR = run(0, True, "first").cp.sh.RR
    run(n - 1, False, "last_open")
    run(n - 1, True, "last")
    for w in (1, 2):  # the row that holds byte w * W - 1 and byte w * W
        r = int(np.searchsorted(starts, w * W, side="right")) - 1
        assert starts[r] < w * W < starts[r + 1] - tl, "no row straddles the window boundary"
        run(r, True, f"straddle{w}")
    # a row of a later tile round: row index >= RR among the rows that end in its window
    for w in (0, 1):
        ends = starts[1:] - tl  # each row's terminator
        inwin = np.nonzero((ends >= w * W) & (ends < (w + 1) * W))[0]
        assert inwin.size > RR + 2, (inwin.size, RR)
        run(int(inwin[RR + 1]), True, f"round2_{w}")
        run(int(inwin[-1]), True, f"lastround_{w}")
    assert len(srcs) == 1
