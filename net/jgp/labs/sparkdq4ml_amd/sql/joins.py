"""Analysis and execution of ``plan.Join`` on ``ops.kernels.join_pairs`` / ``join_mask``.

An equi-join of two tables on one or more key column pairs.  The right table is the build side of
the hash join and the left table probes it, so the smaller table belongs on the right.  Join keys
follow Spark: ``-0.0`` joins ``0.0``, NaN joins NaN, a null key matches nothing.  The result's row
order is defined (``ops/join.py``): left rows in row order, the matches of one left row in right
row order, then (full outer) the unmatched right rows in row order.

Deviations from Spark, all raising ``AnalysisException``: a non-key column name that appears on
both sides (Spark keeps the ambiguous pair; rename one with ``withColumnRenamed``), ``ON``
conditions other than a conjunction of column equalities, cross joins, non-equi joins, and joins
that need a shuffle across data-parallel ranks.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .aggregates import _pending
from .expressions import AnalysisException, BinOp, ColRef, Expr
from .table import ColumnData, DeviceStringColumn, Table, empty_column
from .types import (BooleanType, DataType, DoubleType, FloatType, IntegerType, LongType, StringType, StructField, StructType,
                    TimestampType, VectorUDT)

__all__ = ["HOW_SPELLINGS", "normalize_how", "join_schema", "join_table", "using_keys", "condition_keys"]

HOW_SPELLINGS = {
    "inner": ("inner",),
    "left_outer": ("left", "leftouter", "left_outer"),
    "right_outer": ("right", "rightouter", "right_outer"),
    "full_outer": ("outer", "full", "fullouter", "full_outer"),
    "left_semi": ("semi", "leftsemi", "left_semi"),
    "left_anti": ("anti", "leftanti", "left_anti"),
}
_HOW = {s.replace("_", ""): how for how, ss in HOW_SPELLINGS.items() for s in ss}


def normalize_how(how) -> str:
    """Spark's spellings of the join type (case and underscores ignored) -> the canonical name."""
    if isinstance(how, str):
        got = _HOW.get(how.lower().replace("_", ""))
        if got is not None:
            return got
    if isinstance(how, str) and how.lower().replace("_", "") == "cross":
        raise AnalysisException("cross joins are not implemented")
    raise ValueError(f"Unsupported join type {how!r}. Supported join types include: "
                     + ", ".join(f"'{s}'" for ss in HOW_SPELLINGS.values() for s in ss) + ".")


# ------------------------------------------------------------------------------------------
# analysis
# ------------------------------------------------------------------------------------------
def _key_class(dt: DataType) -> Optional[str]:
    if isinstance(dt, (IntegerType, LongType)):
        return "int"
    if isinstance(dt, (FloatType, DoubleType)):
        return "float"
    if isinstance(dt, BooleanType):
        return "boolean"
    if isinstance(dt, StringType):
        return "string"
    if isinstance(dt, TimestampType):
        return "timestamp"
    return None


def common_key_type(lf: StructField, rf: StructField) -> DataType:
    """int with long gives long; anything with float or double gives double (lossy above 2^53, as
    in Spark); boolean joins boolean, string joins string, timestamp joins timestamp only."""
    lt, rt = lf.dataType, rf.dataType
    lc, rc = _key_class(lt), _key_class(rt)
    if lc is None or rc is None:
        bad = lf if lc is None else rf
        what = "a vector column" if isinstance(bad.dataType, VectorUDT) else f"a {bad.dataType.simpleString()} column"
        raise AnalysisException(f"cannot join on '{bad.name}': {what} cannot be a join key")
    if lc == rc:
        if type(lt) is type(rt):
            return lt
        return LongType() if lc == "int" else DoubleType()
    if {lc, rc} == {"int", "float"}:
        return DoubleType()
    raise AnalysisException(f"cannot join '{lf.name}' ({lt.simpleString()}) with '{rf.name}' ({rt.simpleString()}): the key "
                            f"types have no common type")


def _resolve(schema: StructType, name: str, side: str) -> str:
    got = schema.resolve_ci(name)
    if got is None:
        raise AnalysisException(f"USING column `{name}` cannot be resolved on the {side} side of the join. The {side}-side "
                                f"columns: [{', '.join(schema.names)}]")
    return got


def using_keys(ls: StructType, rs: StructType, names: Sequence[str]) -> List[Tuple[str, str]]:
    if not names:
        raise AnalysisException("cross joins are not implemented: a join needs at least one key column")
    return [(_resolve(ls, n, "left"), _resolve(rs, n, "right")) for n in names]


def condition_keys(ls: StructType, rs: StructType, cond: Expr) -> List[Tuple[str, str]]:
    """The key pairs of a join condition: a conjunction of ``ColRef == ColRef`` in which one name
    resolves only on the left and the other only on the right (a DataFrame's ``df.a`` carries no
    lineage here, so a name both sides have cannot be attributed)."""
    out: List[Tuple[str, str]] = []

    def walk(e: Expr):
        if isinstance(e, BinOp) and e.op == "and":
            walk(e.left)
            walk(e.right)
            return
        if not (isinstance(e, BinOp) and e.op in ("=", "==") and isinstance(e.left, ColRef) and isinstance(e.right, ColRef)):
            raise AnalysisException(f"join condition '{e.sql_name()}' is not implemented: a join takes column names (USING) or a "
                                    f"conjunction of equalities between one column of each side")
        pair = [None, None]
        for ref in (e.left, e.right):
            name = ref.name.rpartition(".")[2]
            inl, inr = ls.resolve_ci(name), rs.resolve_ci(name)
            if inl is not None and inr is not None:
                raise AnalysisException(f"Reference '{name}' is ambiguous: both sides of the join have it. Join on the name "
                                        f"itself (on='{name}') or rename one side with withColumnRenamed")
            if inl is None and inr is None:
                raise AnalysisException(f"cannot resolve '{name}' given input columns: [{', '.join(ls.names + rs.names)}]")
            i = 0 if inl is not None else 1
            if pair[i] is not None:
                raise AnalysisException(f"join condition '{e.sql_name()}' compares two columns of one side")
            pair[i] = inl if inl is not None else inr
        out.append((pair[0], pair[1]))

    walk(cond)
    return out


def join_schema(ls: StructType, rs: StructType, keys: Sequence[Tuple[str, str]], how: str, using: bool) -> StructType:
    """The output schema (Spark's order for a USING join: the key columns once, then the left's
    other columns, then the right's; the key comes from the left for inner / left, from the right
    for right, and is ``coalesce(left, right)`` in the common type for full; the columns of an outer
    side become nullable).  Semi / anti joins return the left's columns.  The condition form keeps
    both sides' columns."""
    common = [common_key_type(ls[l], rs[r]) for l, r in keys]  # raises on a key without a common type
    if how in ("left_semi", "left_anti"):
        return ls
    lkeys, rkeys = {l for l, _ in keys}, {r for _, r in keys}
    lrest = [f for f in ls.fields if not (using and f.name in lkeys)]
    rrest = [f for f in rs.fields if not (using and f.name in rkeys)]
    taken = {f.name.lower() for f in lrest} | ({l.lower() for l in lkeys} if using else set())
    for f in rrest:
        if f.name.lower() in taken:
            raise AnalysisException(f"the column '{f.name}' is on both sides of the join and is not a join key: rename one of "
                                    f"them with withColumnRenamed (ambiguous output columns are not supported)")
    lnull, rnull = how in ("right_outer", "full_outer"), how in ("left_outer", "full_outer")
    fields = []
    if using:
        for (l, r), ct in zip(keys, common):
            lf, rf = ls[l], rs[r]
            if how == "right_outer":
                fields.append(StructField(lf.name, rf.dataType, rf.nullable, dict(rf.metadata)))
            elif how == "full_outer":
                fields.append(StructField(lf.name, ct, True, dict(lf.metadata)))
            else:
                fields.append(StructField(lf.name, lf.dataType, lf.nullable, dict(lf.metadata)))
    fields += [StructField(f.name, f.dataType, f.nullable or lnull, dict(f.metadata)) for f in lrest]
    fields += [StructField(f.name, f.dataType, f.nullable or rnull, dict(f.metadata)) for f in rrest]
    return StructType(fields)


# ------------------------------------------------------------------------------------------
# execution
# ------------------------------------------------------------------------------------------
def _host_valid(c: ColumnData, dev) -> torch.Tensor:
    valid = torch.tensor([v is not None for v in c.values], dtype=torch.bool).to(dev)
    return valid if c.valid is None else (valid & c.valid.to(dev))


def _key_pair(lc: ColumnData, rc: ColumnData, dev):
    """``(left values, left valid, right values, right valid)`` of one key column pair, as tensors
    the kernels compare.  Strings are dictionary-encoded on the host over the union of both sides
    (the documented slow path: a device string column builds its Python strings first).  The two
    sides are cast to double only when they differ in class (int against float): i32 against i64
    and f32 against f64 compare as they are."""
    lstr = isinstance(lc.values, list) or isinstance(lc.dtype, StringType)
    rstr = isinstance(rc.values, list) or isinstance(rc.dtype, StringType)
    if lstr or rstr:
        lv, rv = lc.values, rc.values
        uniq = sorted({v for v in lv if v is not None} | {v for v in rv if v is not None})
        code = {v: i for i, v in enumerate(uniq)}
        enc = lambda vals: torch.tensor([code.get(v, 0) for v in vals], dtype=torch.int32).to(dev)  # noqa: E731
        return enc(lv), _host_valid(lc, dev), enc(rv), _host_valid(rc, dev)
    lv, rv = lc.values.to(dev), rc.values.to(dev)
    if lv.is_floating_point() != rv.is_floating_point():
        lv, rv = lv.to(torch.float64), rv.to(torch.float64)
    lvalid = None if lc.valid is None else lc.valid.to(dev)
    rvalid = None if rc.valid is None else rc.valid.to(dev)
    return lv, lvalid, rv, rvalid


def _keys(lt: Table, rt: Table, keys):
    from ..ops import kernels

    dev = lt.device
    pairs = [_key_pair(lt.column(l), rt.column(r), dev) for l, r in keys]
    if len(pairs) == 1:
        return pairs[0]
    lcols, rcols = [], []
    for lv, _, rv, _ in pairs:  # one dtype per pair for the joint encoding
        if lv.dtype != rv.dtype:
            wide = torch.float64 if lv.is_floating_point() else torch.int64
            lv, rv = lv.to(wide), rv.to(wide)
        lcols.append(lv)
        rcols.append(rv)
    lkey, lvalid, rkey, rvalid = kernels.join_key_columns(lcols, rcols, [p[1] for p in pairs], [p[3] for p in pairs], lt.sel,
                                                          rt.sel)
    return lkey, lvalid, rkey, rvalid


def _gather(c: ColumnData, idx: torch.Tensor, outer: bool, n_src: int, dev) -> ColumnData:
    """Rows ``idx`` of ``c``.  ``outer``: ``idx`` may hold -1, the missing side of an outer join:
    such a row is gathered with its index clamped to 0 and its validity cleared, which works for
    tensors, vectors, string lists and device string spans alike."""
    if not outer:
        return c.index(idx)
    if n_src == 0:  # nothing to clamp to: every row is null
        return empty_column(c.dtype, int(idx.numel()), dev)
    miss = idx < 0
    out = c.index(idx.clamp(min=0))
    ok = ~miss
    out.valid = ok.to(dev) if out.valid is None else (out.valid & ok.to(out.valid.device))
    if not isinstance(out, DeviceStringColumn) and isinstance(out.values, list):  # (device spans: the validity says it all)
        out.values = [v if o else None for v, o in zip(out.values, ok.tolist())]
    return out


def _coalesce(a: ColumnData, b: ColumnData, use_a: torch.Tensor, dtype: DataType, dev) -> ColumnData:
    """``a`` where ``use_a`` else ``b`` (the key column of a full outer USING join)."""
    if isinstance(a.values, list) or isinstance(b.values, list):
        pick = use_a.tolist()
        va, vb = a.to_pylist(), b.to_pylist()
        vals = [x if p else y for x, y, p in zip(va, vb, pick)]
        return ColumnData(dtype, vals, torch.tensor([v is not None for v in vals], dtype=torch.bool).to(dev), dict(a.meta))
    td = dtype.torch_dtype
    vals = torch.where(use_a, a.values.to(td), b.values.to(td))
    valid = torch.where(use_a, a.valid_mask(dev), b.valid_mask(dev))
    return ColumnData(dtype, vals, None if bool(valid.all()) else valid, dict(a.meta))


def join_table(lt: Table, rt: Table, keys: Sequence[Tuple[str, str]], how: str, using: bool, schema: StructType) -> Table:
    """The result table of ``Join``.  Semi and anti joins move no rows: they return ``lt`` with its
    selection vector narrowed (the same column objects).  Every other join returns a compact table:
    every column of each side gathered by its index vector through ``ColumnData.index``.
    ``right_outer`` is the ``left_outer`` of the swapped sides with the columns put back in place:
    its row order is therefore right-major (right rows in row order, the matches of one right row in
    left row order), and its build side is the left table."""
    from ..ops import kernels

    _pending(lt)
    _pending(rt)
    dev = lt.device
    lkey, lvalid, rkey, rvalid = _keys(lt, rt, keys)
    lsel = None if lt.sel is None else lt.sel.to(dev)
    rsel = None if rt.sel is None else rt.sel.to(dev)
    if how in ("left_semi", "left_anti"):
        mask = kernels.join_mask(lkey, rkey, lvalid, rvalid, lsel, rsel).to(dev)
        if how == "left_anti":
            mask = ~mask if lsel is None else (lsel & ~mask)
        return Table(lt.schema, lt.columns, lt.nrows, mask, dev)
    if how == "right_outer":
        ri, li = kernels.join_pairs(rkey, lkey, rvalid, lvalid, rsel, lsel, "left_outer")
    else:
        li, ri = kernels.join_pairs(lkey, rkey, lvalid, rvalid, lsel, rsel, how)
    li, ri = li.to(dev), ri.to(dev)
    louter, router = how in ("right_outer", "full_outer"), how in ("left_outer", "full_outer")
    lkeys, rkeys = {l for l, _ in keys}, {r for _, r in keys}
    cols: List[ColumnData] = []
    fields = schema.fields
    if using:
        for (l, r), f in zip(keys, fields):
            if how == "right_outer":
                cols.append(_gather(rt.column(r), ri, False, rt.nrows, dev))
            elif how == "full_outer":
                a = _gather(lt.column(l), li, True, lt.nrows, dev)
                b = _gather(rt.column(r), ri, True, rt.nrows, dev)
                cols.append(_coalesce(a, b, li >= 0, f.dataType, dev))
            else:
                cols.append(_gather(lt.column(l), li, False, lt.nrows, dev))
    for f, c in zip(lt.schema.fields, lt.columns):
        if not (using and f.name in lkeys):
            cols.append(_gather(c, li, louter, lt.nrows, dev))
    for f, c in zip(rt.schema.fields, rt.columns):
        if not (using and f.name in rkeys):
            cols.append(_gather(c, ri, router, rt.nrows, dev))
    return Table(schema, cols, int(li.numel()), None, dev)
