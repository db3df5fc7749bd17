"""Aggregate expressions (``count`` / ``sum`` / ``avg`` / ``min`` / ``max``), ``GroupedData`` and the
execution of ``plan.Aggregate`` / ``plan.Deduplicate`` on ``ops.kernels.group_encode`` /
``group_agg``.

Results are exact and reproducible: counts, integer sums, minima and maxima are integer work, and
a sum of doubles is the correctly rounded value of a fixed-point accumulation whose window is the
top 128 bits below the column's largest magnitude (``ops/groupby.py``).  Groups follow Spark 3's
rule for floating keys (``-0.0`` and ``0.0`` are one group, so are all NaN; 2.4 kept them apart,
SPARK-26021), null keys form a group of their own, and the result rows ascend with the key, null
first.  On a data-parallel plan every rank encodes its shard, the ranks exchange only their unique
keys and their integer accumulators, and every rank holds the whole result.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops.keys import I64_MIN
from .expressions import Alias, AnalysisException, ColRef, Expr, Lit, to_expr
from .table import ColumnData, Table
from .types import (BooleanType, DoubleType, LongType, StringType, StructField, StructType, VectorUDT, is_numeric)

__all__ = ["AggExpr", "GroupedData", "build_aggregate", "contains_aggregate", "aggregate_table", "dedupe_table",
           "sort_table"]

_FNS = ("count", "sum", "avg", "min", "max")


class AggExpr(Expr):
    """``fn(child)``; ``child`` None is ``count(*)``.  Only ``agg`` / ``GROUP BY`` evaluate it."""

    def __init__(self, fn: str, child: Optional[Expr]):
        fn = {"mean": "avg"}.get(fn.lower(), fn.lower())
        if fn not in _FNS:
            raise AnalysisException(f"Undefined function: '{fn}'")
        if child is None and fn != "count":
            raise AnalysisException(f"Invalid number of arguments for function {fn}")
        self.fn = fn
        self.child = child

    def children(self):
        return [] if self.child is None else [self.child]

    def _outside(self):
        return AnalysisException(f"aggregate function {self.sql_name()} is only allowed in agg() or with GROUP BY")

    def data_type(self, schema):
        raise self._outside()

    def nullable(self, schema):
        return self.fn != "count"

    def eval(self, ctx):
        raise self._outside()

    def sql_name(self):
        if self.child is None or (isinstance(self.child, Lit) and self.child.value == 1):
            return "count(1)"
        return f"{self.fn}({self.child.sql_name()})"

    def result_type(self, schema):
        """Spark's result type over the input ``schema``."""
        if self.fn == "count":
            if self.child is not None:
                self.child.data_type(schema)
            return LongType()
        dt = self.child.data_type(schema)
        if self.fn in ("min", "max"):
            if isinstance(dt, StringType):
                raise AnalysisException(f"{self.sql_name()}: min / max of a string column is not supported yet")
            if isinstance(dt, VectorUDT):
                raise AnalysisException(f"cannot resolve '{self.sql_name()}' due to data type mismatch")
            return dt
        if not is_numeric(dt):
            raise AnalysisException(f"cannot resolve '{self.sql_name()}' due to data type mismatch: function {self.fn} "
                                    f"requires numeric types, not {dt.simpleString()}")
        if self.fn == "avg":
            return DoubleType()
        return LongType() if dt.torch_dtype in (torch.int32, torch.int64) else DoubleType()


def contains_aggregate(e: Expr) -> bool:
    return isinstance(e, AggExpr) or any(contains_aggregate(c) for c in e.children())


def _unalias(e: Expr) -> Tuple[Expr, Optional[str]]:
    return (e.child, e.name) if isinstance(e, Alias) else (e, None)


def build_aggregate(child, key_exprs: Sequence[Expr], agg_exprs: Sequence[Expr]):
    """``Aggregate`` over a ``Project`` that evaluates the key and input expressions, so that the
    node sees only column references.  ``agg_exprs``: ``AggExpr``, possibly under an ``Alias``."""
    from .plan import Aggregate, Project, output_name

    cs = child.schema()
    proj, have = [], set()

    def add(e: Expr, name: str):
        if name.lower() not in have:
            have.add(name.lower())
            proj.append(e)

    from .window import contains_window

    keys = []
    for k in list(key_exprs) + list(agg_exprs):
        if contains_window(k):
            raise AnalysisException(f"window functions are not allowed in GROUP BY or inside an aggregate, but found "
                                    f"{k.sql_name()}")
    for k in key_exprs:
        if contains_aggregate(k):
            raise AnalysisException(f"aggregate functions are not allowed in GROUP BY, but found {k.sql_name()}")
        dt = k.data_type(cs)
        if isinstance(dt, VectorUDT):
            raise AnalysisException(f"expression {k.sql_name()} cannot be used as a grouping expression because its "
                                    f"data type {dt.simpleString()} is not an orderable data type")
        name = output_name(k)
        if isinstance(k, ColRef):
            name = k._field(cs).name
        add(k, name)
        keys.append(name)
    aggs = []
    for i, a in enumerate(agg_exprs):
        base, alias = _unalias(a)
        if not isinstance(base, AggExpr):
            raise AnalysisException(f"expression '{a.sql_name()}' is neither present in the group by, nor is it an "
                                    f"aggregate function")
        if base.child is not None and contains_aggregate(base.child):
            raise AnalysisException("It is not allowed to use an aggregate function in the argument of another "
                                    "aggregate function")
        base.result_type(cs)
        inp = None
        if base.child is not None and not (base.fn == "count" and isinstance(base.child, Lit) and base.child.value is not None):
            if isinstance(base.child, ColRef):
                inp = base.child._field(cs).name
                add(base.child, inp)
            else:
                inp = f"_agg_in_{i}"
                add(Alias(base.child, inp), inp)
        aggs.append((base.fn, inp, alias or base.sql_name()))
    return Aggregate(Project(child, proj), keys, aggs)


# ------------------------------------------------------------------------------------------
# execution
# ------------------------------------------------------------------------------------------
class _Ranks:
    """Cross-rank hooks of ``group_encode`` / ``group_agg`` on a data-parallel plan: integer sum /
    max / min all-reduces of the accumulator words, and the exchange of the unique keys."""

    @staticmethod
    def reduce(acc: torch.Tensor, kinds) -> torch.Tensor:
        from ..ops.groupby import K_ADD, K_MAX, K_MIN, K_OR
        from ..parallel import comm

        out = acc.clone()
        k = torch.tensor(kinds)
        add, mx, mn, orr = (torch.nonzero(k == v).flatten().to(acc.device) for v in (K_ADD, K_MAX, K_MIN, K_OR))
        if add.numel():
            out[:, add] = comm.all_reduce_sum(acc[:, add].contiguous())
        if mx.numel():  # unsigned max: flip the top bit, signed max
            out[:, mx] = comm.all_reduce_max((acc[:, mx] ^ I64_MIN).contiguous()) ^ I64_MIN
        if mn.numel():  # unsigned min: the max of the complements
            out[:, mn] = ~(comm.all_reduce_max((~acc[:, mn] ^ I64_MIN).contiguous()) ^ I64_MIN)
        if orr.numel():  # flag words hold three bits: or = per-bit max
            f = acc[:, orr]
            bits = torch.stack([(f >> b) & 1 for b in range(3)], dim=0).contiguous()
            bits = comm.all_reduce_max(bits)
            out[:, orr] = bits[0] | (bits[1] << 1) | (bits[2] << 2)
        return out

    @staticmethod
    def union(keys: torch.Tensor) -> torch.Tensor:
        from ..parallel import comm

        parts = comm.all_gather_object(keys.cpu().numpy())
        return torch.from_numpy(np.unique(np.concatenate(parts))).to(keys.device)


def _hooks(sharded: bool):
    return (_Ranks.reduce, _Ranks.union) if sharded else (None, None)


def _key_column(c: ColumnData, device, sharded: bool):
    """``(tensor, valid, dictionary)`` of a key column for ``group_encode``.  A string column is
    dictionary-encoded on the host (the documented slow path: a device string column builds its
    Python strings first): its codes index the sorted dictionary, so code order is string order."""
    if isinstance(c.dtype, VectorUDT):
        raise AnalysisException("a vector column cannot be a grouping key")
    if isinstance(c.values, list) or isinstance(c.dtype, StringType):
        vals = c.values
        uniq = sorted({v for v in vals if v is not None})
        if sharded:
            from ..parallel import comm

            uniq = sorted(set().union(*comm.all_gather_object(uniq)))
        code = {v: i for i, v in enumerate(uniq)}
        codes = torch.tensor([code.get(v, 0) for v in vals], dtype=torch.int32).to(device)
        valid = torch.tensor([v is not None for v in vals], dtype=torch.bool).to(device)
        if c.valid is not None:
            valid = valid & c.valid.to(device)
        return codes, valid, uniq
    return c.values, c.valid, None


def _encode(t: Table, names: Sequence[str], sharded: bool):
    from ..ops import kernels

    reduce, union = _hooks(sharded)
    cols = [_key_column(t.column(k), t.device, sharded) for k in names]
    gid, G, keyvals = kernels.group_encode_columns([c[0] for c in cols], [c[1] for c in cols], t.sel, reduce=reduce, union=union)
    return gid, G, keyvals, [c[2] for c in cols]


def _pending(t: Table):
    pending = [ck for c in t.columns for ck in getattr(c, "checks", ())]
    if pending:
        from ..runtime.checks import verify

        verify(pending)


def aggregate_table(t: Table, keys: Sequence[str], aggs, schema: StructType, sharded: bool) -> Table:
    """The result table of ``Aggregate``: one row per group in key order (null first), on ``t``'s
    device.  ``aggs``: ``(fn, input column or None, output name)``."""
    from ..ops import groupby as gb
    from ..ops import kernels

    reduce, _ = _hooks(sharded)
    dev = t.device
    if keys:
        gid, G, keyvals, dicts = _encode(t, keys, sharded)
    else:
        gid, G, keyvals, dicts = None, 1, [], []
    slots, index = [], {}

    def slot(op, name):
        if (op, name) not in index:
            c = t.column(name)
            vals = None if (op == gb.COUNT or isinstance(c.values, list)) else c.values
            if op != gb.COUNT and isinstance(c.dtype, BooleanType):
                vals = c.values.to(torch.uint8)
            valid = c.valid
            if isinstance(c.values, list):  # count(string): only the validity is read
                valid = torch.tensor([v is not None for v in c.values], dtype=torch.bool).to(dev)
            index[(op, name)] = len(slots)
            slots.append((op, vals, valid, None))
        return index[(op, name)]

    plan = []
    for fn, inp, _ in aggs:
        if inp is None:
            plan.append((fn, None, None))
            continue
        c = t.column(inp)
        cnt = slot(gb.COUNT, inp)
        if fn == "count":
            plan.append((fn, cnt, None))
        elif fn == "sum" and not isinstance(c.values, list) and c.values.dtype in (torch.int32, torch.int64):
            plan.append((fn, cnt, slot(gb.SUM_I, inp)))
        elif fn in ("sum", "avg"):
            plan.append((fn, cnt, slot(gb.SUM_F, inp)))
        else:
            plan.append((fn, cnt, slot(gb.MIN if fn == "min" else gb.MAX, inp)))
    # the scale pre-pass of every fixed-point sum in one call
    need = [i for i, s in enumerate(slots) if s[0] == gb.SUM_F]
    es = kernels.group_scale([slots[i][1] for i in need], [slots[i][2] for i in need], t.sel, reduce=reduce)
    for i, e in zip(need, es):
        slots[i] = slots[i][:3] + (e,)
    acc, off = kernels.group_agg(gid, G, slots, t.sel, reduce=reduce, n=t.nrows)
    _pending(t)
    rows = acc[:, 0]
    keep = torch.nonzero(rows > 0).flatten() if keys else torch.arange(1, device=acc.device)
    acc = acc.index_select(0, keep).to(dev)
    cols: List[ColumnData] = []
    fields = schema.fields
    for (vals, valid), d, f in zip(keyvals, dicts, fields):
        vals, valid = vals.to(dev).index_select(0, keep.to(dev)), valid.to(dev).index_select(0, keep.to(dev))
        if d is not None:
            ok = valid.cpu().tolist()
            vals = [d[i] if o else None for i, o in zip(vals.cpu().tolist(), ok)]
        elif vals.dtype != f.dataType.torch_dtype:
            vals = vals.to(f.dataType.torch_dtype)
        cols.append(ColumnData(f.dataType, vals, None if bool(valid.all()) else valid, dict(f.metadata)))
    for (fn, cnt, val), f in zip(plan, fields[len(keyvals):]):
        if cnt is None:
            cols.append(ColumnData(f.dataType, acc[:, 0].clone(), None))
            continue
        n_c = acc[:, off[cnt]]
        if fn == "count":
            cols.append(ColumnData(f.dataType, n_c.clone(), None))
            continue
        op, col, _, e = slots[val]
        w = off[val]
        if op == gb.SUM_I:
            v = acc[:, w].clone()
        elif op == gb.SUM_F:
            v = gb.finalize_sum(acc[:, w:w + 4], acc[:, w + 4], e)
            if fn == "avg":
                v = v / n_c.to(torch.float64)
        else:
            v = gb.keys_to_values(acc[:, w] ^ I64_MIN, col.dtype)
            if v.dtype != f.dataType.torch_dtype:
                v = v.to(f.dataType.torch_dtype)
        valid = n_c > 0
        v = torch.where(valid, v, torch.zeros_like(v))
        cols.append(ColumnData(f.dataType, v, None if bool(valid.all()) else valid))
    return Table(schema, cols, int(keep.numel()), None, dev)


def dedupe_table(t: Table, subset: Sequence[str], sharded: bool) -> Table:
    """``t`` with its selection narrowed to the first live row (in row order) of every group of
    the ``subset`` columns; no row is moved.  On a data-parallel plan a row's index counts the
    rows of the lower ranks, and the groups' minima are all-reduced."""
    from ..ops import groupby as gb
    from ..ops import kernels

    reduce, _ = _hooks(sharded)
    offset = 0
    if sharded:
        from ..parallel import comm

        offset = sum(comm.all_gather_object(int(t.nrows))[:comm.rank()])
    gid, G, _, _ = _encode(t, subset, sharded)
    acc, off = kernels.group_agg(gid, G, [(gb.FIRST, None, None)], t.sel, row_offset=offset, reduce=reduce, n=t.nrows)
    first = acc[:, off[0]][acc[:, 0] > 0] - offset  # G-sized: the surviving row of every group
    first = first[(first >= 0) & (first < t.nrows)].to(t.device)
    keep = torch.zeros(t.nrows, dtype=torch.bool, device=t.device)
    keep[first] = True
    return Table(t.schema, t.columns, t.nrows, keep, t.device)


def sort_table(t: Table, orders) -> Table:
    """The result table of ``Sort``: the live rows of ``t`` in the stable sorted order of
    ``orders`` = ``(column, ascending, nulls_first)``, compact (every column gathered by the
    permutation of ``ops.kernels.sort_permutation``, no selection vector).  A string column sorts
    by its host dictionary codes; the selection vector goes to the sort as it is."""
    from ..ops import kernels

    _pending(t)
    cols, valids = [], []
    for name, _, _ in orders:
        c = t.column(name)
        if isinstance(c.dtype, VectorUDT):
            raise AnalysisException(f"cannot sort by '{name}': {c.dtype.simpleString()} is not an orderable data type")
        vals, valid, _ = _key_column(c, t.device, False)
        cols.append(vals)
        valids.append(valid)
    perm = kernels.sort_permutation(cols, valids, t.sel, [o[1] for o in orders], [o[2] for o in orders])
    perm = perm.to(t.device)
    return Table(t.schema, [c.index(perm) for c in t.columns], int(perm.numel()), None, t.device)


# ------------------------------------------------------------------------------------------
# DataFrame side
# ------------------------------------------------------------------------------------------
def _col_expr(c) -> Expr:
    return ColRef(c) if isinstance(c, str) else to_expr(c)


def count(c="*") -> "AggExpr":
    if isinstance(c, str) and c == "*":
        return AggExpr("count", None)
    return AggExpr("count", _col_expr(c))


class GroupedData:
    """``RelationalGroupedDataset``: the result of ``DataFrame.groupBy``."""

    def __init__(self, df, keys: Sequence[Expr]):
        self._df = df
        self._keys = list(keys)

    def agg(self, *exprs):
        if len(exprs) == 1 and isinstance(exprs[0], dict):
            exprs = [AggExpr(fn, None if (fn.lower() == "count" and c == "*") else ColRef(c)) for c, fn in exprs[0].items()]
        if not exprs:
            raise ValueError("agg() needs at least one aggregate expression")
        aggs = [to_expr(e) for e in exprs]
        return self._df._with(build_aggregate(self._df._plan, self._keys, aggs))

    def count(self):
        return self.agg(Alias(AggExpr("count", None), "count"))

    def _numeric(self, fn: str, cols):
        schema = self._df.schema
        if not cols:
            keyed = {k.name.lower() for k in self._keys if isinstance(k, ColRef)}
            cols = [f.name for f in schema.fields if is_numeric(f.dataType) and f.name.lower() not in keyed]
        else:
            for c in cols:
                n = schema.resolve_ci(c)
                if n is None:
                    raise AnalysisException(f'Cannot resolve column name "{c}" among ({", ".join(schema.names)});')
                if not is_numeric(schema[n].dataType):
                    raise AnalysisException(f'"{c}" is not a numeric column. Aggregation function can only be applied '
                                            f'on a numeric column.;')
        return self.agg(*[AggExpr(fn, ColRef(c)) for c in cols]) if cols else self.agg(Alias(AggExpr("count", None), "count")).drop("count")

    def sum(self, *cols):
        return self._numeric("sum", cols)

    def avg(self, *cols):
        return self._numeric("avg", cols)

    mean = avg

    def min(self, *cols):
        return self._numeric("min", cols)

    def max(self, *cols):
        return self._numeric("max", cols)
