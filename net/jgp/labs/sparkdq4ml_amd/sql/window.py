"""Window functions: ``Window`` / ``WindowSpec`` (``org.apache.spark.sql.expressions.Window``),
the ``WindowExpr`` node behind ``Column.over`` and SQL ``OVER``, and ``window_table``, the execution
of ``plan.Window`` on the scans of ``ops/window.py``.

One sort per distinct (partition, order) specification (``kernels.sort_permutation`` over the
partition columns, then the order columns; strings by their dictionary codes), one heads and one
bounds pass per specification, the value words of all its expressions packed into common prefix
passes, and one finish launch per frame.  No row is moved: the new columns are scattered back to
their rows and the selection vector is kept.

Semantics are Spark's.  Without ``orderBy`` the frame is the whole partition; with it, ``RANGE
BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW`` (the current row's peers included).  Ranking functions
and ``lag`` / ``lead`` need an ``orderBy`` and ignore any frame.  Partition keys group like
``groupBy`` (``-0.0 = 0.0``, all NaN equal, nulls one partition), order keys order like
``orderBy``, ties keep row order.  A sum over a frame is the same correctly rounded double that
``groupBy().sum()`` gives for the same rows, on both engines.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .expressions import AnalysisException, ColRef, EvalContext, Expr, SortOrder, to_expr
from .table import ColumnData, Table
from .types import BooleanType, DoubleType, IntegerType, StringType, StructField, StructType, VectorUDT

__all__ = ["Window", "WindowSpec", "WindowFn", "WindowExpr", "contains_window", "extract_windows", "window_table"]

_RANKING = ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile")
_SHIFTS = ("lag", "lead")
_AGGS = ("count", "sum", "avg", "min", "max")
_UNSUPPORTED = ("first", "last", "first_value", "last_value", "nth_value")
_UNB_PRE, _UNB_FOL = -(1 << 63), (1 << 63) - 1


def _order(c) -> SortOrder:
    e = ColRef(c) if isinstance(c, str) else to_expr(c)
    return e if isinstance(e, SortOrder) else SortOrder(e, True)


def _bound(v: int):
    """A frame boundary: "pre" / "fol" for Spark's unbounded sentinels, else the offset."""
    v = int(v)
    if v <= _UNB_PRE:
        return "pre"
    if v >= _UNB_FOL:
        return "fol"
    return v


class WindowSpec:
    """``partitionBy`` / ``orderBy`` / ``rowsBetween`` / ``rangeBetween``, chainable; immutable."""

    def __init__(self, partition: Sequence[Expr] = (), orders: Sequence[SortOrder] = (), frame: Optional[Tuple] = None):
        self.partition = list(partition)
        self.orders = list(orders)
        self.frame = frame  # (kind "rows" | "range", lo, hi); lo / hi None: unbounded

    def partitionBy(self, *cols) -> "WindowSpec":
        cols = cols[0] if len(cols) == 1 and isinstance(cols[0], (list, tuple)) else cols
        return WindowSpec([ColRef(c) if isinstance(c, str) else to_expr(c) for c in cols], self.orders, self.frame)

    def orderBy(self, *cols) -> "WindowSpec":
        cols = cols[0] if len(cols) == 1 and isinstance(cols[0], (list, tuple)) else cols
        return WindowSpec(self.partition, [_order(c) for c in cols], self.frame)

    def _between(self, kind: str, start: int, end: int) -> "WindowSpec":
        lo, hi = _bound(start), _bound(end)
        if lo == "fol" or hi == "pre":
            raise AnalysisException(f"cannot resolve the window frame: a frame cannot start at UNBOUNDED FOLLOWING or end "
                                    f"at UNBOUNDED PRECEDING ({kind}Between({start}, {end}))")
        lo, hi = (None if lo == "pre" else lo), (None if hi == "fol" else hi)
        if lo is not None and hi is not None and lo > hi:
            raise AnalysisException(f"cannot resolve the window frame: the lower bound {lo} is above the upper bound {hi}")
        return WindowSpec(self.partition, self.orders, (kind, lo, hi))

    def rowsBetween(self, start: int, end: int) -> "WindowSpec":
        return self._between("rows", start, end)

    def rangeBetween(self, start: int, end: int) -> "WindowSpec":
        return self._between("range", start, end)


class Window:
    """``org.apache.spark.sql.expressions.Window``."""

    unboundedPreceding = _UNB_PRE
    unboundedFollowing = _UNB_FOL
    currentRow = 0

    @staticmethod
    def partitionBy(*cols) -> WindowSpec:
        return WindowSpec().partitionBy(*cols)

    @staticmethod
    def orderBy(*cols) -> WindowSpec:
        return WindowSpec().orderBy(*cols)

    @staticmethod
    def rowsBetween(start: int, end: int) -> WindowSpec:
        return WindowSpec().rowsBetween(start, end)

    @staticmethod
    def rangeBetween(start: int, end: int) -> WindowSpec:
        return WindowSpec().rangeBetween(start, end)


class WindowFn(Expr):
    """A ranking or offset function before ``.over``: ``row_number()``, ``lag(c, 1)`` ..."""

    def __init__(self, fn: str, child: Optional[Expr] = None, param: int = 0, default=None):
        self.fn = fn.lower()
        if self.fn in _UNSUPPORTED:
            raise AnalysisException(f"window function {self.fn} is not implemented (first / last / nth_value)")
        if self.fn not in _RANKING + _SHIFTS:
            raise AnalysisException(f"Undefined function: '{fn}'")
        self.child = child
        self.param = int(param)
        self.default = default

    def children(self):
        return [] if self.child is None else [self.child]

    def _outside(self):
        return AnalysisException(f"Window function {self.sql_name()} requires an OVER clause.")

    def data_type(self, schema):
        raise self._outside()

    def eval(self, ctx):
        raise self._outside()

    def sql_name(self):
        if self.fn in _SHIFTS:
            return f"{self.fn}({self.child.sql_name()}, {self.param}, {'NULL' if self.default is None else self.default})"
        return f"{self.fn}({self.param})" if self.fn == "ntile" else f"{self.fn}()"


class WindowExpr(Expr):
    """``fn(child) OVER (PARTITION BY partition ORDER BY orders frame)``.  Only ``plan.Window``
    evaluates it: ``extract_windows`` moves it out of a select list into that node."""

    def __init__(self, fn: str, child: Optional[Expr], partition: Sequence[Expr], orders: Sequence[SortOrder],
                 frame: Optional[Tuple] = None, param: int = 0, default=None):
        self.fn = {"mean": "avg"}.get(fn.lower(), fn.lower())
        self.child = child
        self.partition = list(partition)
        self.orders = list(orders)
        self.param = int(param)
        self.default = default
        if self.fn in _UNSUPPORTED:
            raise AnalysisException(f"window function {self.fn} is not implemented (first / last / nth_value)")
        if self.fn not in _RANKING + _SHIFTS + _AGGS:
            raise AnalysisException(f"Undefined function: '{fn}'")
        if self.fn in _RANKING + _SHIFTS:
            if not self.orders:
                raise AnalysisException(f"Window function {self.fn} requires window to be ordered, please add ORDER BY "
                                        f"clause. For example SELECT {self.fn}(value_expr) OVER (PARTITION BY "
                                        f"window_partition ORDER BY window_ordering) from table")
            frame = None  # a fixed frame of their own
        if self.fn == "ntile" and self.param < 1:
            raise AnalysisException(f"cannot resolve 'ntile({self.param})': Buckets expression must be positive, but got: "
                                    f"{self.param}")
        if self.fn in _SHIFTS and self.param < 0:
            raise AnalysisException(f"cannot resolve '{self.fn}': the offset must not be negative, but got: {self.param}")
        if frame is not None:
            kind, lo, hi = frame
            if kind == "range" and any(v not in (None, 0) for v in (lo, hi)):
                raise AnalysisException("rangeBetween with numeric offsets is not implemented: a RANGE frame is bounded by "
                                        "UNBOUNDED PRECEDING / CURRENT ROW / UNBOUNDED FOLLOWING")
            if self.fn in ("min", "max") and lo is not None and hi is not None:
                raise AnalysisException(f"{self.fn} over a frame bounded on both sides is not implemented: one end of the "
                                        f"frame must be UNBOUNDED")
            frame = (kind, lo, hi)
        self.frame = frame

    def children(self):
        return ([] if self.child is None else [self.child]) + self.partition + [o.child for o in self.orders]

    def engine_frame(self) -> Tuple:
        """``(is_range, lo, hi)`` of ``ops.window.window_finish``, Spark's default applied."""
        if self.frame is None:
            return (True, None, 0) if self.orders else (False, None, None)
        kind, lo, hi = self.frame
        return (kind == "range", lo, hi)

    def data_type(self, schema):
        for e in self.partition + [o.child for o in self.orders]:
            if isinstance(e.data_type(schema), VectorUDT):
                raise AnalysisException(f"cannot resolve '{self.sql_name()}': a vector column is not an orderable data type")
        if self.fn in ("row_number", "rank", "dense_rank", "ntile"):
            return IntegerType()
        if self.fn in ("percent_rank", "cume_dist"):
            return DoubleType()
        if self.fn in _SHIFTS:
            return self.child.data_type(schema)
        from .aggregates import AggExpr

        dt = AggExpr(self.fn, self.child).result_type(schema)
        if self.fn in ("min", "max") and isinstance(dt, StringType):  # (AggExpr already refuses; kept for the wording)
            raise AnalysisException(f"{self.sql_name()}: min / max of a string column is not implemented")
        return dt

    def nullable(self, schema):
        return self.fn not in ("count",) + _RANKING

    def sql_name(self):
        if self.fn in _SHIFTS:
            call = f"{self.fn}({self.child.sql_name()}, {self.param}, {'NULL' if self.default is None else self.default})"
        elif self.fn == "ntile":
            call = f"ntile({self.param})"
        elif self.fn in _RANKING:
            call = f"{self.fn}()"
        else:
            call = f"{self.fn}({'1' if self.child is None else self.child.sql_name()})"
        parts = []
        if self.partition:
            parts.append("PARTITION BY " + ", ".join(e.sql_name() for e in self.partition))
        if self.orders:
            parts.append("ORDER BY " + ", ".join(o.sql_name() for o in self.orders))
        if self.frame is not None:
            def b(v, pre):
                if v is None:
                    return "UNBOUNDED PRECEDING" if pre else "UNBOUNDED FOLLOWING"
                return "CURRENT ROW" if v == 0 else (f"{-v} PRECEDING" if v < 0 else f"{v} FOLLOWING")
            parts.append(f"{self.frame[0].upper()} BETWEEN {b(self.frame[1], True)} AND {b(self.frame[2], False)}")
        return f"{call} OVER ({' '.join(parts)})"

    def eval(self, ctx):
        raise AnalysisException(f"window function {self.sql_name()} is only allowed in a select list (select / withColumn / "
                                f"SELECT)")


def over(e: Expr, spec: WindowSpec) -> WindowExpr:
    """``Column.over``: an aggregate or a window function over ``spec``."""
    from .aggregates import AggExpr

    if not isinstance(spec, WindowSpec):
        raise TypeError("over() takes a WindowSpec")
    if isinstance(e, AggExpr):
        return WindowExpr(e.fn, e.child, spec.partition, spec.orders, spec.frame)
    if isinstance(e, WindowFn):
        return WindowExpr(e.fn, e.child, spec.partition, spec.orders, spec.frame, e.param, e.default)
    raise AnalysisException(f"Expression '{e.sql_name()}' not supported within a window function.")


def contains_window(e: Expr) -> bool:
    return isinstance(e, (WindowExpr, WindowFn)) or any(contains_window(c) for c in e.children())


def _rewrite(e: Expr, found: List[Tuple[WindowExpr, str]]) -> Expr:
    """``e`` with every ``WindowExpr`` replaced by a reference to a hidden column (a copy where
    something changed: parsed trees are shared between plans)."""
    import copy

    from .skey import expr_key

    if isinstance(e, WindowExpr):
        if any(contains_window(c) for c in e.children()):
            raise AnalysisException("It is not allowed to use a window function inside another window function.")
        k = expr_key(e)
        for w, name in found:
            if w is e or (k is not None and expr_key(w) == k):
                return ColRef(name)
        name = f"_window_{len(found)}: {e.sql_name()}"  # (the fused-chain cache keys a Project by its output names)
        found.append((e, name))
        return ColRef(name)
    if isinstance(e, WindowFn):
        raise e._outside()
    if not contains_window(e):
        return e
    c = copy.copy(e)
    c.__dict__.pop("_skey", None)
    for attr, v in list(c.__dict__.items()):
        if isinstance(v, Expr):
            setattr(c, attr, _rewrite(v, found))
        elif isinstance(v, list) and v and all(isinstance(x, Expr) for x in v):
            setattr(c, attr, [_rewrite(x, found) for x in v])
        elif isinstance(v, list) and v and all(isinstance(x, tuple) for x in v):
            setattr(c, attr, [tuple(_rewrite(x, found) if isinstance(x, Expr) else x for x in t) for t in v])
    return c


def extract_windows(exprs: Sequence[Expr]):
    """``(rewritten expressions, [(WindowExpr, hidden name)])``: the window expressions anywhere
    inside a select list, each replaced by a reference to the hidden column that a ``plan.Window``
    underneath the ``Project`` computes."""
    found: List[Tuple[WindowExpr, str]] = []
    out = []
    for e in exprs:
        r = _rewrite(e, found)
        if isinstance(e, WindowExpr):  # a bare window expression keeps its own name
            from .expressions import Alias

            r = Alias(r, e.sql_name())
        out.append(r)
    return out, found


def window_fields(child_schema: StructType, wexprs) -> List[StructField]:
    return [StructField(name, w.data_type(child_schema), w.nullable(child_schema)) for w, name in wexprs]


# ------------------------------------------------------------------------------------------
# execution
# ------------------------------------------------------------------------------------------
def _spec_key(w: WindowExpr):
    from .skey import expr_key

    def k(e):
        v = expr_key(e)
        return ("n", e.sql_name()) if v is None else ("k", v)
    return tuple(k(e) for e in w.partition), tuple(k(o) for o in w.orders)


def _value_column(c: ColumnData):
    """``(tensor or None, valid)`` of an aggregate's input: a string column gives only its validity."""
    if isinstance(c.values, list):
        return None, torch.tensor([v is not None for v in c.values], dtype=torch.bool)
    vals = c.values.to(torch.uint8) if isinstance(c.dtype, BooleanType) else c.values
    return vals, c.valid


def window_table(t: Table, wexprs, schema: Optional[StructType] = None, session=None) -> Table:
    """``t`` with one new column per ``(WindowExpr, name)`` appended; no row is moved and the
    selection vector is kept."""
    from ..ops import kernels
    from ..ops import window as wn
    from .aggregates import _key_column, _pending

    _pending(t)
    dev, n = t.device, t.nrows
    ctx = EvalContext(t, session)
    if schema is None:
        schema = StructType(list(t.schema.fields) + window_fields(t.schema, wexprs))
    new_fields = schema.fields[len(t.schema.fields):]
    groups: dict = {}
    for i, (w, _) in enumerate(wexprs):
        groups.setdefault(_spec_key(w), []).append(i)
    results: List[Optional[ColumnData]] = [None] * len(wexprs)
    for idxs in groups.values():
        first = wexprs[idxs[0]][0]
        # ---- the value slots of every expression of the specification, then their scales (the
        # one host read, before the sort)
        slots, slot_of, args = [], {}, {}

        def arg(e):
            k = e.sql_name()
            if k not in args:
                args[k] = e.eval(ctx)
            return k, args[k]

        def slot(op, e):
            if e is None:
                key = (wn.ROWS, None)
                if key not in slot_of:
                    slot_of[key] = len(slots)
                    slots.append((wn.ROWS, None, None, 0))
                return slot_of[key]
            k, c = arg(e)
            if (op, k) not in slot_of:
                vals, valid = _value_column(c)
                valid = None if valid is None else valid.to(dev)
                slot_of[(op, k)] = len(slots)
                slots.append((op, None if op == wn.COUNT else vals, valid, None))
            return slot_of[(op, k)]

        plans = {}
        for i in idxs:
            w = wexprs[i][0]
            if w.fn not in _AGGS:
                continue
            if w.child is None:
                plans[i] = (slot(wn.ROWS, None), None)
                continue
            _, c = arg(w.child)
            cnt = slot(wn.COUNT, w.child)
            if w.fn == "count":
                plans[i] = (cnt, None)
            elif w.fn == "sum" and not isinstance(c.values, list) and c.values.dtype in (torch.int32, torch.int64):
                plans[i] = (cnt, slot(wn.SUM_I, w.child))
            elif w.fn in ("sum", "avg"):
                plans[i] = (cnt, slot(wn.SUM_F, w.child))
            else:
                plans[i] = (cnt, None)
        need = [s for s, sl in enumerate(slots) if sl[0] == wn.SUM_F]
        es = kernels.group_scale([slots[s][1] for s in need], [slots[s][2] for s in need], t.sel)
        for s, e in zip(need, es):
            slots[s] = slots[s][:3] + (e,)
        # ---- one sort, one heads pass, one bounds pass
        keys = [_key_column(e.eval(ctx), dev, False) for e in first.partition]
        okeys = [_key_column(o.child.eval(ctx), dev, False) for o in first.orders]
        if keys or okeys:
            perm = kernels.sort_permutation([k[0] for k in keys + okeys], [k[1] for k in keys + okeys], t.sel,
                                            [True] * len(keys) + [o.ascending for o in first.orders],
                                            [True] * len(keys) + [o.nulls_first for o in first.orders])
        elif t.sel is not None:
            perm = kernels.selected_indices(t.sel)
        else:
            perm = torch.arange(n, dtype=torch.int64, device=dev)
        perm = perm.to(dev)
        heads = kernels.window_heads([k[0] for k in keys], [k[1] for k in keys], [k[0] for k in okeys], [k[1] for k in okeys],
                                     perm, n)
        bounds = kernels.window_bounds(heads)
        P, off = kernels.window_prefix(slots, perm, n) if slots else (None, [])
        # ---- one finish per frame
        by_frame: dict = {}
        for i in idxs:
            w = wexprs[i][0]
            by_frame.setdefault(w.engine_frame() if w.fn in _AGGS else (True, None, 0), []).append(i)
        scans = {}
        for frame, members in by_frame.items():
            outs, where = [], {}

            def word(key, make):
                if key not in where:
                    where[key] = len(outs)
                    outs.extend(make())
                return where[key]

            def diff(s):
                return word(("p", s), lambda: [(wn.O_DIFF, P[off[s] + k], 0) for k in range(wn.word_count(slots[s][0]))])

            todo = []
            for i in members:
                w = wexprs[i][0]
                if w.fn in _AGGS:
                    cnt, val = plans[i]
                    c_w = diff(cnt)
                    v_w = None
                    if val is not None:
                        v_w = diff(val)
                    elif w.fn in ("min", "max"):
                        k, c = arg(w.child)
                        back = frame[1] is not None  # the frame ends with its partition: scan from the end
                        sk = (k, w.fn == "max", back)
                        if sk not in scans:
                            vals, valid = _value_column(c)
                            scans[sk] = kernels.window_minmax(vals, None if valid is None else valid.to(dev), perm, heads,
                                                              w.fn == "max", back)
                        v_w = word(("m",) + sk, lambda: [(wn.O_PICK_LO if back else wn.O_PICK_HI, scans[sk], 0)])
                    todo.append((i, c_w, v_w))
                elif w.fn in _SHIFTS:
                    d = -w.param if w.fn == "lag" else w.param
                    todo.append((i, word(("s", d), lambda: [(wn.O_SHIFT, None, d)]), None))
                else:
                    kinds = {"row_number": (wn.O_ROW_NUMBER,), "rank": (wn.O_RANK,), "dense_rank": (wn.O_DENSE_RANK,),
                             "percent_rank": (wn.O_RANK, wn.O_PART_SIZE), "cume_dist": (wn.O_PEER_END, wn.O_PART_SIZE),
                             "ntile": (wn.O_ROW_NUMBER, wn.O_PART_SIZE)}[w.fn]
                    ws = [word(("r", k), lambda k=k: [(k, None, 0)]) for k in kinds]
                    todo.append((i, ws[0], ws[1] if len(ws) > 1 else None))
            raw = kernels.window_finish(bounds, perm, n, frame, outs)
            for i, a, b in todo:
                results[i] = _finalize(wexprs[i][0], new_fields[i], raw, a, b, slots, plans.get(i), arg, t, dev)
    return Table(schema, list(t.columns) + results, n, t.sel, dev)


def _finalize(w: WindowExpr, field: StructField, raw, a, b, slots, plan, arg, t: Table, dev) -> ColumnData:
    """The column of one expression from the raw words of ``window_finish`` (shared by both engines)."""
    from ..ops import window as wn

    td = field.dataType.torch_dtype
    if w.fn in _AGGS:
        cnt = raw[:, a]
        if w.fn == "count":
            return ColumnData(field.dataType, cnt.clone(), None)
        valid = cnt > 0
        if plan[1] is not None:
            op, _, _, e = slots[plan[1]]
            if op == wn.SUM_I:
                v = raw[:, b].clone()
            else:
                v = wn.sum_from_words(raw[:, b:b + wn.SUM_WORDS], e)
                if w.fn == "avg":
                    v = v / cnt.to(torch.float64)
        else:
            _, c = arg(w.child)
            src = c.values.to(torch.uint8) if isinstance(c.dtype, BooleanType) else c.values
            v = wn.minmax_from_keys(raw[:, b], src.dtype)
        if v.dtype != td:
            v = v.to(td)
        v = torch.where(valid, v, torch.zeros_like(v))
        return ColumnData(field.dataType, v, valid)
    if w.fn in _SHIFTS:
        src = raw[:, a]
        _, c = arg(w.child)
        inside = src >= 0
        g = c.index(torch.clamp(src, min=0))
        valid = inside & g.valid_mask(dev).to(dev)
        if isinstance(g.values, list):
            ok = inside.cpu().tolist()
            vals = [x if o else w.default for x, o in zip(g.values, ok)]
            valid = torch.tensor([x is not None for x in vals], dtype=torch.bool, device=dev)
            if t.sel is not None:
                valid = valid & t.sel
            return ColumnData(field.dataType, vals, valid)
        vals = g.values
        if w.default is not None:
            vals = torch.where(inside, vals, torch.full_like(vals, w.default))
            valid = valid | ~inside
        if t.sel is not None:
            valid = valid & t.sel
        return ColumnData(field.dataType, torch.where(valid, vals, torch.zeros_like(vals)), valid, dict(g.meta))
    x = raw[:, a]
    if w.fn == "percent_rank":
        v = wn.percent_rank(x, raw[:, b])
    elif w.fn == "cume_dist":
        v = wn.cume_dist(x, raw[:, b])
    elif w.fn == "ntile":
        v = wn.ntile(x, torch.clamp(raw[:, b], min=1), w.param)
    else:
        v = x
    return ColumnData(field.dataType, v.to(td), None)

