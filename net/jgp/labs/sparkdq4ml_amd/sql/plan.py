"""Lazy logical plans and their executor.

Spark builds a lazy lineage and re-executes it from the CSV on every action (the
lab re-scans ``dataset-abstract.csv`` ~10 times).  Here every node memoizes its materialized
:class:`Table` (plans are immutable and all supported expressions are deterministic, so this is
observationally identical) and the executor fuses Project/Filter chains into one device
kernel launch where the expressions allow it (``ops.dqvm``).
"""
from __future__ import annotations

import threading
from typing import List, Optional, Sequence, Tuple

import torch

from .expressions import (Alias, AnalysisException, ColRef, EvalContext, Expr, SortOrder, UdfCall)
from .skey import expr_key, exprs_key, intern
from .table import ColumnData, Table
from .types import BooleanType, StructField, StructType, VectorUDT

__all__ = ["LogicalPlan", "LocalRelation", "CsvScanRelation", "Project", "Filter", "Limit", "Union", "Join", "Aggregate", "Deduplicate",
           "Sort", "build_sort", "Window", "build_project", "execute", "prune_columns"]


class LogicalPlan:
    _memo: Optional[Table] = None
    _skey = 0  # structural key (sql/skey.py): 0 = not computed yet, None = unkeyable

    def children(self) -> List["LogicalPlan"]:
        return []

    def skey(self) -> Optional[int]:
        """Interned structural key: equal for two nodes that denote the same computation over the
        same input (an action's rebuilt chain), None when the node cannot be keyed."""
        return None

    def fresh(self, child: Optional["LogicalPlan"] = None) -> "LogicalPlan":
        """A copy of this (analyzed) node with no execution result, over ``child``: the DataFrame
        layer's structural sharing hands every action its own nodes."""
        n = object.__new__(type(self))
        d = n.__dict__
        d.update(self.__dict__)
        d.pop("_memo", None)
        if child is not None:
            d["child"] = child
        return n

    def schema(self) -> StructType:
        raise NotImplementedError

    def _compute(self, session) -> Table:
        raise NotImplementedError

    def describe(self, indent=0) -> str:
        s = "  " * indent + self._label() + "\n"
        for c in self.children():
            s += c.describe(indent + 1)
        return s

    def _label(self):
        return type(self).__name__


class LocalRelation(LogicalPlan):
    """A materialized relation.  ``sharded``: this process holds one data-parallel shard of it
    (rank order = global row order); defaults to True whenever a multi-process group is up, which
    is the SPMD contract of the engine: every source (reader byte range, ``createDataFrame``,
    ``range``) contributes this rank's rows."""

    def __init__(self, table: Table, label: str = "LocalRelation", sharded: Optional[bool] = None):
        from ..parallel import comm

        self.table = table
        self._memo = table
        self.label = label
        self.sharded = comm.world_size() > 1 if sharded is None else bool(sharded)

    def schema(self):
        return self.table.schema

    def skey(self):
        # one key per relation object (a serial, not the table's id: nothing is pinned); chains
        # rebuilt over the same relation share their analysis
        k = self.__dict__.get("_skey")
        if k is None:
            k = self._skey = intern(("local", next(_SERIAL)))
        return k

    def _compute(self, session):
        return self.table

    def _label(self):
        return f"{self.label} [{', '.join(self.table.schema.names)}]"


class CsvScanRelation(LocalRelation):
    """A device CSV relation scanned lazily, at its first action (Spark also reads the file at
    every action).  Created only when an earlier device scan of the same cached
    bytes already fixed its schema, null columns and line count (``fused``: those facts plus the
    HBM-resident bytes): a Project/Filter chain directly on top then runs fused INTO the scan
    (``ops/scanfuse.py``); any other consumer gets the plain device scan (``scan()``)."""

    def __init__(self, schema: StructType, scan, fused: Optional[dict], label: str = "CsvScan",
                 sharded: Optional[bool] = None):
        from ..parallel import comm

        self._schema = schema
        self._scan = scan
        self.fused = fused
        self.label = label
        self.sharded = comm.world_size() > 1 if sharded is None else bool(sharded)
        self._memo = None

    @property
    def table(self) -> Table:
        if self._memo is None:
            self._memo = self._scan()
        return self._memo

    def schema(self):
        return self._schema

    def _compute(self, session):
        return self._scan()

    def skey(self):
        return self.__dict__.get("_skey")  # set by the reader from the cached input's identity

    def fresh(self, child=None):
        n = super().fresh()
        n._memo = None
        return n

    def _label(self):
        return f"{self.label} [{', '.join(self._schema.names)}]"


_SCHEMAS: dict = {}   # Project skey -> analyzed schema
_SERIAL = __import__("itertools").count(1)
_CHECKED: set = set()  # Filter skeys whose condition type-checked


def is_sharded(plan) -> bool:
    """True when any leaf relation of ``plan`` is a data-parallel shard (actions then combine
    ranks: counts all-reduce, rows gather in rank order)."""
    if isinstance(plan, LocalRelation):
        return plan.sharded
    if isinstance(plan, Aggregate):
        return False  # every rank holds the whole (small) result
    return any(is_sharded(c) for c in plan.children())


def output_name(e: Expr) -> str:
    if isinstance(e, Alias):
        return e.name
    if isinstance(e, ColRef):
        return e.name
    return e.sql_name()


class Project(LogicalPlan):
    def __init__(self, child: LogicalPlan, exprs: Sequence[Expr]):
        self.child = child
        self.exprs = list(exprs)
        self._schema = None

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            ek = exprs_key(self.exprs) if ck is not None else None
            k = self._skey = intern(("Project", ck, ek)) if ek is not None else None
        return k

    def schema(self):
        if self._schema is None:
            k = self.skey()
            s = _SCHEMAS.get(k) if k is not None else None
            if s is not None:
                self._schema = s
                return s
            cs = self.child.schema()
            fields = []
            for e in self.exprs:
                dt = e.data_type(cs)
                meta = {}
                base = e.child if isinstance(e, Alias) else e
                if isinstance(base, ColRef):
                    meta = dict(cs[base._resolve(cs)].metadata)
                elif hasattr(base, "metadata"):
                    meta = base.metadata(cs)
                fields.append(StructField(output_name(e), dt, e.nullable(cs), meta))
            self._schema = StructType(fields)
            if k is not None:
                if len(_SCHEMAS) >= 4096:
                    _SCHEMAS.clear()
                _SCHEMAS[k] = self._schema
        return self._schema

    def _compute(self, session):
        base = execute(self.child, session)
        ctx = EvalContext(base, session)
        cols = []
        schema = self.schema()
        for e, f in zip(self.exprs, schema.fields):
            c = e.eval(ctx)
            if c.dtype != f.dataType:
                from .expressions import cast_column

                c = cast_column(c, f.dataType, base.device)
            if f.metadata and not c.meta:
                c = ColumnData(c.dtype, c.values, c.valid, dict(f.metadata))
            cols.append(c)
        return base.with_columns(schema, cols)

    def _label(self):
        return "Project [" + ", ".join(output_name(e) for e in self.exprs) + "]"


class Filter(LogicalPlan):
    def __init__(self, child: LogicalPlan, cond: Expr):
        self.child = child
        self.cond = cond
        k = self.skey()
        if k is not None and k in _CHECKED:
            return
        from .window import contains_window

        if contains_window(cond):
            raise AnalysisException("It is not allowed to use window functions inside WHERE and HAVING clauses: select the "
                                    "window expression under an alias and filter on the alias")
        dt = cond.data_type(child.schema())
        if not isinstance(dt, BooleanType):
            raise AnalysisException(f"filter expression '{cond.sql_name()}' of type {dt.simpleString()} "
                                    f"is not a boolean.")
        if k is not None:
            if len(_CHECKED) >= 4096:
                _CHECKED.clear()
            _CHECKED.add(k)

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            ek = expr_key(self.cond) if ck is not None else None
            k = self._skey = intern(("Filter", ck, ek)) if ek is not None else None
        return k

    def schema(self):
        return self.child.schema()

    def _compute(self, session):
        base = execute(self.child, session)
        c = self.cond.eval(EvalContext(base, session))
        keep = c.values.to(torch.bool)
        if c.valid is not None:
            keep = keep & c.valid
        sel = keep if base.sel is None else (base.sel & keep)
        t = Table(base.schema, base.columns, base.nrows, sel, base.device)
        return _maybe_compact(t)

    def _label(self):
        return f"Filter {self.cond.sql_name()}"


def _maybe_compact(t: Table, threshold: float = 0.25) -> Table:
    """Keep the selection vector unless the live fraction got small (then compact).  Device
    tables keep it unconditionally: every device consumer (DQ VM, pack, Gram, metrics) reads the
    selection natively, and deciding would cost a host sync per filter."""
    if t.sel is None or t.nrows < 4096 or t.sel.is_cuda:
        return t
    live = int(t.sel.sum().item())
    return t.compact() if live < threshold * t.nrows else t


class Limit(LogicalPlan):
    def __init__(self, child: LogicalPlan, n: int):
        self.child, self.n = child, int(n)

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            k = self._skey = intern(("Limit", ck, self.n)) if ck is not None else None
        return k

    def schema(self):
        return self.child.schema()

    def _compute(self, session):
        t = execute(self.child, session)
        if not is_sharded(self.child):
            return t.head_rows(self.n)
        # global LIMIT over shards: keep what is left of n after the ranks before this one
        from ..parallel import comm

        counts = comm.all_gather_object(int(t.count()))
        before = sum(counts[:comm.rank()])
        return t.head_rows(max(0, min(self.n - before, counts[comm.rank()])))

    def _label(self):
        return f"Limit {self.n}"


class Union(LogicalPlan):
    def __init__(self, left: LogicalPlan, right: LogicalPlan):
        if len(left.schema()) != len(right.schema()):
            raise AnalysisException("Union can only be performed on tables with the same number of columns")
        self.left, self.right = left, right

    def children(self):
        return [self.left, self.right]

    def schema(self):
        return self.left.schema()

    def _compute(self, session):
        a, b = execute(self.left, session).compact(), execute(self.right, session).compact()
        cols = []
        for ca, cb in zip(a.columns, b.columns):
            if isinstance(ca.values, list):
                vals = ca.values + cb.values
            else:
                dim = 1 if ca.values.dim() == 2 else 0
                vals = torch.cat([ca.values, cb.values.to(ca.values.dtype)], dim=dim)
            if ca.valid is None and cb.valid is None:
                valid = None
            else:
                valid = torch.cat([ca.valid_mask(a.device), cb.valid_mask(b.device)])
            cols.append(ColumnData(ca.dtype, vals, valid, dict(ca.meta)))
        return Table(a.schema, cols, a.nrows + b.nrows, None, a.device)


class Join(LogicalPlan):
    """Equi-join of ``left`` and ``right`` on ``keys`` = ``(left column, right column)`` pairs;
    ``how`` one of inner / left_outer / right_outer / full_outer / left_semi / left_anti
    (``sql/joins.py``).  ``using``: the key columns come out once (Spark's USING join), else both
    sides keep all their columns.  The right child is the build side of the hash join: the smaller
    table belongs there.  The result rows come in a defined order: left rows in row order, the
    matches of one left row in right row order (``right_outer``: right-major).  On a data-parallel
    plan a sharded left joins a right that every rank holds whole (an ``Aggregate`` result, a
    replicated relation) for inner / left_outer / left_semi / left_anti, and the result is sharded
    like the left; anything else would need a shuffle across ranks and raises."""

    def __init__(self, left: LogicalPlan, right: LogicalPlan, keys: Sequence[Tuple[str, str]], how: str = "inner",
                 using: bool = True):
        from .joins import join_schema

        self.left, self.right = left, right
        self.keys = [(str(l), str(r)) for l, r in keys]
        self.how, self.using = how, bool(using)
        self._schema = join_schema(left.schema(), right.schema(), self.keys, how, self.using)
        ls, rs = is_sharded(left), is_sharded(right)
        if rs or (ls and how not in ("inner", "left_outer", "left_semi", "left_anti")):
            raise AnalysisException(f"a {how} join of a {'sharded' if ls else 'replicated'} left with a "
                                    f"{'sharded' if rs else 'replicated'} right over data-parallel ranks: a shuffle join across "
                                    f"ranks is not implemented (a sharded left joins a right that every rank holds whole, for "
                                    f"inner / left / semi / anti)")

    def children(self):
        return [self.left, self.right]

    def skey(self):
        k = self._skey
        if k == 0:
            lk, rk = self.left.skey(), self.right.skey()
            k = self._skey = (intern(("Join", lk, rk, tuple(self.keys), self.how, self.using))
                              if lk is not None and rk is not None else None)
        return k

    def schema(self):
        return self._schema

    def _compute(self, session):
        from .joins import join_table

        return join_table(execute(self.left, session), execute(self.right, session), self.keys, self.how, self.using,
                          self._schema)

    def _label(self):
        return f"Join {self.how} [{', '.join(l if l == r else f'{l} = {r}' for l, r in self.keys)}]"


class Aggregate(LogicalPlan):
    """``GROUP BY keys`` with the aggregates ``aggs`` = ``(fn, input column or None, output name)``
    (``fn`` one of count / sum / avg / min / max; input None: ``count(*)``).  Keys and inputs are
    column references of the child (``aggregates.build_aggregate`` puts a Project underneath for
    anything else).  No key: one global row, even over an empty input.  No aggregate: the distinct
    keys.  The result is a small table on the session's device, one row per group in key order
    (null first); on a data-parallel plan every rank holds all of it."""

    def __init__(self, child: LogicalPlan, keys: Sequence[str], aggs: Sequence[Tuple]):
        self.child = child
        self.keys = list(keys)
        self.aggs = [tuple(a) for a in aggs]
        self._schema = None

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            k = self._skey = intern(("Aggregate", ck, tuple(self.keys), tuple(self.aggs))) if ck is not None else None
        return k

    def schema(self):
        if self._schema is None:
            from .aggregates import AggExpr

            cs = self.child.schema()
            fields = []
            for k in self.keys:
                f = ColRef(k)._field(cs)
                fields.append(StructField(f.name, f.dataType, f.nullable, dict(f.metadata)))
            for fn, inp, name in self.aggs:
                a = AggExpr(fn, None if inp is None else ColRef(inp))
                fields.append(StructField(name, a.result_type(cs), fn != "count"))
            self._schema = StructType(fields)
        return self._schema

    def references(self) -> set:
        return set(self.keys) | {inp for _, inp, _ in self.aggs if inp is not None}

    def _compute(self, session):
        from .aggregates import aggregate_table

        return aggregate_table(execute(self.child, session), self.keys, self.aggs, self.schema(), is_sharded(self.child))

    def _label(self):
        aggs = ", ".join(name for _, _, name in self.aggs)
        return f"Aggregate [{', '.join(self.keys)}] [{aggs}]"


class Deduplicate(LogicalPlan):
    """``dropDuplicates(subset)``: the child's table with its selection narrowed to the first live
    row of every group of the ``subset`` columns (row order; across shards, rank order)."""

    def __init__(self, child: LogicalPlan, subset: Sequence[str]):
        self.child = child
        cs = child.schema()
        self.subset = [ColRef(c)._field(cs).name for c in subset]

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            k = self._skey = intern(("Deduplicate", ck, tuple(self.subset))) if ck is not None else None
        return k

    def schema(self):
        return self.child.schema()

    def _compute(self, session):
        from .aggregates import dedupe_table

        return dedupe_table(execute(self.child, session), self.subset, is_sharded(self.child))

    def _label(self):
        return f"Deduplicate [{', '.join(self.subset)}]"


class Sort(LogicalPlan):
    """``ORDER BY orders``: the child's live rows in the stable sorted order of ``orders``
    (``SortOrder`` over column references of the child; ``build_sort`` puts a Project underneath
    for anything else), the first order the most significant.  Doubles order as Spark orders them
    (``-0.0 = 0.0``, every NaN one value above ``+inf``), strings by their dictionary codes.  The
    result is compact: every column gathered by the permutation, no selection vector.  On a
    data-parallel plan the node sorts this rank's rows."""

    def __init__(self, child: LogicalPlan, orders: Sequence[SortOrder]):
        self.child = child
        cs = child.schema()
        self.orders = []
        for o in orders:
            if not isinstance(o, SortOrder) or not isinstance(o.child, ColRef):
                raise AnalysisException(f"Sort takes orders over column references, got {o.sql_name()}")
            f = o.child._field(cs)
            _orderable(o, f.dataType)
            self.orders.append(SortOrder(ColRef(f.name), o.ascending, o.nulls_first))

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            ek = exprs_key(self.orders) if ck is not None else None
            k = self._skey = intern(("Sort", ck, ek)) if ek is not None else None
        return k

    def schema(self):
        return self.child.schema()

    def references(self) -> set:
        return {o.child.name for o in self.orders}

    def _compute(self, session):
        from .aggregates import sort_table

        return sort_table(execute(self.child, session), [(o.child.name, o.ascending, o.nulls_first) for o in self.orders])

    def _label(self):
        return "Sort [" + ", ".join(o.sql_name() for o in self.orders) + "]"


class Window(LogicalPlan):
    """The child's table with one column per window expression appended: ``wexprs`` =
    ``(WindowExpr, output name)`` (``sql/window.py``).  No row is moved and the selection vector is
    kept.  ``build_project`` puts this node under a ``Project`` whose expressions contain window
    expressions and replaces each by a reference to its (hidden) column."""

    def __init__(self, child: LogicalPlan, wexprs: Sequence[Tuple]):
        if is_sharded(child):
            raise AnalysisException("a window function over a data-parallel (sharded) input: the rows of a partition may "
                                    "lie on several ranks, and a shuffle across ranks is not implemented")
        self.child = child
        self.wexprs = [(w, str(name)) for w, name in wexprs]
        self._schema = None

    def children(self):
        return [self.child]

    def skey(self):
        k = self._skey
        if k == 0:
            ck = self.child.skey()
            ek = exprs_key([w for w, _ in self.wexprs]) if ck is not None else None
            k = self._skey = intern(("Window", ck, ek, tuple(n for _, n in self.wexprs))) if ek is not None else None
        return k

    def schema(self):
        if self._schema is None:
            from .window import window_fields

            cs = self.child.schema()
            self._schema = StructType(list(cs.fields) + window_fields(cs, self.wexprs))
        return self._schema

    def references(self) -> set:
        out = set()
        for w, _ in self.wexprs:
            out |= w.references()
        return out

    def _compute(self, session):
        from .window import window_table

        return window_table(execute(self.child, session), self.wexprs, self.schema(), session)

    def _label(self):
        return "Window [" + ", ".join(w.sql_name() for w, _ in self.wexprs) + "]"


def build_project(child: LogicalPlan, exprs: Sequence[Expr]) -> LogicalPlan:
    """``Project`` over ``child``.  A window expression anywhere inside ``exprs`` is computed by a
    ``Window`` node underneath, under a hidden name, and replaced by a reference."""
    from .window import contains_window, extract_windows

    if not any(contains_window(e) for e in exprs):
        return Project(child, exprs)
    cs = child.schema()
    for e in exprs:
        e.data_type(cs)
    out, found = extract_windows(exprs)
    return Project(Window(child, found), out)


def _orderable(o: SortOrder, dt) -> None:
    if isinstance(dt, VectorUDT):
        raise AnalysisException(f"cannot resolve '{o.sql_name()}' due to data type mismatch: cannot sort data type "
                                f"{dt.simpleString()}: it is not an orderable data type")


def build_sort(child: LogicalPlan, orders: Sequence[SortOrder], global_sort: bool = True) -> LogicalPlan:
    """``Sort`` over ``child``.  An order that is not a plain column reference is computed by a
    ``Project`` underneath, under a hidden name, and dropped again above the ``Sort``.
    ``global_sort``: the total order of ``orderBy`` / ``ORDER BY``, which a data-parallel (sharded)
    input does not have yet; ``sortWithinPartitions`` sorts every rank's rows."""
    from .aggregates import contains_aggregate

    if global_sort and is_sharded(child):
        raise AnalysisException("orderBy / ORDER BY over a data-parallel (sharded) input: a global sort across ranks is "
                                "not implemented; sortWithinPartitions sorts the rows of every rank")
    cs = child.schema()
    names = cs.names
    hidden, out = [], []
    for i, o in enumerate(orders):
        if contains_aggregate(o.child):
            raise AnalysisException(f"aggregate functions are not allowed in a sort order, but found {o.child.sql_name()}")
        _orderable(o, o.child.data_type(cs))
        if isinstance(o.child, ColRef):
            out.append(o)
        else:
            name = f"_sort_key_{i}: {o.child.sql_name()}"  # (the fused-chain cache keys a Project by its output names)
            hidden.append(Alias(o.child, name))
            out.append(SortOrder(ColRef(name), o.ascending, o.nulls_first))
    if not hidden:
        return Sort(child, out)
    return Project(Sort(Project(child, [ColRef(n) for n in names] + hidden), out), [ColRef(n) for n in names])


def prune_columns(plan: LogicalPlan, required) -> LogicalPlan:
    """Catalyst-style ColumnPruning: a plan whose Projects compute only the output columns some
    consumer needs (``required``: column names, case-insensitive; None = all).  Filters keep
    what their condition references, Sorts what their orders reference, Windows what their kept
    expressions reference (a window column nobody reads is dropped); leaves, Limit, Union and Join are
    not pruned through.  Unchanged
    subtrees are returned as-is, so their memoized tables are reused.

    Spark's ``LinearRegression.train`` selects (label, features, weight) before aggregating and the
    optimizer prunes every other derived column out of the whole-stage code — e.g. a DQ rule
    output only used by a filter is evaluated in registers, never materialized."""
    if required is None:
        return plan
    req = {r.lower() for r in required}
    if isinstance(plan, Project):
        keep = [e for e in plan.exprs if output_name(e).lower() in req]
        child_req = set()
        for e in keep:
            child_req |= e.references()
        child = prune_columns(plan.child, child_req)
        if len(keep) == len(plan.exprs) and child is plan.child:
            return plan
        return Project(child, keep)
    if isinstance(plan, Filter):
        child = prune_columns(plan.child, req | {r.lower() for r in plan.cond.references()})
        f = plan if child is plan.child else Filter(child, plan.cond)
        names = f.schema().names
        if any(n.lower() not in req for n in names):
            # columns only the condition needs: drop them right above the filter, so a fused
            # Project/Filter chain evaluates them in registers and never stores them
            return Project(f, [ColRef(n) for n in names if n.lower() in req])
        return f
    if isinstance(plan, Sort):
        child = prune_columns(plan.child, req | {r.lower() for r in plan.references()})
        srt = plan if child is plan.child else Sort(child, plan.orders)
        names = srt.schema().names
        if any(n.lower() not in req for n in names):  # columns only the orders need
            return Project(srt, [ColRef(n) for n in names if n.lower() in req])
        return srt
    if isinstance(plan, Window):
        keep = [(w, n) for w, n in plan.wexprs if n.lower() in req]
        child_req = req - {n.lower() for _, n in plan.wexprs}
        for w, _ in keep:
            child_req |= {r.lower() for r in w.references()}
        child = prune_columns(plan.child, child_req)
        if not keep:
            return child
        if len(keep) == len(plan.wexprs) and child is plan.child:
            return plan
        return Window(child, keep)
    if isinstance(plan, Aggregate):
        # exactly the key and input references pass through, whatever the consumer asks for
        child = prune_columns(plan.child, plan.references())
        return plan if child is plan.child else Aggregate(child, plan.keys, plan.aggs)
    return plan


_exec_lock = threading.RLock()


def execute(plan: LogicalPlan, session=None) -> Table:
    if plan._memo is not None:
        return plan._memo
    with _exec_lock:
        if plan._memo is None:
            from ..ops import dqvm

            fused = dqvm.try_execute_fused(plan, session)
            plan._memo = fused if fused is not None else plan._compute(session)
    return plan._memo


_ = (Tuple, UdfCall)
