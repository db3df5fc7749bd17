"""Recursive-descent parser for the Spark SQL subset the lab uses:

    SELECT cast(guest as int) guest, price_no_min AS price FROM price WHERE price_no_min > 0
    SELECT guest, price_correct_correl AS price FROM price WHERE price_correct_correl > 0

(``DataQuality4MachineLearningApp.java:77-78,89-90``) — projections with ``CAST``, aliases with or
without ``AS``, single-table ``FROM`` of a temp view, ``WHERE`` with arithmetic / comparisons /
boolean logic / ``IS [NOT] NULL`` / ``BETWEEN`` / ``IN``, ``CASE WHEN``, ``GROUP BY``,
``ORDER BY expr [ASC|DESC] [NULLS FIRST|NULLS LAST]``, ``LIMIT``,
``FROM a [INNER | LEFT [OUTER] | RIGHT [OUTER] | FULL [OUTER] | LEFT SEMI | LEFT ANTI] JOIN b USING (c1, ...)``
(chainable, left-associative), UDF and built-in function calls.  It produces the same plan nodes as the DataFrame API.
"""
from __future__ import annotations

import re
from typing import List, Optional, Tuple

from .expressions import (Alias, AnalysisException, BinOp, CaseWhen, Cast, ColRef, Coalesce,
                          Expr, If, IsNotNull, IsNull, Lit, Neg, Not, SortOrder, UdfCall)
from .aggregates import AggExpr, build_aggregate, contains_aggregate
from .fn import MathFn, BUILTIN_MATH
from .plan import Aggregate, Filter, Join, Limit, Project, build_project, build_sort, output_name
from .skey import expr_key

__all__ = ["parse_expression", "parse_select_item", "plan_sql", "ParseException"]


class ParseException(AnalysisException):
    pass


_TOKEN = re.compile(r"""
    (?P<ws>\s+)
  | (?P<num>(?:\d+\.\d*|\.\d+|\d+)(?:[eE][+-]?\d+)?[dDlL]?)
  | (?P<str>'(?:[^'\\]|\\.|'')*')
  | (?P<bq>`[^`]+`)
  | (?P<ident>[A-Za-z_][A-Za-z_0-9]*)
  | (?P<op><=>|<=|>=|<>|!=|==|\|\||[=<>+\-*/%(),.])
""", re.VERBOSE)

_KEYWORDS = {"select", "from", "where", "as", "and", "or", "not", "cast", "is", "null", "true", "false",
             "case", "when", "then", "else", "end", "limit", "between", "in", "distinct", "like", "group", "by", "order"}


_WINDOW_FNS = {"row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead", "first", "last",
               "first_value", "last_value", "nth_value"}
_JOIN_WORDS = {"inner", "left", "right", "full", "outer", "semi", "anti", "cross", "join", "on", "using"}
_JOIN_TYPES = {(): "inner", ("inner",): "inner", ("left",): "left_outer", ("left", "outer"): "left_outer",
               ("right",): "right_outer", ("right", "outer"): "right_outer", ("full",): "full_outer",
               ("full", "outer"): "full_outer", ("left", "semi"): "left_semi", ("left", "anti"): "left_anti"}


def _tokenize(text: str) -> List[Tuple[str, str]]:
    out, pos = [], 0
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            raise ParseException(f"\nmismatched input '{text[pos]}' expecting <EOF>(line 1, pos {pos})")
        pos = m.end()
        kind = m.lastgroup
        val = m.group(kind)
        if kind == "ws":
            continue
        if kind == "ident" and val.lower() in _KEYWORDS:
            out.append(("kw", val.lower()))
        elif kind == "bq":
            out.append(("ident", val[1:-1]))
        else:
            out.append((kind, val))
    out.append(("eof", ""))
    return out


class _Parser:
    def __init__(self, text):
        self.toks = _tokenize(text)
        self.i = 0
        self.text = text

    def peek(self, k=0):
        return self.toks[self.i + k]

    def next(self):
        t = self.toks[self.i]
        self.i += 1
        return t

    def accept(self, kind, val=None):
        t = self.peek()
        if t[0] == kind and (val is None or t[1].lower() == val):
            self.i += 1
            return t
        return None

    def expect(self, kind, val=None):
        t = self.accept(kind, val)
        if t is None:
            got = self.peek()
            raise ParseException(f"\nmismatched input '{got[1] or '<EOF>'}' expecting {val or kind}")
        return t

    # ---- query -------------------------------------------------------------------------------
    def query(self, session):
        return _bind_query(self.query_syntax(), self.text, session)

    def query_syntax(self):
        """The statement's syntax: (select items, view name, WHERE, LIMIT, DISTINCT, GROUP BY,
        ORDER BY) -- nothing of the catalog is read here, so the result is cached per text
        (``plan_sql``)."""
        self.expect("kw", "select")
        distinct = bool(self.accept("kw", "distinct"))
        items = self.select_list()
        self.expect("kw", "from")
        tname, alias = self.relation()
        joins = []
        while True:
            how = self.join_type()
            if how is None:
                break
            jname, jalias = self.relation()
            if self.accept("ident", "on"):
                raise AnalysisException("JOIN ... ON is not implemented; use USING (c1, ...) with the key columns' names")
            if not self.accept("ident", "using"):
                raise AnalysisException("cross joins are not implemented: a JOIN takes USING (c1, ...)")
            self.expect("op", "(")
            cols = [self.expect("ident")[1]]
            while self.accept("op", ","):
                cols.append(self.expect("ident")[1])
            self.expect("op", ")")
            joins.append((how, jname, jalias, cols))
        where = None
        if self.accept("kw", "where"):
            where = self.expr()
        group = None
        if self.accept("kw", "group"):
            self.expect("kw", "by")
            group = [self.expr()]
            while self.accept("op", ","):
                group.append(self.expr())
        order = None
        if self.accept("kw", "order"):
            self.expect("kw", "by")
            order = [self.order_item()]
            while self.accept("op", ","):
                order.append(self.order_item())
        limit = None
        if self.accept("kw", "limit"):
            limit = int(self.expect("num")[1])
        self.expect("eof")
        quals = {tname.lower()} | ({alias.lower()} if alias else set())
        for _, jname, jalias, _ in joins:  # every name of the joined schema is unambiguous (a duplicate raises)
            quals |= {jname.lower()} | ({jalias.lower()} if jalias else set())
        items = [(_strip_qual(e, quals)) for e in items]
        if where is not None:
            where = _strip_qual(where, quals)
        if group is not None:
            group = [_strip_qual(e, quals) for e in group]
        if order is not None:
            order = [(_strip_qual(e, quals), asc, nf) for e, asc, nf in order]
        return items, tname, where, limit, distinct, group, order, joins

    def relation(self):
        """``view [[AS] alias]`` (a join word is never an alias)."""
        name = self.expect("ident")[1]
        alias = None
        if self.accept("kw", "as"):
            alias = self.expect("ident")[1]
        elif self.peek()[0] == "ident" and self.peek()[1].lower() not in _JOIN_WORDS:
            alias = self.next()[1]
        return name, alias

    def join_type(self):
        """``[INNER | LEFT [OUTER] | RIGHT [OUTER] | FULL [OUTER] | LEFT SEMI | LEFT ANTI | CROSS]
        JOIN`` -> the canonical join type, or None when no JOIN follows."""
        t = self.peek()
        if t[0] != "ident" or t[1].lower() not in _JOIN_WORDS or t[1].lower() in ("on", "using"):
            return None
        words = []
        while self.peek()[0] == "ident" and self.peek()[1].lower() in _JOIN_WORDS and self.peek()[1].lower() != "join":
            words.append(self.next()[1].lower())
        self.expect("ident", "join")
        how = _JOIN_TYPES.get(tuple(words))
        if how is None:
            if words == ["cross"]:
                raise AnalysisException("cross joins are not implemented")
            raise ParseException(f"\nmismatched input '{' '.join(words)} join': not a join type")
        return how

    def over(self, e: Expr) -> Expr:
        """``fn(...) [OVER ([PARTITION BY e, ...] [ORDER BY e [ASC|DESC] [NULLS FIRST|LAST], ...]
        [ROWS | RANGE BETWEEN bound AND bound])]``."""
        if not self.accept("ident", "over"):
            return e
        from .window import WindowSpec, over

        self.expect("op", "(")
        partition, orders, frame = [], [], None
        if self.accept("ident", "partition"):
            self.expect("kw", "by")
            partition = [self.expr()]
            while self.accept("op", ","):
                partition.append(self.expr())
        if self.accept("kw", "order"):
            self.expect("kw", "by")
            orders = [SortOrder(*self.order_item())]
            while self.accept("op", ","):
                orders.append(SortOrder(*self.order_item()))
        spec = WindowSpec(partition, orders)
        t = self.peek()
        if t[0] == "ident" and t[1].lower() in ("rows", "range"):
            kind = self.next()[1].lower()
            self.expect("kw", "between")
            lo = self.frame_bound()
            self.expect("kw", "and")
            hi = self.frame_bound()
            spec = spec.rowsBetween(lo, hi) if kind == "rows" else spec.rangeBetween(lo, hi)
        self.expect("op", ")")
        return over(e, spec)

    def frame_bound(self) -> int:
        """``UNBOUNDED PRECEDING | n PRECEDING | CURRENT ROW | n FOLLOWING | UNBOUNDED FOLLOWING``
        as the integers ``rowsBetween`` takes."""
        from .window import Window

        def side():
            t = self.expect("ident")
            if t[1].lower() not in ("preceding", "following"):
                raise ParseException(f"\nmismatched input '{t[1]}' expecting PRECEDING or FOLLOWING")
            return t[1].lower() == "preceding"

        if self.accept("ident", "unbounded"):
            return Window.unboundedPreceding if side() else Window.unboundedFollowing
        if self.accept("ident", "current"):
            self.expect("ident", "row")
            return Window.currentRow
        neg = bool(self.accept("op", "-"))
        t = self.expect("num")
        if not t[1].isdigit():
            raise ParseException(f"\nmismatched input '{t[1]}' expecting an integer frame offset")
        v = -int(t[1]) if neg else int(t[1])
        return -v if side() else v

    def order_item(self):
        """``expr [ASC|DESC] [NULLS FIRST|NULLS LAST]`` -> (expr, ascending, nulls_first or None)."""
        e = self.expr()
        asc = True
        if self.accept("ident", "desc"):
            asc = False
        else:
            self.accept("ident", "asc")
        nf = None
        if self.accept("ident", "nulls"):
            t = self.expect("ident")
            if t[1].lower() not in ("first", "last"):
                raise ParseException(f"\nmismatched input '{t[1]}' expecting FIRST or LAST")
            nf = t[1].lower() == "first"
        return e, asc, nf

    def select_list(self):
        items = [self.select_item()]
        while self.accept("op", ","):
            items.append(self.select_item())
        return items

    def select_item(self):
        if self.accept("op", "*"):
            return ColRef("*")
        e = self.expr()
        if self.accept("kw", "as"):
            return Alias(e, self.expect("ident")[1])
        if self.peek()[0] == "ident":
            return Alias(e, self.next()[1])
        return e

    # ---- expressions ---------------------------------------------------------------------------
    def expr(self):
        return self.or_()

    def or_(self):
        e = self.and_()
        while self.accept("kw", "or"):
            e = BinOp("or", e, self.and_())
        return e

    def and_(self):
        e = self.not_()
        while self.accept("kw", "and"):
            e = BinOp("and", e, self.not_())
        return e

    def not_(self):
        if self.accept("kw", "not"):
            return Not(self.not_())
        return self.predicate()

    def predicate(self):
        e = self.additive()
        t = self.peek()
        if t[0] == "op" and t[1] in ("=", "==", "<", ">", "<=", ">=", "<>", "!=", "<=>"):
            self.next()
            return BinOp(t[1], e, self.additive())
        if self.accept("kw", "is"):
            neg = bool(self.accept("kw", "not"))
            self.expect("kw", "null")
            return IsNotNull(e) if neg else IsNull(e)
        neg = bool(self.accept("kw", "not"))
        if self.accept("kw", "between"):
            lo = self.additive()
            self.expect("kw", "and")
            hi = self.additive()
            r = BinOp("and", BinOp(">=", e, lo), BinOp("<=", e, hi))
            return Not(r) if neg else r
        if self.accept("kw", "in"):
            self.expect("op", "(")
            vals = [self.expr()]
            while self.accept("op", ","):
                vals.append(self.expr())
            self.expect("op", ")")
            r = BinOp("=", e, vals[0])
            for v in vals[1:]:
                r = BinOp("or", r, BinOp("=", e, v))
            return Not(r) if neg else r
        if neg:
            raise ParseException("\nmismatched input 'NOT'")
        return e

    def additive(self):
        e = self.mult()
        while self.peek()[0] == "op" and self.peek()[1] in ("+", "-"):
            op = self.next()[1]
            e = BinOp(op, e, self.mult())
        return e

    def mult(self):
        e = self.unary()
        while self.peek()[0] == "op" and self.peek()[1] in ("*", "/", "%"):
            op = self.next()[1]
            e = BinOp(op, e, self.unary())
        return e

    def unary(self):
        if self.accept("op", "-"):
            e = self.unary()
            if isinstance(e, Lit) and isinstance(e.value, (int, float)) and not isinstance(e.value, bool):
                return Lit(-e.value, e.dtype)
            return Neg(e)
        if self.accept("op", "+"):
            return self.unary()
        return self.primary()

    def primary(self):
        t = self.next()
        kind, val = t
        if kind == "num":
            v = val.lower()
            if v.endswith("d"):
                return Lit(float(v[:-1]))
            if v.endswith("l"):
                from .types import LongType

                return Lit(int(v[:-1]), LongType())
            if "." in v or "e" in v:
                return Lit(float(v))
            return Lit(int(v))
        if kind == "str":
            return Lit(val[1:-1].replace("''", "'").replace("\\'", "'"))
        if kind == "kw":
            if val == "null":
                return Lit(None)
            if val in ("true", "false"):
                return Lit(val == "true")
            if val == "cast":
                self.expect("op", "(")
                e = self.expr()
                self.expect("kw", "as")
                tname = self.expect("ident")[1]
                if self.accept("op", "("):
                    args = [self.expect("num")[1]]
                    while self.accept("op", ","):
                        args.append(self.expect("num")[1])
                    self.expect("op", ")")
                    tname += "(" + ",".join(args) + ")"
                self.expect("op", ")")
                return Cast(e, tname)
            if val == "case":
                branches = []
                operand = None
                if not (self.peek()[0] == "kw" and self.peek()[1] == "when"):
                    operand = self.expr()
                while self.accept("kw", "when"):
                    c = self.expr()
                    if operand is not None:
                        c = BinOp("=", operand, c)
                    self.expect("kw", "then")
                    branches.append((c, self.expr()))
                other = None
                if self.accept("kw", "else"):
                    other = self.expr()
                self.expect("kw", "end")
                return CaseWhen(branches, other)
            raise ParseException(f"\nmismatched input '{val}'")
        if kind == "op" and val == "(":
            e = self.expr()
            self.expect("op", ")")
            return e
        if kind == "ident":
            if self.accept("op", "("):
                if val.lower() == "count" and self.accept("op", "*"):
                    self.expect("op", ")")
                    return self.over(AggExpr("count", None))
                args = []
                if not self.accept("op", ")"):
                    args.append(self.expr())
                    while self.accept("op", ","):
                        args.append(self.expr())
                    self.expect("op", ")")
                return self.over(_function(val, args))
            if self.accept("op", "."):
                field = self.expect("ident")[1]
                return ColRef(val + "." + field)
            return ColRef(val)
        raise ParseException(f"\nmismatched input '{val or '<EOF>'}'")


def _int_arg(fn: str, e: Expr) -> int:
    if not (isinstance(e, Lit) and isinstance(e.value, int) and not isinstance(e.value, bool)):
        raise AnalysisException(f"{fn}: the offset / bucket count must be an integer literal, got {e.sql_name()}")
    return e.value


def _window_function(low: str, args: List[Expr]) -> Expr:
    """``row_number()`` ... ``lead(c, k, default)``: a window function awaiting its OVER clause."""
    from .window import WindowFn

    if low not in ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead"):
        return WindowFn(low)  # (raises: first / last / nth_value are not implemented)
    if low in ("lag", "lead"):
        if not 1 <= len(args) <= 3:
            raise AnalysisException(f"Invalid number of arguments for function {low}")
        default = None
        if len(args) == 3:
            if not isinstance(args[2], Lit):
                raise AnalysisException(f"{low}: the default must be a literal, got {args[2].sql_name()}")
            default = args[2].value
        return WindowFn(low, args[0], _int_arg(low, args[1]) if len(args) > 1 else 1, default)
    if low == "ntile":
        if len(args) != 1:
            raise AnalysisException("Invalid number of arguments for function ntile")
        return WindowFn(low, None, _int_arg(low, args[0]))
    if args:
        raise AnalysisException(f"Invalid number of arguments for function {low}")
    return WindowFn(low)


def _function(name: str, args: List[Expr]) -> Expr:
    low = name.lower()
    if low in _WINDOW_FNS:
        return _window_function(low, args)
    if low == "coalesce":
        return Coalesce(*args)
    if low == "isnull":
        return IsNull(args[0])
    if low == "isnotnull":
        return IsNotNull(args[0])
    if low == "if":
        return If(*args)
    if low in BUILTIN_MATH:
        return MathFn(low, args)
    if low in ("count", "sum", "avg", "mean", "min", "max"):
        if len(args) != 1:
            raise AnalysisException(f"Invalid number of arguments for function {low}")
        return AggExpr(low, args[0])
    return UdfCall(name, args)


def _strip_qual(e: Expr, quals) -> Expr:
    """``p.guest`` -> ``guest`` when ``p`` names the FROM relation."""
    if isinstance(e, ColRef) and "." in e.name:
        q, _, f = e.name.partition(".")
        if q.lower() in quals:
            return ColRef(f)
        return e
    for attr in ("child", "left", "right", "cond", "a", "b", "otherwise"):
        if hasattr(e, attr) and isinstance(getattr(e, attr), Expr):
            setattr(e, attr, _strip_qual(getattr(e, attr), quals))
    if hasattr(e, "args"):
        e.args = [_strip_qual(a, quals) for a in e.args]
    if hasattr(e, "partition") and hasattr(e, "orders"):  # a window specification
        e.partition = [_strip_qual(a, quals) for a in e.partition]
        e.orders = [_strip_qual(a, quals) for a in e.orders]
    if hasattr(e, "branches"):
        e.branches = [(_strip_qual(c, quals), _strip_qual(v, quals)) for c, v in e.branches]
    return e


def parse_expression(text: str) -> Expr:
    p = _Parser(text)
    e = p.expr()
    p.expect("eof")
    return e


def parse_select_item(text: str) -> Expr:
    p = _Parser(text)
    e = p.select_item()
    p.expect("eof")
    return e


_BOUND: dict = {}  # (statement, view plan skey) -> analyzed [Filter?, Project, Limit?] templates


def _bind_query(syntax, text: str, session):
    """The plan of a parsed SELECT over the session's CURRENT view of its FROM name (a temp view
    replaced between two runs of the same text binds to the new plan).  Expression trees are
    immutable once parsed, so plans may share them; a statement bound over a view of the same
    structure (sql/skey.py) reuses the analyzed nodes (fresh copies: no result is shared)."""
    items, tname, where, limit, distinct, group, order, joins = syntax

    def view(name):
        p = session.catalog._views.get(name.lower())
        if p is None:
            raise AnalysisException(f"Table or view not found: {name}; line 1 pos {text.lower().find(name.lower())}")
        return p

    plan = view(tname)
    if joins:  # (the template cache below walks a single .child chain: a statement with a JOIN is bound anew)
        from .joins import using_keys

        for how, jname, _, cols in joins:  # left-associative
            right = view(jname)
            plan = Join(plan, right, using_keys(plan.schema(), right.schema(), cols), how, True)
        return _bind_new(items, where, limit, plan, distinct, group, order)
    vk = plan.skey()
    key = (text, vk) if vk is not None else None
    tmpl = _BOUND.get(key) if key is not None else None
    if tmpl is not None:
        for t in tmpl:
            plan = t.fresh(plan)
        return plan
    out = _bind_new(items, where, limit, plan, distinct, group, order)
    if key is not None and out.skey() is not None:
        nodes, p = [], out
        while p is not plan:
            nodes.append(p)
            p = p.child
        tmpl = []
        for n in reversed(nodes):  # bottom-up, detached from the lineage
            n.schema()
            t = n.fresh()
            t.child = None
            tmpl.append(t)
        if len(_BOUND) >= 1024:
            _BOUND.clear()
        _BOUND[key] = tmpl
    return out


def _bind_new(items, where, limit, plan, distinct=False, group=None, order=None):
    from .window import contains_window

    if where is not None:
        if contains_window(where):
            raise AnalysisException("It is not allowed to use window functions inside WHERE and HAVING clauses: select the "
                                    "window expression under an alias and filter on the alias")
        if contains_aggregate(where):
            raise AnalysisException("Aggregate/Window/Generate expressions are not valid in where clause of the query.")
        plan = Filter(plan, where)
    exprs = []
    for e in items:
        if isinstance(e, ColRef) and e.name == "*":
            exprs += [ColRef(n) for n in plan.schema().names]
        else:
            exprs.append(e)
    grouped = group is not None or any(contains_aggregate(e) for e in exprs)
    windowed = any(contains_window(e) for e in exprs)
    if any(contains_window(g) for g in group or []):
        raise AnalysisException("window functions are not allowed in GROUP BY")
    if grouped and windowed:
        raise AnalysisException("a window function over the result of GROUP BY / aggregates in one SELECT is not "
                                "implemented: aggregate in a first statement and window over its result")
    if grouped:
        plan = _bind_grouped(exprs, group or [], plan)
    elif windowed:
        plan = build_project(plan, exprs)
    else:
        plan = Project(plan, exprs)
        cs = plan.child.schema()
        for e in exprs:
            e.data_type(cs)
    if distinct:  # the distinct rows of the select list
        plan = Aggregate(plan, plan.schema().names, [])
    if order:
        plan = _bind_order(order, plan, grouped or distinct)
    if limit is not None:
        plan = Limit(plan, limit)
    return plan


def _bind_order(order, plan, closed: bool):
    """``ORDER BY`` over ``plan``, the node that produces the select list.  An item resolves against
    the select list's output names first; then, as a positive integer literal, it is an ordinal
    into the select list; then, unless the query is ``closed`` (GROUP BY / aggregates / DISTINCT),
    against the columns of the FROM view, which are carried through the select list's Project as
    hidden columns and dropped above the sort."""
    schema = plan.schema()
    names = schema.names
    orders, hidden = [], []
    for i, (e, asc, nf) in enumerate(order):
        if contains_aggregate(e):
            raise AnalysisException(f"aggregate functions are not supported in ORDER BY, but found {e.sql_name()}: select "
                                    f"it under an alias and order by the alias")
        if isinstance(e, Lit) and isinstance(e.value, int) and not isinstance(e.value, bool):
            if not 1 <= e.value <= len(names):
                raise AnalysisException(f"ORDER BY position {e.value} is not in select list (valid range is [1, {len(names)}])")
            orders.append(SortOrder(ColRef(names[e.value - 1]), asc, nf))
        elif all(schema.resolve_ci(r) is not None for r in e.references()):
            orders.append(SortOrder(e, asc, nf))
        elif closed:
            raise AnalysisException(f"cannot resolve '{e.sql_name()}' given input columns: [{', '.join(names)}]")
        else:
            e.data_type(plan.child.schema())  # (raises on a column the view does not have either)
            name = f"_order_by_{i}: {e.sql_name()}"  # (the fused-chain cache keys a Project by its output names)
            hidden.append(Alias(e, name))
            orders.append(SortOrder(ColRef(name), asc, nf))
    if not hidden:
        return build_sort(plan, orders)
    return Project(build_sort(Project(plan.child, plan.exprs + hidden), orders), [ColRef(n) for n in names])


def _bind_grouped(exprs, group, plan):
    """``SELECT key..., agg(...) ... GROUP BY key...``: the aggregate over the grouping
    expressions, then a Project that puts the select list in its order under its names.  A select
    item that is neither a grouping expression nor an aggregate is an AnalysisException."""
    def same(a, b):
        ka, kb = expr_key(a), expr_key(b)
        if ka is not None and ka == kb:
            return True
        return a.sql_name().lower() == b.sql_name().lower()

    aggs, out = [], []
    for i, e in enumerate(exprs):
        base = e.child if isinstance(e, Alias) else e
        if isinstance(base, AggExpr):
            name = f"_agg_out_{i}"
            aggs.append(Alias(base, name))
            out.append(Alias(ColRef(name), output_name(e)))
            continue
        if contains_aggregate(base):
            raise AnalysisException(f"expressions over aggregates are not supported: {base.sql_name()}")
        k = next((g for g in group if same(g, base)), None)
        if k is None:
            raise AnalysisException(f"expression '{base.sql_name()}' is neither present in the group by, nor is it an "
                                    f"aggregate function. Add to group by or wrap in first() (or first_value) if you "
                                    f"don't care which value you get.;")
        out.append(Alias(ColRef(output_name(k)), output_name(e)))
    agg = build_aggregate(plan, group, aggs)
    return Project(agg, out)


_SYNTAX: dict = {}


def plan_sql(text: str, session):
    """``spark.sql(text)``: Spark re-parses every statement; the app re-runs the same two
    statements on every action (``DataQuality4MachineLearningApp.java:77-78, 89-90``), so the
    syntax is parsed once per text and only bound to the current catalog per call."""
    syn = _SYNTAX.get(text)
    if syn is None:
        syn = _Parser(text).query_syntax()
        if len(_SYNTAX) >= 256:
            _SYNTAX.clear()
        _SYNTAX[text] = syn
    return _bind_query(syn, text, session)


_ = Optional
