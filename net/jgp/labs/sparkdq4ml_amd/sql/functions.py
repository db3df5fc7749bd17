"""``org.apache.spark.sql.functions`` subset (``callUDF`` is imported statically by the lab,
``DataQuality4MachineLearningApp.java:3``)."""
from __future__ import annotations

from .column import Column
from .expressions import CaseWhen, Coalesce, ColRef, IsNull, Lit, UdfCall, to_expr

__all__ = ["col", "column", "lit", "callUDF", "call_udf", "udf", "when", "coalesce", "isnull", "expr",
           "count", "sum", "avg", "mean", "min", "max", "asc", "desc", "asc_nulls_first", "asc_nulls_last",
           "desc_nulls_first", "desc_nulls_last", "row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile",
           "lag", "lead"]


def col(name: str) -> Column:
    return Column(ColRef(name))


column = col


def lit(v) -> Column:
    return v if isinstance(v, Column) else Column(Lit(v))


def callUDF(name: str, *cols) -> Column:
    return Column(UdfCall(name, [c._expr if isinstance(c, Column) else ColRef(c) if isinstance(c, str) else to_expr(c)
                                 for c in cols]))


call_udf = callUDF


def when(cond: Column, value) -> Column:
    return Column(CaseWhen([(to_expr(cond), to_expr(value))]))


def coalesce(*cols) -> Column:
    return Column(Coalesce(*[c._expr if isinstance(c, Column) else ColRef(c) for c in cols]))


def isnull(c) -> Column:
    return Column(IsNull(c._expr if isinstance(c, Column) else ColRef(c)))


def _agg(fn: str, c) -> Column:
    from .aggregates import AggExpr

    if fn == "count" and isinstance(c, str) and c == "*":
        return Column(AggExpr("count", None))
    return Column(AggExpr(fn, ColRef(c) if isinstance(c, str) else to_expr(c)))


def count(c="*") -> Column:
    """``count(col)``: the non-null rows; ``count("*")``: all rows (named ``count(1)``)."""
    return _agg("count", c)


def sum(c) -> Column:  # noqa: A001 (pyspark's names)
    return _agg("sum", c)


def avg(c) -> Column:
    return _agg("avg", c)


mean = avg


def min(c) -> Column:  # noqa: A001
    return _agg("min", c)


def max(c) -> Column:  # noqa: A001
    return _agg("max", c)


def _order_col(c) -> Column:
    return c if isinstance(c, Column) else col(c)


def asc(c) -> Column:
    """Ascending sort order of a column (name or Column), nulls first."""
    return _order_col(c).asc()


def desc(c) -> Column:
    """Descending sort order, nulls last."""
    return _order_col(c).desc()


def asc_nulls_first(c) -> Column:
    return _order_col(c).asc_nulls_first()


def asc_nulls_last(c) -> Column:
    return _order_col(c).asc_nulls_last()


def desc_nulls_first(c) -> Column:
    return _order_col(c).desc_nulls_first()


def desc_nulls_last(c) -> Column:
    return _order_col(c).desc_nulls_last()


def _window_fn(fn: str, c=None, param: int = 0, default=None) -> Column:
    from .window import WindowFn

    child = None if c is None else (ColRef(c) if isinstance(c, str) else to_expr(c))
    return Column(WindowFn(fn, child, param, default))


def row_number() -> Column:
    """The 1-based position of the row in its window partition; needs ``.over`` an ordered window."""
    return _window_fn("row_number")


def rank() -> Column:
    return _window_fn("rank")


def dense_rank() -> Column:
    return _window_fn("dense_rank")


def percent_rank() -> Column:
    return _window_fn("percent_rank")


def cume_dist() -> Column:
    return _window_fn("cume_dist")


def ntile(n: int) -> Column:
    return _window_fn("ntile", None, n)


def lag(c, offset: int = 1, default=None) -> Column:
    """The value of ``c`` ``offset`` rows before the current row of its window partition
    (``default`` where there is none)."""
    return _window_fn("lag", c, offset, default)


def lead(c, offset: int = 1, default=None) -> Column:
    return _window_fn("lead", c, offset, default)


def expr(text: str) -> Column:
    from .parser import parse_expression

    return Column(parse_expression(text))


def udf(f=None, returnType=None):
    """``pyspark.sql.functions.udf``: wrap a python scalar function as an (anonymous) UDF."""
    from .udf import UserDefinedFunction
    from .types import DoubleType, StringType, parse_type_name

    def wrap(fn):
        rt = returnType if returnType is not None else StringType()
        rt = parse_type_name(rt) if isinstance(rt, str) else rt
        u = UserDefinedFunction(getattr(fn, "__name__", "udf"), fn, rt)
        return u

    if f is None or not callable(f) or isinstance(f, str):
        if f is not None and returnType is None:
            returnType = f
        return wrap
    return wrap(f)
