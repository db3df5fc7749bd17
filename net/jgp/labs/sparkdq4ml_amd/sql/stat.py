"""``DataFrame.stat`` / ``approxQuantile`` / ``summary`` — order statistics on the table's device.

Every quantile here is exact: the columns go through ``ops.kernels.quantiles`` (a radix select
over order-preserving 64-bit keys), never through a sort or a host copy of the rows.  On a
data-parallel plan the per-pass histograms are all-reduced and every rank gets the same values;
the quantiles never gather rows (``summary``'s count / mean / stddev / min / max cells are
``describe``'s, which on a sharded plan gathers them as ``describe`` does).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from .describe import _fmt, _integral, describe
from .plan import LocalRelation, is_sharded
from .types import StringType, StructField, StructType, VectorUDT, is_numeric

__all__ = ["DataFrameStatFunctions", "column_quantiles", "summary", "replicated_frame"]

_DEFAULT_STATS = ("count", "mean", "stddev", "min", "25%", "50%", "75%", "max")
_KERNEL_DTYPES = (torch.float64, torch.float32, torch.int32, torch.int64)


def replicated_frame(session, rows, schema):
    """A small result frame that every rank holds whole (never one shard of a larger frame)."""
    from .dataframe import DataFrame
    from .localdata import table_from_data

    return DataFrame(LocalRelation(table_from_data(rows, schema, session.device), sharded=False), session)


def quantile_reduce(df):
    """The ``reduce`` hook of ``kernels.quantiles`` for ``df``: the cross-rank sum of the int64
    histogram counters on a sharded plan, else None."""
    if not is_sharded(df._plan):
        return None
    from ..parallel import comm

    return comm.all_reduce_sum


def column_quantiles(df, cols: Sequence[str], probs: Sequence[float], valids=None):
    """``(values [C, Q] float64 ndarray, counts [C] int list)`` of the numeric columns ``cols`` of
    ``df`` over its live rows, nulls and NaN ignored: ONE ``kernels.quantiles`` call per 16
    probabilities for all the columns, one host read each.  ``valids`` overrides the columns'
    validity masks (the Imputer adds its ``missingValue``)."""
    from ..ops import kernels
    from ..runtime.checks import verify

    t = df._table()
    data = [t.column(c) for c in cols]
    vals = [c.values if c.values.dtype in _KERNEL_DTYPES else c.values.to(torch.float64) for c in data]
    valids = [c.valid for c in data] if valids is None else list(valids)
    reduce = quantile_reduce(df)
    probs = [float(p) for p in probs]
    out, counts = [], None
    for i in range(0, len(probs), kernels.MAX_QUANTILES):
        v, n = kernels.quantiles(vals, valids, t.sel, probs[i:i + kernels.MAX_QUANTILES], reduce=reduce)
        out.append(v.cpu().numpy())
        counts = n
    pending = [ck for c in data for ck in c.checks]
    if pending:
        verify(pending)
    return np.concatenate(out, axis=1), [int(x) for x in counts.cpu().tolist()]


class DataFrameStatFunctions:
    """``df.stat`` (``org.apache.spark.sql.DataFrameStatFunctions``)."""

    def __init__(self, df):
        self.df = df

    def approxQuantile(self, col, probabilities, relativeError):
        """Quantiles of one numeric column (``col`` a string: ``List[float]``) or several (a list
        or tuple of names: ``List[List[float]]``) at ``probabilities``.

        The result is always EXACT — the element of rank ``ceil(p * n)`` among the n non-null,
        non-NaN values cast to double (the minimum for p = 0, the maximum for p = 1), which is what
        Spark returns for ``relativeError = 0`` and satisfies every ``relativeError >= 0``; the
        argument is validated and otherwise unused.  Nulls and NaN are ignored; a column without
        any other value yields ``[]`` (Spark 2.4).  All the columns of one call share one kernel
        call; on a sharded frame the histograms are all-reduced and no row leaves its rank."""
        if isinstance(col, str):
            names, single = [col], True
        elif isinstance(col, (list, tuple)):
            names, single = list(col), False
        else:
            raise ValueError(f"col should be a string, list or tuple, but got {type(col)!r}")
        for c in names:
            if not isinstance(c, str):
                raise ValueError(f"columns should be strings, but got {type(c)!r}")
        if not isinstance(probabilities, (list, tuple)):
            raise ValueError("probabilities should be a list or tuple")
        probs = []
        for p in probabilities:
            if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
                raise ValueError("probabilities should be numerical (float, int) in [0,1].")
            probs.append(float(p))
        if isinstance(relativeError, bool) or not isinstance(relativeError, (int, float)) or relativeError < 0:
            raise ValueError("relativeError should be numerical (float, int) >= 0.")
        schema = self.df.schema
        for c in names:
            rc = schema.resolve_ci(c)
            if rc is None:
                raise ValueError(f'Cannot resolve column name "{c}" among ({", ".join(schema.names)})')
            f = schema[rc]
            if not is_numeric(f.dataType):
                raise ValueError(f"Quantile calculation for column {c} with data type {f.dataType.simpleString()}"
                                 " is not supported.")
        if not names:
            return []
        if not probs:
            return [] if single else [[] for _ in names]
        values, counts = column_quantiles(self.df, names, probs)
        out = [[float(v) for v in values[i]] if counts[i] > 0 else [] for i in range(len(names))]
        return out[0] if single else out


def _percent(stat: str):
    """``"NN%"`` / ``"NN.N%"`` -> probability, None when ``stat`` is no percentile."""
    if not stat.endswith("%"):
        return None
    try:
        p = float(stat[:-1]) / 100.0
    except ValueError:
        return None
    if math.isnan(p) or not 0.0 <= p <= 1.0:
        raise ValueError(f"Percentile {stat} must be between 0% and 100%")
    return p


def summary(df, statistics: Sequence[str]):
    """``DataFrame.summary(*statistics)`` (Spark 2.4 ``StatFunctions.summary``)."""
    stats = [str(s) for s in statistics] or list(_DEFAULT_STATS)
    basic = ("count", "mean", "stddev", "min", "max")
    probs = {}
    for s in stats:
        if s in basic:
            continue
        p = _percent(s)
        if p is None:
            raise ValueError(f"{s} is not a recognised statistic")
        probs[s] = p
    fields = [f for f in df.schema.fields if not isinstance(f.dataType, VectorUDT)]
    fields = [f for f in fields if is_numeric(f.dataType) or isinstance(f.dataType, StringType)]
    cells = {}
    if any(s in basic for s in stats) and fields:
        # describe()'s own cells (its frame repeats per rank on a sharded plan: same rows, read by name)
        for r in describe(df, [f.name for f in fields]).collect():
            for f, v in zip(fields, list(r)[1:]):
                cells[(r[0], f.name)] = v
    numeric = [f for f in fields if is_numeric(f.dataType)]
    if probs and numeric:
        order = list(probs)
        values, counts = column_quantiles(df, [f.name for f in numeric], [probs[s] for s in order])
        for i, f in enumerate(numeric):
            for j, s in enumerate(order):
                cells[(s, f.name)] = _fmt(values[i, j], _integral(f)) if counts[i] > 0 else None
    rows = [tuple([s] + [cells.get((s, f.name)) for f in fields]) for s in stats]
    schema = StructType([StructField("summary", StringType(), True)] +
                        [StructField(f.name, StringType(), True) for f in fields])
    return replicated_frame(df.sparkSession, rows, schema)

