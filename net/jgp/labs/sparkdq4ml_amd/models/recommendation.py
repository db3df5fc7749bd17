"""``org.apache.spark.ml.recommendation``: ``ALS`` (Spark 2.4 semantics, explicit feedback).

The half-steps, the start and the fit are ``ops/als.py``'s: on the device one half-step over one
side's segment table is one launch of ``csrc/hip/als.hip`` (plus a small one for long segments) and
all iterations are enqueued before the fit's one host read; the CPU engine runs the fp64 twin.
Starting factors come from the project's own seeded rule, so they agree with Spark's in
distribution, not bit for bit.

Not implemented, each raising an error that says so: ``implicitPrefs=True`` (and ``alpha`` with
it), ``nonnegative=True``, persistence of the fitted model, ``recommendForAllUsers`` /
``recommendForAllItems``, and a data-parallel (sharded) input -- the ratings of a user or an item
may lie on several ranks, and a shuffle across ranks is not implemented.  ``numUserBlocks``,
``numItemBlocks``, ``checkpointInterval`` and the storage levels are accepted and ignored.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ops import als as A
from ..sql.dataframe import DataFrame
from ..sql.expressions import Alias, AnalysisException, ColRef, EvalContext, Expr
from ..sql.plan import Filter, Project, is_sharded
from ..sql.table import ColumnData
from ..sql.types import BooleanType, FloatType, is_numeric
from ..utils import tracing
from .linalg import DenseVector
from .param import Param, Params, param_accessors

__all__ = ["ALS", "ALSModel"]

_INT_MIN, _INT_MAX = -(1 << 31), (1 << 31) - 1


def _not_implemented(what: str) -> NotImplementedError:
    return NotImplementedError(f"ALS: {what} is not implemented")


class _ALSParams(Params):
    _params = {
        "rank": Param("rank", "rank of the factorization", 10, lambda v: v >= 1, converter=int),
        "maxIter": Param("maxIter", "maximum number of iterations (>= 0)", 10, lambda v: v >= 0, converter=int),
        "regParam": Param("regParam", "regularization parameter (>= 0)", 0.1, lambda v: v >= 0, converter=float),
        "userCol": Param("userCol", "column name for user ids. Ids must be within the integer value range.", "user"),
        "itemCol": Param("itemCol", "column name for item ids. Ids must be within the integer value range.", "item"),
        "ratingCol": Param("ratingCol", "column name for ratings", "rating"),
        "predictionCol": Param("predictionCol", "prediction column name", "prediction"),
        "seed": Param("seed", "random seed", 1994790107, converter=int),
        "coldStartStrategy": Param("coldStartStrategy", "strategy for dealing with unknown or new users/items at "
                                   "prediction time. Supported values: 'nan', 'drop'.", "nan",
                                   lambda v: v in ("nan", "drop")),
        "implicitPrefs": Param("implicitPrefs", "whether to use implicit preference", False, converter=bool),
        "alpha": Param("alpha", "alpha for implicit preference", 1.0, lambda v: v >= 0, converter=float),
        "nonnegative": Param("nonnegative", "whether to use nonnegative constraint for least squares", False,
                             converter=bool),
        # accepted and ignored: one process holds the whole table and nothing is checkpointed or cached
        "numUserBlocks": Param("numUserBlocks", "number of user blocks", 10, lambda v: v >= 1, converter=int),
        "numItemBlocks": Param("numItemBlocks", "number of item blocks", 10, lambda v: v >= 1, converter=int),
        "checkpointInterval": Param("checkpointInterval", "set checkpoint interval (>= 1) or disable checkpoint (-1)", 10,
                                    lambda v: v == -1 or v >= 1, converter=int),
        "intermediateStorageLevel": Param("intermediateStorageLevel", "StorageLevel for intermediate datasets.",
                                          "MEMORY_AND_DISK"),
        "finalStorageLevel": Param("finalStorageLevel", "StorageLevel for ALS model factors.", "MEMORY_AND_DISK"),
    }

    def set(self, name, value):
        if name == "implicitPrefs" and value:
            raise _not_implemented("implicitPrefs=True (implicit feedback, and alpha with it)")
        if name == "alpha":
            raise _not_implemented("alpha (implicit feedback)")
        if name == "nonnegative" and value:
            raise _not_implemented("nonnegative=True (the NNLS solver)")
        return super().set(name, value)

    _set = set


def _int_ids(c: ColumnData, live: Optional[torch.Tensor], name: str) -> torch.Tensor:
    """The ids of a column as int64 (dead rows: 0), Spark's rule: a numeric column whose live values
    are integers within the int range; a live null raises."""
    if not is_numeric(c.dtype) or not torch.is_tensor(c.values) or c.values.dim() != 1:
        raise AnalysisException(f"ALS: column {name} must be numeric, not {c.dtype.simpleString()}")
    v = c.values
    keep = torch.ones(v.numel(), dtype=torch.bool, device=v.device) if live is None else live.to(torch.bool)
    if c.valid is not None and bool((keep & ~c.valid).any()):
        raise ValueError(f"ALS: column {name} has a null id in a live row")
    x = torch.where(keep, v, torch.zeros_like(v))
    if x.dtype.is_floating_point and not bool(((x == torch.floor(x)) & torch.isfinite(x)).all()):
        raise ValueError(f"ALS only supports values in Integer range for column {name}: a value is not an integer")
    if x.numel() and (float(x.min()) < _INT_MIN or float(x.max()) > _INT_MAX):
        raise ValueError(f"ALS only supports values in Integer range for column {name}: a value is out of range")
    return x.to(torch.int64)


def _encode(ids: torch.Tensor, live: Optional[torch.Tensor]):
    """``(sorted distinct live ids int64 [k], dense index int32 per row, -1 for dead rows)`` from
    ``group_encode``'s slots: the slots that received a row, renumbered in key order."""
    from ..ops.groupby import group_encode

    enc = group_encode(ids, None, live)
    gid = enc.gid.to(torch.int64)
    used = torch.bincount(gid[gid > 0], minlength=enc.G) > 0
    slots = torch.nonzero(used).flatten()
    keys, order = torch.sort(enc.keys[slots])
    dense = torch.full((enc.G,), -1, dtype=torch.int32, device=ids.device)
    dense[slots[order]] = torch.arange(int(slots.numel()), dtype=torch.int32, device=ids.device)
    return keys, torch.where(gid > 0, dense[gid.clamp(min=0)], torch.full((), -1, dtype=torch.int32, device=ids.device))


def _lookup(keys: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """int32 position of each id in the sorted ``keys``, -1 where it is absent."""
    keys = keys.to(ids.device)
    pos = torch.searchsorted(keys, ids).clamp(max=max(int(keys.numel()) - 1, 0))
    return torch.where(keys[pos] == ids, pos, torch.full_like(pos, -1)).to(torch.int32)


@param_accessors
class ALS(_ALSParams):
    uid_prefix = "als"

    def __init__(self, uid=None, **kw):
        super().__init__(uid)
        for k, v in kw.items():
            if v is not None:
                self.set(k, v)

    def fit(self, dataset: DataFrame, params=None) -> "ALSModel":
        est = self.copy(params) if params else self
        return est._train(dataset)

    # persistence (params only, DefaultParamsWriter layout) -----------------------------------
    def write(self):
        from .persistence import ParamsWriter

        return ParamsWriter(self, "org.apache.spark.ml.recommendation.ALS")

    def save(self, path):
        self.write().save(path)

    @classmethod
    def load(cls, path):
        from .persistence import load_params_only

        return load_params_only(cls, path)

    def _train(self, df: DataFrame) -> "ALSModel":
        g = self.getOrDefault
        if is_sharded(df._plan):
            raise AnalysisException("ALS over a data-parallel (sharded) input: the ratings of a user or an item may lie on "
                                    "several ranks, and a shuffle across ranks is not implemented")
        for name in (g("userCol"), g("itemCol"), g("ratingCol")):
            ColRef(name).data_type(df.schema)
        tbl = df._table()
        live = tbl.sel
        rc = tbl.column(g("ratingCol"))
        if not is_numeric(rc.dtype) or not torch.is_tensor(rc.values) or rc.values.dim() != 1:
            raise AnalysisException(f"ALS: column {g('ratingCol')} must be numeric, not {rc.dtype.simpleString()}")
        if rc.valid is not None and bool(((rc.valid_mask() ^ True) & tbl.sel_mask()).any()):
            raise ValueError(f"ALS: column {g('ratingCol')} has a null rating in a live row")
        uid = _int_ids(tbl.column(g("userCol")), live, g("userCol"))
        iid = _int_ids(tbl.column(g("itemCol")), live, g("itemCol"))
        ukeys, u = _encode(uid, live)
        ikeys, i = _encode(iid, live)
        if int(ukeys.numel()) == 0:
            raise ValueError("ALS: the input has no rows")
        rows = torch.nonzero(u >= 0).flatten() if live is not None else slice(None)
        with tracing.span("als"):
            res = A.fit(u[rows], i[rows], rc.values[rows].to(torch.float64), int(ukeys.numel()), int(ikeys.numel()), g("rank"),
                        g("maxIter"), g("regParam"), g("seed"))
        tracing.add_rows("als", tbl.nrows)
        model = ALSModel(self.uid, g("rank"), ukeys.cpu().numpy(), res.user_factors, ikeys.cpu().numpy(), res.item_factors)
        self.copyValues(model)
        model._session, model._route = df.sparkSession, res.route
        return model


class _Lookup:
    """The factor-row indices of a table's id columns, computed once per table and shared by the
    prediction column and the cold-start filter."""

    def __init__(self, model: "ALSModel"):
        self.model = model
        self._table = self._out = None

    def of(self, table):
        if self._table is not table:
            m, g = self.model, self.model.getOrDefault
            uc, ic = table.column(g("userCol")), table.column(g("itemCol"))
            out = []
            for c, keys, name in ((uc, m._user_ids, g("userCol")), (ic, m._item_ids, g("itemCol"))):
                live = table.sel if c.valid is None else (c.valid if table.sel is None else table.sel & c.valid)
                t = _lookup(torch.from_numpy(keys), _int_ids(c, live, name))  # (a null id is an unseen one)
                out.append((t if live is None else torch.where(live, t, torch.full_like(t, -1))).contiguous())
            self._out, self._table = tuple(out), table
        return self._out


class ALSPredictExpr(Expr):
    """``which`` 0: the prediction (f32, NaN where either id was not seen in the fit); 1: whether both
    ids were seen (the cold-start filter)."""

    def __init__(self, run: _Lookup, which: int):
        self.run, self.which = run, which

    def children(self):
        g = self.run.model.getOrDefault
        return [ColRef(g("userCol")), ColRef(g("itemCol"))]

    def data_type(self, schema):
        return BooleanType() if self.which else FloatType()

    def nullable(self, schema):
        return False

    def sql_name(self):
        return ("prediction", "seen")[self.which]

    def eval(self, ctx: EvalContext) -> ColumnData:
        u, i = self.run.of(ctx.table)
        if self.which:
            return ColumnData(BooleanType(), (u >= 0) & (i >= 0), None)
        m = self.run.model
        with tracing.span("als_predict"):
            U, V = (torch.from_numpy(f).to(u.device) for f in (m._user_factors, m._item_factors))
            return ColumnData(FloatType(), A.predict(u, i, None, U, V).to(torch.float32), None)


@param_accessors
class ALSModel(_ALSParams):
    uid_prefix = "als"

    def __init__(self, uid: Optional[str], rank: int, user_ids, user_factors, item_ids, item_factors):
        super().__init__(uid)
        self._rank = int(rank)
        self._user_ids, self._item_ids = np.asarray(user_ids, dtype=np.int64), np.asarray(item_ids, dtype=np.int64)
        self._user_factors = np.ascontiguousarray(user_factors, dtype=np.float32)
        self._item_factors = np.ascontiguousarray(item_factors, dtype=np.float32)
        self._session = self._route = None

    @property
    def rank(self) -> int:
        return self._rank

    def _factors_df(self, ids, factors) -> DataFrame:
        if self._session is None:
            raise RuntimeError("userFactors / itemFactors need the session of the fit: this model was not fitted")
        return self._session.createDataFrame([(int(k), DenseVector(f.astype(np.float64))) for k, f in zip(ids, factors)],
                                             ["id", "features"])

    @property
    def userFactors(self) -> DataFrame:
        """``id`` and ``features`` per user, in id order (a vector column, as ``gaussiansDF``: the
        engine has no array column type)."""
        return self._factors_df(self._user_ids, self._user_factors)

    @property
    def itemFactors(self) -> DataFrame:
        return self._factors_df(self._item_ids, self._item_factors)

    @property
    def route(self) -> str:
        """Which route of ``ops/als.py`` ran the fit's half-steps (engine diagnostic, not Spark's)."""
        return self._route

    def transform(self, df: DataFrame) -> DataFrame:
        g = self.getOrDefault
        for name in (g("userCol"), g("itemCol")):
            ColRef(name).data_type(df.schema)
        run, pc, plan = _Lookup(self), g("predictionCol"), df._plan
        if g("coldStartStrategy") == "drop":
            plan = Filter(plan, ALSPredictExpr(run, 1))
        exprs = [ColRef(n) for n in df.columns if n != pc] + [Alias(ALSPredictExpr(run, 0), pc)]
        return DataFrame(Project(plan, exprs), df.sparkSession)

    def recommendForAllUsers(self, numItems: int):
        raise _not_implemented("recommendForAllUsers")

    def recommendForAllItems(self, numUsers: int):
        raise _not_implemented("recommendForAllItems")

    # persistence: out of scope ---------------------------------------------------------------
    def write(self):
        raise _not_implemented("persistence of the fitted model")

    def save(self, path):
        self.write()

    @classmethod
    def read(cls):
        raise _not_implemented("persistence of the fitted model")

    @classmethod
    def load(cls, path):
        cls.read()

    def __repr__(self):
        return (f"ALSModel: uid={self.uid}, rank={self._rank}, users={self._user_ids.size}, "
                f"items={self._item_ids.size}")
