"""Decision trees (Spark 2.4 ``RandomForest.run`` with one tree, all features, continuous features
only): the thresholds, the level passes and the level loop.

A fit chooses per-feature thresholds from a sample on the host (:func:`find_splits`), bins every
row once -- ``bin(x)`` = the number of the feature's thresholds below x, so ``x <= t_b`` goes left of
split b -- and then, per level, builds the (node, feature, bin) statistics of the open nodes, picks
each node's best split (the first maximum of the gain in (feature, split) order) and routes the
rows to the children.  Children are numbered as Spark numbers them: left ``2 i``, right ``2 i + 1``
from root 1.

Accumulator words of a cell are integers: one count per class, or a count and ``sum y`` / ``sum
y^2`` as four fixed-point limbs each (the cut of ``ops/groupby.py``; exponents ``e`` and ``2 e``, ``e``
the frexp exponent of the largest ``|y|``, ``y * y`` rounded once to f64).  So the histogram depends
on neither grid, schedule nor shard split, and the twin matches the kernel bit for bit.  A limb sum
becomes a double by :func:`limbs_to_f64`: carry-normalise in integers from the bottom, Horner from
the top limb down in f64, scale by ``2^(e - 128)``.

Three routes run a level:

* the fused device passes (``csrc/hip/tree.hip`` through ``ops/device.py``): dense f32 / f64,
  d <= 64, at most 256 bins and 16 classes, one node's cells inside the block's 64 KiB of LDS;
* their fp64 twins here (``bin_host``, ``hist_host``, ``split_host``, ``route_host``,
  ``predict_host``): the CPU engine and the kernel tests' oracle;
* the composite: the same binning, routing and walk from torch ops on the device and
  :func:`composite_hist` (``bincount`` in f64) -- shapes outside the kernels, and the benchmark's
  comparator.

The threshold sample is every live row up to ``max(maxBins^2, 10000)`` rows, otherwise the rows
whose seeded uniform (``ops/kmeans.row_uniforms``, global row numbers in rank order) falls below
that fraction: it agrees with Spark's in distribution, not bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

__all__ = ["REG", "CLS", "VARIANCE", "GINI", "ENTROPY", "RECORD", "words", "group_size", "find_splits", "pack_splits",
           "row_words", "limbs_to_f64", "bin_host", "hist_host", "split_host", "split_stats", "route_host", "predict_host",
           "composite_hist", "route", "class_offsets", "fit", "predict", "TreeResult"]

REG, CLS = 0, 1                      # codes of csrc/hip/tree.h
VARIANCE, GINI, ENTROPY = 0, 1, 2
IMPURITIES = {"variance": VARIANCE, "gini": GINI, "entropy": ENTROPY}
RECORD = 64
REG_WORDS = 9
FUSED_MAX_D, FUSED_MAX_BINS, FUSED_MAX_CLASSES, LDS_BYTES = 64, 256, 16, 64 * 1024


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def class_offsets(classes: int):
    """Offsets of the node / left / right class counts in a node record, and the record's length.
    Up to 16 classes this is the kernel's 64-double record (csrc/hip/tree.h); the host and composite
    routes widen the three fields for more classes."""
    cw = max(16, int(classes))
    return 16, 16 + cw, 16 + 2 * cw, 16 + 3 * cw


def words(kind: int, classes: int) -> int:
    return int(classes) if kind == CLS else REG_WORDS


def group_size(kind: int, d: int, nb: int, classes: int) -> int:
    """Open nodes whose cells fit one block's LDS (``tree_group`` of csrc/hip/tree.h)."""
    return LDS_BYTES // (int(d) * int(nb) * words(kind, classes) * (4 if kind == CLS else 8))


# ---- thresholds ------------------------------------------------------------------------------------
def find_splits(sample, max_bins: int, n_rows: int) -> List[np.ndarray]:
    """Per feature, the thresholds of Spark's ``findSplitsForContinuousFeature`` from the sample rows
    ``[m, d]``; ``n_rows`` is the table's live row count (``numBins = min(maxBins, n_rows)``)."""
    S = np.asarray(sample, dtype=np.float64)
    num_splits = min(int(max_bins), int(n_rows)) - 1
    out = []
    for f in range(S.shape[1]):
        v, c = np.unique(S[:, f], return_counts=True)
        m = v.size - 1
        if m <= 0 or num_splits <= 0:
            out.append(np.zeros(0))
        elif m <= num_splits:
            out.append((v[:-1] + v[1:]) / 2.0)
        else:
            stride = S.shape[0] / (num_splits + 1)
            target, cur, cut = stride, int(c[0]), []
            for i in range(1, m + 1):
                prev, cur = cur, cur + int(c[i])
                if abs(prev - target) < abs(cur - target):
                    cut.append((v[i - 1] + v[i]) / 2.0)
                    target += stride
            out.append(np.array(cut[:num_splits]))
    return out


def pack_splits(splits):
    """``(thr [d, S] f64 padded with +inf, nsplit [d] int32)``, S >= 1."""
    ns = np.array([len(s) for s in splits], dtype=np.int32)
    T = np.full((len(splits), max(1, int(ns.max(initial=0)))), np.inf)
    for f, s in enumerate(splits):
        T[f, :len(s)] = s
    return T, ns


# ---- the twins ---------------------------------------------------------------------------------------
def bin_host(X, sel, thr, nsplit):
    """``(uint8 B [n, dpad], flag)`` from torch ops on X's device: the twin of ``tree_bin_kernel``.
    Dead rows and pad bytes are 0; the flag says that a live row holds a NaN.  A feature with more
    than 255 splits (``maxBins`` > 256: outside the kernels) makes B int16."""
    d, n = int(X.shape[0]), int(X.shape[1])
    live = torch.ones(n, dtype=torch.bool, device=X.device) if sel is None else sel.to(torch.bool)
    bdt = torch.uint8 if int(np.max(nsplit, initial=0)) <= 255 else torch.int16
    B = torch.zeros(n, (d + 3) // 4 * 4, dtype=bdt, device=X.device)
    T = torch.as_tensor(np.asarray(thr, dtype=np.float64), device=X.device)
    bad = torch.zeros((), dtype=torch.bool, device=X.device)
    for f in range(d):
        x = X[f].to(torch.float64)
        nan = torch.isnan(x)
        bad = bad | (nan & live).any()
        b = torch.searchsorted(T[f, :int(nsplit[f])].contiguous(), x.contiguous(), right=False)  # thresholds below x
        B[:, f] = torch.where(live & ~nan, b, torch.zeros_like(b)).to(bdt)
    return B, bad.reshape(1)


def row_words(y, kind: int, classes: int, e: int):
    """``(int64 words [n, W], usable [n])`` of the labels: a one-hot class row, or 1 and the limbs of
    y (exponent e) and of y * y (exponent 2 e)."""
    yv = _np(y).astype(np.float64)
    if kind == CLS:
        ok = (yv >= 0) & (yv < classes)
        c = np.where(ok, yv, 0).astype(np.int64)
        return (np.arange(int(classes))[None, :] == c[:, None]).astype(np.int64), ok
    ok = np.isfinite(yv)
    y0 = np.where(ok, yv, 0.0)
    w = np.ones((yv.size, REG_WORDS), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for off, v, ex in ((1, y0, int(e)), (5, y0 * y0, 2 * int(e))):
            t = np.ldexp(v, 32 - ex)
            for k in range(4):
                c = np.trunc(t)
                w[:, off + k] = c.astype(np.int64)
                t = np.ldexp(t - c, 32)
    return w, ok


def hist_host(B, node, y, kind: int, nodes: int, d: int, nb: int, classes: int, e: int) -> torch.Tensor:
    """The int64 histogram ``[nodes, d, nb, W]``: the twin of ``tree_hist_kernel`` (the same words)."""
    Bn, s = _np(B), _np(node).astype(np.int64)
    w, ok = row_words(y, kind, classes, e)
    ok = ok & (s >= 0) & (s < nodes)
    H = np.zeros((int(nodes), int(d), int(nb), w.shape[1]), dtype=np.int64)
    for f in range(int(d)):
        m = ok & (Bn[:, f] < nb)
        np.add.at(H[:, f], (s[m], Bn[m, f].astype(np.int64)), w[m])
    return torch.from_numpy(H)


def limbs_to_f64(L: np.ndarray, e: int) -> np.ndarray:
    """A four-limb fixed-point sum (last axis) as a double: the statement shared with the kernel."""
    L = np.asarray(L, dtype=np.int64)
    l, carry = [None] * 4, np.zeros(L.shape[:-1], dtype=np.int64)
    for k in (3, 2, 1):
        v = L[..., k] + carry
        carry, l[k] = v >> 32, v & 0xFFFFFFFF
    v = (L[..., 0] + carry).astype(np.float64)
    for k in (1, 2, 3):
        v = v * 4294967296.0 + l[k].astype(np.float64)
    return np.ldexp(v, int(e) - 128)


def _node_stats(w: np.ndarray, kind: int, impurity: int, e: int):
    """``(count, impurity, prediction)`` of cell words ``[..., W]``: int64 words, or the composite's
    f64 ``(count, sum y, sum y^2)`` / class counts."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == REG:
            if w.dtype == np.int64:
                n, s1, s2 = w[..., 0].astype(np.float64), limbs_to_f64(w[..., 1:5], e), limbs_to_f64(w[..., 5:9], 2 * int(e))
            else:
                n, s1, s2 = w[..., 0], w[..., 1], w[..., 2]
            return n, (s2 - s1 * s1 / n) / n, s1 / n
        c = w.astype(np.float64)
        n = w.sum(axis=-1).astype(np.float64)
        acc = np.full(n.shape, 1.0 if impurity == GINI else 0.0)
        for k in range(c.shape[-1]):
            f = c[..., k] / n
            pos = c[..., k] > 0
            term = f * f if impurity == GINI else f * np.log2(np.where(pos, f, 1.0))
            acc = acc - np.where(pos, term, 0.0)
        return n, acc, np.argmax(c, axis=-1).astype(np.float64)


def split_stats(H: np.ndarray, nsplit, kind: int, impurity: int, e: int, min_rows: int, min_gain: float,
                force_leaf: bool, child_leaf: bool, with_gains: bool = False):
    """The node records ``[nodes, RECORD]`` (layout: csrc/hip/tree.h; wider beyond 16 classes, see
    :func:`class_offsets`) of a histogram ``[nodes, d, nb, W]``
    of int64 words or of the composite's f64 statistics.  ``with_gains``: also the gain of every
    (feature, split) ``[nodes, d, nb]``, -inf where the split is invalid."""
    H = np.asarray(H)
    nodes, d, nb, W = H.shape
    ns = np.minimum(np.asarray(nsplit, dtype=np.int64), nb - 1)
    left = np.cumsum(H, axis=2)            # [nodes, d, nb, W]: bins 0 .. b
    tot = left[:, 0, -1, :]                # feature 0 sees every row of the node
    right = tot[:, None, None, :] - left
    pn, pimp, ppred = _node_stats(tot, kind, impurity, e)
    ln, limp, lpred = _node_stats(left, kind, impurity, e)
    rn, rimp, rpred = _node_stats(right, kind, impurity, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = (pimp[:, None, None] - (ln / pn[:, None, None]) * limp) - (rn / pn[:, None, None]) * rimp
        valid = (np.arange(nb)[None, None, :] < ns[None, :, None]) & (ln >= min_rows) & (rn >= min_rows) & (gain >= min_gain)
    c0, cl, cr, width = class_offsets(W if kind == CLS else 0)
    rec = np.zeros((nodes, width))
    for s in range(nodes):
        if not pn[s] > 0:
            rec[s, 0], rec[s, 10] = -1.0, 1.0
            continue
        g = np.where(valid[s], gain[s], -np.inf).reshape(-1)
        found = bool(valid[s].any())
        f, b = divmod(int(np.argmax(g)), nb)  # the first maximum in (feature, split) order
        rec[s, 0] = f if found else -1.0
        rec[s, 3], rec[s, 4], rec[s, 5] = pimp[s], pn[s], ppred[s]
        rec[s, 10] = float(force_leaf or not found or not gain[s, f, b] > 0.0)
        if kind == CLS:
            rec[s, c0:c0 + W] = tot[s]
        if not found:
            continue
        rec[s, 1], rec[s, 2] = b, gain[s, f, b]
        rec[s, 6], rec[s, 7], rec[s, 8], rec[s, 9] = ln[s, f, b], rn[s, f, b], limp[s, f, b], rimp[s, f, b]
        rec[s, 11] = float(child_leaf or limp[s, f, b] == 0.0)
        rec[s, 12] = float(child_leaf or rimp[s, f, b] == 0.0)
        rec[s, 13], rec[s, 14] = lpred[s, f, b], rpred[s, f, b]
        if kind == CLS:
            rec[s, cl:cl + W], rec[s, cr:cr + W] = left[s, f, b], right[s, f, b]
    return (rec, np.where(valid, gain, -np.inf)) if with_gains else rec


def split_host(H, nsplit, kind: int, impurity: int, e: int, min_rows: int, min_gain: float, force_leaf: bool,
               child_leaf: bool) -> np.ndarray:
    """The twin of ``tree_split_kernel`` on the int64 words."""
    return split_stats(_np(H).astype(np.int64), nsplit, kind, impurity, e, min_rows, min_gain, force_leaf, child_leaf)


def route_host(B, node, tab) -> torch.Tensor:
    """The next level's slot of every row (torch ops on B's device): the twin of ``tree_route_kernel``."""
    t = torch.as_tensor(np.asarray(tab, dtype=np.int64).reshape(-1, 4), device=B.device)
    s = node.to(torch.int64)
    sc = s.clamp(0, t.shape[0] - 1)
    f = t[sc, 0]
    ok = (s >= 0) & (s < t.shape[0]) & (f >= 0)
    b = B[torch.arange(B.shape[0], device=B.device), f.clamp(min=0)].to(torch.int64)
    nxt = torch.where(b <= t[sc, 1], t[sc, 2], t[sc, 3])
    return torch.where(ok, nxt, torch.full_like(nxt, -1)).to(torch.int32)


def predict_host(X, sel, feat, thr, left, right) -> torch.Tensor:
    """int32 leaf index per row, -1 for dead rows (torch ops on X's device): the twin of
    ``tree_predict_kernel``.  ``x <= thr`` goes left, so a NaN goes right."""
    dev, n = X.device, int(X.shape[1])
    fe, lo, hi = (torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev) for a in (feat, left, right))
    th = torch.as_tensor(np.asarray(thr, dtype=np.float64), device=dev)
    i, rows = torch.zeros(n, dtype=torch.int64, device=dev), torch.arange(n, device=dev)
    for _ in range(64):
        f = fe[i]
        inner = f >= 0
        if not bool(inner.any()):
            break
        x = X[f.clamp(min=0), rows].to(torch.float64)
        i = torch.where(inner, torch.where(x <= th[i], lo[i], hi[i]), i)
    if sel is not None:
        i = torch.where(sel.to(torch.bool), i, torch.full_like(i, -1))
    return i.to(torch.int32)


def composite_hist(B, node, y, kind: int, nodes: int, d: int, nb: int, classes: int) -> torch.Tensor:
    """The level's statistics from torch ops in f64 (any shape, host or device): per feature a
    ``bincount`` on the key ``node * nb + bin``.  ``[nodes, d, nb, 3]`` = (count, sum y, sum y^2), or
    ``[nodes, d, nb, classes]`` counts."""
    s = node.to(torch.int64)
    yv = y.to(torch.float64)
    ok = (s >= 0) & (s < nodes) & ((yv >= 0) & (yv < classes) if kind == CLS else torch.isfinite(yv))
    yz = torch.where(ok, yv, torch.zeros_like(yv))
    size = int(nodes) * int(nb)
    cols = ([(yz == c).to(torch.float64) for c in range(int(classes))] if kind == CLS
            else [torch.ones_like(yz), yz, yz * yz])
    out = torch.empty(int(nodes), int(d), int(nb), len(cols), dtype=torch.float64, device=B.device)
    for f in range(int(d)):
        b = B[:, f].to(torch.int64)
        key = torch.where(ok & (b < nb), s * int(nb) + b, torch.full_like(s, size))  # unusable rows: a dropped key
        for k, c in enumerate(cols):
            out[:, f, :, k] = torch.bincount(key, weights=c, minlength=size + 1)[:size].reshape(int(nodes), int(nb))
    return out


# ---- routes and the level loop ---------------------------------------------------------------------
def route(X, kind: int, nb: int, classes: int, e: int = 0) -> str:
    """"fused" (device tensors inside the kernels' range), "composite" (other device tensors) or
    "host" (host tensors: the twins).  Measured (profiles/tree.md: 1 to 1024 open nodes, up to 512
    node groups, 32 and 256 bins, 1e6 and 1e7 rows), the fused level was 3x to over 10000x faster
    than the composite in 41 of 42 cases and 1.17x slower in one: regression, 1e7 rows, 256 open
    nodes in 86 groups (16.7 ms against 14.3).  That band stays fused all the same: the composite
    sums in f64 with float atomics, so among tied splits it may choose another one than the integer
    words do, and a device fit is to grow the CPU engine's tree node for node."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and 1 <= X.shape[0] <= FUSED_MAX_D
          and 1 <= X.shape[1] < 1 << 31 and 1 <= int(nb) <= FUSED_MAX_BINS and -400 <= int(e) <= 400
          and (kind == REG or 1 <= int(classes) <= FUSED_MAX_CLASSES)
          and group_size(kind, X.shape[0], nb, max(int(classes), 1)) >= 1)
    return "fused" if ok else "composite"


@dataclass
class TreeResult:
    """A fitted tree in creation (breadth-first) order; node 0 is the root."""
    kind: int
    feature: np.ndarray       # [m] int32, -1: leaf
    threshold: np.ndarray     # [m] f64
    left: np.ndarray          # [m] int32 index of the children (-1: leaf)
    right: np.ndarray
    gain: np.ndarray          # [m]
    impurity: np.ndarray      # [m]
    count: np.ndarray         # [m] rows
    prediction: np.ndarray    # [m] mean | first maximal class
    class_counts: Optional[np.ndarray]  # [m, classes]
    node_id: np.ndarray       # [m] Spark's numbering
    num_features: int
    num_classes: int
    route: str

    @property
    def depth(self) -> int:
        return int(np.floor(np.log2(self.node_id.max())))


def _first_read(y, live, kind: int):
    """The fit's first host read, summed / maximised over the ranks: ``(live rows of every rank,
    bad-label flag, largest finite |y| or label)``."""
    from ..parallel import comm

    yv = y.to(torch.float64)
    fin = torch.isfinite(yv)
    bad = live & (~fin if kind == REG else (~fin | (yv < 0) | (yv != torch.floor(yv))))
    top = torch.where(live & fin, yv.abs(), torch.zeros_like(yv)).max() if yv.numel() else torch.zeros((), dtype=torch.float64)
    mine = torch.stack([live.sum().to(torch.float64), bad.any().to(torch.float64), top.to(torch.float64)]).cpu().tolist()
    parts = comm.all_gather_object(mine)
    return [int(p[0]) for p in parts], any(p[1] != 0 for p in parts), max(p[2] for p in parts)


def _sample(X, live, counts, max_bins: int, seed: int) -> np.ndarray:
    """The threshold sample ``[m, d]`` (host f64), the same on every rank."""
    from ..parallel import comm
    from .kmeans import row_uniforms

    n, total, cap = int(X.shape[1]), sum(counts), max(int(max_bins) ** 2, 10000)
    keep = live
    if total > cap:
        sizes = comm.all_gather_object(n)
        u = row_uniforms(seed, n, 0, int(sum(sizes[:comm.rank()])), X.device)
        keep = live & (u < cap / total)
    idx = torch.nonzero(keep).reshape(-1)
    rows = X[:, idx].to(torch.float64).t().cpu().numpy().reshape(int(idx.numel()), int(X.shape[0]))
    return np.concatenate(comm.all_gather_object(rows))


def fit(X, y, sel, kind: int, impurity: int, max_depth: int = 5, max_bins: int = 32, min_rows: int = 1,
        min_gain: float = 0.0, seed: int = 0, how: str = "auto", blocks: Optional[int] = None) -> TreeResult:
    """Fit one tree on feature-major ``X`` ``[d, n]`` and labels ``y`` ``[n]``.  ``how``: "auto"
    (:func:`route`) or "fused" / "composite" / "host" to force one (tests, benchmarks; "host" takes
    host tensors only).  Host reads: the label checks and scale first, then the threshold sample,
    then one read of the node records per level.  The NaN-feature flag is set by the binning pass,
    which needs the thresholds, so it cannot come with the first read: it rides with the first
    level's records."""
    from ..parallel import comm
    from . import kernels

    if how not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"tree fit: unknown route {how!r}")
    if how == "host" and X.is_cuda:
        raise ValueError("tree fit: the host route takes host tensors")
    d, n = int(X.shape[0]), int(X.shape[1])
    live = torch.ones(n, dtype=torch.bool, device=X.device) if sel is None else sel.to(torch.bool)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float64)
    y = y.contiguous()
    counts, bad_label, top = _first_read(y, live, kind)
    who = "DecisionTreeClassifier" if kind == CLS else "DecisionTreeRegressor"
    if bad_label:
        raise ValueError(f"{who}: " + ("labels must be integers in [0, numClasses)" if kind == CLS
                                       else "a live row has a NaN or infinite label"))
    if sum(counts) == 0:
        raise ValueError(f"{who}: the input has no rows")
    classes = int(top) + 1 if kind == CLS else 0
    e = int(np.frexp(top)[1]) if kind == REG else 0
    thr, nsplit = pack_splits(find_splits(_sample(X, live, counts, max_bins, seed), max_bins, sum(counts)))
    nb = int(nsplit.max()) + 1
    if how == "auto":
        how = route(X, kind, nb, classes, e)
    if how == "fused" and route(X, kind, nb, classes, e) != "fused":
        raise ValueError("tree fit: the fused passes do not serve this shape")
    if how == "fused":
        B, nan = kernels.tree_bin(X, sel, thr, nsplit, blocks)
    else:
        B, nan = bin_host(X, sel, thr, nsplit)
    node = torch.where(live, 0, -1).to(torch.int32)

    feat, thre, lch, rch, gain, imp, cnt, pred, ids, cc = [-1], [0.0], [-1], [-1], [0.0], [0.0], [0.0], [0.0], [1], [None]
    open_nodes, lvl = [0], 0
    c0, cl, cr, _ = class_offsets(classes)
    while open_nodes:
        k, force, child = len(open_nodes), lvl >= max_depth, lvl + 1 >= max_depth
        if how == "composite":
            H = comm.all_reduce_sum(composite_hist(B, node, y, kind, k, d, nb, classes))
            rec = split_stats(_np(H), nsplit, kind, impurity, e, min_rows, min_gain, force, child)
        else:
            H = comm.all_reduce_sum(kernels.tree_hist(B, node, y, kind, k, d, nb, classes, e, blocks))
            rec = kernels.tree_split(H, nsplit, kind, impurity, e, min_rows, min_gain, force, child)
            if lvl == 0 and torch.is_tensor(rec):  # the NaN flag rides with the first records
                both = torch.cat([rec.reshape(-1), nan.to(torch.float64)]).cpu().numpy()
                rec, nan = both[:-1].reshape(k, RECORD), both[-1:]
            rec = _np(rec)
        if lvl == 0 and any(comm.all_gather_object(bool(_np(nan).any()))):
            raise ValueError(f"{who}: a live row has a NaN feature")
        tab, nxt = np.full((k, 4), -1, dtype=np.int32), []
        for s, i in enumerate(open_nodes):
            r = rec[s]
            imp[i], cnt[i], pred[i] = r[3], r[4], r[5]
            cc[i] = r[c0:c0 + classes].copy() if kind == CLS else None
            if r[10] != 0.0:
                continue
            f, b = int(r[0]), int(r[1])
            feat[i], thre[i], gain[i] = f, float(thr[f, b]), r[2]
            for side, (c_, i_, leaf, p_) in enumerate(((r[6], r[8], r[11], r[13]), (r[7], r[9], r[12], r[14]))):
                j = len(feat)
                feat.append(-1), thre.append(0.0), lch.append(-1), rch.append(-1), gain.append(0.0)
                imp.append(i_), cnt.append(c_), pred.append(p_), ids.append(2 * ids[i] + side)
                cc.append(r[(cl, cr)[side]:(cl, cr)[side] + classes].copy() if kind == CLS else None)
                (lch if side == 0 else rch)[i] = j
                if leaf == 0.0:
                    tab[s, 2 + side] = len(nxt)
                    nxt.append(j)
            tab[s, 0], tab[s, 1] = f, b
        if not nxt:
            break
        node = kernels.tree_route(B, node, tab, blocks) if how == "fused" else route_host(B, node, tab)
        open_nodes, lvl = nxt, lvl + 1
    return TreeResult(kind, np.array(feat, dtype=np.int32), np.array(thre), np.array(lch, dtype=np.int32),
                      np.array(rch, dtype=np.int32), np.array(gain), np.array(imp), np.array(cnt), np.array(pred),
                      np.array(cc) if kind == CLS else None, np.array(ids, dtype=np.int64), d, classes, how)


def predict(X, sel, tree: TreeResult, how: Optional[str] = None) -> torch.Tensor:
    """int32 leaf index per row (-1 for dead rows) on X's device: the fused walk for device tensors it
    serves, the torch walk otherwise."""
    from . import kernels

    fused = (torch.is_tensor(X) and X.is_cuda and X.dtype in (torch.float32, torch.float64)
             and 1 <= X.shape[0] <= FUSED_MAX_D and 1 <= X.shape[1] < 1 << 31)
    if (how or ("fused" if fused else "host")) == "fused":
        return kernels.tree_predict(X, sel, tree.feature, tree.threshold, tree.left, tree.right)
    return predict_host(X, sel, tree.feature, tree.threshold, tree.left, tree.right)
