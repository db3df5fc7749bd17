"""Random forests (Spark 2.4 ``RandomForest.run`` with ``numTrees`` trees, bagging and per-node feature
subsets; continuous features only): the bag rule, the subsets, the level passes and the level loop.

Thresholds and bins are those of one tree (``ops/tree.py``).  Every tree then keeps one int32 *node
word* per row, ``node[T, n]``: -1 (dead, outside the tree's bag, or in a leaf), else ``(c << 24) |
slot`` with c the row's bag count in that tree and slot the number of its open node in the level.
The slots of a level are numbered tree-major over all trees, so one histogram pass serves the open
nodes of every tree: ``H[slots, m, nb, W]`` holds, for the m features of the slot's subset in
ascending order, ``c x`` the label words of ``ops/tree.py`` (integers: the histogram depends on
neither grid, schedule, slot group nor shard split).  The split search is the tree's, told which
feature sits at which position; counts, and with them ``minInstancesPerNode``, are bag-weighted as
in Spark.  The sums are exact while a tree's bag holds fewer than 2^31 rows (counts included).

Seeded choices are pure functions, not RNG streams, so host, device and data-parallel fits grow
the same forest; they agree with Spark's in distribution, not bit for bit:

* the bag count of (tree t, global row g) is the number of thresholds of :func:`bag_thresholds`
  that ``fold_hash(fold_seed(seed + 1 + t, 0), g)`` reaches -- the Poisson(``subsamplingRate``) CDF
  for a forest, one Bernoulli threshold for a single tree below rate 1, else the constant 1;
* the subset of (tree t, Spark node id i) is the m features with the smallest ``(fold_hash(fold_seed(
  seed, t + 1), 64 i + f), f)``.

Two routes run a level: the fused device passes (``csrc/hip/forest.hip`` through ``ops/device.py``: the
range of ``tree.route`` with a slot's m nb W cells and its mask inside the block's 64 KiB of LDS)
and their twins here for the CPU engine.  There is no composite route: its float-atomic sums could
break ties differently from the integer words.
"""
from __future__ import annotations

import math
import re
from typing import List, Optional

import numpy as np
import torch

from . import tree as T
from .tree import CLS, REG, TreeResult

__all__ = ["COUNT_SHIFT", "SLOT_MASK", "bag_thresholds", "tree_seeds", "features_per_node", "node_subset", "group_size",
           "bag_host", "hist_host", "split_host", "route_host", "predict_host", "route", "fit", "tables", "predict"]

COUNT_SHIFT, SLOT_MASK, MAX_COUNT = 24, (1 << 24) - 1, 15  # csrc/hip/forest.h


# ---- the seeded rules --------------------------------------------------------------------------------
def bag_thresholds(num_trees: int, rate: float) -> np.ndarray:
    """The uint32 thresholds of the bag rule (at most 15, ascending): a row's count is the number of
    them that its hash reaches.  Entries that would reach 2^32 are left out."""
    if not (int(num_trees) >= 1 and 0.0 < float(rate) <= 1.0):
        raise ValueError("bag rule: needs numTrees >= 1 and subsamplingRate in (0, 1]")
    if int(num_trees) > 1:    # P(c > j) = 1 - CDF(j) of Poisson(rate)
        terms = [math.exp(-rate) * rate ** i / math.factorial(i) for i in range(MAX_COUNT)]
        cut = [math.floor(math.fsum(terms[:j + 1]) * 4294967296.0) for j in range(MAX_COUNT)]
    elif rate < 1.0:          # P(c = 1) = rate
        cut = [math.floor((1.0 - rate) * 4294967296.0)]
    else:
        cut = [0]
    return np.array([c for c in cut if c < 1 << 32], dtype=np.uint32)


def tree_seeds(seed: int, num_trees: int) -> np.ndarray:
    from . import kernels

    return np.array([kernels.fold_seed(int(seed) + 1 + t, 0) for t in range(int(num_trees))], dtype=np.uint64)


def features_per_node(strategy, d: int, kind: int, num_trees: int) -> int:
    """Spark 2.4's ``featureSubsetStrategy``: "auto" (all for one tree, "sqrt" for classification,
    "onethird" for regression), "all", "sqrt", "log2", "onethird", an integer in [1, d] or a fraction
    in (0, 1]."""
    d, s = int(d), str(strategy).strip().lower()
    if s == "auto":
        s = "all" if int(num_trees) == 1 else ("sqrt" if kind == CLS else "onethird")
    if s == "all":
        return d
    if s == "sqrt":
        r = math.isqrt(d)
        return r if r * r == d else r + 1
    if s == "log2":
        return max(1, (d - 1).bit_length())
    if s == "onethird":
        return (d + 2) // 3
    if re.fullmatch(r"[0-9]+", s):
        if 1 <= int(s) <= d:
            return int(s)
    else:
        try:
            f = float(s)
        except ValueError:
            f = 0.0
        if 0.0 < f <= 1.0:
            return max(1, min(d, math.ceil(f * d)))
    raise ValueError(f"featureSubsetStrategy: unsupported value {strategy!r} for {d} features")


def node_subset(seed: int, tree: int, node_id: int, d: int, m: int) -> np.ndarray:
    """The ascending int32 features of (tree, Spark node id): the m smallest ``(hash, f)``."""
    from . import kernels

    f = np.arange(int(d), dtype=np.uint64)
    if int(m) >= int(d):
        return f.astype(np.int32)
    key = kernels.fold_hash(kernels.fold_seed(int(seed), int(tree) + 1), np.uint64(64 * int(node_id)) + f)
    return np.sort(np.lexsort((f, key))[:int(m)]).astype(np.int32)


def _mask(feats) -> int:
    return sum(1 << int(f) for f in feats)


def group_size(kind: int, m: int, nb: int, classes: int) -> int:
    """Slots whose cells and masks fit one block's LDS (``forest_group`` of csrc/hip/forest.h)."""
    return T.LDS_BYTES // (int(m) * int(nb) * T.words(kind, classes) * (4 if kind == CLS else 8) + 8)


# ---- the twins ---------------------------------------------------------------------------------------
def bag_host(n: int, row_offset: int, sel, seeds, thr) -> torch.Tensor:
    """int32 node words ``[trees, n]`` of the bagged roots: the twin of ``forest_bag_kernel``."""
    from . import kernels

    live = np.ones(int(n), dtype=bool) if sel is None else T._np(sel).astype(bool)
    g = np.arange(int(n), dtype=np.uint64) + np.uint64(int(row_offset))
    th = np.asarray(thr, dtype=np.uint32)
    out = np.full((len(seeds), int(n)), -1, dtype=np.int32)
    for t, s in enumerate(seeds):
        c = np.searchsorted(th, kernels.fold_hash(int(s), g), side="right").astype(np.int32)  # = #{j : u >= thr_j}
        out[t] = np.where(live & (c >= 1), (c << COUNT_SHIFT) | t, -1)
    return torch.from_numpy(out)


def hist_host(B, node, y, kind: int, d: int, m: int, nb: int, classes: int, e: int, masks) -> torch.Tensor:
    """The int64 histogram ``[slots, m, nb, W]``: the twin of ``forest_hist_kernel`` (the same words)."""
    Bn, words = T._np(B), T._np(node).astype(np.int64)
    mk = [int(v) for v in np.asarray(masks, dtype=np.uint64).reshape(-1)]
    w, ok = T.row_words(y, kind, classes, e)
    H = np.zeros((len(mk), int(m), int(nb), w.shape[1]), dtype=np.int64)
    below = np.array([[bin(v & ((1 << f) - 1)).count("1") for f in range(int(d))] for v in mk], dtype=np.int64)
    has = np.array([[(v >> f) & 1 for f in range(int(d))] for v in mk], dtype=bool)
    for word in words:
        s, c = word & SLOT_MASK, word >> COUNT_SHIFT
        hit = ok & (word >= 0) & (s < len(mk))
        sc = np.where(hit, s, 0)
        for f in range(int(d)):
            r = hit & has[sc, f] & (Bn[:, f] < nb) & (below[sc, f] < m)
            np.add.at(H, (sc[r], below[sc[r], f], Bn[r, f].astype(np.int64)), w[r] * c[r, None])
    return torch.from_numpy(H)


def split_host(H, feats, nsplit, kind: int, impurity: int, e: int, min_rows: int, min_gain: float, force_leaf: bool,
               child_leaf: bool, with_gains: bool = False):
    """The twin of ``tree_split_kernel`` given ``feats`` ``[slots, m]``: the tree's split statistics of
    each slot over its own features' split counts, the record naming the real feature."""
    Hn, fs, ns = T._np(H).astype(np.int64), np.asarray(feats, dtype=np.int64), np.asarray(nsplit, dtype=np.int64)
    recs, gains = [], []
    for s in range(Hn.shape[0]):
        rec, g = T.split_stats(Hn[s:s + 1], ns[fs[s]], kind, impurity, e, min_rows, min_gain, force_leaf, child_leaf, True)
        if rec[0, 0] >= 0:
            rec[0, 0] = fs[s, int(rec[0, 0])]
        recs.append(rec[0]), gains.append(g[0])
    return (np.stack(recs), np.stack(gains)) if with_gains else np.stack(recs)


def route_host(B, node, tab) -> torch.Tensor:
    """The next level's words ``[trees, n]``: the twin of ``forest_route_kernel`` (count bits kept)."""
    out = torch.empty_like(node)
    for t in range(node.shape[0]):
        word = node[t]
        nxt = T.route_host(B, torch.where(word >= 0, word & SLOT_MASK, word), tab)
        out[t] = torch.where((word >= 0) & (nxt >= 0), (word & ~SLOT_MASK) | nxt, torch.full_like(nxt, -1))
    return out


def predict_host(X, sel, feat, thr, left, right, root, val) -> torch.Tensor:
    """f64 ``[C, n]``, per row the leaf values of the trees added in tree order, NaN for dead rows
    (torch ops on X's device): the twin of ``forest_predict_kernel``."""
    dev, n = X.device, int(X.shape[1])
    fe, lo, hi = (torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev) for a in (feat, left, right))
    th = torch.as_tensor(np.asarray(thr, dtype=np.float64), device=dev)
    v = torch.as_tensor(np.asarray(val, dtype=np.float64), device=dev)
    rows, out = torch.arange(n, device=dev), torch.zeros(n, v.shape[1], dtype=torch.float64, device=dev)
    for r0 in np.asarray(root, dtype=np.int64).reshape(-1):
        i = torch.full((n,), int(r0), dtype=torch.int64, device=dev)
        for _ in range(64):
            f = fe[i]
            inner = f >= 0
            if not bool(inner.any()):
                break
            x = X[f.clamp(min=0), rows].to(torch.float64)
            i = torch.where(inner, torch.where(x <= th[i], lo[i], hi[i]), i)
        out = out + v[i]
    if sel is not None:
        out = torch.where(sel.to(torch.bool)[:, None], out, torch.full_like(out, float("nan")))
    return out.t().contiguous()


# ---- routes and the level loop ---------------------------------------------------------------------
def route(X, kind: int, nb: int, classes: int, e: int, m: int) -> str:
    """"fused" (device tensors inside the kernels' range) or "host" (host tensors: the twins).  Other
    device tensors raise: a forest has no composite route."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and 1 <= X.shape[0] <= T.FUSED_MAX_D
          and 1 <= X.shape[1] < 1 << 31 and 1 <= int(nb) <= T.FUSED_MAX_BINS and -400 <= int(e) <= 400
          and (kind == REG or 1 <= int(classes) <= T.FUSED_MAX_CLASSES) and 1 <= int(m) <= X.shape[0]
          and group_size(kind, m, nb, max(int(classes), 1)) >= 1)
    if not ok:
        raise NotImplementedError(
            "random forest: the device passes serve dense f32 / f64 features with d <= 64, at most 256 bins and 16 classes "
            "and one node's subset cells inside 64 KiB of LDS; there is no composite route for forests")
    return "fused"


class _Grow:
    """One tree's nodes in creation order while the level loop runs."""

    def __init__(self):
        self.feat, self.thr, self.left, self.right, self.gain = [-1], [0.0], [-1], [-1], [0.0]
        self.imp, self.cnt, self.pred, self.ids, self.cc = [0.0], [0.0], [0.0], [1], [None]

    def add(self, imp, cnt, pred, node_id, cc) -> int:
        for lst, v in ((self.feat, -1), (self.thr, 0.0), (self.left, -1), (self.right, -1), (self.gain, 0.0), (self.imp, imp),
                       (self.cnt, cnt), (self.pred, pred), (self.ids, node_id), (self.cc, cc)):
            lst.append(v)
        return len(self.feat) - 1

    def result(self, kind, d, classes, how) -> TreeResult:
        return TreeResult(kind, np.array(self.feat, dtype=np.int32), np.array(self.thr), np.array(self.left, dtype=np.int32),
                          np.array(self.right, dtype=np.int32), np.array(self.gain), np.array(self.imp), np.array(self.cnt),
                          np.array(self.pred), np.array(self.cc) if kind == CLS else None,
                          np.array(self.ids, dtype=np.int64), d, classes, how)


def fit(X, y, sel, kind: int, impurity: int, num_trees: int = 20, strategy="auto", rate: float = 1.0, max_depth: int = 5,
        max_bins: int = 32, min_rows: int = 1, min_gain: float = 0.0, seed: int = 0, how: str = "auto",
        blocks: Optional[int] = None, group: Optional[int] = None) -> List[TreeResult]:
    """Fit ``num_trees`` trees on feature-major ``X`` ``[d, n]`` and labels ``y`` ``[n]``.  ``how``: "auto"
    (:func:`route`), "fused" or "host" ("host" takes host tensors only).  Host reads are those of
    ``tree.fit``: the label checks and scale, the threshold sample, then one read of the records of
    all trees per level (the NaN-feature flag rides with the first)."""
    from ..parallel import comm
    from . import kernels

    if how not in ("auto", "fused", "host"):
        raise ValueError(f"forest fit: unknown route {how!r}")
    if how == "host" and X.is_cuda:
        raise ValueError("forest fit: the host route takes host tensors")
    d, n, trees = int(X.shape[0]), int(X.shape[1]), int(num_trees)
    live = torch.ones(n, dtype=torch.bool, device=X.device) if sel is None else sel.to(torch.bool)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float64)
    y = y.contiguous()
    counts, bad_label, top = T._first_read(y, live, kind)
    who = "RandomForestClassifier" if kind == CLS else "RandomForestRegressor"
    if bad_label:
        raise ValueError(f"{who}: " + ("labels must be integers in [0, numClasses)" if kind == CLS
                                       else "a live row has a NaN or infinite label"))
    if sum(counts) == 0:
        raise ValueError(f"{who}: the input has no rows")
    classes = int(top) + 1 if kind == CLS else 0
    e = int(np.frexp(top)[1]) if kind == REG else 0
    m = features_per_node(strategy, d, kind, trees)
    thr, nsplit = T.pack_splits(T.find_splits(T._sample(X, live, counts, max_bins, seed), max_bins, sum(counts)))
    nb = int(nsplit.max()) + 1
    fused = route(X, kind, nb, classes, e, m) == "fused"
    if how == "fused" and not fused:
        raise ValueError("forest fit: the fused passes take device tensors")
    how = "fused" if fused else "host"
    B, nan = kernels.tree_bin(X, sel, thr, nsplit, blocks) if fused else T.bin_host(X, sel, thr, nsplit)
    sizes = comm.all_gather_object(n)
    node = kernels.forest_bag(n, int(sum(sizes[:comm.rank()])), live, tree_seeds(seed, trees), bag_thresholds(trees, rate),
                              X.device, blocks)

    grow = [_Grow() for _ in range(trees)]
    open_nodes, lvl = [(t, 0) for t in range(trees)], 0  # tree-major: a slot's number is its index here
    c0, cl, cr, _ = T.class_offsets(classes)
    while open_nodes:
        k, force, child = len(open_nodes), lvl >= max_depth, lvl + 1 >= max_depth
        if k > SLOT_MASK:
            raise ValueError(f"{who}: more than 2^24 open nodes in one level")
        feats = np.stack([node_subset(seed, t, grow[t].ids[i], d, m) for t, i in open_nodes])
        H = comm.all_reduce_sum(kernels.forest_hist(B, node, y, kind, d, m, nb, classes, e, [_mask(f) for f in feats],
                                                    [t for t, _ in open_nodes], blocks, group))
        rec = kernels.forest_split(H, feats, nsplit, kind, impurity, e, min_rows, min_gain, force, child)
        if lvl == 0 and torch.is_tensor(rec):  # the NaN flag rides with the first records
            both = torch.cat([rec.reshape(-1), nan.to(torch.float64)]).cpu().numpy()
            rec, nan = both[:-1].reshape(k, T.RECORD), both[-1:]
        rec = T._np(rec)
        if lvl == 0 and any(comm.all_gather_object(bool(T._np(nan).any()))):
            raise ValueError(f"{who}: a live row has a NaN feature")
        tab, nxt = np.full((k, 4), -1, dtype=np.int32), []
        for s, (t, i) in enumerate(open_nodes):
            r, g = rec[s], grow[t]
            g.imp[i], g.cnt[i], g.pred[i] = r[3], r[4], r[5]
            g.cc[i] = r[c0:c0 + classes].copy() if kind == CLS else None
            if r[10] != 0.0:
                continue
            f, b = int(r[0]), int(r[1])
            g.feat[i], g.thr[i], g.gain[i] = f, float(thr[f, b]), r[2]
            for side, (c_, i_, leaf, p_) in enumerate(((r[6], r[8], r[11], r[13]), (r[7], r[9], r[12], r[14]))):
                o = (cl, cr)[side]
                j = g.add(i_, c_, p_, 2 * g.ids[i] + side, r[o:o + classes].copy() if kind == CLS else None)
                (g.left if side == 0 else g.right)[i] = j
                if leaf == 0.0:
                    tab[s, 2 + side] = len(nxt)
                    nxt.append((t, j))
            tab[s, 0], tab[s, 1] = f, b
        if not nxt:
            break
        node = kernels.forest_route(B, node, tab, blocks)
        open_nodes, lvl = nxt, lvl + 1
    return [g.result(kind, d, classes, how) for g in grow]


def tables(trees: List[TreeResult]):
    """``(feat, thr, left, right, root, val)`` of the concatenated trees for the forest walk: ``val`` is
    ``[nodes, 1]`` means, or ``[nodes, classes]`` class counts over their sum (the division is done
    here, once)."""
    off = np.cumsum([0] + [t.feature.size for t in trees])
    shift = lambda a, o: np.where(a >= 0, a + o, -1).astype(np.int32)  # noqa: E731
    if trees[0].kind == CLS:
        cc = np.concatenate([np.asarray(t.class_counts, dtype=np.float64) for t in trees])
        tot = cc.sum(axis=1, keepdims=True)
        val = np.divide(cc, tot, out=np.zeros_like(cc), where=tot > 0)
    else:
        val = np.concatenate([t.prediction for t in trees]).astype(np.float64)[:, None]
    return (np.concatenate([t.feature for t in trees]).astype(np.int32), np.concatenate([t.threshold for t in trees]),
            np.concatenate([shift(t.left, o) for t, o in zip(trees, off)]),
            np.concatenate([shift(t.right, o) for t, o in zip(trees, off)]), off[:-1].astype(np.int32), val)


def predict(X, sel, tabs) -> torch.Tensor:
    """f64 ``[C, n]`` sums over the trees of :func:`tables` on X's device: the fused walk for device
    tensors, the twin for host tensors."""
    from . import kernels

    if torch.is_tensor(X) and X.is_cuda and not (X.dtype in (torch.float32, torch.float64) and 1 <= X.shape[0] <= T.FUSED_MAX_D
                                                 and 1 <= X.shape[1] < 1 << 31 and tabs[5].shape[1] <= T.FUSED_MAX_CLASSES):
        raise NotImplementedError("random forest: the device walk serves dense f32 / f64 features with d <= 64 and at most "
                                  "16 classes")
    return kernels.forest_predict(X, sel, *tabs)
