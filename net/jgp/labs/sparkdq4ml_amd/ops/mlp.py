"""Multilayer perceptron (Spark 2.4 ``ml.classification.MultilayerPerceptronClassifier``): the loss /
gradient pass, its routes and the fit.

The network is ``FeedForwardTopology.multiLayerPerceptron(layers, softmaxOnTop = true)``: every
layer affine, ``z_l = W_l a_{l-1} + b_l``, a sigmoid after the hidden layers, softmax with
cross-entropy on top.  ``weights`` is ONE flat f64 vector in Spark's layout -- per affine layer
``W_l`` column-major as ``numOut x numIn``, then ``b_l`` -- of length ``P = weight_count(layers)``;
the gradient has the same layout, so the optimizer's vector is the model's ``weights``.

One evaluation takes feature-major ``X[d, n]`` and class-index labels.  GRAD gives the flat f64
statistics ``[P gradient (summed over rows, not divided), loss sum, live rows, bad labels]``;
PREDICT gives ``pred[n]`` (f64): the first maximum of the output layer, -1 for dead rows.  A live
row whose label is no integer in ``[0, K)`` counts as a bad label and adds nothing else; dead rows
are selected to zero before any product, so their features and labels may hold NaN.

Three routes compute a pass:

* the fused device pass (``csrc/hip/mlp.hip`` through ``device.mlp_pass``): dense f32 / f64, one or
  two hidden layers, d <= 64, hidden widths and K <= 32, X read by one kernel per evaluation;
* its fp64 twin :func:`mlp_pass_host`: the CPU engine and the kernel tests' oracle;
* the composite :func:`composite_pass`: torch f64 matmuls, any depth and width, on any device --
  shapes outside the fused range, and the benchmark's comparator.

:func:`fit` minimises ``loss / live rows`` with Breeze's L-BFGS (``models/qn_device.minimize``), as
Spark's trainer does through ``mllib.optimization.LBFGS``.  Spark stacks rows into blocks of
``blockSize`` and averages the block means, so a ragged last block weighs its rows more and the
result depends on the partitioning; the plain mean over live rows used here is Spark's value
whenever every block is full.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

__all__ = ["GRAD", "PREDICT", "FUSED_MIN_LAYERS", "FUSED_MAX_LAYERS", "FUSED_MAX_D", "FUSED_MAX_WIDTH", "weight_count",
           "stats_size", "fused_range", "random_weights", "mlp_pass_host", "composite_pass", "route", "predict", "fit",
           "MlpResult"]

GRAD, PREDICT = 0, 1  # codes of csrc/hip/mlp.h
# the fused range: the constants of csrc/hip/mlp.h
FUSED_MIN_LAYERS, FUSED_MAX_LAYERS = 3, 4
FUSED_MAX_D = 64
FUSED_MAX_WIDTH = 32


def _layers(layers) -> list:
    ls = [int(v) for v in layers]
    if len(ls) < 2 or any(v < 1 for v in ls):
        raise ValueError("mlp_pass: layers must have at least 2 positive entries")
    return ls


def weight_count(layers: Sequence[int]) -> int:
    return sum((i + 1) * o for i, o in zip(layers[:-1], layers[1:]))


def stats_size(layers: Sequence[int]) -> int:
    return weight_count(layers) + 3


def fused_range(layers: Sequence[int]) -> bool:
    ls = list(layers)
    return (FUSED_MIN_LAYERS <= len(ls) <= FUSED_MAX_LAYERS and 1 <= ls[0] <= FUSED_MAX_D
            and all(1 <= v <= FUSED_MAX_WIDTH for v in ls[1:]) and ls[-1] >= 2)


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _split(weights, layers, lib=np):
    """``[(W_l [numOut, numIn], b_l [numOut])]`` views of the flat vector."""
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        W = weights[off:off + i * o].reshape(i, o)
        out.append((W.T if lib is np else W.t(), weights[off + i * o:off + (i + 1) * o]))
        off += (i + 1) * o
    return out


def _weights(weights, layers) -> np.ndarray:
    w = np.asarray(_np(weights), dtype=np.float64).reshape(-1)
    if w.size != weight_count(layers):
        raise ValueError(f"mlp_pass: weights must have length {weight_count(layers)} for layers {list(layers)}")
    return w


def random_weights(layers: Sequence[int], seed: int) -> np.ndarray:
    """Spark 2.4's ``AffineLayerModel.randomWeights``: every weight and bias of a layer uniform in
    ``+-2.4 / sqrt(numIn)``, drawn from the project's hash keyed by (seed, index): the same vector on
    the host, the device and every rank (Spark's distribution, not its bits)."""
    from .kmeans import row_hashes

    P = weight_count(layers)
    u = (row_hashes(int(seed), P).numpy().astype(np.float64) + 0.5) / 4294967296.0
    bound = np.concatenate([np.full((i + 1) * o, 2.4 / np.sqrt(i)) for i, o in zip(layers[:-1], layers[1:])])
    return (2.0 * u - 1.0) * bound


def mlp_pass_host(X, y, sel, weights, layers, mode: int, absolute: bool = False):
    """The fp64 twin of the fused device pass on host data (numpy; torch f64 results).
    ``absolute`` (GRAD): every statistic as the sum of its absolute per-row terms, ``|delta_l[u]|
    |a_{l-1}[j]|``, ``|delta_l[u]|`` and ``|row loss|`` -- the scale of the kernel tests' bound."""
    layers = _layers(layers)
    Xd = _np(X).astype(np.float64)
    d, n = Xd.shape
    if d != layers[0]:
        raise ValueError("mlp_pass: the feature width must equal layers[0]")
    w = _weights(weights, layers)
    K = layers[-1]
    live = np.ones(n, dtype=bool) if sel is None else _np(sel).astype(bool)
    if live.shape != (n,):
        raise ValueError("mlp_pass: row-count mismatch between features and selection")
    if mode not in (GRAD, PREDICT):
        raise ValueError("mlp_pass: mode must be GRAD (0) or PREDICT (1)")
    with np.errstate(all="ignore"):
        if mode == GRAD:
            yv = _np(y).astype(np.float64)
            ok = live & (yv >= 0) & (yv < K) & (yv == np.floor(yv))
            yi = np.where(ok, yv, 0).astype(np.int64)
        else:
            ok = live
        acts = [np.where(ok[None, :], Xd, 0.0)]
        wb = _split(w, layers)
        for W, b in wb[:-1]:
            z = W @ acts[-1] + b[:, None]
            t = np.exp(-np.abs(z))
            acts.append(np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t)))
        W, b = wb[-1]
        z = W @ acts[-1] + b[:, None]
        if mode == PREDICT:
            return torch.from_numpy(np.where(live, np.argmax(z, axis=0).astype(np.float64), -1.0))
        mx = z.max(axis=0)
        e = np.exp(z - mx)
        sm = e.sum(axis=0)
        cols = np.arange(n)
        mag = np.abs if absolute else (lambda v: v)
        loss = mag(np.where(ok, mx + np.log(sm) - z[yi, cols], 0.0)).sum()
        delta = e / sm
        delta[yi, cols] -= 1.0
        delta = np.where(ok[None, :], delta, 0.0)
        out = np.empty(stats_size(layers))
        off = weight_count(layers)
        out[off:] = loss, live.sum(), (live & ~ok).sum()
        for l in range(len(wb) - 1, -1, -1):
            i, o = layers[l], layers[l + 1]
            off -= (i + 1) * o
            out[off:off + i * o] = (mag(acts[l]) @ mag(delta).T).reshape(-1)  # [numIn, numOut] row-major = W column-major
            out[off + i * o:off + (i + 1) * o] = mag(delta).sum(axis=1)
            if l > 0:
                delta = (wb[l][0].T @ delta) * (acts[l] * (1.0 - acts[l]))
    return torch.from_numpy(out)


def composite_pass(X, y, sel, weights, layers, mode: int):
    """The same pass from torch ops in f64 (any depth and width, host or device): ``[h, n]``
    activations and deltas per layer; the backward pass is three lines per layer, no autograd."""
    layers = _layers(layers)
    Xd = X.to(torch.float64)
    d, n = Xd.shape
    dev = Xd.device
    if d != layers[0]:
        raise ValueError("mlp_pass: the feature width must equal layers[0]")
    w = (weights if torch.is_tensor(weights) else torch.as_tensor(_weights(weights, layers))).to(device=dev, dtype=torch.float64)
    if w.numel() != weight_count(layers):
        raise ValueError(f"mlp_pass: weights must have length {weight_count(layers)} for layers {layers}")
    K = layers[-1]
    live = torch.ones(n, dtype=torch.bool, device=dev) if sel is None else sel.to(torch.bool)
    if mode == GRAD:
        yv = y.to(torch.float64)
        ok = live & (yv >= 0) & (yv < K) & (yv == torch.floor(yv))
        yi = torch.where(ok, yv, torch.zeros_like(yv)).to(torch.long)
    else:
        ok = live
    acts = [torch.where(ok[None, :], Xd, torch.zeros_like(Xd))]
    wb = _split(w.reshape(-1), layers, torch)
    for W, b in wb[:-1]:
        acts.append(torch.sigmoid(torch.addmm(b[:, None], W, acts[-1])))
    W, b = wb[-1]
    z = torch.addmm(b[:, None], W, acts[-1])
    if mode == PREDICT:
        pred = torch.argmax(z, dim=0).to(torch.float64)
        return torch.where(live, pred, torch.full_like(pred, -1.0))
    lp = torch.log_softmax(z, dim=0)
    cols = torch.arange(n, device=dev)
    okf = ok.to(torch.float64)
    loss = -(okf * lp[yi, cols]).sum()
    delta = lp.exp()
    delta[yi, cols] -= 1.0
    delta = delta * okf[None, :]
    parts = []
    for l in range(len(wb) - 1, -1, -1):
        parts.append(torch.cat([(acts[l] @ delta.t()).reshape(-1), delta.sum(dim=1)]))
        if l > 0:
            delta = (wb[l][0].t() @ delta) * (acts[l] * (1.0 - acts[l]))
    tail = torch.stack([loss, live.sum().to(torch.float64), (live & ~ok).sum().to(torch.float64)])
    return torch.cat(parts[::-1] + [tail])


def route(X, layers) -> str:
    """"fused" (device tensors inside the kernel's range), "composite" (other device tensors) or
    "host" (host tensors: the twin).  See profiles/mlp.md for what stands behind the fused default."""
    if not (torch.is_tensor(X) and X.is_cuda):
        return "host"
    ok = (X.dim() == 2 and X.dtype in (torch.float32, torch.float64) and X.shape[1] >= 1
          and fused_range([int(v) for v in layers]) and int(layers[0]) == X.shape[0])
    return "fused" if ok else "composite"


def _pass(X, y, sel, weights, layers, mode: int, how: str):
    if how == "composite":
        return composite_pass(X, y, sel, weights, layers, mode)
    if how == "host":
        return mlp_pass_host(X, y, sel, weights, layers, mode)
    from . import device

    return device.mlp_pass(X, y, sel, weights, layers, mode)


def predict(X, sel, weights, layers, how: Optional[str] = None):
    """``pred[n]`` on X's device, by the route of (X, layers)."""
    return _pass(X, None, sel, weights, layers, PREDICT, how or route(X, layers))


# ---- the fit -----------------------------------------------------------------------------------------
@dataclass
class MlpResult:
    weights: np.ndarray  # [P], Spark's layout
    layers: list
    objective_history: list
    route: str


def fit(X, y, sel, layers, max_iter: int = 100, tol: float = 1e-6, seed: int = 0, initial_weights=None,
        how: str = "auto") -> MlpResult:
    """Fit on feature-major ``X`` ``[d, n]`` with class-index labels ``y`` from ``initial_weights``
    (default: :func:`random_weights` of ``seed``).  ``how``: "auto" (:func:`route`) or "fused" /
    "composite" / "host" to force one (tests, benchmarks)."""
    from ..models.qn_device import minimize
    from ..parallel import comm

    if how not in ("auto", "fused", "composite", "host"):
        raise ValueError(f"mlp fit: unknown route {how!r}")
    layers = _layers(layers)
    if int(X.shape[0]) != layers[0]:
        raise ValueError(f"MultilayerPerceptronClassifier: the feature width {int(X.shape[0])} must equal layers[0] = {layers[0]}")
    P = weight_count(layers)
    x0 = random_weights(layers, seed) if initial_weights is None else _weights(initial_weights, layers)
    if how == "auto":
        how = route(X, layers)
    dev = X.device
    plan, first = None, [True]
    if how == "fused":
        from . import device

        plan = device._MlpPlan(X, y, sel, layers)

    def fg(x):
        stats = plan.grad(x) if plan is not None else _pass(X, y, sel, x, layers, GRAD, how)
        stats = comm.all_reduce_sum(stats.to(dev))
        if first[0]:
            first[0] = False
            if float(stats[P + 2]) != 0.0:
                raise ValueError(f"MultilayerPerceptronClassifier: {int(stats[P + 2])} labels are no class index in [0, {layers[-1]})")
            if float(stats[P + 1]) <= 0.0:
                raise ValueError("MultilayerPerceptronClassifier: the input has no rows")
        live = stats[P + 1]
        return stats[P] / live, stats[:P] / live

    x, hist, _ = minimize(fg, torch.from_numpy(x0.copy()).to(dev), int(max_iter), float(tol))
    return MlpResult(x.cpu().numpy(), layers, [float(v) for v in hist], how)
