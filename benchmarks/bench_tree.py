#!/usr/bin/env python3
"""Decision tree: one level's statistics over the binned rows, two ways, in one process:

  fused      the histogram launches of csrc/hip/tree.hip (one per node group) and the split search
  composite  ``ops.tree.composite_hist`` (torch ``bincount`` in f64 per feature) and the host split

for regression (variance) and classification (gini, 4 classes), at d in {8, 32}, ``--bins`` (32) bins, and 1 / 8 /
64 open nodes (the root, a middle level, a level that takes several node groups), at every ``--rows``
size.  Every figure is the median of ``--steps`` separately synchronised steps after ``--warmup``,
with the min and max beside it.  Then the binning pass, the routing pass, the prediction walk and a
whole ``ops.tree.fit`` of depth 5 on both routes.

    python benchmarks/bench_tree.py [--rows 1e6,1e7] [--steps 7] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the host routes at a toy size on the CPU (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_kmeans import median_ms  # noqa: E402
from harness import check_world, emit, world_info  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="1e6,1e7")
    ap.add_argument("--dims", default="8,32")
    ap.add_argument("--opens", default="1,8,64")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--no-fit", action="store_true", help="levels only: skip the whole fits and the walk")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host routes only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels, tree as T
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_tree needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    bins, cases, ok = a.bins, [], True
    for n in rows:
        for d in (int(v) for v in a.dims.split(",")):
            g = torch.Generator(device=dev).manual_seed(77 + d)
            X = torch.rand(d, n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0
            thr, ns = T.pack_splits([np.linspace(-1, 1, bins + 1)[1:-1]] * d)
            base = {"d": d, "rows": n, "bins": bins}
            base["bin"], (B, _) = median_ms(torch, lambda: kernels.tree_bin(X, None, thr, ns), a.steps, a.warmup, dev)
            for kind, imp, classes in ((T.REG, T.VARIANCE, 0), (T.CLS, T.GINI, 4)):
                y = (X[0] > 0.1).to(torch.float64) + (X[d - 1] > -0.3).to(torch.float64) * 2.0
                if kind == T.REG:
                    y = y + 0.25 * X[1 % d].to(torch.float64)
                e = int(np.frexp(float(y.abs().max()))[1])
                for k in (int(v) for v in a.opens.split(",")):
                    node = (torch.arange(n, device=dev) % k).to(torch.int32)
                    case = dict(base, kind="regression" if kind == T.REG else "classification", open=k,
                                groups=-(-k // max(T.group_size(kind, d, bins, classes), 1)))

                    def comp():
                        H = T.composite_hist(B, node, y, kind, k, d, bins, classes)
                        return T.split_stats(H.cpu().numpy(), ns, kind, imp, e, 1, 0.0, False, False)
                    case["composite_level"], ref = median_ms(torch, comp, max(1, a.steps // 2), 1, dev)
                    if on_gpu and T.route(X, kind, bins, classes, e) == "fused":
                        def fused():
                            H = kernels.tree_hist(B, node, y, kind, k, d, bins, classes, e)
                            return kernels.tree_split(H, ns, kind, imp, e, 1, 0.0, False, False).cpu().numpy()
                        case["fused_level"], got = median_ms(torch, fused, a.steps, a.warmup, dev)
                        case["fused_hist"], _ = median_ms(
                            torch, lambda: kernels.tree_hist(B, node, y, kind, k, d, bins, classes, e), a.steps, a.warmup, dev)
                        same = bool((got[:, :2] == ref[:, :2]).all())  # the same (feature, split) per node
                        case["same_splits"], ok = same, ok and same
                        case["gain_max_abs_diff"] = float(np.abs(got[:, 2] - ref[:, 2]).max())
                        case["fused_over_composite"] = case["fused_level"]["median_ms"] / case["composite_level"]["median_ms"]
                        case["fused_hist_gbps"] = (d + 12) * n / case["fused_hist"]["median_ms"] / 1e6
                    print(f"[bench] {case}", file=sys.stderr, flush=True)
                    cases.append(case)
                if a.no_fit:
                    continue
                fit = dict(base, kind="regression" if kind == T.REG else "classification")
                hows = ("host",) if not on_gpu else (("fused", "composite") if T.route(X, kind, bins, classes, e) == "fused"
                                                     else ("composite",))  # (regression beyond d nb = 910 cells: no fused pass)
                for how in hows:
                    fit["fit_depth5_" + how], res = median_ms(
                        torch, lambda: T.fit(X, y, None, kind, imp, 5, bins, how=how), 3, 1, dev)
                fit["nodes"] = int(res.feature.size)
                fit["predict"], _ = median_ms(torch, lambda: T.predict(X, None, res), a.steps, a.warmup, dev)
                print(f"[bench] {fit}", file=sys.stderr, flush=True)
                cases.append(fit)
            del X, B
    head = next((c for c in cases if c["d"] == 32 and c.get("open") == 8 and "fused_level" in c), cases[0])  # classification
    value = (head.get("fused_level") or head["composite_level"])["median_ms"]
    emit({"metric": "ms per tree level (classification, d = 32, 32 bins, 8 open nodes, first --rows size; fused on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform f32 features, step labels)", "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
