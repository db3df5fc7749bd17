#!/usr/bin/env python3
"""Random forest: one level's histogram of all trees over the binned rows, two ways, in one process:

  forest    the launches of ``forest_hist`` (csrc/hip/forest.hip): every tree's open slots together, m
            features per slot, one launch per slot group
  per_tree  ``numTrees`` times the launches of ``tree_hist`` (csrc/hip/tree.hip) on the same bins, each
            tree's slots alone over all d features: what growing the forest tree by tree costs

for regression (m = ceil(d / 3)) and classification (m = ceil(sqrt d), 4 classes), at d in ``--dims``,
``--bins`` bins, ``--trees`` trees and ``--opens`` open nodes per tree (the root, a deep level), at every
``--rows`` size.  The per-tree path ignores the bag counts, so it does no more work per row than the
forest pass.  Every figure is the median of ``--steps`` separately synchronised steps after
``--warmup``, with the min and max beside it.  Then the bagging pass, the routing pass, a whole
``ops.forest.fit`` of depth 5 and the forest walk.

    python benchmarks/bench_forest.py [--rows 1e6,1e7] [--steps 7] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the twins at a toy size on the CPU (no rate is a measurement
there).
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
    ap.add_argument("--opens", default="1,16")
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--no-fit", action="store_true", help="levels only: skip the whole fit and the walk")
    ap.add_argument("--rehearse", action="store_true", help="toy size, twins only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import forest as F, kernels, tree as T
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_forest needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [3000]
    bins, trees, cases, ok = a.bins, a.trees, [], True
    for n in rows:
        for d in (int(v) for v in a.dims.split(",")):
            g = torch.Generator(device=dev).manual_seed(77 + d)
            X = torch.rand(d, n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0
            thr, ns = T.pack_splits([np.linspace(-1, 1, bins + 1)[1:-1]] * d)
            B, _ = kernels.tree_bin(X, None, thr, ns)
            base = {"d": d, "rows": n, "bins": bins, "trees": trees}
            seeds, rule = F.tree_seeds(1, trees), F.bag_thresholds(trees, 1.0)
            base["bag"], roots = median_ms(torch, lambda: kernels.forest_bag(n, 0, None, seeds, rule, dev), a.steps, a.warmup, dev)
            for kind, imp, classes in ((T.REG, T.VARIANCE, 0), (T.CLS, T.GINI, 4)):
                y = (X[0] > 0.1).to(torch.float64) + (X[d - 1] > -0.3).to(torch.float64) * 2.0
                if kind == T.REG:
                    y = y + 0.25 * X[1 % d].to(torch.float64)
                e = int(np.frexp(float(y.abs().max()))[1])
                m = F.features_per_node("auto", d, kind, trees)
                for k in (int(v) for v in a.opens.split(",")):
                    spread = (torch.arange(n, device=dev) % k).to(torch.int32)[None, :]
                    node = torch.where(roots >= 0, (roots & ~F.SLOT_MASK) | ((roots & F.SLOT_MASK) * k + spread), roots).contiguous()
                    slot_tree = np.repeat(np.arange(trees), k)
                    feats = [F.node_subset(1, int(t), 1 + s, d, m) for s, t in enumerate(slot_tree)]
                    masks = [F._mask(f) for f in feats]
                    case = dict(base, kind="regression" if kind == T.REG else "classification", m=m, open_per_tree=k,
                                forest_groups=-(-k * trees // max(F.group_size(kind, m, bins, classes), 1)),
                                per_tree_groups=trees * -(-k // max(T.group_size(kind, d, bins, classes), 1)))
                    hist = lambda: kernels.forest_hist(B, node, y, kind, d, m, bins, classes, e, masks, slot_tree)  # noqa: E731
                    case["forest_hist"], H = median_ms(torch, hist, a.steps, a.warmup, dev)
                    if on_gpu and T.route(X, kind, bins, classes, e) == "fused":
                        own = [torch.where(node[t] >= 0, (node[t] & F.SLOT_MASK) - t * k, node[t]).contiguous() for t in range(trees)]
                        per = lambda: [kernels.tree_hist(B, own[t], y, kind, k, d, bins, classes, e) for t in range(trees)]  # noqa: E731
                        case["per_tree_hist"], _ = median_ms(torch, per, a.steps, a.warmup, dev)
                        case["forest_over_per_tree"] = case["forest_hist"]["median_ms"] / case["per_tree_hist"]["median_ms"]
                    rec = kernels.forest_split(H, np.stack(feats), ns, kind, imp, e, 1, 0.0, False, False)
                    rec = rec.cpu().numpy() if torch.is_tensor(rec) else rec
                    tab = np.stack([rec[:, 0], rec[:, 1], np.arange(len(masks)), np.arange(len(masks))], axis=1).astype(np.int32)
                    case["route"], _ = median_ms(torch, lambda: kernels.forest_route(B, node.clone(), tab), a.steps, a.warmup, dev)
                    sane = bool((rec[:, 4] > 0).all())
                    case["sane"], ok = sane, ok and sane
                    print(f"[bench] {case}", file=sys.stderr, flush=True)
                    cases.append(case)
                if a.no_fit:
                    continue
                fit = dict(base, kind="regression" if kind == T.REG else "classification", m=m)
                fit["fit_depth5"], res = median_ms(torch, lambda: F.fit(X, y, None, kind, imp, trees, "auto", 1.0, 5, bins), 3, 1, dev)
                fit["nodes"] = int(sum(t.feature.size for t in res))
                tabs = F.tables(res)
                fit["predict"], _ = median_ms(torch, lambda: F.predict(X, None, tabs), a.steps, a.warmup, dev)
                print(f"[bench] {fit}", file=sys.stderr, flush=True)
                cases.append(fit)
            del X, B
    head = next((c for c in cases if c["d"] == 32 and c.get("open_per_tree") == 1 and c["kind"] == "classification"), cases[0])
    value = head["forest_hist"]["median_ms"]
    emit({"metric": "ms per forest root level (classification, d = 32, 32 bins, 20 trees, first --rows size)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform f32 features, step labels)", "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
