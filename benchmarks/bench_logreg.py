#!/usr/bin/env python3
"""LogisticRegression: one loss / gradient evaluation, three ways, in one process:

  fused      the fused pass (csrc/hip/logreg.hip) and its slab sum: ``device._LogregPlan.grad``
  composite  ``ops.logreg.composite_pass`` (torch matmul into a [K, n] margin matrix, log_softmax,
             matmul, all f64)
  floor      the plain fp64 ``gram_stats`` pass over the same X: it reads the same bytes

at d in {8, 32, 64}, K in {binomial, 3, 16, 64}, f32 and f64 features and every ``--rows`` size.
Every figure is the median of ``--steps`` separately synchronised calls after ``--warmup``, with the
min and max beside it (the run-to-run spread that the routing decision of profiles/logreg.md is
read against).  Then one whole fit (``ops.logreg.fit``, regParam 0.1, 20 iterations, tol 0) per
(d, K) at f32, on the fused and the composite route.

    python benchmarks/bench_logreg.py [--rows 1e7] [--steps 7] [--warmup 2]

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
    ap.add_argument("--rows", default="1e7")
    ap.add_argument("--dims", default="8,32,64")
    ap.add_argument("--ks", default="1,3,16,64", help="coefficient rows; 1 = binomial")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--composite-steps", type=int, default=3, help="timed composite evaluations (after one warm-up)")
    ap.add_argument("--fit-iters", type=int, default=20, help="iterations of the timed fit (0: no fit)")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host routes only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels, logreg as L
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_logreg needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    cases, ok = [], True
    for n in rows:
        for d in (int(v) for v in a.dims.split(",")):
            for dt in a.dtypes.split(","):
                dtype = torch.float32 if dt == "f32" else torch.float64
                g = torch.Generator(device=dev).manual_seed(77 + d)
                X = torch.rand(d, n, generator=g, device=dev, dtype=dtype) * 2.0 - 1.0
                floor, _ = median_ms(torch, lambda: kernels.gram_stats(X, X[0].to(torch.float64), None, None, "fp64"),
                                     a.steps, a.warmup, dev)
                for K in (int(v) for v in a.ks.split(",")):
                    rng = np.random.default_rng(K)
                    C = torch.from_numpy(rng.normal(size=(K, d + 1))).to(dev)
                    # labels drawn from the model itself, so the fit below has something to find
                    M = C[:, :d] @ X.to(torch.float64) + C[:, d:]
                    M = torch.cat([torch.zeros_like(M), M]) if K == 1 else M
                    noise = torch.rand(M.shape, generator=g, device=dev, dtype=torch.float64)
                    y = torch.argmax(M - torch.log(-torch.log(noise)), dim=0).to(torch.float64)
                    del M, noise
                    case = {"d": d, "K": K, "dtype": dt, "rows": n, "pass_bytes": X.element_size() * d * n,
                            "floor_gram": floor}
                    case["composite"], ref = median_ms(
                        torch, lambda: L.composite_pass(X, y, None, None, C, L.GRAD), a.composite_steps, 1, dev)
                    if on_gpu:
                        from net.jgp.labs.sparkdq4ml_amd.ops import device

                        plan = device._LogregPlan(X, y, None, None, K)
                        case["fused"], got = median_ms(torch, lambda: plan.grad(C), a.steps, a.warmup, dev)
                        # same statistics, to reordered-sum accuracy, at the size that is timed
                        rel = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
                        case["fused_vs_composite_max_rel"] = rel
                        ok = ok and rel < 1e-9
                        case["fused_gbps"] = case["pass_bytes"] / case["fused"]["median_ms"] / 1e6
                        case["fused_over_composite"] = case["fused"]["median_ms"] / case["composite"]["median_ms"]
                        case["fused_over_floor"] = case["fused"]["median_ms"] / floor["median_ms"]
                        if a.fit_iters and dt == "f32":
                            for how in ("fused", "composite"):
                                case["fit_" + how], _ = median_ms(
                                    torch, lambda: L.fit(X, y, None, None, reg=0.1, max_iter=a.fit_iters, tol=0.0, how=how),
                                    1 if how == "composite" else 3, 1 if how == "fused" else 0, dev)
                    print(f"[bench] {case}", file=sys.stderr, flush=True)
                    cases.append(case)
                    del y
                del X
    head = next((c for c in cases if c["d"] == 32 and c["K"] == 3 and "fused" in c), cases[0])
    value = (head.get("fused") or head["composite"])["median_ms"]
    emit({"metric": "ms per logistic loss / gradient evaluation (d = 32, K = 3, first --rows size and dtype; fused "
                    "route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform features, labels drawn from a random softmax model)", "vs_baseline": None,
          **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
