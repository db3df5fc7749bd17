#!/usr/bin/env python3
"""MultilayerPerceptronClassifier: one loss / gradient evaluation, three ways, in one process:

  fused      the fused pass (csrc/hip/mlp.hip) and its slab sum: ``device._MlpPlan.grad``
  composite  ``ops.mlp.composite_pass`` (torch f64 matmuls into [h, n] activations and deltas)
  floor      the plain fp64 ``gram_stats`` pass over the same X: it reads the same bytes

at layers in {[8, 8, 3], [32, 32, 16], [64, 32, 32, 32]}, f32 and f64 features and every ``--rows``
size.  Every figure is the median of ``--steps`` separately synchronised calls after ``--warmup``,
with the min and max beside it (the run-to-run spread that the routing decision of profiles/mlp.md
is read against).  Then one whole fit (``ops.mlp.fit``, 20 iterations, tol 0) per case, on the fused
and the composite route.

    python benchmarks/bench_mlp.py [--rows 1e7] [--steps 7] [--warmup 2]

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
    ap.add_argument("--layers", default="8,8,3;32,32,16;64,32,32,32", help="topologies, ';' between them")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--composite-steps", type=int, default=3, help="timed composite evaluations (after one warm-up)")
    ap.add_argument("--fit-iters", type=int, default=20, help="iterations of the timed fit (0: no fit)")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host routes only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels, mlp as M
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_mlp needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    cases, ok = [], True
    for n in rows:
        for layers in ([int(v) for v in t.split(",")] for t in a.layers.split(";")):
            d = layers[0]
            w = torch.from_numpy(M.random_weights(layers, 77)).to(dev)
            for dt in a.dtypes.split(","):
                dtype = torch.float32 if dt == "f32" else torch.float64
                g = torch.Generator(device=dev).manual_seed(77 + d)
                X = torch.rand(d, n, generator=g, device=dev, dtype=dtype) * 2.0 - 1.0
                # labels from a random network of the same shape, so the fit below has something to find
                y = M.composite_pass(X, None, None, torch.from_numpy(M.random_weights(layers, 5)).to(dev) * 4.0, layers,
                                     M.PREDICT)
                case = {"layers": layers, "dtype": dt, "rows": n, "pass_bytes": X.element_size() * d * n}
                case["floor_gram"], _ = median_ms(torch, lambda: kernels.gram_stats(X, y, None, None, "fp64"), a.steps,
                                                  a.warmup, dev)
                case["composite"], ref = median_ms(torch, lambda: M.composite_pass(X, y, None, w, layers, M.GRAD),
                                                   a.composite_steps, 1, dev)
                if on_gpu:
                    from net.jgp.labs.sparkdq4ml_amd.ops import device

                    plan = device._MlpPlan(X, y, None, layers)
                    case["fused"], got = median_ms(torch, lambda: plan.grad(w), a.steps, a.warmup, dev)
                    # same statistics, to reordered-sum accuracy, at the size that is timed
                    rel = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
                    case["fused_vs_composite_max_rel"] = rel
                    ok = ok and rel < 1e-9
                    case["fused_gbps"] = case["pass_bytes"] / case["fused"]["median_ms"] / 1e6
                    case["fused_over_composite_min"] = case["fused"]["median_ms"] / case["composite"]["min_ms"]
                    case["fused_over_floor"] = case["fused"]["median_ms"] / case["floor_gram"]["median_ms"]
                    if a.fit_iters:
                        for how in ("fused", "composite"):
                            case["fit_" + how], _ = median_ms(
                                torch, lambda: M.fit(X, y, None, layers, max_iter=a.fit_iters, tol=0.0, seed=1, how=how), 1,
                                0, dev)
                print(f"[bench] {case}", file=sys.stderr, flush=True)
                cases.append(case)
                del X, y
    head = next((c for c in cases if c["layers"] == [32, 32, 16] and "fused" in c), cases[0])
    value = (head.get("fused") or head["composite"])["median_ms"]
    emit({"metric": "ms per perceptron loss / gradient evaluation (layers [32, 32, 16], first --rows size and dtype; "
                    "fused route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform features, labels predicted by a random network of the same shape)",
          "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
