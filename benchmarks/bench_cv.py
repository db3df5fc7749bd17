#!/usr/bin/env python3
"""Cross-validation: one ``CrossValidator.fit`` of a normal-equation ``LinearRegression`` over a
regParam x elasticNetParam grid, per route (``models/tuning.py``):

* ``onepass``  one ``gram_folds`` pass yields the k per-fold statistics vectors;
* ``masked``   the same vectors from k masked ``gram_stats`` passes (forced here by closing the
  one-pass kernel's feature range, ``ops.device.ONEPASS_MIN_D``);
* ``generic``  Spark's loop: k x grid fits and scoring passes plus one refit
  (``dq4ml.cv.onePass=false``).

``--kernels`` times the statistics passes alone instead (device events, alternating): one plain
``gram_stats`` fp64 pass, the one-pass kernel and the masked route's k passes, for k in 3, 5, 10.

Synthetic rows: f32 N(0,1) features, label = linear model + 5 + N(0,1).

    python benchmarks/bench_cv.py [--rows 4e6] [--features 32] [--folds 5] [--grid 6] [--route all]
    python benchmarks/bench_cv.py --kernels [--rows 4e6] [--features 32]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, self_launch, timed, world_info  # noqa: E402

ROUTES = ("onepass", "masked", "generic")


def _grid(size: int):
    from net.jgp.labs.sparkdq4ml_amd import ParamGridBuilder

    regs = [0.0, 0.1, 1.0, 0.01, 0.3, 3.0, 0.03, 10.0][:max(1, (size + 1) // 2)]
    maps = ParamGridBuilder().addGrid("regParam", regs).addGrid("elasticNetParam", [0.0, 1.0]).build()
    return maps[:size]


def _kernel_table(X, y, reps: int):
    """ms per call of the three statistics passes, the variants alternating inside each repetition."""
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import device

    def ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rows = []
    for k in (3, 5, 10):
        variants = {
            "plain": lambda: device.gram_stats(X, y, None, None, "fp64"),
            "onepass": lambda k=k: device.gram_stats_folds(X, y, None, k, 42, 64, "fp64", route="onepass"),
            "masked": lambda k=k: device.gram_stats_folds(X, y, None, k, 42, 64, "fp64", route="masked"),
        }
        for fn in variants.values():  # warm every shape
            fn()
        torch.cuda.synchronize()
        best = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                best[name].append(ms(fn))
        med = {name: sorted(v)[len(v) // 2] for name, v in best.items()}
        rows.append({"k": k, **{f"{name}_ms": round(v, 4) for name, v in med.items()},
                     "onepass_over_plain": round(med["onepass"] / med["plain"], 3),
                     "masked_over_onepass": round(med["masked"] / med["onepass"], 3)})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=float, default=4e6, help="global rows (strong scaling)")
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--grid", type=int, default=6, help="number of param maps")
    ap.add_argument("--route", default="all", choices=("all",) + ROUTES)
    ap.add_argument("--kernels", action="store_true", help="time the statistics passes alone (k = 3, 5, 10)")
    ap.add_argument("--reps", type=int, default=20, help="repetitions of --kernels")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.folds < 2 or a.grid < 1:
        ap.error("--steps >= 1, --folds >= 2, --grid >= 1")
    rc = self_launch(a.gpus, __file__, argv)
    if rc is not None:
        return rc
    import torch

    from net.jgp.labs.sparkdq4ml_amd import CrossValidator, LinearRegression, SparkSession
    from net.jgp.labs.sparkdq4ml_amd.models.evaluation import RegressionEvaluator
    from net.jgp.labs.sparkdq4ml_amd.ops import device
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    rank, world = comm.rank(), comm.world_size()
    spark = SparkSession.builder().appName("bench-cv").master("local[*]") \
        .config("dq4ml.cv.foldGranule", "64").getOrCreate()
    dev = spark.device
    d, total = a.features, int(a.rows)
    if dev.type != "cuda":
        total = min(total, 20_000 * world)
    n = total // world if rank < world - 1 else total - (world - 1) * (total // world)
    g = torch.Generator(device=dev).manual_seed(97 + rank)
    X = torch.randn(d, n, generator=g, device=dev)
    beta = torch.linspace(-1.0, 2.0, d, device=dev)
    y = (beta @ X + 5.0 + torch.randn(n, generator=g, device=dev)).double()
    base = {"n_gpus": world, "steps": a.steps, "warmup": a.warmup, "higher_is_better": False, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32 storage, fp64 statistics",
            "data": "synthetic (N(0,1) features, linear label + N(0,1))"}
    if a.kernels:
        if dev.type != "cuda":
            print("[bench] --kernels needs the GPU", file=sys.stderr)
            return 2
        emit({"metric": "ms per fold-statistics pass", "unit": "ms", "rows": n, "features": d,
              "table": _kernel_table(X, y, a.reps), **base, **world_info(dev)}, a.json_out)
        comm.shutdown()
        return 0
    df = spark.createDataFrame({"features": X, "label": y})
    cv = CrossValidator(estimator=LinearRegression(), estimatorParamMaps=_grid(a.grid),
                        evaluator=RegressionEvaluator(metricName="rmse"), numFolds=a.folds, seed=42)
    lo, hi = device.ONEPASS_MIN_D, device.ONEPASS_MAX_D
    results = {}
    for route in (ROUTES if a.route == "all" else (a.route,)):
        spark.conf.set("dq4ml.cv.onePass", "false" if route == "generic" else "true")
        # the dispatcher's measured range decides between onepass and masked; force either here
        device.ONEPASS_MIN_D, device.ONEPASS_MAX_D = {"onepass": (1, 64), "masked": (65, 64)}.get(route, (lo, hi))
        last = {}

        def step():
            m = cv.fit(df)
            m.bestModel.coefficients
            last["m"] = m
            return m

        elapsed, _ = timed(step, a.steps, a.warmup, dev)
        m = last["m"]
        want = route if dev.type == "cuda" or route == "generic" else "masked"  # the CPU engine has no one-pass kernel
        if m._cv_route != want:
            print(f"[bench] asked for route {route}, the fit took {m._cv_route}", file=sys.stderr)
            return 2
        results[route] = {"ms_per_fit": elapsed / a.steps * 1e3, "avgMetrics": list(m.avgMetrics),
                          "best": m._bestIndex}
    device.ONEPASS_MIN_D, device.ONEPASS_MAX_D = lo, hi
    first = next(iter(results))
    ms = results[first]["ms_per_fit"]
    emit({"metric": f"ms per CrossValidator.fit ({first})", "value": ms, "unit": "ms", "ms_per_step": ms,
          "routes": results,
          "config": {"model": f"CrossValidator(LinearRegression d={d}, k={a.folds}, grid={a.grid})",
                     "global_batch": total, "seq_len": d, "parallelism": f"dp{world}"},
          **base, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
