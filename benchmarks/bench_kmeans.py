#!/usr/bin/env python3
"""KMeans: one Lloyd iteration over f32 features, three ways, in one process:

  fused      the fused pass (csrc/hip/kmeans.hip), slab reduce and centre update: one iteration of the
             enqueued loop (``device.KMeansLoop``), no host read
  composite  ``ops.kmeans.composite_pass`` (torch matmul into a [k, n] score matrix, argmin,
             index_add_, all f64) and the host update: one iteration of the host loop; run up to
             ``--composite-max-rows`` rows, ``--composite-steps`` times (one takes tens of seconds)
  floor      the plain fp64 ``gram_stats`` pass over the same X: it reads the same bytes

at d in {8, 32, 64}, k in {8, 64} and every ``--rows`` size.  Every figure is the median of
``--steps`` separately synchronised steps after ``--warmup``, with the min and max beside it (the
run-to-run spread that the routing decision of profiles/kmeans.md is read against).  Then whole
fits (``device.kmeans_fit``, 20 iterations, tol 0) and the seeding (``ops.kmeans.seed_centers``, both
init modes) that ``KMeans().fit`` runs in front of them.

    python benchmarks/bench_kmeans.py [--rows 1e7,1e8] [--steps 7] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the host routes at a toy size on the CPU (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, world_info  # noqa: E402


def median_ms(torch, step, steps, warmup, dev):
    """(median, min, max) milliseconds of ``steps`` separately synchronised calls, and the last result."""
    out, ts = None, []
    for i in range(warmup + steps):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = step()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="1e7,1e8")
    ap.add_argument("--dims", default="8,32,64")
    ap.add_argument("--ks", default="8,64")
    ap.add_argument("--composite-max-rows", default="1e7",
                    help="largest --rows size at which the composite runs (0: never); it takes tens of seconds per "
                         "iteration at 1e7 rows and its [k, n] f64 temporaries do not fit at 1e8 (profiles/kmeans.md)")
    ap.add_argument("--composite-steps", type=int, default=1, help="timed composite iterations (no warm-up)")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host routes only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels, kmeans as K
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_kmeans needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    cases, ok = [], True
    for n in rows:
        for d in (int(v) for v in a.dims.split(",")):
            g = torch.Generator(device=dev).manual_seed(77 + d)
            X = torch.rand(d, n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0
            y = torch.zeros(n, dtype=torch.float64, device=dev)
            floor, _ = median_ms(torch, lambda: kernels.gram_stats(X, y, None, None, "fp64"), a.steps, a.warmup, dev)
            for k in (int(v) for v in a.ks.split(",")):
                C = np.random.default_rng(k).uniform(-1, 1, (k, d))
                case = {"d": d, "k": k, "rows": n, "pass_bytes": 4 * d * n, "floor_gram": floor}

                last = {}

                def comp_iter():
                    last["stats"] = K.composite_pass(X, None, C, K.STEP)
                    return K.update_host(last["stats"], C, 0.0)[0]
                ref = None
                if n <= int(float(a.composite_max_rows)):
                    case["composite_iter"], _ = median_ms(torch, comp_iter, a.composite_steps, 0, dev)
                    ref = last["stats"]
                else:
                    case["composite_iter"] = None
                if on_gpu:
                    from net.jgp.labs.sparkdq4ml_amd.ops import device

                    got = device.kmeans_pass(X, None, C, K.STEP)
                    # same statistics, to reordered-sum accuracy, at the size that is timed
                    if ref is not None:
                        rel = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
                        case["fused_vs_composite_max_rel"] = rel
                        ok = ok and rel < 1e-9
                    loop = device.KMeansLoop(X, None, C, 0.0)  # tol 0: done only if no centre moves at all
                    case["fused_iter"], _ = median_ms(torch, lambda: loop.iterate(1), a.steps, a.warmup, dev)
                    case["fused_gbps"] = case["pass_bytes"] / case["fused_iter"]["median_ms"] / 1e6
                    if ref is not None:
                        case["fused_over_composite"] = (case["fused_iter"]["median_ms"]
                                                        / case["composite_iter"]["median_ms"])
                    case["fused_over_floor"] = case["fused_iter"]["median_ms"] / floor["median_ms"]
                    case["fit_20_iterations"], _ = median_ms(
                        torch, lambda: device.kmeans_fit(X, None, C, 20, 0.0, K.DEVICE_BATCH), 3, 1, dev)
                    # what KMeans().fit adds in front of the iterations: the starting centres
                    for mode in ("random", "k-means||"):
                        case["seed_" + mode], _ = median_ms(
                            torch, lambda: K.seed_centers(X, None, k, mode, 2, 7), 3, 1, dev)
                print(f"[bench] {case}", file=sys.stderr, flush=True)
                cases.append(case)
            del X, y
    head = next((c for c in cases if c["d"] == 32 and c["k"] == 8 and "fused_iter" in c), cases[0])
    value = (head.get("fused_iter") or head["composite_iter"] or head["floor_gram"])["median_ms"]
    emit({"metric": "ms per Lloyd iteration (d = 32, k = 8, first --rows size; fused route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform f32 features and centres)", "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
