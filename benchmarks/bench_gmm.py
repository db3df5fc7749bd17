#!/usr/bin/env python3
"""GaussianMixture: one EM iteration over f32 features, two ways, in one process:

  fused      the fused pass (csrc/hip/gmm.hip) and slab reduce, then the host's share of an iteration:
             the read of the statistics, the M-step (``ops.gmm.m_step_host``), the k eigendecompositions
             of the next parameter buffer and its upload.  The two parts are timed apart
             (``fused_pass`` ends in a device synchronise; ``fused_host`` is host work plus one copy
             each way) and together (``fused_iter``).
  composite  ``ops.gmm.composite_pass`` (torch f64 over [k, n] densities, one weighted Gram per
             component) and the same host M-step; run up to ``--composite-max-rows`` rows.

at d in {8, 16, 32}, k in {2, 8, 16} inside the fused range and every ``--rows`` size.  Every figure
is the median of ``--steps`` separately synchronised steps after ``--warmup``, with the min and max
beside it (the run-to-run spread that the routing decision of profiles/gmm.md is read against).

    python benchmarks/bench_gmm.py [--rows 1e6,1e7] [--steps 7] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the host route at a toy size on the CPU (no rate is a
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
    ap.add_argument("--dims", default="8,16,32")
    ap.add_argument("--ks", default="2,8,16")
    ap.add_argument("--composite-max-rows", default="1e7", help="largest --rows size at which the composite runs (0: never)")
    ap.add_argument("--composite-steps", type=int, default=3, help="timed composite iterations (after one warm-up)")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host route only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import gmm as G
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_gmm needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    cases, ok = [], True
    for n in rows:
        for d in (int(v) for v in a.dims.split(",")):
            g = torch.Generator(device=dev).manual_seed(77 + d)
            X = torch.rand(d, n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0
            for k in (int(v) for v in a.ks.split(",")):
                if not G.fused_range(d, k):
                    continue
                # (narrow covariances and means near the centre: wider ones leave every density of a
                # row in [-1, 1]^32 below EPS, and an iteration would time a degenerate mixture)
                rng = np.random.default_rng(k)
                A = rng.uniform(-0.5, 0.5, (k, d, d)) / np.sqrt(d)
                par = (np.full(k, 1.0 / k), rng.uniform(-0.3, 0.3, (k, d)), A @ A.transpose(0, 2, 1) + 0.5 * np.eye(d))
                # MFMA work of the fused pass: 2 * 16 * 16 * 4 flops each
                nt = (d + 15) // 16
                mfma = (n / 64) * (k * nt * nt * 16 + 16 * (k * nt * (nt + 1) // 2 + nt))
                case = {"d": d, "k": k, "rows": n, "pass_bytes": 4 * d * n, "pass_mfma_flop": mfma * 2048}
                ref = None
                if n <= int(float(a.composite_max_rows)):
                    def comp_iter():
                        stats = G.composite_pass(X, None, *par, G.STEP)
                        G.m_step_host(stats, k, d)
                        return stats
                    case["composite_iter"], ref = median_ms(torch, comp_iter, a.composite_steps, 1, dev)
                if on_gpu:
                    from net.jgp.labs.sparkdq4ml_amd.ops import device

                    plan = device._GmmPlan(X, None, k, None)
                    buf = plan.params(*par)
                    got = plan.step(buf)
                    if ref is not None:  # same statistics, to reordered-sum accuracy, at the size that is timed
                        rel = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
                        case["fused_vs_composite_max_rel"] = rel
                        ok = ok and rel < 1e-9

                    def host_part():
                        return plan.params(*G.m_step_host(plan.stats, k, d))

                    def fused_iter():
                        plan.step(buf)
                        return host_part()
                    case["fused_pass"], _ = median_ms(torch, lambda: plan.step(buf), a.steps, a.warmup, dev)
                    case["fused_host"], _ = median_ms(torch, host_part, a.steps, a.warmup, dev)
                    case["fused_iter"], _ = median_ms(torch, fused_iter, a.steps, a.warmup, dev)
                    case["host_share"] = case["fused_host"]["median_ms"] / case["fused_iter"]["median_ms"]
                    case["fused_rows_per_s"] = n / case["fused_iter"]["median_ms"] * 1e3
                    case["fused_pass_tflops"] = case["pass_mfma_flop"] / case["fused_pass"]["median_ms"] / 1e9
                    if ref is not None:
                        case["composite_rows_per_s"] = n / case["composite_iter"]["median_ms"] * 1e3
                        case["fused_over_composite"] = case["fused_iter"]["median_ms"] / case["composite_iter"]["median_ms"]
                print(f"[bench] {case}", file=sys.stderr, flush=True)
                cases.append(case)
            del X
    head = next((c for c in cases if c["d"] == 16 and c["k"] == 8 and "fused_iter" in c), cases[0])
    value = (head.get("fused_iter") or head["composite_iter"])["median_ms"]
    emit({"metric": "ms per EM iteration (d = 16, k = 8, first --rows size; fused route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform f32 features, random narrow mixtures)", "vs_baseline": None, **world_info(dev)},
         a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
