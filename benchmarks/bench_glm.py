#!/usr/bin/env python3
"""GeneralizedLinearRegression: one IRLS iteration over f32 features, three ways, in one process:

  fused      the fused reweighting + Gram pass (csrc/hip/glm_irls.hip), slab fold, device WLS solve
             and step kernel: one iteration of the enqueued loop (``device.GlmLoop``), no host read
  composite  ``ops.glm.composite_pass`` (``predict``, elementwise torch, weighted fp64 ``gram_stats``)
             and the host WLS solve: one iteration of the host loop; the pass alone is timed too
  floor      the plain fp64 ``gram_stats`` pass over the same X and label: it reads the same bytes

for binomial / logit and poisson / log at d in {8, 32, 64} and every ``--rows`` size, with the
bytes a pass must read (4 d n of features + 8 n of label) over its time.  Then whole fits
(``device.glm_fit``) at the ``--batch`` sizes: iterations enqueued per host read of the state.

    python benchmarks/bench_glm.py [--rows 1e7,1e8] [--steps 5] [--warmup 1]

Needs the GPU; ``--rehearse`` runs the host routes at a toy size on the CPU (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, timed, world_info  # noqa: E402

HBM_COPY_BPS = 6.29e12  # measured float4 copy rate of the MI355X (8.0 TB/s spec)
PAIRS = (("binomial", "logit"), ("poisson", "log"))


def make(torch, family, d, n, dev):
    """f32 features in [-1, 1), f64 labels drawn from the family at fixed coefficients (|eta| <= 1.7)."""
    g = torch.Generator(device=dev).manual_seed(4242 + d)
    X = torch.rand(d, n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0
    coef = (torch.arange(d, dtype=torch.float64) % 3 - 1.0) * (1.5 / d)
    coef[0] = 1.5 / d
    eta = (coef.to(dev).to(torch.float32) @ X).to(torch.float64) + 0.2
    if family == "binomial":
        y = torch.bernoulli(torch.sigmoid(eta), generator=g)
    else:
        y = torch.poisson(torch.exp(eta), generator=g)
    return X, y.to(torch.float64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="1e7,1e8")
    ap.add_argument("--dims", default="8,32,64")
    ap.add_argument("--batch", default="1,2,4,8,25")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host routes only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import numpy as np
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import glm, kernels
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_glm needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rows = [int(float(r)) for r in a.rows.split(",")] if on_gpu else [5000]
    dims = [int(v) for v in a.dims.split(",")]
    batches = [int(v) for v in a.batch.split(",")]
    ms = lambda el: el / a.steps * 1e3  # noqa: E731
    cases, ok = [], True
    for n in rows:
        for d in dims:
            for family, link in PAIRS:
                X, y = make(torch, family, d, n, dev)
                nbytes = 4 * d * n + 8 * n
                beta = np.concatenate([(np.arange(d) % 3 - 1.0) * (1.2 / d), [0.1]])
                case = {"family": family, "link": link, "d": d, "rows": n, "pass_bytes": nbytes}

                def rate(t_ms):
                    return nbytes / (t_ms * 1e-3) / 1e9

                def comp_iter():
                    flat = glm.composite_pass(X, y, None, None, beta, family, link, glm.STEP)
                    return glm._solve(flat, d, True, 0.0)[0].coefficients
                t, ref = timed(lambda: glm.composite_pass(X, y, None, None, beta, family, link, glm.STEP), a.steps,
                               a.warmup, dev)
                case["composite_pass_ms"], case["composite_pass_gbps"] = ms(t), rate(ms(t))
                t, _ = timed(comp_iter, a.steps, a.warmup, dev)
                case["composite_iter_ms"] = ms(t)
                t, _ = timed(lambda: kernels.gram_stats(X, y, None, None, "fp64"), a.steps, a.warmup, dev)
                case["floor_gram_ms"], case["floor_gram_gbps"] = ms(t), rate(ms(t))
                if on_gpu:
                    from net.jgp.labs.sparkdq4ml_amd.ops import device

                    t, got = timed(lambda: device.glm_pass(X, y, None, None, beta, family, link, glm.STEP), a.steps,
                                   a.warmup, dev)
                    case["fused_pass_ms"], case["fused_pass_gbps"] = ms(t), rate(ms(t))
                    case["fused_pass_hbm_copy_fraction"] = rate(ms(t)) * 1e9 / HBM_COPY_BPS
                    # same statistics, to reordered-sum accuracy, at the size that is timed
                    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
                    case["fused_vs_composite_max_rel"] = rel
                    ok = ok and rel < 1e-9
                    loop = device.GlmLoop(X, y, None, None, family, link, True, 0.0, 0.0)  # tol 0: never done
                    loop.start()
                    t, _ = timed(lambda: loop.iterate(1), a.steps, a.warmup, dev)
                    case["fused_iter_ms"] = ms(t)
                    case["fused_over_composite_iter"] = case["fused_iter_ms"] / case["composite_iter_ms"]
                    fits = {}
                    for b in batches:  # whole fits, host reads included
                        torch.cuda.synchronize()
                        best = None
                        for _ in range(max(a.steps // 2, 2)):
                            t0 = time.perf_counter()
                            r = device.glm_fit(X, y, None, None, family, link, True, 0.0, 25, 1e-6, b)
                            torch.cuda.synchronize()
                            el = (time.perf_counter() - t0) * 1e3
                            best = el if best is None else min(best, el)
                        fits[str(b)] = {"fit_ms_best": best, "iterations": r["iterations"], "status": r["status"]}
                    case["fit_by_batch"] = fits
                print(f"[bench] {case}", file=sys.stderr, flush=True)
                cases.append(case)
                del X, y
    head = next((c for c in cases if c["d"] == 32 and c["family"] == "binomial" and "fused_iter_ms" in c), cases[0])
    value = head.get("fused_iter_ms", head["composite_iter_ms"])
    emit({"metric": "ms per IRLS iteration (binomial / logit, d = 32, first --rows size; fused route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform f32 features, labels drawn from the family)", "vs_baseline": None,
          **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
