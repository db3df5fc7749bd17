#!/usr/bin/env python3
"""Exact quantiles: one ``kernels.quantiles`` call (radix select, ``ops/csrc/hip/quantile.hip``) of
C f64 columns under a 70 % selection at p = (0.25, 0.5, 0.75), against what a user could do
before it existed: ``torch.sort`` of ONE compacted column on the device, timed in the same process.

Reported per data shape (``random`` N(0,1), ``constant``, ``sorted``): ms per call, the number of
histogram passes, GB/s per pass (the bytes a pass must read -- C columns of 8-byte values, each
with the 1-byte selection -- over a pass's share of the call, pick kernels and launch gaps
included) and that rate's share of the HBM streaming rate the headline Gram reaches.  The constant
and the sorted column put every lane of a wave into one bin: the contention path.

    python benchmarks/bench_quantiles.py [--rows 1e8] [--cols 4] [--steps 5] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the same code at a toy size on the CPU engine (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, timed, world_info  # noqa: E402

PROBS = (0.25, 0.5, 0.75)
HBM_STREAM_BPS = 6.5e12  # the headline Gram's measured streaming rate (profiles/r5_pmc.md)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--live", type=float, default=0.7, help="selected fraction of the rows")
    ap.add_argument("--rehearse", action="store_true", help="toy size on the CPU engine")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.cols < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --cols >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_quantiles needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    n, C = (int(a.rows) if on_gpu else 20_000), a.cols
    g = torch.Generator(device=dev).manual_seed(1234)
    sel = torch.rand(n, generator=g, device=dev) < a.live
    passes = 64 // kernels.QUANT_BITS
    pass_bytes = C * n * (8 + 1)

    def run(cols):
        def step():
            v, c = kernels.quantiles(cols, None, sel, PROBS)
            return v, c
        el, (v, c) = timed(step, a.steps, a.warmup, dev)
        ms = el / a.steps * 1e3
        bps = pass_bytes / (ms * 1e-3 / passes)
        return {"ms_per_call": ms, "passes": passes, "gbps_per_pass": bps / 1e9,
                "hbm_stream_fraction": bps / HBM_STREAM_BPS, "counts": c.cpu().tolist(),
                "values_col0": v[0].cpu().tolist()}

    shapes = {}
    cols = [torch.randn(n, generator=g, device=dev, dtype=torch.float64) for _ in range(C)]
    shapes["random"] = run(cols)

    def sort_step():  # today's route for ONE column: compact, sort, index
        x = cols[0][sel]
        s, _ = torch.sort(x)
        return s
    el, s = timed(sort_step, a.steps, a.warmup, dev)
    sort_ms = el / a.steps * 1e3
    m = int(s.numel())
    idx = [max(1, math.ceil(p * m)) - 1 for p in PROBS]
    want = [float(s[i]) for i in idx]
    if want != shapes["random"]["values_col0"]:
        print(f"[bench] select {shapes['random']['values_col0']} != sort {want}", file=sys.stderr)
        return 2
    del s
    first = cols[0]
    del cols
    shapes["constant"] = run([torch.full((n,), 3.25, device=dev, dtype=torch.float64) for _ in range(C)])
    srt = torch.sort(first)[0]
    del first
    shapes["sorted"] = run([srt] + [srt.clone() for _ in range(C - 1)])  # distinct buffers: no cache sharing
    ms = shapes["random"]["ms_per_call"]
    emit({"metric": f"ms per quantiles call ({C} f64 columns, 3 probabilities)", "value": ms, "unit": "ms",
          "ms_per_step": ms, "higher_is_better": False, "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
          "rows": n, "cols": C, "live_fraction": a.live, "probs": list(PROBS), "shapes": shapes,
          "sort_one_column_ms": sort_ms, "sort_one_column_over_call": sort_ms / ms,
          "sort_all_columns_over_call": sort_ms * C / ms, "measured_on": str(dev),
          "data": "synthetic (N(0,1) f64; constant; sorted)", "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
