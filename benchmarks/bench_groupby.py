#!/usr/bin/env python3
"""Grouped aggregation: ``count, sum(f64), min, max`` of one f64 column per int32 key under a 70 %
selection (``kernels.group_encode`` + ``group_agg``, ``ops/csrc/hip/groupby.hip``), for G in
{16, 4096, 1e6} groups, against what a user could do before it existed, timed in the same process:
compact the live rows, ``torch.unique(return_inverse=True)`` (a sort of every row), then
``index_add_`` / ``scatter_reduce_``.

Reported per G: ms per call of the whole route and of its parts (the encode with its min / max
pre-pass, the ``ABSMAX`` scale pre-pass, the aggregation pass), the bytes the aggregation pass must
read (gid 4 + selection 1 + value 8 per row) over its time against the HBM streaming rate, and the
torch route's ms.  The two routes' counts, minima and maxima must be equal and their sums agree to
1e-12 of the summed absolute terms (a reordered f64 sum); a mismatch exits 2.

    python benchmarks/bench_groupby.py [--rows 1e8] [--steps 10] [--warmup 3]

The torch route is timed with the same warm-up and steps unless its first call already takes more
than ``--torch-budget`` seconds (its f64 ``amin`` / ``amax`` scatter is a compare-and-swap loop,
which crawls when 7e7 rows meet 16 addresses): then that one call is the measurement.  Every part
prints its time to stderr as it finishes.

Needs the GPU; ``--rehearse`` runs the same code at a toy size on the CPU engine (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, timed, world_info  # noqa: E402

HBM_STREAM_BPS = 6.5e12  # the streaming rate quoted in profiles/quantiles.md
GROUPS = (16, 4096, 1_000_000)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--live", type=float, default=0.7, help="selected fraction of the rows")
    ap.add_argument("--torch-budget", type=float, default=2.0, help="seconds of one torch-route call above which it runs once")
    ap.add_argument("--rehearse", action="store_true", help="toy size on the CPU engine")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import groupby as gb
    from net.jgp.labs.sparkdq4ml_amd.ops import kernels
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_groupby needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    n = int(a.rows) if on_gpu else 20_000
    g = torch.Generator(device=dev).manual_seed(1234)
    sel = torch.rand(n, generator=g, device=dev) < a.live
    x = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    agg_bytes = n * (4 + 1 + 8)
    shapes, bad = {}, False
    for G in GROUPS:
        G = min(G, max(1, n // 4))
        key = torch.randint(0, G, (n,), generator=g, device=dev, dtype=torch.int32)

        def encode():
            return kernels.group_encode(key, None, sel)

        def scale():
            return kernels.group_scale([x], [None], sel)

        def say(what, el, steps=a.steps):
            print(f"[bench] G={G} {what}: {el / steps * 1e3:.3f} ms per call", file=sys.stderr, flush=True)

        el_enc, enc = timed(encode, a.steps, a.warmup, dev)
        say("encode", el_enc)
        el_scale, (e,) = timed(scale, a.steps, a.warmup, dev)
        say("absmax pre-pass", el_scale)
        slots = [(gb.COUNT, None, None, 0), (gb.SUM_F, x, None, e), (gb.MIN, x, None, 0), (gb.MAX, x, None, 0)]

        def agg():
            return kernels.group_agg(enc.gid, enc.G, slots, sel)

        def whole():
            c = kernels.group_encode(key, None, sel)
            acc, off = kernels.group_agg(c.gid, c.G, [(op, col, v, None if op == gb.SUM_F else 0) for op, col, v, _ in slots], sel)
            keep = acc[:, 0] > 0
            acc = acc[keep]
            w = off[1]
            return (c.keys[keep], acc[:, off[0]], gb.finalize_sum(acc[:, w:w + 4], acc[:, w + 4], e),
                    gb.keys_to_values(acc[:, off[2]] ^ -(1 << 63), torch.float64),
                    gb.keys_to_values(acc[:, off[3]] ^ -(1 << 63), torch.float64))

        el_agg, _ = timed(agg, a.steps, a.warmup, dev)
        say("agg", el_agg)
        el_all, ours = timed(whole, a.steps, a.warmup, dev)
        say("whole route", el_all)

        def torch_route():
            k, v = key[sel], x[sel]
            uniq, inv = torch.unique(k, return_inverse=True)
            m = int(uniq.numel())
            cnt = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(inv))
            s = torch.zeros(m, dtype=torch.float64, device=dev).index_add_(0, inv, v)
            lo = torch.full((m,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, inv, v, "amin")
            hi = torch.full((m,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, inv, v, "amax")
            absum = torch.zeros(m, dtype=torch.float64, device=dev).index_add_(0, inv, v.abs())
            return uniq, cnt, s, lo, hi, absum

        t0 = time.perf_counter()
        ref = torch_route()
        if on_gpu:
            torch.cuda.synchronize()
        el_t, t_steps = time.perf_counter() - t0, 1
        if el_t <= a.torch_budget:
            el_t, ref = timed(torch_route, a.steps, max(0, a.warmup - 1), dev)
            t_steps = a.steps
        say("torch route", el_t, t_steps)
        ok = (torch.equal(ours[0], ref[0].to(torch.int64)) and torch.equal(ours[1], ref[1]) and torch.equal(ours[3], ref[3])
              and torch.equal(ours[4], ref[4]) and bool(((ours[2] - ref[2]).abs() <= 1e-12 * ref[5]).all()))
        if not ok:
            print(f"[bench] G={G}: the kernels and the torch route disagree", file=sys.stderr)
            bad = True
        ms = lambda el: el / a.steps * 1e3  # noqa: E731
        bps = agg_bytes / (ms(el_agg) * 1e-3)
        shapes[str(G)] = {"groups": int(ours[0].numel()), "mode": enc.mode, "ms_per_call": ms(el_all), "encode_ms": ms(el_enc),
                          "absmax_prepass_ms": ms(el_scale), "agg_ms": ms(el_agg), "agg_gbps": bps / 1e9,
                          "agg_hbm_stream_fraction": bps / HBM_STREAM_BPS, "torch_route_ms": el_t / t_steps * 1e3,
                          "torch_route_steps": t_steps, "torch_over_ours": (el_t / t_steps) / (el_all / a.steps), "equal": ok}
        del key, enc, ours, ref
    first = shapes[str(min(GROUPS[0], max(1, n // 4)))]
    emit({"metric": "ms per grouped count/sum/min/max call (int32 key, f64 value, G=16)", "value": first["ms_per_call"],
          "unit": "ms", "ms_per_step": first["ms_per_call"], "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "rows": n, "live_fraction": a.live, "agg_bytes_per_call": agg_bytes, "shapes": shapes,
          "measured_on": str(dev), "data": "synthetic (uniform int32 keys, N(0,1) f64)", "vs_baseline": None,
          **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 2 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
