#!/usr/bin/env python3
"""Window functions over 1e8 rows: an int64 partition key with about 1e6 partitions, an f64 order
key, an f64 value.  Timed in one process:

  sort         ``kernels.sort_permutation`` over (partition key, order key) alone
  row_number   sort + heads + bounds + finish (one ranking word)
  sum_default  scale + sort + heads + bounds + prefix (count + 7 sum words) + finish, default frame
               (RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW) + the shared finalisation
  sum_slide    the same over rowsBetween(-3, 3)

and every pass after the sort on its own (heads, bounds, prefix, finish), with the bytes the pass
must move computed from the shapes below and the HBM rate that implies.  A gathered 8-byte value
counts as 8 bytes, although a random gather fetches a whole line for it: the rate is the useful one.

    python benchmarks/bench_window.py [--rows 1e8] [--steps 3] [--warmup 1]

Needs the GPU; ``--rehearse`` runs the same code at a toy size on the CPU engine (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, timed, world_info  # noqa: E402

HBM_COPY_BPS = 6.29e12  # measured float4 copy rate of the MI355X (8.0 TB/s spec)


def pass_bytes(words: int):
    """Bytes per position each pass must move (m positions, two 8-byte key columns, one 8-byte value)."""
    return {
        # perm (the neighbour's entry and keys come from the cache), two gathered keys, one byte out
        "heads": 4 + 2 * 8 + 1,
        # forward: heads twice (reduce, scan) + three u32 out; backward: heads twice + two u32 out
        "bounds": 2 * 1 + 3 * 4 + 2 * 1 + 2 * 4,
        # reduce and scan each read perm and gather the value; the scan writes the words
        "prefix": 2 * (4 + 8) + 8 * words,
        # four bounds + perm in, two prefix values per word in, one word out
        "finish": 4 * 4 + 4 + 3 * 8 * words,
        "finish_rank": 4 * 4 + 4 + 8,
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--partitions", type=float, default=1e6)
    ap.add_argument("--rehearse", action="store_true", help="toy size on the CPU engine")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels
    from net.jgp.labs.sparkdq4ml_amd.ops import window as wn
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_window needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    n = int(a.rows) if on_gpu else 20_000
    parts = int(a.partitions) if on_gpu else 200
    g = torch.Generator(device=dev).manual_seed(977)
    key = torch.randint(0, parts, (n,), generator=g, device=dev, dtype=torch.int64)
    ts = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    val = torch.floor(torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 18000.0) / 100.0 + 20.0

    def sort():
        return kernels.sort_permutation([key, ts], [None, None], None, [True, True])

    def heads(perm):
        return kernels.window_heads([key], [None], [ts], [None], perm, n)

    def prefix(perm, e):
        return kernels.window_prefix([(wn.COUNT, None, None, 0), (wn.SUM_F, val, None, e)], perm, n)[0]

    def finish_sum(bounds, perm, P, frame):
        return kernels.window_finish(bounds, perm, n, frame, [(wn.O_DIFF, P[w], 0) for w in range(8)])

    def finish_rank(bounds, perm):
        return kernels.window_finish(bounds, perm, n, (True, None, 0), [(wn.O_ROW_NUMBER, None, 0)])

    def row_number():
        perm = sort()
        return finish_rank(kernels.window_bounds(heads(perm)), perm)[:, 0]

    def window_sum(frame):
        e = kernels.group_scale([val], [None], None)[0]
        perm = sort()
        bounds = kernels.window_bounds(heads(perm))
        raw = finish_sum(bounds, perm, prefix(perm, e), frame)
        return wn.sum_from_words(raw[:, 1:8], e)

    DEFAULT, SLIDE = (True, None, 0), (False, -3, 3)
    ms = lambda el: el / a.steps * 1e3  # noqa: E731

    def run(name, fn):
        el, out = timed(fn, a.steps, a.warmup, dev)
        print(f"[bench] {name}: {ms(el):.3f} ms per call", file=sys.stderr, flush=True)
        return ms(el), out

    t_sort, perm = run("sort", sort)
    e = kernels.group_scale([val], [None], None)[0]
    t_heads, hd = run("heads", lambda: heads(perm))
    t_bounds, bounds = run("bounds", lambda: kernels.window_bounds(hd))
    t_prefix, P = run("prefix (8 words)", lambda: prefix(perm, e))
    t_fin, raw = run("finish (8 words, default frame)", lambda: finish_sum(bounds, perm, P, DEFAULT))
    t_fin_s, _ = run("finish (8 words, rows -3..3)", lambda: finish_sum(bounds, perm, P, SLIDE))
    t_fin_r, _ = run("finish (row_number)", lambda: finish_rank(bounds, perm))
    t_final, _ = run("finalisation (torch, shared)", lambda: wn.sum_from_words(raw[:, 1:8], e))
    del raw, P, bounds, hd, perm, _
    t_rn, rn = run("row_number", row_number)
    t_def, s_def = run("sum, default frame", lambda: window_sum(DEFAULT))
    t_sl, s_sl = run("sum, rowsBetween(-3, 3)", lambda: window_sum(SLIDE))
    # a light check on the results: every partition has a row number 1, and the sums are finite
    ok = bool((rn >= 1).all()) and int((rn == 1).sum()) == int(torch.unique(key).numel()) and bool(
        torch.isfinite(s_def).all() and torch.isfinite(s_sl).all())
    if not ok:
        print("[bench] the window results fail their sanity check", file=sys.stderr)
    pb = pass_bytes(8)
    passes = {}
    for name, t, b in (("heads", t_heads, pb["heads"]), ("bounds", t_bounds, pb["bounds"]), ("prefix", t_prefix, pb["prefix"]),
                       ("finish_default", t_fin, pb["finish"]), ("finish_slide", t_fin_s, pb["finish"]),
                       ("finish_row_number", t_fin_r, pb["finish_rank"])):
        bps = b * n / (t * 1e-3)
        passes[name] = {"ms": t, "bytes_per_position": b, "implied_gbps": bps / 1e9, "hbm_copy_fraction": bps / HBM_COPY_BPS}
    cases = {}
    for name, t in (("row_number", t_rn), ("sum_default", t_def), ("sum_slide", t_sl)):
        cases[name] = {"ms_per_call": t, "after_sort_ms": t - t_sort, "after_sort_share": (t - t_sort) / t}
    emit({"metric": "ms per row_number() over (partition, order) call", "value": t_rn, "unit": "ms", "ms_per_step": t_rn,
          "higher_is_better": False, "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "rows": n, "partitions": parts,
          "sort_ms": t_sort, "finalisation_ms": t_final, "cases": cases, "passes": passes, "sane": ok,
          "measured_on": str(dev), "data": "synthetic (uniform int64 keys, uniform f64 order key, two-decimal prices)",
          "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
