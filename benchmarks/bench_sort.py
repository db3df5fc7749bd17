#!/usr/bin/env python3
"""Stable sort of 1e8 rows: ``kernels.sort_permutation`` (``ops/csrc/hip/sort.hip``) and the gather
of the sorted key columns, for

  int32      an int32 key with 4096 distinct values
  f64        a full-range f64 key (random bits: every finite exponent, both signs)
  price      a price-like f64 key (two decimals in [20, 200)) with 10 % nulls under a 50 % selection
  two        a two-key sort: the int32 key ascending, then the price descending

against the torch route a user had before, timed in the same process: the live rows compacted and
the keys and null masks materialised with torch ops, ``torch.sort(stable=True)`` (once per key,
last key first), and the same gather.  The two routes' permutations must be equal; a mismatch
exits 2.

Reported per case: ms per call of the whole route, of the permutation alone and of the torch route,
which digits' passes ran per column, the bytes the live passes must move (32 per row and pass: 8 for
the count read, 12 + 12 for the scatter; the key build reads the column and writes 12) and the HBM
rate that implies.

    python benchmarks/bench_sort.py [--rows 1e8] [--steps 5] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the same code at a toy size on the CPU engine (no rate is a
measurement there).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harness import check_world, emit, timed, world_info  # noqa: E402

HBM_STREAM_BPS = 6.5e12  # the streaming rate quoted in profiles/quantiles.md
PASS_BYTES = 32          # per row and live pass: count reads the key (8), scatter reads and writes key + index (12 + 12)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--cases", default="int32,f64,price,two")
    ap.add_argument("--rehearse", action="store_true", help="toy size on the CPU engine")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_sort needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    n = int(a.rows) if on_gpu else 20_000
    g = torch.Generator(device=dev).manual_seed(4321)
    key32 = torch.randint(0, 4096, (n,), generator=g, device=dev, dtype=torch.int32)
    bits = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), generator=g, device=dev, dtype=torch.int64)
    # finite values only: torch's device sort orders NaNs by their bits (negative ones first), not as one value on top
    bits = torch.where(((bits >> 52) & 0x7FF) == 0x7FF, bits & ~(1 << 52), bits).view(torch.float64)
    price = torch.floor(torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 18000.0) / 100.0 + 20.0
    valid = torch.rand(n, generator=g, device=dev) >= 0.1
    sel = torch.rand(n, generator=g, device=dev) < 0.5
    ninf = float("-inf")

    def torch_sort(keys, valids, sel_, asc):
        """LSD over the keys with torch.sort(stable=True); a null sorts first (ascending) / last
        (descending) by taking the place of -inf."""
        idx = torch.nonzero(sel_).flatten() if sel_ is not None else None
        perm = None
        for k, v, up in reversed(list(zip(keys, valids, asc))):
            rows = idx if perm is None else perm
            kk = k if rows is None else k[rows]
            if v is not None:
                kk = torch.where(v if rows is None else v[rows], kk, torch.full_like(kk, ninf))
            order = torch.sort(kk, stable=True, descending=not up).indices
            perm = order if rows is None else rows[order]
        return perm

    cases = {
        "int32": ([key32], [None], None, [True]),
        "f64": ([bits], [None], None, [True]),
        "price": ([price], [valid], sel, [True]),
        "two": ([key32, price], [None, None], None, [True, False]),
    }
    shapes, bad = {}, False
    for name in [c for c in a.cases.split(",") if c]:
        keys, valids, sel_, asc = cases[name]

        def say(what, el):
            print(f"[bench] {name} {what}: {el / a.steps * 1e3:.3f} ms per call", file=sys.stderr, flush=True)

        stats = []
        kernels.sort_permutation(keys, valids, sel_, asc, stats=stats)  # (which passes run)
        live = [s["live"] for s in reversed(stats)]  # in column order

        def perm_only():
            return kernels.sort_permutation(keys, valids, sel_, asc)

        def ours():
            p = kernels.sort_permutation(keys, valids, sel_, asc)
            return p, [k.index_select(0, p) for k in keys]

        def theirs():
            p = torch_sort(keys, valids, sel_, asc)
            return p, [k.index_select(0, p) for k in keys]

        el_p, _ = timed(perm_only, a.steps, a.warmup, dev)
        say("permutation", el_p)
        el_o, (po, _) = timed(ours, a.steps, a.warmup, dev)
        say("permutation + gather", el_o)
        el_t, (pt, _) = timed(theirs, a.steps, max(0, a.warmup - 1), dev)
        say("torch route", el_t)
        ok = torch.equal(po, pt)
        if not ok:
            print(f"[bench] {name}: the kernels and the torch route disagree", file=sys.stderr)
            bad = True
        m = int(po.numel())
        passes = sum(len(x) for x in live)
        build = sum(m * (k.element_size() + 12 + (1 if v is not None else 0)) for k, v in zip(keys, valids)) + 4 * m * (len(keys) - 1)
        moved = passes * PASS_BYTES * m + build
        ms = lambda el: el / a.steps * 1e3  # noqa: E731
        bps = moved / (ms(el_p) * 1e-3)
        shapes[name] = {"live_rows": m, "live_digits_per_column": live, "passes": passes, "permutation_ms": ms(el_p),
                        "ms_per_call": ms(el_o), "torch_route_ms": ms(el_t), "torch_over_ours": el_t / el_o,
                        "bytes_moved": moved, "implied_gbps": bps / 1e9, "hbm_stream_fraction": bps / HBM_STREAM_BPS,
                        "equal": ok}
        del po, pt
    first = shapes[next(iter(shapes))]
    emit({"metric": "ms per stable sort + gather call (int32 key, 4096 distinct values)", "value": first["ms_per_call"],
          "unit": "ms", "ms_per_step": first["ms_per_call"], "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "rows": n, "pass_bytes_per_row": PASS_BYTES, "shapes": shapes, "measured_on": str(dev),
          "data": "synthetic (uniform int32 keys, random-bit f64, two-decimal prices)", "vs_baseline": None,
          **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 2 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
