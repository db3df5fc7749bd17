#!/usr/bin/env python3
"""Hash equi-join: ``kernels.join_pairs`` / ``join_mask`` (``ops/csrc/hip/join.hip``) on int64 keys, for

  lookup       1e8 left rows against 1e6 unique right keys, inner (the dimension-table case)
  lookup_miss  the same as a left outer join with 10 % misses
  fanout       2e7 left rows against 1e6 right rows over 2.5e5 keys (4 matches each, 8e7 pairs)
  skew         fanout with one key holding 1 % of the right rows
  semi         1e8 against 1e6, the mask only

against the torch route a user has today, timed in the same process: a stable ``torch.sort`` of
the right keys, two ``searchsorted`` of the left keys, then ``repeat_interleave`` and arithmetic.
Both routes must return equal pairs in the same order; a mismatch exits 2.

Reported per case: ms per call of both routes, the split build / layout / probe / expand (build
and layout timed on their own, probe as the mask-only join minus the build, expand as the rest),
the bytes each phase must move at the least (keys read once, every result array written once; the
table's random accesses are not counted) and the HBM rate that implies.

    python benchmarks/bench_join.py [--rows 1e8] [--steps 5] [--warmup 2]

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=float, default=1e8, help="left rows of the lookup cases (fanout: a fifth; right: a hundredth)")
    ap.add_argument("--cases", default="lookup,lookup_miss,fanout,skew,semi")
    ap.add_argument("--rehearse", action="store_true", help="toy size on the CPU engine")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import kernels
    from net.jgp.labs.sparkdq4ml_amd.ops.join import join_capacity
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_join needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    n = int(a.rows) if on_gpu else 20_000
    nr = max(n // 100, 8)
    nf, nk = max(n // 5, 8), max(nr // 4, 2)
    g = torch.Generator(device=dev).manual_seed(8642)
    ri64 = lambda hi, m: torch.randint(0, hi, (m,), generator=g, device=dev, dtype=torch.int64)  # noqa: E731
    r_unique = torch.randperm(nr, generator=g, device=dev)
    r_fan = (torch.arange(nr, device=dev) % nk)[torch.randperm(nr, generator=g, device=dev)]
    r_skew = r_fan.clone()
    r_skew[torch.randperm(nr, generator=g, device=dev)[:max(nr // 100, 1)]] = 0
    l_hit, l_miss, l_fan = ri64(nr, n), ri64(int(nr / 0.9), n), ri64(nk, nf)

    def torch_route(lk, rk, how):
        srk, order = torch.sort(rk, stable=True)
        lo = torch.searchsorted(srk, lk, right=False)
        c = torch.searchsorted(srk, lk, right=True) - lo
        if how == "semi":
            return (c > 0,)
        pc = c if how == "inner" else torch.clamp(c, min=1)
        li = torch.repeat_interleave(torch.arange(lk.numel(), device=dev), pc)
        off = torch.cumsum(pc, 0) - pc
        k = torch.arange(li.numel(), device=dev) - off[li]
        ri = torch.where(c[li] > 0, order[(lo[li] + k).clamp(max=rk.numel() - 1)], torch.full_like(li, -1))
        return li, ri

    cases = {
        "lookup": (l_hit, r_unique, "inner"),
        "lookup_miss": (l_miss, r_unique, "left_outer"),
        "fanout": (l_fan, r_fan, "inner"),
        "skew": (l_fan, r_skew, "inner"),
        "semi": (l_miss, r_unique, "semi"),
    }
    shapes, bad = {}, False
    for name in [c for c in a.cases.split(",") if c]:
        lk, rk, how = cases[name]
        ms = lambda el: el / a.steps * 1e3  # noqa: E731

        def say(what, el):
            print(f"[bench] {name} {what}: {ms(el):.3f} ms per call", file=sys.stderr, flush=True)

        def mask_only():
            return (kernels.join_mask(lk, rk),)

        def ours():
            return mask_only() if how == "semi" else kernels.join_pairs(lk, rk, how=how)

        stats = []
        (kernels.join_mask(lk, rk, stats=stats) if how == "semi" else kernels.join_pairs(lk, rk, how=how, stats=stats))
        st = stats[0]
        el_o, out_o = timed(ours, a.steps, a.warmup, dev)
        say("join", el_o)
        el_t, out_t = timed(lambda: torch_route(lk, rk, how), a.steps, max(0, a.warmup - 1), dev)
        say("torch route", el_t)
        ok = len(out_o) == len(out_t) and all(torch.equal(x, y) for x, y in zip(out_o, out_t))
        if not ok:
            print(f"[bench] {name}: the kernels and the torch route disagree", file=sys.stderr)
            bad = True
        pairs = int(out_o[0].numel()) if how != "semi" else 0
        del out_o, out_t
        nl, nrr, cap = int(lk.numel()), int(rk.numel()), join_capacity(int(rk.numel()))
        # the least each phase moves: keys read once (8 bytes), every array it produces written once
        byts = {"build": nrr * (8 + 4) + cap * (8 + 4 + 4), "layout": 0 if st["unique_build"] else nrr * (4 + 4 + 4) + cap * 8,
                "probe": nl * (8 + (1 if how == "semi" else 4 + 4)),
                "expand": 0 if how == "semi" else nl * (4 + 8 + 8 + 4) + pairs * 16}
        split = {}
        if on_gpu:
            from net.jgp.labs.sparkdq4ml_amd.ops import device, native

            h = native.hip()
            el_b, _ = timed(lambda: device._JoinBuild(h, rk, None, None, None, None), a.steps, 1, dev)

            def build_layout():
                b = device._JoinBuild(h, rk, None, None, None, None)
                b.layout(None)
                return b

            el_bl, _ = timed(build_layout, a.steps, 1, dev)
            el_m, _ = (el_o, None) if how == "semi" else timed(mask_only, a.steps, 1, dev)
            split = {"build_ms": ms(el_b), "layout_ms": ms(el_bl - el_b), "probe_ms": ms(el_m - el_b),
                     "expand_ms": ms(el_o - el_m - (el_bl - el_b))}
            for k, v in split.items():
                print(f"[bench] {name} {k}: {v:.3f}", file=sys.stderr, flush=True)
        moved = sum(byts.values())
        bps = moved / (ms(el_o) * 1e-3)
        shapes[name] = {"left_rows": nl, "right_rows": nrr, "how": how, "pairs": st["pairs"], "distinct": st["distinct"],
                        "unique_build": st["unique_build"], "capacity": st.get("capacity"), "ms_per_call": ms(el_o),
                        "torch_route_ms": ms(el_t), "torch_over_ours": el_t / el_o, **split, "bytes_least": byts,
                        "implied_gbps": bps / 1e9, "hbm_stream_fraction": bps / HBM_STREAM_BPS, "equal": ok}
    first = shapes[next(iter(shapes))]
    emit({"metric": "ms per inner hash join call (1e8 left rows, 1e6 unique int64 right keys)", "value": first["ms_per_call"],
          "unit": "ms", "ms_per_step": first["ms_per_call"], "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "rows": n, "shapes": shapes, "measured_on": str(dev),
          "data": "synthetic (uniform int64 keys; fanout: 4 right rows per key; skew: one key with 1 % of the right rows)",
          "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 2 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
