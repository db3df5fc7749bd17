#!/usr/bin/env python3
"""ALS: one half-step (users from items) over one segment table, two ways, in one process:

  fused      the fused pass (csrc/hip/als.hip): ``device._AlsPlan.half``, at every ``--chunks`` size
  composite  torch pieces: a gather of the rated rows, ``index_add_`` of their outer products into
             [D, rank, rank] (in slices of the ratings, so the products fit), ``torch.linalg.cholesky``
             and ``torch.cholesky_solve`` -- it lives here only, not in the package

at ranks {10, 64}, f32 factors, on a uniform and a Zipf-distributed (log-uniform destination) rating
table of ``--ratings`` ratings.  Every figure is the median of ``--steps`` separately synchronised
calls after ``--warmup``, with the min and max beside it.  The gather rate counts the bytes the
algorithm needs: per rating one factor row, its index and its rating.

    python benchmarks/bench_als.py [--ratings 1e7] [--steps 7] [--warmup 2]

Needs the GPU; ``--rehearse`` runs the host twin at a toy size on the CPU (no rate is a measurement
there).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_kmeans import median_ms  # noqa: E402
from harness import check_world, emit, world_info  # noqa: E402


def composite(torch, seg, dst, Y, reg, budget=1 << 29):
    """The half-step from torch ops in f64; ``budget``: doubles of outer products per slice."""
    D, rank = seg.D, int(Y.shape[1])
    A = torch.zeros(D, rank, rank, dtype=torch.float64, device=Y.device)
    b = torch.zeros(D, rank, dtype=torch.float64, device=Y.device)
    step = max(1, budget // (rank * rank))
    for s in range(0, int(seg.src.numel()), step):
        d, Ys = dst[s:s + step], Y[seg.src[s:s + step].long()].double()
        A.index_add_(0, d, Ys[:, :, None] * Ys[:, None, :])
        b.index_add_(0, d, Ys * seg.rating[s:s + step, None])
    m = (seg.offsets[1:] - seg.offsets[:-1]).double()
    A += (reg * m.clamp_min(1.0))[:, None, None] * torch.eye(rank, dtype=torch.float64, device=Y.device)  # (empty: I x = 0)
    return torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(A))[:, :, 0].to(Y.dtype)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ratings", default="1e7")
    ap.add_argument("--users", default="2e5")
    ap.add_argument("--items", default="2e4")
    ap.add_argument("--ranks", default="10,64")
    ap.add_argument("--chunks", default="128,256,512,1024,2048", help="fused chunk sizes (ops.als.CHUNK is the default)")
    ap.add_argument("--composite-steps", type=int, default=1, help="timed composite half-steps (after one warm-up)")
    ap.add_argument("--rehearse", action="store_true", help="toy size, host twin only, on the CPU")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.gpus != 1:
        ap.error("--steps >= 1, --gpus 1")
    import torch

    from net.jgp.labs.sparkdq4ml_amd.ops import als as A
    from net.jgp.labs.sparkdq4ml_amd.parallel import comm

    comm.init()
    if not check_world(a.gpus):
        return 2
    on_gpu = torch.cuda.is_available()
    if not on_gpu and not a.rehearse:
        print("[bench] bench_als needs the GPU (--rehearse for a CPU dry run)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    nnz, D, S = (int(float(v)) for v in (a.ratings, a.users, a.items)) if on_gpu else (5000, 200, 50)
    reg, cases, ok = 0.1, [], True
    for dist in ("uniform", "zipf"):
        g = torch.Generator(device=dev).manual_seed(11)
        u = torch.rand(nnz, generator=g, device=dev, dtype=torch.float64)
        dst = (u * D).long() if dist == "uniform" else (torch.pow(float(D), u).long() - 1)  # zipf: P(d) ~ 1 / (d + 1)
        dst = dst.clamp_(0, D - 1)
        src = torch.randint(0, S, (nnz,), generator=g, device=dev)
        rating = torch.randint(1, 11, (nnz,), generator=g, device=dev).double() / 2.0
        seg = A.build_segments(dst, src, rating, D, S)
        sdst = torch.repeat_interleave(torch.arange(D, device=dev), seg.offsets[1:] - seg.offsets[:-1])
        longest = int((seg.offsets[1:] - seg.offsets[:-1]).max())
        for rank in (int(v) for v in a.ranks.split(",")):
            Y = torch.from_numpy(A.initial_factors(S, rank, 7, 1)).to(dev)
            case = {"dist": dist, "rank": rank, "ratings": nnz, "destinations": D, "sources": S, "longest_segment": longest,
                    "gather_bytes": nnz * (rank * Y.element_size() + 12)}
            if not on_gpu:
                case["host"], _ = median_ms(torch, lambda: A.als_half_step_host(seg.offsets, seg.src, seg.rating, Y, reg), 1, 0, dev)
            else:
                from net.jgp.labs.sparkdq4ml_amd.ops import device

                case["composite"], ref = median_ms(torch, lambda: composite(torch, seg, sdst, Y, reg), a.composite_steps, 1, dev)
                X = torch.empty(D, rank, dtype=Y.dtype, device=dev)
                for chunk in (int(v) for v in a.chunks.split(",")):
                    plan = device._AlsPlan(None, seg, rank, reg, Y.dtype, chunk)
                    t, _ = median_ms(torch, lambda: plan.half(1, Y, X), a.steps, a.warmup, dev)
                    t["chunks"], t["long_destinations"] = plan.sides[1].nchunks, plan.sides[1].nlong
                    case[f"fused_c{chunk}"] = t
                    # the same factors, to f32 rounding, at the size that is timed
                    rel = float((X - ref).abs().max() / ref.abs().max())
                    t["vs_composite_max_rel"], t["status"] = rel, plan.status.tolist()
                    ok = ok and rel < 1e-5 and plan.status.tolist() == [0, 0]
                    if chunk == A.CHUNK:
                        case["fused"] = t
                        case["fused_gather_gbps"] = case["gather_bytes"] / t["median_ms"] / 1e6
                        case["fused_over_composite_min"] = t["median_ms"] / case["composite"]["min_ms"]
            print(f"[bench] {case}", file=sys.stderr, flush=True)
            cases.append(case)
        del seg, dst, src, rating, sdst
    head = next((c for c in cases if c["rank"] == 10 and "fused" in c), cases[0])
    value = (head.get("fused") or head["host"])["median_ms"]
    emit({"metric": "ms per ALS half-step (rank 10, uniform table, f32 factors; fused route on the GPU)",
          "value": value, "unit": "ms", "ms_per_step": value, "higher_is_better": False, "n_gpus": 1, "steps": a.steps,
          "warmup": a.warmup, "cases": cases, "sane": ok, "measured_on": str(dev),
          "data": "synthetic (uniform sources, uniform or log-uniform destinations, half-integer ratings, unit-norm factors)",
          "vs_baseline": None, **world_info(dev)}, a.json_out)
    comm.shutdown()
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
