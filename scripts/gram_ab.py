"""A/B of Gram kernel variants in ONE process (interleaved rounds), 1e8 x 32 bf16."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from net.jgp.labs.sparkdq4ml_amd.ops import device  # noqa: E402

n = int(float(os.environ.get("N", "1e8")))
d = int(os.environ.get("D", "32"))
rounds = int(os.environ.get("ROUNDS", "5"))
X = torch.randn(d, n, device="cuda").to(torch.bfloat16)
y = torch.randn(n, device="cuda")
T = device.tile_bf16(X, pack=False)
# the same tiles with their 12-bit packed companion (N=1.25e7 for the 8-GPU shard)
torch.cuda.synchronize()
t0 = time.perf_counter()
Tp = device.TiledBF16(T.buf, d, n, T.shift, packed=device.pack_tiles(T))
print(f"pack_tiles {1e3 * (time.perf_counter() - t0):.2f} ms (with its counter read), packed fraction "
      f"{Tp.packed.fraction:.4f}")
# and with the patched (all-packed) companion, where the table takes it
torch.cuda.synchronize()
t0 = time.perf_counter()
Tq = device.TiledBF16(T.buf, d, n, T.shift, packed=device.patch_tiles(T))
torch.cuda.synchronize()
if Tq.packed is None:
    print("patch_tiles: the table does not take the patched form")
else:
    extra = Tq.packed.dir.numel() * 4 + Tq.packed.ovf.numel() * 4
    print(f"patch_tiles {1e3 * (time.perf_counter() - t0):.2f} ms (count pass, two reads, fill pass), "
          f"{Tq.packed.nexc} exceptions in {Tq.packed.npacked} entries ({Tq.packed.nexc / Tq.packed.npacked:.4f} each, "
          f"most {int(Tq.packed.counts.max())}), {Tq.packed.ovf.numel()} overflow records, "
          f"directory + overflow {extra / 1e6:.2f} MB beside {Tq.packed.a.numel() * 4 / 1e9:.2f} GB of slots")
ref = device.gram_stats(X, y, None, None, "bf16")
got = device.gram_stats(T, y, None, None, "bf16")
print("tiled vs plain max rel diff", float((got - ref).abs().max() / ref.abs().max()))
print("packed == tiled bitwise", bool(torch.equal(device.gram_stats(Tp, y, None, None, "bf16"), got)))
if Tq.packed is not None:
    print("patched == tiled bitwise", bool(torch.equal(device.gram_stats(Tq, y, None, None, "bf16"), got)))
bytes_x = X.numel() * 2 + y.numel() * 4


def timeit(fn, reps=10):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


variants = {
    "plain": lambda: device.gram_stats(X, y, None, None, "bf16"),
    "tiled": lambda: device.gram_stats(T, y, None, None, "bf16"),
    "packed": lambda: device.gram_stats(Tp, y, None, None, "bf16"),
    "patched": lambda: device.gram_stats(Tq, y, None, None, "bf16"),
    "read_sum": lambda: torch.sum(T.buf.view(torch.int16), dtype=torch.int64),
    "copy": lambda: T.buf.clone(),
}
only = os.environ.get("ONLY")  # e.g. ONLY=tiled,packed
if only:
    variants = {k: f for k, f in variants.items() if k in only.split(",")}
res = {k: [] for k in variants}
for r in range(rounds):
    for k, f in variants.items():
        res[k].append(timeit(f))
for k, v in res.items():
    v.sort()
    ms = v[len(v) // 2]
    # ("packed", "patched": the rate in bytes of the raw tiles they stand for, to compare with "tiled")
    gbs = (bytes_x if k in ("plain", "tiled", "packed", "patched") else T.buf.numel() * 2 * (2 if k == "copy" else 1)) / ms / 1e6
    print(f"{k:10s} median {ms:.3f} ms  min {v[0]:.3f}  -> {gbs:.0f} GB/s")
