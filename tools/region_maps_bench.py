#!/usr/bin/env python3
"""Region maps and region alignments against the whole-image calls on the same features, in one process, all legs alternated;
prints one JSON line and writes it to profiles/region_maps_bench_<dtype>.json (--out; the name ends in the dtype, as
profiles/region_bench_bf16.json does: profiles/r*_bench.json are the round snapshots of bench.py, which tests/test_host.py reads).
Workload: 64 pairs of SD1.5 512-px default-tap features, (N, H, D) = (256, 8, 160), synthetic values, bf16.
  maps:  engine.pair_score_maps_regions at mask fractions f = 1, 1/2, 1/4 (seeded positions, the same size in every image)
         against engine.pair_score_maps on the same tensors -- the reference cost: the parent has no region variant to compare
         against.  At f = 1 the two do the same MFMA, exponential and product work: the ratio is the cost of the list launch, the
         index loads and the scatter;
  align: engine.pair_align_regions at the same fractions against engine.pair_align.
HIP-event times of whole calls (workspace allocation included, as a caller pays it) after warm-up, the legs alternated within
every repetition; per leg the median and the spread (min, max, the quartiles).
    python tools/region_maps_bench.py [--dtype bf16 --pairs 64 --reps 30 --warmup 3 --out profiles/region_maps_bench_bf16.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402

B = 2
FRACTIONS = (1.0, 0.5, 0.25)


def timed_alternating(fns, reps, warmup):
    """per fn: the sorted HIP-event times (ms) of reps calls, the fns taking turns inside every repetition"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, a in zip(fns, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            a.append(e0.elapsed_time(e1))
    return [sorted(a) for a in acc]


def stats(ts):
    n = len(ts)
    return {"median_ms": round(ts[n // 2], 4), "min_ms": round(ts[0], 4), "q1_ms": round(ts[n // 4], 4), "q3_ms": round(ts[(3 * n) // 4], 4),
            "max_ms": round(ts[-1], 4)}


def masks_of(n, N, frac, seed):
    g = torch.Generator().manual_seed(seed)
    r = max(1, int(N * frac))
    m = torch.zeros(n, N, dtype=torch.bool)
    for i in range(n):
        m[i, torch.randperm(N, generator=g)[:r]] = True
    return m.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/region_maps_bench_<dtype>.json; '' writes no file")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", f"region_maps_bench_{a.dtype}.json")
    if not torch.cuda.is_available():
        raise SystemExit("region_maps_bench measures on the GPU: no device found")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    N, H, D = 256, 8, 160
    n = 2 * a.pairs
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    ia = torch.arange(0, n, 2, dtype=torch.int32).cuda()
    ib = ia + 1
    masks = {f: masks_of(n, N, f, 1 + i) for i, f in enumerate(FRACTIONS)}
    legs = {"pair_score_maps": lambda: engine.pair_score_maps(q, k, v, ia, ib, H, a.similarity),
            "pair_align": lambda: engine.pair_align(q, k, ia, ib, H)}
    for f in FRACTIONS:
        legs[f"region_maps_f{f}"] = lambda m=masks[f]: engine.pair_score_maps_regions(q, k, v, m, ia, ib, H, a.similarity)
        legs[f"region_align_f{f}"] = lambda m=masks[f]: engine.pair_align_regions(q, k, m, ia, ib, H)
    names = list(legs)
    times = dict(zip(names, timed_alternating([legs[x] for x in names], a.reps, a.warmup)))
    res = {"dtype": a.dtype, "similarity": a.similarity, "N": N, "H": H, "D": D, "pairs": a.pairs, "reps": a.reps,
           "legs": {x: stats(times[x]) for x in names}}
    med = {x: res["legs"][x]["median_ms"] for x in names}
    res["ratio_over_whole_image"] = {**{f"region_maps_f{f}": round(med[f"region_maps_f{f}"] / med["pair_score_maps"], 3) for f in FRACTIONS},
                                     **{f"region_align_f{f}": round(med[f"region_align_f{f}"] / med["pair_align"], 3) for f in FRACTIONS}}
    # full masks must give the whole-image bits
    full = masks[1.0]
    res["f1_bit_identical"] = bool(all(torch.equal(x, y) for x, y in zip(engine.pair_score_maps_regions(q, k, v, full, ia, ib, H, a.similarity),
                                                                        engine.pair_score_maps(q, k, v, ia, ib, H, a.similarity))) and
                                   all(torch.equal(x, y) for x, y in zip(engine.pair_align_regions(q, k, full, ia, ib, H),
                                                                        engine.pair_align(q, k, ia, ib, H))))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
