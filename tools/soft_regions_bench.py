#!/usr/bin/env python3
"""Soft region scores against region scores on the same work, in one process, the two alternated; prints one JSON line and writes it
to profiles/soft_regions_bench.json.
  engine.pair_score_weights with every byte 255 against engine.pair_score_regions with full masks -- the same rows, MFMAs,
  exponentials and products (the scores agree bit for bit), the difference being the soft tail's extra work: one f32 add per score
  element, the bias loads, the query weight and the weights kernel -- on the same 64 pairs of synthetic bf16 features at
  (N, H, D) = (256, 8, 160) and (1024, 8, 80), HIP-event medians of whole calls after warm-up.
    python tools/soft_regions_bench.py [--dtype bf16 --pairs 64 --reps 50 --warmup 5 --out profiles/soft_regions_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402
from tools.maps_bench import B  # noqa: E402


def timed_alternating(fns, reps, warmup):
    """tools/maps_bench.py's alternation, keeping the quartiles: [(median, p25, p75) ms per fn]"""
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
    return [(sorted(a)[len(a) // 2], sorted(a)[len(a) // 4], sorted(a)[3 * len(a) // 4]) for a in acc]


def leg(N, H, D, dt, n_pairs, sim, reps, warmup):
    g = torch.Generator().manual_seed(0)
    n = 2 * n_pairs
    q, k, v = (torch.randn(n, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    mask = torch.ones(n, N, dtype=torch.bool, device="cuda")
    w = torch.full((n, N), 255, dtype=torch.uint8, device="cuda")
    ia = torch.arange(0, n, 2, dtype=torch.int32).cuda()
    ib = ia + 1
    run_w = lambda: engine.pair_score_weights(q, k, v, w, ia, ib, H, sim)            # noqa: E731
    run_r = lambda: engine.pair_score_regions(q, k, v, mask, ia, ib, H, sim)         # noqa: E731
    (ms_w, w25, w75), (ms_r, r25, r75) = timed_alternating([run_w, run_r], reps, warmup)
    same = bool(torch.equal(run_w(), run_r()))
    return {"N": N, "H": H, "D": D, "pairs": n_pairs, "weights_ms": round(ms_w, 4), "weights_ms_quartiles": [round(w25, 4), round(w75, 4)],
            "regions_ms": round(ms_r, 4), "regions_ms_quartiles": [round(r25, 4), round(r75, 4)],
            "ratio_weights_over_regions": round(ms_w / ms_r, 4), "scores_bit_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_regions_bench.json"))
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    res = {"tool": "tools/soft_regions_bench.py", "device": torch.cuda.get_device_name(0), "dtype": a.dtype, "similarity": a.similarity,
           "reps": a.reps, "warmup": a.warmup, "timing": "HIP events around whole calls, the two alternated, medians",
           "legs": [leg(N, H, D, dt, a.pairs, a.similarity, a.reps, a.warmup) for N, H, D in ((256, 8, 160), (1024, 8, 80))]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
