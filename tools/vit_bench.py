#!/usr/bin/env python3
"""clip_cross and dino_cross throughput: pairs/s of one scoring call over P pairs of preprocessed pixels (the ViT forward of 2 P
images to the tapped layer, then the score tail), for CLIP-B/32 and DINOv2-S/14 at 224 px, synthetic weights, and the per-family
times of one profiled forward (dsim_vit_profile) plus the tail's own wall time.  Prints one JSON line.  Report only: there is no
earlier number to compare with.
    python tools/vit_bench.py [--dtype bf16 --pairs 256 --layer 11 --reps 5 --out profiles/vit_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def bench(name, cfg, scorer_cls, args, dtype):
    from diffsim_amd import synth as S
    from diffsim_amd.engine import pair_score
    sd = S.make_state_dict(cfg, 3)
    sc = scorer_cls(cfg, sd, "cuda", dtype)
    P, L = args.pairs, min(args.layer, cfg.depth - 1)
    g = torch.Generator().manual_seed(1)
    pix = torch.randn(2 * P, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    eng = sc.engine(L)
    tail = sc.pair_tail(L) or pair_score
    ia = torch.arange(0, 2 * P, 2, dtype=torch.int32, device="cuda")
    ib = ia + 1
    feats = {}

    def forward():
        feats["f"] = eng.qkv(pix)

    def score():
        return tail(*feats["f"], ia, ib, eng.heads, "cosine")

    def whole():
        forward()
        return score()
    t_whole = median_ms(whole, args.reps, args.warmup)
    t_fwd = median_ms(forward, args.reps, 1)
    t_tail = median_ms(score, args.reps, 1)
    eng.profile(True)
    forward()
    fam = {}
    for f, fl, by, ms in eng.profile_records():
        e = fam.setdefault(f, {"launches": 0, "ms": 0.0, "gflop": 0.0})
        e["launches"] += 1
        e["ms"] += ms
        e["gflop"] += fl / 1e9
    eng.profile(False)
    for e in fam.values():
        e["ms"], e["gflop"] = round(e["ms"], 4), round(e["gflop"], 3)
    return {"model": name, "tokens": eng.tokens, "heads": eng.heads, "head_dim": eng.head_dim, "layer": L, "pairs": P,
            "call_ms": round(t_whole, 3), "pairs_per_s": round(P / (t_whole / 1e3), 1), "forward_ms": round(t_fwd, 3),
            "tail_ms": round(t_tail, 3), "tail": "pair_score_proj" if sc.pair_tail(L) else "pair_score",
            "forward_families": dict(sorted(fam.items(), key=lambda kv: -kv[1]["ms"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--layer", type=int, default=11, help="tapped layer (the deepest: the longest forward)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON here")
    args = ap.parse_args()
    from diffsim_amd import config as C
    from diffsim_amd.vit import CLIPScore, Dinov2Score
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    res = {"bench": "vit_bench", "dtype": args.dtype, "side": 224, "device": torch.cuda.get_device_name(0),
           "results": [bench("clip-vit-base-patch32", C.CLIP_B32, CLIPScore, args, dtype),
                       bench("dinov2-small", C.DINOV2_S14, Dinov2Score, args, dtype)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
