#!/usr/bin/env python3
"""--metric gram throughput: images/s of the VGG-19 forward to conv5_1 plus the Gram rows (the reference's last row, and with --full
the whole matrix) on batches of normalised pixels at 512 x 512 and 512 x 768, synthetic He-initialised weights, and the time per
kernel family (conv, ReLU / pool, Gram) of one profiled forward (dsim_vgg_profile) with the Gram rows' own wall time.  Prints one
JSON line.  Report only: nothing about this path has been measured before, so there is no target and no earlier number to compare with.
    python tools/gram_bench.py [--dtype bf16 --images 8 --reps 5 --out profiles/gram_bench.json]"""
import argparse
import json
import math
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


def he_state_dict(plan, seed=0):
    from diffsim_amd.gram import conv_indices
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for idx, cout in zip(conv_indices(plan), [e for e in plan if e != "P"]):
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.1
        cin = cout
    return sd


def family_of(name):
    if "conv" in name or name.startswith("gemm"):
        return "conv"
    return "relu_pool" if name.startswith("relu") else name


def bench(sc, H, W, args):
    from diffsim_amd.engine import gram_rows
    n = args.images
    pix = torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    eng = sc.engine
    step = eng.max_images(H, W, n)
    out = {}

    def forward():
        out["f"] = [eng.features(pix[i:i + step].contiguous()) for i in range(0, n, step)]

    def rows(full):
        c = sc.channels
        return [gram_rows(f, 0 if full else c - 1, c if full else 1) for f in out["f"]]

    def whole():
        forward()
        return rows(args.full)
    t_whole = median_ms(whole, args.reps, args.warmup)
    t_fwd = median_ms(forward, args.reps, 1)
    t_last = median_ms(lambda: rows(False), args.reps, 1)
    t_full = median_ms(lambda: rows(True), args.reps, 1)
    eng.profile(True)
    forward()
    fam, kernels = {}, {}
    for f, fl, by, ms in eng.profile_records():
        for table, key in ((fam, family_of(f)), (kernels, f)):
            e = table.setdefault(key, {"launches": 0, "ms": 0.0, "gflop": 0.0})
            e["launches"] += 1
            e["ms"] += ms
            e["gflop"] += fl / 1e9
    eng.profile(False)
    fam["gram_last_row"] = {"launches": len(out["f"]), "ms": t_last, "gflop": 2e-9 * n * (H // 16) * (W // 16) * sc.channels}
    fam["gram_full"] = {"launches": len(out["f"]), "ms": t_full, "gflop": 2e-9 * n * (H // 16) * (W // 16) * sc.channels ** 2}
    for table in (fam, kernels):
        for e in table.values():
            e["ms"], e["gflop"] = round(e["ms"], 4), round(e["gflop"], 3)
            e["tflops"] = round(e["gflop"] / e["ms"], 2) if e["ms"] > 0 else 0.0
    return {"H": H, "W": W, "images": n, "images_per_call": step, "descriptor": "full" if args.full else "last_row",
            "call_ms": round(t_whole, 3), "images_per_s": round(n / (t_whole / 1e3), 1), "forward_ms": round(t_fwd, 3),
            "families": dict(sorted(fam.items(), key=lambda kv: -kv[1]["ms"])),
            "kernels": dict(sorted(kernels.items(), key=lambda kv: -kv[1]["ms"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--full", action="store_true", help="time the whole-matrix descriptor in the call (default: the reference's last row)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON here")
    args = ap.parse_args()
    from diffsim_amd.gram import VGG19_PLAN, VGGGram
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    sc = VGGGram(VGG19_PLAN, he_state_dict(VGG19_PLAN), "cuda", dtype)
    res = {"bench": "gram_bench", "dtype": args.dtype, "device": torch.cuda.get_device_name(0),
           "target": "none: nothing about this path had been measured before; these figures are a first report, not a gate",
           "results": [bench(sc, 512, 512, args), bench(sc, 512, 768, args)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
