#!/usr/bin/env python3
"""What text-guided regions cost on top of region scores with the masks handed in, in one process, the legs alternated; prints one
JSON line and writes it to profiles/text_attn_bench_sd15.json.
  regions: regions.score_latent_pair_regions with the masks the text leg produced -- the path that existed before: the walk stops at
           the tap, the region tail scores;
  text:    textattn.score_latent_pairs_text -- the walk runs on through the tapped block's self-attention, to_out, norm2 + to_q and
           the prompt's K | V projection, then text_attn_kernel + text_region_kernel, then the same region tail.
SD1.5 at 512 px (64 x 64 latents), the default tap (up_blocks 0: 256 tokens, 8 heads x 160, 77 prompt tokens), synthetic weights,
latents resident, P pairs (default 64) in one engine batch, one synthetic context, weights 1 on tokens 1-5.  Whole-call wall times
(the calls synchronise at the end): median and the spread (min - max) over the repetitions; the scores of the two legs compared
with torch.equal.  The new kernels' own time: device events around engine.text_attention alone on one batch's operands.
    python tools/text_attn_bench.py [--dtype bf16 --pairs 64 --reps 9]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed_alternating(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, a in zip(fns, acc):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            a.append(1e3 * (time.perf_counter() - t0))
    return [{"median_ms": round(sorted(a)[len(a) // 2], 3), "min_ms": round(min(a), 3), "max_ms": round(max(a), 3)} for a in acc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_attn_bench_sd15.json"))
    a = ap.parse_args()
    from diffsim_amd import config as C, engine as E, regions as RG, synth as S, textattn as TA
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.scorer import stack_rows
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    n = a.pairs
    g = torch.Generator().manual_seed(5)
    latA, latB = (torch.randn(n, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g).cuda() for _ in range(2))
    ctx = S.make_context(cfg).cuda()
    w = torch.zeros(cfg.ctx_len)
    w[1:6] = 1.0
    block, layer, step = "up_blocks", 0, 600

    def text():
        return TA.score_latent_pairs_text(ds, latA, latB, na, nb, ctx, block, layer, step, "cosine", weights=w, batch_pairs=n,
                                          return_regions=True)
    s_text, masks, counts = text()
    mA, mB = masks[:, 0].contiguous(), masks[:, 1].contiguous()

    def regions():
        return RG.score_latent_pair_regions(ds, latA, latB, na, nb, mA, mB, ctx, block, layer, step, "cosine", batch_pairs=n)
    t_regions, t_text = timed_alternating([regions, text], a.reps, a.warmup)
    equal = bool(torch.equal(regions(), s_text))
    # the two kernels alone, on one batch's operands
    tap = ds.tap_of(block, layer)
    heads = ds.engine_at(tap).heads
    _q, _k, _v, xq, xkv = ds.tap_features_text(*stack_rows([latA, latB], [na, nb], 0, n), ctx, tap, step)
    wd = w.cuda()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps + a.warmup)]
    for e0, e1 in ev:
        e0.record()
        E.text_attention(xq, xkv, heads, wd, 1.0, want=("mask", "counts"))
        e1.record()
    torch.cuda.synchronize()
    ks = sorted(e0.elapsed_time(e1) for e0, e1 in ev[a.warmup:])
    extra = t_text["median_ms"] - t_regions["median_ms"]
    res = {"model": "sd15", "px": 512, "dtype": a.dtype, "pairs": n, "tap": [block, layer], "tokens": int(xq.shape[2]), "ctx_len": int(xkv.shape[1]),
           "reps": a.reps, "regions": t_regions, "text": t_text, "text_over_regions": round(t_text["median_ms"] / t_regions["median_ms"], 4),
           "extra_ms": round(extra, 3),
           "text_attention_call": {"median_ms": round(ks[len(ks) // 2], 4), "min_ms": round(ks[0], 4), "max_ms": round(ks[-1], 4),
                                   "share_of_text_call": round(ks[len(ks) // 2] / t_text["median_ms"], 5)},
           "mean_on_fraction": round(float(counts.sum()) / masks.numel(), 4), "scores_equal": equal}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
