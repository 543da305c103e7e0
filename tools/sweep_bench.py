#!/usr/bin/env python3
"""Tap sweep against one scoring call per tap, in one process, the two alternated; prints one JSON line with two legs.
  latents: seven DiffSim.score_latent_pairs calls (one per SD1.5 tap) against one sweep.score_latent_pairs_taps(..., "all") over
           the same P latent pairs;
  pixels:  seven DiffSim.score_pairs calls (one per tap, each decoding and VAE-encoding every image with the HIP encoder) against
           one sweep.score_path_pairs_taps over the same P generated 512-px image pairs.
SD1.5 at 512 px (64 x 64 latents), synthetic weights, whole-call wall medians (the calls synchronise at the end), and the largest
score difference between the two paths of each leg (0: bit-identical).
    python tools/sweep_bench.py [--dtype bf16 --pairs 64 --reps 3 --no_pixels]"""
import argparse
import json
import os
import sys
import tempfile
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
    return [sorted(a)[len(a) // 2] for a in acc]


def _images(root, n_pairs):
    from PIL import Image
    from diffsim_amd import synth as S
    pairs = []
    for i in range(n_pairs):
        ims = []
        for j, t in enumerate(S.make_image_pair(i, 512)):
            px = ((t[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
            p = os.path.join(root, f"p{i}_{j}.png")
            Image.fromarray(px).save(p)
            ims.append(p)
        pairs.append(tuple(ims))
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no_pixels", action="store_true")
    a = ap.parse_args()
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    from diffsim_amd.sweep import all_taps, score_latent_pairs_taps, score_path_pairs_taps
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("conv_norm_out", "conv_out"))])
    vae = None if a.no_pixels else VAEEncoder(C.VAE_SD15, S.make_state_dict(C.VAE_SD15, seed=1), torch.bfloat16, "cuda")
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd, vae=vae)
    ctx = S.make_context(cfg)
    taps = all_taps(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = (torch.randn(a.pairs, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    sim = a.similarity
    run_one = lambda: torch.stack([ds.score_latent_pairs(la, lb, na, nb, ctx, b, l, 600, sim) for b, l in taps])   # noqa: E731
    run_sw = lambda: score_latent_pairs_taps(ds, la, lb, na, nb, ctx, "all", 600, sim)                            # noqa: E731
    ms_one, ms_sw = timed_alternating([run_one, run_sw], a.reps, a.warmup)
    res = {"dtype": a.dtype, "pairs": a.pairs, "taps": len(taps), "similarity": sim,
           "latents": {"per_tap_calls_ms": round(ms_one, 2), "sweep_ms": round(ms_sw, 2), "ratio_sweep_over_calls": round(ms_sw / ms_one, 4),
                       "max_abs_score_diff": (run_one() - run_sw()).abs().max().item()}}
    if not a.no_pixels:
        with tempfile.TemporaryDirectory() as tmp:
            pairs = _images(tmp, a.pairs)
            one = lambda: torch.stack([ds.score_pairs(pairs, 512, ctx, b, l, 600, seed=2333, similarity=sim) for b, l in taps])  # noqa
            sw = lambda: score_path_pairs_taps(ds, pairs, 512, ctx, "all", 600, sim, 2333)                                   # noqa
            ms_one, ms_sw = timed_alternating([one, sw], a.reps, a.warmup)
            res["pixels"] = {"per_tap_calls_ms": round(ms_one, 2), "sweep_ms": round(ms_sw, 2),
                             "ratio_sweep_over_calls": round(ms_sw / ms_one, 4), "max_abs_score_diff": (one() - sw()).abs().max().item()}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
