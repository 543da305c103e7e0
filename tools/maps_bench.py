#!/usr/bin/env python3
"""Similarity maps against the pair score, in one process, the two alternated; prints one JSON line with two legs.
  tail: engine.pair_score_maps against engine.pair_score on the same 64 pairs of synthetic features, HIP-event medians after
        warm-up, at SD1.5's default tap (256 tokens, 8 heads x 160: the 16-bit pair path is the persistent d = 160 kernel there,
        the maps path the generic pair_map_kernel) and at (N, H, D) = (1024, 8, 80);
  e2e:  maps.score_latent_pair_maps against DiffSim.score_latent_pairs for P SD1.5 512-px latent pairs (synthetic weights, the
        default tap), HIP-event medians of whole calls, in pairs/s.
    python tools/maps_bench.py [--dtype bf16 --pairs 64 --reps 20 --e2e_reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402

B = 2


def timed_alternating(fns, reps, warmup):
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
    return [sorted(a)[len(a) // 2] for a in acc]


def tail_leg(N, H, D, dt, n_pairs, sim, reps, warmup):
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2 * n_pairs, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    ia = torch.arange(0, 2 * n_pairs, 2, dtype=torch.int32).cuda()
    ib = ia + 1
    run_m = lambda: engine.pair_score_maps(q, k, v, ia, ib, H, sim)          # noqa: E731
    run_p = lambda: engine.pair_score(q, k, v, ia, ib, H, sim)               # noqa: E731
    ms_m, ms_p = timed_alternating([run_m, run_p], reps, warmup)
    diff = (run_m()[0] - run_p()).abs().max().item()
    return {"N": N, "H": H, "D": D, "pairs": n_pairs, "maps_ms": round(ms_m, 4), "pair_ms": round(ms_p, 4),
            "ratio_maps_over_pair": round(ms_m / ms_p, 3), "max_abs_score_diff": diff}


def e2e_leg(dt, n_pairs, sim, reps):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = (torch.randn(n_pairs, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    run_m = lambda: ds.score_latent_pair_maps(la, lb, na, nb, ctx, similarity=sim)     # noqa: E731
    run_p = lambda: ds.score_latent_pairs(la, lb, na, nb, ctx, similarity=sim)         # noqa: E731
    ms_m, ms_p = timed_alternating([run_m, run_p], reps, 1)
    diff = (run_m().score - run_p()).abs().max().item()
    return {"pairs": n_pairs, "maps_pairs_per_s": round(1e3 * n_pairs / ms_m, 1), "pairs_per_s": round(1e3 * n_pairs / ms_p, 1),
            "ratio_maps_over_pairs_rate": round(ms_p / ms_m, 4), "max_abs_score_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e_reps", type=int, default=5)
    ap.add_argument("--no_e2e", action="store_true")
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    res = {"dtype": a.dtype, "similarity": a.similarity,
           "tail": [tail_leg(N, H, D, dt, a.pairs, a.similarity, a.reps, a.warmup) for N, H, D in ((256, 8, 160), (1024, 8, 80))]}
    if not a.no_e2e:
        res["e2e"] = e2e_leg(dt, a.pairs, a.similarity, a.e2e_reps)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
