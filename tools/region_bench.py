#!/usr/bin/env python3
"""Region scores against the pair score on physically compacted features, in one process, the two alternated; prints one JSON
line with two legs.
  tail: engine.pair_score_regions over regions of a fraction f of the tokens (seeded positions, the same size in every image)
        against engine.pair_score on the (n, B, f N, H*D) tensors of the regions' rows -- the same MFMA, exponential and product
        work, the gather being the difference -- on the same 64 pairs of synthetic features, HIP-event medians after warm-up, at
        (N, H, D) = (1024, 8, 80) and (256, 8, 160), f = 1, 1/2, 1/4.  At f = 1 of (256, 8, 160) the 16-bit pair score is the
        persistent kernel: the partner there is engine.pair_score_maps, the tiled kernel;
  e2e:  regions.score_latent_pair_regions (half masks) against DiffSim.score_latent_pairs for P SD1.5 512-px latent pairs
        (synthetic weights, the default tap), HIP-event medians of whole calls, in pairs/s.
    python tools/region_bench.py [--dtype bf16 --pairs 64 --reps 20 --e2e_reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402
from tools.maps_bench import B, timed_alternating  # noqa: E402


def tail_leg(N, H, D, dt, frac, n_pairs, sim, reps, warmup):
    g = torch.Generator().manual_seed(0)
    n = 2 * n_pairs
    q, k, v = (torch.randn(n, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    r = max(1, int(N * frac))
    mask = torch.zeros(n, N, dtype=torch.bool)
    for i in range(n):
        mask[i, torch.randperm(N, generator=g)[:r]] = True
    mask = mask.cuda()
    rows = mask.nonzero()[:, 1].view(n, r)
    cq, ck, cv = (torch.stack([t[i].index_select(1, rows[i]) for i in range(n)]).contiguous() for t in (q, k, v))
    ia = torch.arange(0, n, 2, dtype=torch.int32).cuda()
    ib = ia + 1
    persistent = dt != torch.float32 and (r, D) == (256, 160)
    run_r = lambda: engine.pair_score_regions(q, k, v, mask, ia, ib, H, sim)                                   # noqa: E731
    run_p = (lambda: engine.pair_score_maps(cq, ck, cv, ia, ib, H, sim)[0]) if persistent else \
            (lambda: engine.pair_score(cq, ck, cv, ia, ib, H, sim))                                            # noqa: E731
    ms_r, ms_p = timed_alternating([run_r, run_p], reps, warmup)
    diff = (run_r() - run_p()).abs().max().item()
    return {"N": N, "H": H, "D": D, "fraction": frac, "region": r, "pairs": n_pairs, "partner": "pair_score_maps" if persistent else "pair_score",
            "regions_ms": round(ms_r, 4), "compacted_ms": round(ms_p, 4), "ratio_regions_over_compacted": round(ms_r / ms_p, 3),
            "max_abs_score_diff": diff}


def e2e_leg(dt, n_pairs, sim, reps):
    from diffsim_amd import config as C, regions as R, synth as S
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = (torch.randn(n_pairs, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    ma, mb = (torch.rand(n_pairs, 16, 16, generator=g) < 0.5 for _ in range(2))
    ma[:, 0, 0] = mb[:, 0, 0] = True
    run_r = lambda: R.score_latent_pair_regions(ds, la, lb, na, nb, ma, mb, ctx, similarity=sim)    # noqa: E731
    run_p = lambda: ds.score_latent_pairs(la, lb, na, nb, ctx, similarity=sim)                     # noqa: E731
    ms_r, ms_p = timed_alternating([run_r, run_p], reps, 1)
    return {"pairs": n_pairs, "regions_pairs_per_s": round(1e3 * n_pairs / ms_r, 1), "pairs_per_s": round(1e3 * n_pairs / ms_p, 1),
            "ratio_regions_over_pairs_rate": round(ms_p / ms_r, 4)}


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
           "tail": [tail_leg(N, H, D, dt, f, a.pairs, a.similarity, a.reps, a.warmup)
                    for N, H, D in ((1024, 8, 80), (256, 8, 160)) for f in (1.0, 0.5, 0.25)]}
    if not a.no_e2e:
        res["e2e"] = e2e_leg(dt, a.pairs, a.similarity, a.e2e_reps)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
