#!/usr/bin/env python3
"""Exemplar-guided retrieval against the routes that existed before it, in one process, the sides alternated; prints one JSON line
with three legs (report only, no target) for an 8 x 64 matrix of bf16 features.
  transfer: engine.region_transfer_matrix (one launch, 512 cells) against engine.pair_region_transfer(directions=2) over the same
            512 cells on torch.cat of the sets, HIP-event medians of 20 after a warm-up, at (N, H, D) = (256, 8, 160) (SD1.5's
            default tap) and (1024, 8, 80);
  cells:    engine.score_matrix_cell_regions against engine.score_matrix_regions with the same regions handed in per image (every
            cell of a column gets the gallery image's one mask): a floor, not a target -- three attentions per cell against two;
  e2e:      a whole retrieval.score_latent_matrix_exemplar call on SD1.5 512-px latents (synthetic weights, the default tap)
            against the same call with both masks handed in (the region matrix) and against the 512 cells through
            transfer.score_latent_pairs_exemplar, HIP-event medians of whole calls.
    python tools/exemplar_matrix_bench.py [--n_a 8 --n_b 64 --reps 20 --e2e_reps 3 --no_e2e --out profiles/exemplar_matrix_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402
from tools.maps_bench import timed_alternating  # noqa: E402

B = 2


def _sets(N, H, D, n_a, n_b, seed):
    g = torch.Generator().manual_seed(seed)
    ts = tuple(torch.randn(n_a + n_b, B, N, H * D, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    return ts, tuple(t[:n_a].contiguous() for t in ts), tuple(t[n_a:].contiguous() for t in ts), g


def transfer_leg(N, H, D, n_a, n_b, reps, warmup):
    (q, k, _v), fa, fb, g = _sets(N, H, D, n_a, n_b, 0)
    w = torch.randint(0, 256, (n_a + n_b, N), generator=g, dtype=torch.uint8).cuda()
    wa = w[:n_a].contiguous()
    ia = torch.arange(n_a, dtype=torch.int32).repeat_interleave(n_b).cuda()
    ib = (n_a + torch.arange(n_b, dtype=torch.int32)).repeat(n_a).cuda()
    new = lambda: engine.region_transfer_matrix(fa, fb, wa, H)                                   # noqa: E731
    old = lambda: engine.pair_region_transfer(q, k, w, ia, ib, H, directions=2)                  # noqa: E731
    same = bool(torch.equal(new().view(n_a * n_b, N), old()[:, 1]))
    ms_new, ms_old = timed_alternating([new, old], reps, warmup)
    return {"dtype": "bf16", "N": N, "H": H, "D": D, "n_a": n_a, "n_b": n_b, "transfer_matrix_ms": round(ms_new, 4),
            "pair_transfer_ms": round(ms_old, 4), "speedup": round(ms_old / ms_new, 2), "bit_equal": same}


def cells_leg(N, H, D, n_a, n_b, reps, warmup):
    _ts, fa, fb, g = _sets(N, H, D, n_a, n_b, 1)
    m = torch.rand(n_a + n_b, N, generator=g) < 0.5
    m[:, 0] = True
    ma, mb = m[:n_a].cuda().contiguous(), m[n_a:].cuda().contiguous()
    cells = mb.unsqueeze(0).expand(n_a, n_b, N).contiguous()
    new = lambda: engine.score_matrix_cell_regions(fa, fb, ma, cells, H, "cosine")               # noqa: E731
    old = lambda: engine.score_matrix_regions(fa, fb, ma, mb, H, "cosine")                       # noqa: E731
    same = bool(torch.equal(new(), old()))
    ms_new, ms_old = timed_alternating([new, old], reps, warmup)
    return {"dtype": "bf16", "N": N, "H": H, "D": D, "n_a": n_a, "n_b": n_b, "cell_regions_ms": round(ms_new, 4),
            "region_matrix_ms": round(ms_old, 4), "ratio_cell_over_region_matrix": round(ms_new / ms_old, 3), "bit_equal": same}


def e2e_leg(n_a, n_b, reps):
    from diffsim_amd import config as C, regions as R, retrieval, synth as S, transfer as X
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = torch.randn(n_a, 4, 64, 64, generator=g).cuda(), torch.randn(n_b, 4, 64, 64, generator=g).cuda()
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    grid = R.tap_grid(ds, ds.tap_of("up_blocks", 0), 64)
    mA = torch.rand(n_a, *grid, generator=g) < 0.5
    mA[:, 0, 0] = True
    _m, regs, _mass = retrieval.score_latent_matrix_exemplar(ds, la, lb, na, nb, ctx, masks_a=mA, exemplar=X.ExemplarGuide(), return_regions=True)
    mB = regs[0].cpu()                                             # one mask per gallery image for the region matrix: query 0's row
    pa, pb, pm = la.repeat_interleave(n_b, 0), lb.repeat(n_a, 1, 1, 1), mA.repeat_interleave(n_b, 0)
    run_x = lambda: retrieval.score_latent_matrix_exemplar(ds, la, lb, na, nb, ctx, masks_a=mA, exemplar=X.ExemplarGuide())      # noqa: E731
    run_r = lambda: retrieval.score_latent_matrix(ds, la, lb, na, nb, ctx, masks_a=mA, masks_b=mB)                     # noqa: E731
    run_p = lambda: X.score_latent_pairs_exemplar(ds, pa, pb, na, nb, pm, ctx)                                         # noqa: E731
    same = bool(torch.equal(run_x().flatten(), run_p()))
    ms_x, ms_r, ms_p = timed_alternating([run_x, run_r, run_p], reps, 1)
    return {"dtype": "bf16", "n_a": n_a, "n_b": n_b, "exemplar_matrix_ms": round(ms_x, 2), "region_matrix_masks_handed_in_ms": round(ms_r, 2),
            "pairs_exemplar_ms": round(ms_p, 2), "ratio_exemplar_over_region_matrix": round(ms_x / ms_r, 3),
            "speedup_over_pairs": round(ms_p / ms_x, 2), "bit_equal_to_pairs": same, "mean_share_on": round(float(regs.float().mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_a", type=int, default=8)
    ap.add_argument("--n_b", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e_reps", type=int, default=3)
    ap.add_argument("--no_e2e", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON there")
    a = ap.parse_args()
    sizes = ((256, 8, 160), (1024, 8, 80))
    res = {"transfer": [transfer_leg(N, H, D, a.n_a, a.n_b, a.reps, a.warmup) for N, H, D in sizes],
           "cells": [cells_leg(N, H, D, a.n_a, a.n_b, a.reps, a.warmup) for N, H, D in sizes]}
    if not a.no_e2e:
        res["e2e"] = e2e_leg(a.n_a, a.n_b, a.e2e_reps)
    text = json.dumps(res)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
