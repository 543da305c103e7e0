#!/usr/bin/env python3
"""Region transfer against the route that existed before it, in one process, the two alternated; prints one JSON line with two legs
(report only, no target).
  kernel: engine.pair_region_transfer against engine.pair_align(..., return_attention=True) followed by the torch contraction of
          the attention with the key image's weights, on the same 64 pairs of synthetic bf16 features with random byte weights,
          HIP-event medians of 20 after a warm-up, at (N, H, D) = (256, 8, 160) (SD1.5's default tap) and (1024, 8, 80);
  e2e:    score_latent_pairs_exemplar (a mask for image A alone; B's region transferred) against score_latent_pair_regions with the
          same two masks handed in, for P SD1.5 512-px latent pairs (synthetic weights, the default tap), HIP-event medians of whole
          calls, in pairs/s: what the transfer launch and the region rule add to a region-score run.
    python tools/transfer_bench.py [--pairs 64 --reps 20 --e2e_reps 5 --no_e2e --out profiles/transfer_bench.json]"""
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


def kernel_leg(N, H, D, n_pairs, reps, warmup):
    g = torch.Generator().manual_seed(0)
    q, k = (torch.randn(2 * n_pairs, B, N, H * D, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    w = torch.randint(0, 256, (2 * n_pairs, N), generator=g, dtype=torch.uint8).cuda()
    ia = torch.arange(0, 2 * n_pairs, 2, dtype=torch.int32).cuda()
    ib = ia + 1

    def old():
        attn = engine.pair_align(q, k, ia, ib, H, return_attention=True)[3]
        wk = torch.stack([w[ib.long()], w[ia.long()]], 1).float() / 255.0               # the key image's weights per direction
        return torch.einsum("pdij,pdj->pdi", attn, wk)
    new = lambda: engine.pair_region_transfer(q, k, w, ia, ib, H)                        # noqa: E731
    diff = (old() - new()).abs().max().item()
    ms_new, ms_old = timed_alternating([new, old], reps, warmup)
    return {"dtype": "bf16", "N": N, "H": H, "D": D, "pairs": n_pairs, "transfer_ms": round(ms_new, 4),
            "align_attention_contraction_ms": round(ms_old, 4), "speedup": round(ms_old / ms_new, 2), "max_abs_difference": diff}


def e2e_leg(n_pairs, reps):
    from diffsim_amd import config as C, regions as R, synth as S, transfer as X
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = (torch.randn(n_pairs, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    grid = R.tap_grid(ds, ds.tap_of("up_blocks", 0), 64)
    mA = torch.rand(n_pairs, *grid, generator=g) < 0.5
    mA[:, 0, 0] = True
    _s, regs, _m = X.score_latent_pairs_exemplar(ds, la, lb, na, nb, mA, ctx, return_regions=True)
    mB = regs[:, 1].cpu()
    run_x = lambda: X.score_latent_pairs_exemplar(ds, la, lb, na, nb, mA, ctx)           # noqa: E731
    run_r = lambda: R.score_latent_pair_regions(ds, la, lb, na, nb, mA, mB, ctx)         # noqa: E731
    ms_x, ms_r = timed_alternating([run_x, run_r], reps, 1)
    return {"dtype": "bf16", "pairs": n_pairs, "exemplar_pairs_per_s": round(1e3 * n_pairs / ms_x, 1),
            "regions_pairs_per_s": round(1e3 * n_pairs / ms_r, 1), "ratio_exemplar_over_regions_rate": round(ms_r / ms_x, 4),
            "mean_share_on": round(float(mB.float().mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e_reps", type=int, default=5)
    ap.add_argument("--no_e2e", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON there")
    a = ap.parse_args()
    res = {"kernel": [kernel_leg(N, H, D, a.pairs, a.reps, a.warmup) for N, H, D in ((256, 8, 160), (1024, 8, 80))]}
    if not a.no_e2e:
        res["e2e"] = e2e_leg(a.pairs, a.e2e_reps)
    text = json.dumps(res)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
