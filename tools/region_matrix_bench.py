#!/usr/bin/env python3
"""The region score matrix against region pairs over the same cells, in one process, the legs alternated; prints one JSON line.
  op:     engine.score_matrix_regions over 32 x 32 images against engine.pair_score_regions over the same 1024 cells (features and
          masks concatenated), regions of a fraction f of the tokens at seeded positions, f = 1, 1/2, 1/4, at (N, H, D) =
          (256, 8, 160) and (1024, 8, 80); HIP-event medians after a warm-up; max_abs_score_diff must be 0.
  parent: the same two legs without masks -- engine.score_matrix against engine.pair_score, the tiled matrix_tail_kernel against the
          tiled pair_tail_kernel -- where both are tiled: (1024, 8, 80) in the run's dtype and (256, 8, 160) in fp32, each beside
          the region legs at f = 1 of the same shape and dtype.  A cell runs one attention where a pair runs two, the self pass
          amortised over the row: pairs_over_matrix of the region kernels at f = 1 should land near the parents'.
  e2e:    retrieval.score_latent_matrix with half masks against regions.score_latent_pair_regions over the same Q x G cells (SD1.5
          512 px, synthetic weights, the default tap): wall-clock of whole calls and whether the scores are bit-equal.
    python tools/region_matrix_bench.py [--dtype bf16 --side 32 --reps 20 --queries 16 --gallery 256 --e2e_reps 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402
from tools.maps_bench import B, timed_alternating  # noqa: E402


def _sets(N, H, D, dt, side, frac):
    g = torch.Generator().manual_seed(0)
    n = 2 * side
    ts = tuple(torch.randn(n, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    r = max(1, int(N * frac))
    mask = torch.zeros(n, N, dtype=torch.bool)
    for i in range(n):
        mask[i, torch.randperm(N, generator=g)[:r]] = True
    mask = mask.cuda()
    fa, fb = tuple(t[:side].contiguous() for t in ts), tuple(t[side:].contiguous() for t in ts)
    ia = torch.arange(side, dtype=torch.int32).repeat_interleave(side).cuda()
    ib = (side + torch.arange(side, dtype=torch.int32)).repeat(side).cuda()
    return ts, mask, fa, fb, mask[:side].contiguous(), mask[side:].contiguous(), ia, ib, r


def op_leg(N, H, D, dt, side, frac, sim, reps, warmup, parent=False):
    ts, mask, fa, fb, ma, mb, ia, ib, r = _sets(N, H, D, dt, side, frac)
    run_m = lambda: engine.score_matrix_regions(fa, fb, ma, mb, H, sim)               # noqa: E731
    run_p = lambda: engine.pair_score_regions(*ts, mask, ia, ib, H, sim)              # noqa: E731
    fns = [run_m, run_p]
    if parent:
        fns += [lambda: engine.score_matrix(fa, fb, H, sim), lambda: engine.pair_score(*ts, ia, ib, H, sim)]
    ms = timed_alternating(fns, reps, warmup)
    out = {"N": N, "H": H, "D": D, "dtype": str(dt).replace("torch.", ""), "fraction": frac, "region": r, "cells": side * side,
           "matrix_regions_ms": round(ms[0], 4), "pair_regions_ms": round(ms[1], 4), "pairs_over_matrix": round(ms[1] / ms[0], 3),
           "max_abs_score_diff": (run_m().flatten() - run_p()).abs().max().item()}
    if parent:
        out.update({"score_matrix_ms": round(ms[2], 4), "pair_score_ms": round(ms[3], 4), "parent_pairs_over_matrix": round(ms[3] / ms[2], 3),
                    "region_ratio_over_parent_ratio": round((ms[1] / ms[0]) / (ms[3] / ms[2]), 3),
                    "matrix_regions_over_score_matrix": round(ms[0] / ms[2], 3)})
    return out


def e2e_leg(dt, n_q, n_g, sim, reps):
    from diffsim_amd import config as C, regions as R, retrieval as RT, synth as S
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la, lb = torch.randn(n_q, 4, 64, 64, generator=g).cuda(), torch.randn(n_g, 4, 64, 64, generator=g).cuda()
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    ma, mb = torch.rand(n_q, 16, 16, generator=g) < 0.5, torch.rand(n_g, 16, 16, generator=g) < 0.5
    ma[:, 0, 0] = mb[:, 0, 0] = True
    A, Bm = la.repeat_interleave(n_g, 0), lb.repeat(n_q, 1, 1, 1)
    mA, mB = ma.repeat_interleave(n_g, 0), mb.repeat(n_q, 1, 1)
    run_m = lambda: RT.score_latent_matrix(ds, la, lb, na, nb, ctx, similarity=sim, masks_a=ma, masks_b=mb)      # noqa: E731
    run_p = lambda: R.score_latent_pair_regions(ds, A, Bm, na, nb, mA, mB, ctx, similarity=sim)                  # noqa: E731
    m, p = run_m(), run_p()                    # (the warm-up)
    torch.cuda.synchronize()
    wall = [[], []]
    for _ in range(reps):
        for fn, w in zip((run_m, run_p), wall):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            w.append(time.perf_counter() - t0)
    s_m, s_p = (sorted(w)[len(w) // 2] for w in wall)
    return {"queries": n_q, "gallery": n_g, "cells": n_q * n_g, "matrix_s": round(s_m, 4), "pairs_s": round(s_p, 4),
            "pairs_over_matrix_wall": round(s_p / s_m, 2), "scores_bit_equal": bool(torch.equal(m.flatten(), p))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--side", type=int, default=32, help="images per set of the op legs")
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--gallery", type=int, default=256)
    ap.add_argument("--e2e_reps", type=int, default=2)
    ap.add_argument("--no_e2e", action="store_true")
    ap.add_argument("--no_op", action="store_true")
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    res = {"dtype": a.dtype, "similarity": a.similarity}
    if not a.no_op:
        res["op"] = [op_leg(N, H, D, dt, a.side, f, a.similarity, a.reps, a.warmup)
                     for N, H, D in ((256, 8, 160), (1024, 8, 80)) for f in (1.0, 0.5, 0.25)]
        res["parent"] = [op_leg(1024, 8, 80, dt, a.side, 1.0, a.similarity, a.reps, a.warmup, parent=True),
                         op_leg(256, 8, 160, torch.float32, a.side, 1.0, a.similarity, a.reps, a.warmup, parent=True)]
    if not a.no_e2e:
        res["e2e"] = e2e_leg(dt, a.queries, a.gallery, a.similarity, a.e2e_reps)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
