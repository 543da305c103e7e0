#!/usr/bin/env python3
"""Score matrix against the pair path at SD1.5's default tap (256 tokens, 8 heads x 160, CFG batch 2), op level: score_matrix of
n_a x n_b features against pair_score over the same n_a * n_b index pairs, in one process, the two alternated and timed by HIP
events after warm-up.  Algorithmic FLOPs: an SDPA of (2, 8, 256, 160) is 4 * 2 * 8 * 256 * 256 * 160 = 671 MFLOP; a matrix
counts 2 per cell plus n_a + n_b self SDPAs, the pair path 4 per pair.  Prints one JSON line.
--e2e Q G: then the end-to-end leg in the same process -- retrieval.score_latent_matrix of Q query x G gallery latents (SD1.5 at
512 px, synthetic weights, the default tap) in cells/s beside DiffSim.score_latent_pairs over G pairs in pairs/s, wall clock after
a warm-up call of each; prints a second JSON line.
    python tools/matrix_bench.py [--na 64 --nb 64 --dtype bf16 --reps 20] [--e2e 16 1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402

B, H, N, D = 2, 8, 256, 160
SDPA_FLOP = 4.0 * B * H * N * N * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=64)
    ap.add_argument("--nb", type=int, default=64)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--e2e", type=int, nargs=2, default=None, metavar=("Q", "G"))
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(0)
    fa = tuple(torch.randn(a.na, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    fb = tuple(torch.randn(a.nb, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    q, k, v = (torch.cat([x, y]).contiguous() for x, y in zip(fa, fb))
    ia = torch.arange(a.na, dtype=torch.int32).repeat_interleave(a.nb).cuda()
    ib = (a.na + torch.arange(a.nb, dtype=torch.int32)).repeat(a.na).cuda()
    run_m = lambda: engine.score_matrix(fa, fb, H, a.similarity)              # noqa: E731
    run_p = lambda: engine.pair_score(q, k, v, ia, ib, H, a.similarity)       # noqa: E731
    for _ in range(a.warmup):
        run_m(), run_p()
    torch.cuda.synchronize()
    tm, tp = [], []
    for _ in range(a.reps):
        for fn, acc in ((run_m, tm), (run_p, tp)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    med = lambda xs: sorted(xs)[len(xs) // 2]                                 # noqa: E731
    cells = a.na * a.nb
    ms_m, ms_p = med(tm), med(tp)
    fl_m = (2.0 * cells + a.na + a.nb) * SDPA_FLOP
    fl_p = 4.0 * cells * SDPA_FLOP
    diff = (run_m().flatten() - run_p()).abs().max().item()
    res = {"dtype": a.dtype, "similarity": a.similarity, "n_a": a.na, "n_b": a.nb, "reps": a.reps,
           "matrix_ms": round(ms_m, 4), "pair_ms": round(ms_p, 4),
           "matrix_us_per_cell": round(1e3 * ms_m / cells, 3), "pair_us_per_pair": round(1e3 * ms_p / cells, 3),
           "ratio_cell_over_pair": round(ms_m / ms_p, 4),
           "matrix_tflops": round(fl_m / ms_m / 1e9, 1), "pair_tflops": round(fl_p / ms_p / 1e9, 1),
           "max_abs_diff_matrix_vs_pair": diff,
           "matrix_ms_all": [round(x, 4) for x in tm], "pair_ms_all": [round(x, 4) for x in tp]}
    print(json.dumps(res), flush=True)
    if a.e2e:
        del fa, fb, q, k, v
        print(json.dumps(e2e(a.e2e[0], a.e2e[1], dt, a.similarity)), flush=True)
    return 0


def e2e(nq, ng, dt, sim):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    ctx = S.make_context(cfg)
    g = torch.Generator().manual_seed(5)
    la = torch.randn(nq, 4, 64, 64, generator=g).cuda()
    lb = torch.randn(ng, 4, 64, 64, generator=g).cuda()
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    pa = la[torch.arange(ng) % nq]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    ds.score_latent_matrix(la[:2], lb[:8], na, nb, ctx, similarity=sim)           # warm-up (code objects, workspaces)
    ds.score_latent_pairs(pa[:64], lb[:64], na, nb, ctx, similarity=sim)
    tm, m = timed(lambda: ds.score_latent_matrix(la, lb, na, nb, ctx, similarity=sim))
    tp, p = timed(lambda: ds.score_latent_pairs(pa, lb, na, nb, ctx, similarity=sim))
    same = bool(torch.equal(m[torch.arange(ng) % nq, torch.arange(ng)], p))
    return {"leg": "e2e", "dtype": str(dt).split(".")[-1], "similarity": sim, "queries": nq, "gallery": ng,
            "matrix_s": round(tm, 3), "matrix_cells_per_s": round(nq * ng / tm, 1), "matrix_forwards": nq + ng,
            "pairs": ng, "pairs_s": round(tp, 3), "pairs_per_s": round(ng / tp, 1), "pair_forwards": 2 * ng,
            "matrix_cells_equal_pair_scores": same}


if __name__ == "__main__":
    sys.exit(main())
