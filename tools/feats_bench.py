#!/usr/bin/env python3
"""diffeats and dinofeats beside diffsim and dino_cross at the same tap, and the Gram matrix at retrieval sizes.  Report only: nothing
about this path had been measured before, so there is no target.
  * tails: at SD1.5's default tap (256 tokens, 8 heads x 160, CFG batch 2, C = 1280) and DINOv2-S/14's (257 tokens, 6 x 64, batch 1),
    on synthetic q, k, v of P pairs: pairs/s of the attention score's tail (engine.pair_score) and of the feature metric's (features
    of the 2 P images, then feature_pair_score), alternated in one process, HIP events after warm-up; the feature call is also timed
    in its parts (engine.attn_features, engine.feature_pair_score).
  * matrix: engine.feature_matrix of n_a in {8, 512} queries against a gallery of 2048 at L = 2 x 256 x 1280 = 655 360 elements per
    image: the call's time (the Gram kernel and its f64 finish), and its achieved FLOP/s (2 n_a n_b L) and bytes/s ((n_a + n_b) L
    elements read once, the split-K partials written and read).  With few queries the call streams the gallery and is bound by HBM;
    with hundreds it is bound by the matrix cores.
  * e2e (--e2e P): pairs/s of whole scoring calls, forward included, through the scorers (synthetic weights): DiffSim at 512 px
    against its FeatureView, Dinov2Score at 224 px against its FeatureView.
Per-kernel times: run the same command under `rocprofv3 --kernel-trace` in a run of its own, as profiles/feats_bench_kernels.json was
taken (the kernels are
feat_attend_kernel, nt_gemm_kernel<T, false> the projection and <T, true> the Gram product, feat_stats_kernel, feat_normalise_kernel,
feat_fold_kernel, feat_pair_dot_kernel, feat_pair_finish_kernel, gram_finish_kernel).
    python tools/feats_bench.py [--dtype bf16 --pairs 128 --gallery 2048 --reps 10 --e2e 64 --out profiles/feats_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsim_amd import engine  # noqa: E402

TAPS = {"sd15 up_blocks:0": dict(B=2, H=8, N=256, D=160, proj=True), "dinov2-small layer": dict(B=1, H=6, N=257, D=64, proj=False)}


def event_ms(fns, reps, warmup):
    """median HIP-event time of each fn, the fns alternated inside every repetition"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, acc in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return [sorted(t)[len(t) // 2] for t in ts], ts


def tails(name, B, H, N, D, proj, P, dt, reps, warmup):
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2 * P, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    Cc = H * D
    kw = {"minmax": proj}
    if proj:
        kw.update(w_out=(torch.randn(Cc, Cc, generator=g) / math.sqrt(Cc)).to(dt).cuda(), bias=(0.1 * torch.randn(Cc, generator=g)).cuda())
    ia = torch.arange(0, 2 * P, 2, dtype=torch.int32, device="cuda")
    ib = ia + 1
    held = {}

    def feats():
        held["f"] = engine.attn_features(q, k, v, H, **kw)

    def pairs():
        return engine.feature_pair_score(*held["f"], ia, ib)

    def both():
        feats()
        return pairs()
    attn = lambda: engine.pair_score(q, k, v, ia, ib, H, "cosine")       # noqa: E731
    (t_attn, t_feat, t_f, t_p), _ = event_ms([attn, both, feats, pairs], reps, warmup)
    L = B * N * Cc
    # the feature call's algorithmic work: one SDPA per image and (b, h), the projection, the streamed passes
    sdpa = 4.0 * B * H * N * N * D * 2 * P
    gemm = 2.0 * 2 * P * B * N * Cc * Cc if proj else 0.0
    return {"tap": name, "B": B, "H": H, "N": N, "D": D, "L": L, "pairs": P, "projection": proj, "minmax": proj,
            "attention_score_tail_ms": round(t_attn, 4), "attention_score_pairs_per_s": round(P / t_attn * 1e3, 1),
            "feature_tail_ms": round(t_feat, 4), "feature_pairs_per_s": round(P / t_feat * 1e3, 1),
            "attn_features_ms": round(t_f, 4), "attn_features_tflops": round((sdpa + gemm) / t_f / 1e9, 2),
            "feature_pair_score_ms": round(t_p, 4), "feature_pair_score_gbytes_per_s": round(2.0 * P * L * q.element_size() / t_p / 1e6, 1)}


def matrix(n_a, n_b, L, dt, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(1)

    def make(n):
        x = torch.rand(n, L, generator=g, device="cuda", dtype=torch.float32).to(dt)
        st = torch.zeros(n, 4, device="cuda")
        for i0 in range(0, n, 64):
            st[i0:i0 + 64, 0] = (x[i0:i0 + 64].double() ** 2).sum(1).float()
        return x, st
    fa, fb = make(n_a), make(n_b)
    run = lambda: engine.feature_matrix(fa, fb)         # noqa: E731
    (ms,), (all_ms,) = event_ms([run], reps, warmup)
    es, splits = fa[0].element_size(), -(-L // 16384)
    flop = 2.0 * n_a * n_b * L
    byts = (n_a + n_b) * L * es + 2.0 * splits * n_a * n_b * 4
    # the least time the hardware could take: the larger of FLOPs over the peak rate and bytes over the peak bandwidth
    peak_flops = 2.5e15 if es == 2 else 157.3e12
    floor_ms = 1e3 * max(flop / peak_flops, byts / 8.0e12)
    return {"n_a": n_a, "n_b": n_b, "L": L, "call_ms": round(ms, 4), "call_ms_all": [round(t, 4) for t in all_ms],
            "tflops": round(flop / ms / 1e9, 2), "gbytes_per_s": round(byts / ms / 1e6, 1), "split_k": splits,
            "bound_by": "HBM" if byts / 8.0e12 > flop / peak_flops else "matrix cores", "floor_ms_at_spec_peak": round(floor_ms, 4),
            "share_of_floor": round(floor_ms / ms, 4), "us_per_cell": round(1e3 * ms / (n_a * n_b), 4)}


def e2e(P, dt):
    """pairs/s of whole scoring calls (forward and tail) through the scorers, the attention score beside the feature metric"""
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.feats import FeatureView
    from diffsim_amd.vit import Dinov2Score
    g = torch.Generator().manual_seed(5)

    def timed(fn):
        fn()                                # warm-up: code objects, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    out = []
    cfg = C.SD15
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))]
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=S.make_state_dict(cfg, seed=0, keys=keys))
    ctx = S.make_context(cfg)
    la, lb = (torch.randn(P, 4, 64, 64, generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    view, tap = FeatureView(ds), ("up_blocks", 0)

    def run(tail):
        return [s for _, _, s in ds.pair_chunks(la, lb, na, nb, ctx, tap, 600, "cosine", min(P, 64), tail)]
    t_attn, t_feat = timed(lambda: run(engine.pair_score)), timed(lambda: run(view.pair_tail(tap)))
    out.append({"model": "sd15 512 px, up_blocks:0", "pairs": P, "diffsim_pairs_per_s": round(P / t_attn, 1),
                "diffeats_pairs_per_s": round(P / t_feat, 1)})
    dino = Dinov2Score(C.DINOV2_S14, S.make_state_dict(C.DINOV2_S14, 3), "cuda", dt)
    dview, layer = FeatureView(dino), C.DINOV2_S14.depth - 1
    pa, pb = (torch.randn(P, 3, 224, 224, generator=g) for _ in range(2))
    t_attn = timed(lambda: dino.score_pixel_pairs(pa, pb, layer))
    t_feat = timed(lambda: dino.score_pixel_pairs(pa, pb, layer, tail=dview.pair_tail(layer)))
    out.append({"model": f"dinov2-small 224 px, layer {layer}", "pairs": P, "dino_cross_pairs_per_s": round(P / t_attn, 1),
                "dinofeats_pairs_per_s": round(P / t_feat, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--gallery", type=int, default=2048)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 512])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", type=int, default=0, metavar="P", help="also whole scoring calls over P pairs (builds both models)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON here")
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    res = {"bench": "feats_bench", "dtype": a.dtype, "device": torch.cuda.get_device_name(0), "timing": "median of HIP events, alternated",
           "tails": [tails(name, P=a.pairs, dt=dt, reps=a.reps, warmup=a.warmup, **shape) for name, shape in TAPS.items()],
           "matrix": [matrix(n_a, a.gallery, 2 * 256 * 1280, dt, a.reps, a.warmup) for n_a in a.queries]}
    if a.e2e:
        res["e2e"] = e2e(a.e2e, dt)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
