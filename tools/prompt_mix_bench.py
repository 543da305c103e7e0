#!/usr/bin/env python3
"""Prompt-grouped triplet batches against mixed-prompt batches, in one process, every leg alternated; prints one JSON line and writes
it to profiles/prompt_mix_bench_sd15.json.
  grouped: one harness.score_latent_triplets call per prompt group -- what the path harness did before its engine batches carried
           several prompts (each group its own U-Net forwards);
  mixed:   one score_latent_triplets call carrying every triplet's prompt (a context table per engine batch).
SD1.5 at 512 px (64 x 64 latents), synthetic weights, latents in, T triplets (default 64) with k distinct synthetic contexts
(synth.make_context(cfg, seed=i)) assigned round-robin, k in {1, 8, 64}.  Whole-call wall medians (the calls synchronise at the
end), the two legs' scores compared with torch.equal, and mixed at k against mixed at k = 1 on the same images.
    python tools/prompt_mix_bench.py [--dtype bf16 --triplets 64 --k 1 8 64 --reps 7]"""
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
    return [sorted(a)[len(a) // 2] for a in acc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--triplets", type=int, default=64)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_mix_bench_sd15.json"))
    a = ap.parse_args()
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.harness import score_latent_triplets
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("conv_norm_out", "conv_out"))])
    ds = DiffSim(torch_dtype=dt, device="cuda", unet_config=cfg, state_dict=sd)
    n = a.triplets
    g = torch.Generator().manual_seed(5)
    ref, left, right = (torch.randn(n, 4, 64, 64, generator=g).cuda() for _ in range(3))
    na, nb = (torch.randn(1, 4, 64, 64, generator=g) for _ in range(2))
    ctxs = [S.make_context(cfg, seed=i).cuda() for i in range(max(a.k))]

    def grouped(prompts):
        s_l, s_r = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        groups = {}
        for i, p in enumerate(prompts):
            groups.setdefault(id(p), (p, []))[1].append(i)
        for p, rows in groups.values():
            sel = torch.tensor(rows, device="cuda")
            l_, r_ = score_latent_triplets(ds, ref[sel], left[sel], right[sel], na, nb, p)
            s_l[sel], s_r[sel] = l_, r_
        return s_l, s_r

    def mixed(prompts):
        return score_latent_triplets(ds, ref, left, right, na, nb, prompts)

    fns, names = [], []
    for k in a.k:
        prompts = [ctxs[i % k] for i in range(n)]
        fns += [lambda p=prompts: grouped(p), lambda p=prompts: mixed(p)]
        names += [(k, "grouped"), (k, "mixed")]
    ms = timed_alternating(fns, a.reps, a.warmup)
    res = {"model": "sd15", "px": 512, "dtype": a.dtype, "triplets": n, "reps": a.reps, "assignment": "round-robin", "k": {}}
    base = None
    for k in a.k:
        prompts = [ctxs[i % k] for i in range(n)]
        gl, gr = grouped(prompts)
        ml, mr = mixed(prompts)
        g_ms, m_ms = ms[names.index((k, "grouped"))], ms[names.index((k, "mixed"))]
        if k == 1:
            base = m_ms
        res["k"][str(k)] = {"grouped_ms": round(g_ms, 2), "mixed_ms": round(m_ms, 2),
                            "speedup_mixed_over_grouped": round(g_ms / m_ms, 3),
                            "scores_equal": bool(torch.equal(gl, ml) and torch.equal(gr, mr))}
    if base is not None:
        for k in a.k:
            res["k"][str(k)]["mixed_over_mixed_k1"] = round(res["k"][str(k)]["mixed_ms"] / base, 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(v["scores_equal"] for v in res["k"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
