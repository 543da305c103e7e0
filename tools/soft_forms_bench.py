#!/usr/bin/env python3
"""Each soft form against its region form on the same work, the two alternated; prints one JSON line and writes it to
profiles/soft_forms_bench.json.  Report only: there is no target.
  engine.score_matrix_weights (an 8 x 64 matrix), engine.pair_score_maps_weights and engine.pair_align_weights (64 pairs) with every
  byte 255 against engine.score_matrix_regions, pair_score_maps_regions and pair_align_regions with full masks -- the same rows,
  MFMAs, exponentials and products (the outputs agree bit for bit), the difference being the soft form's extra work: one f32 add per
  score element, the bias loads, the weights kernel -- on synthetic bf16 features at (N, H, D) = (256, 8, 160) and (1024, 8, 80),
  HIP-event medians of whole calls after warm-up.
Each form and shape runs in a child process of its own under its own time limit, and one that fails ends the run: nothing more is
started on the GPU after it.
    python tools/soft_forms_bench.py [--dtype bf16 --queries 8 --gallery 64 --reps 50 --warmup 5 --out profiles/soft_forms_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((256, 8, 160), (1024, 8, 80))
LEG_SECONDS = 120


FORMS = ("score_matrix", "maps", "align")


def leg(form, N, H, D, dtype, n_a, n_b, sim, reps, warmup):
    import torch
    from diffsim_amd import engine
    from tools.maps_bench import B
    from tools.soft_regions_bench import timed_alternating
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]
    g = torch.Generator().manual_seed(0)
    if form != "score_matrix":
        n = 2 * n_b                                                                  # n_b pairs
        q, k, v = (torch.randn(n, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
        mask = torch.ones(n, N, dtype=torch.bool, device="cuda")
        w = torch.full((n, N), 255, dtype=torch.uint8, device="cuda")
        ia = torch.arange(0, n, 2, dtype=torch.int32).cuda()
        ib = ia + 1
        if form == "maps":
            run_w = lambda: engine.pair_score_maps_weights(q, k, v, w, ia, ib, H, sim)       # noqa: E731
            run_r = lambda: engine.pair_score_maps_regions(q, k, v, mask, ia, ib, H, sim)    # noqa: E731
        else:
            gw = 16 if N == 256 else 32
            run_w = lambda: engine.pair_align_weights(q, k, w, ia, ib, H, gw)                # noqa: E731
            run_r = lambda: engine.pair_align_regions(q, k, mask, ia, ib, H, gw)             # noqa: E731
        (ms_w, w25, w75), (ms_r, r25, r75) = timed_alternating([run_w, run_r], reps, warmup)
        same = all(bool(torch.equal(a, b)) for a, b in zip(run_w(), run_r()))
        return {"form": form, "N": N, "H": H, "D": D, "pairs": n_b, "device": torch.cuda.get_device_name(0),
                "weights_ms": round(ms_w, 4), "weights_ms_quartiles": [round(w25, 4), round(w75, 4)],
                "regions_ms": round(ms_r, 4), "regions_ms_quartiles": [round(r25, 4), round(r75, 4)],
                "ratio_weights_over_regions": round(ms_w / ms_r, 4), "outputs_bit_equal": same}
    fa = tuple(torch.randn(n_a, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    fb = tuple(torch.randn(n_b, B, N, H * D, generator=g).to(dt).cuda() for _ in range(3))
    ma, mb = (torch.ones(n, N, dtype=torch.bool, device="cuda") for n in (n_a, n_b))
    wa, wb = (torch.full((n, N), 255, dtype=torch.uint8, device="cuda") for n in (n_a, n_b))
    run_w = lambda: engine.score_matrix_weights(fa, fb, wa, wb, H, sim)            # noqa: E731
    run_r = lambda: engine.score_matrix_regions(fa, fb, ma, mb, H, sim)            # noqa: E731
    (ms_w, w25, w75), (ms_r, r25, r75) = timed_alternating([run_w, run_r], reps, warmup)
    same = bool(torch.equal(run_w(), run_r()))
    return {"form": "score_matrix", "N": N, "H": H, "D": D, "queries": n_a, "gallery": n_b, "device": torch.cuda.get_device_name(0),
            "weights_ms": round(ms_w, 4), "weights_ms_quartiles": [round(w25, 4), round(w75, 4)],
            "regions_ms": round(ms_r, 4), "regions_ms_quartiles": [round(r25, 4), round(r75, 4)],
            "ratio_weights_over_regions": round(ms_w / ms_r, 4), "outputs_bit_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--gallery", type=int, default=64)
    ap.add_argument("--similarity", choices=["cosine", "mse"], default="cosine")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_forms_bench.json"))
    ap.add_argument("--leg", type=int, nargs=3, metavar=("N", "H", "D"), help="(internal) run one shape in this process")
    ap.add_argument("--form", choices=FORMS, default="score_matrix", help="(internal) the form of --leg")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.form, *a.leg, a.dtype, a.queries, a.gallery, a.similarity, a.reps, a.warmup)), flush=True)
        return 0
    legs = []
    for form, (N, H, D) in ((f, sh) for f in FORMS for sh in SHAPES):      # (this process never opens the GPU: every leg is a fresh child)
        cmd = [sys.executable, os.path.abspath(__file__), "--form", form, "--leg", str(N), str(H), str(D), "--dtype", a.dtype, "--queries", str(a.queries),
               "--gallery", str(a.gallery), "--similarity", a.similarity, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_SECONDS)
        except subprocess.TimeoutExpired:
            print(f"{form} {(N, H, D)} passed its {LEG_SECONDS} s limit: stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{form} {(N, H, D)} failed with status {r.returncode}: stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        legs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"tool": "tools/soft_forms_bench.py", "device": legs[0]["device"], "dtype": a.dtype, "similarity": a.similarity, "reps": a.reps,
           "warmup": a.warmup, "timing": "HIP events around whole calls, the two alternated, medians; one child process per form and shape",
           "legs": legs}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
