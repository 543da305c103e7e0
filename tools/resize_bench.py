#!/usr/bin/env python3
"""Measurement of the device resize (report only; nothing gates on it) -> profiles/gpu_resize_bench.json.

  (a) kernels    HIP-event medians of one dsim_resize_u8 call (both passes and the call's descriptor copy) per image, batches of 64
                 equal sources of 768^2, 2048x1536 and 4032x3024, to 512^2 Lanczos and to the 224 crop of a shortest-edge-256 bicubic
                 resize; beside them the bytes a call moves (source rows read, temp written and read, output written) and that
                 figure over the HBM peak.
  (b) files in   images/s from generated JPEG sets (768^2, 2048x1536) through DecodePool(procs=16): SD1.5 ``path_latents`` and
                 ``Dinov2Score.dino_cross_score`` pairs with ``gpu_resize`` off and on, alternated, and the engines' from-tensors
                 rates beside both.

Usage: python tools/resize_bench.py [--out profiles/gpu_resize_bench.json] [--images 96] [--procs 16]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsim_amd import _lib, config as C, resize as rz, synth as S         # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, the MI355X's specified peak


def photo(w, h, seed):
    """A photo-like image: a smooth random field plus mild noise (so that a JPEG of it decodes at a realistic cost)."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (max(2, h // 64), max(2, w // 64), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.Resampling.BICUBIC), dtype=np.int16)
    return np.clip(a + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def kernel_case(w, h, out_w, out_h, filt, crop, n=64, reps=7):
    """One batch of n equal (w, h) sources, built on the device; the median time of dsim_resize_u8 and the bytes it moves."""
    L = _lib.lib()
    ox, oy, cw, ch = crop or (0, 0, out_w, out_h)
    tabs_np, descr, ints = [], [], 0
    for n_in, n_out in ((w, out_w), (h, out_h)):
        b, k = rz.coeff_table(n_in, n_out, filt)
        descr.append((ints, n_in, n_out, k.shape[1], b))
        tabs_np += [b.reshape(-1), k.reshape(-1)]
        ints += b.size + k.size
    tables = torch.from_numpy(np.concatenate(tabs_np)).cuda()
    per = (3 * w * h + 15) // 16 * 16
    one = torch.from_numpy(np.pad(photo(w, h, 1).reshape(-1), (0, per - 3 * w * h))).cuda()
    src = one.repeat(n)
    vb = descr[1][4]
    y0 = int(vb[oy, 0])
    rows = int(vb[oy + ch - 1, 0] + vb[oy + ch - 1, 1]) - y0
    tstride = (cw * 3 + 15) // 16 * 16
    imgs = (_lib.ResizeImageC * n)()
    for i, d in enumerate(imgs):
        d.src_offset, d.w, d.h, d.h_table, d.v_table, d.y_first, d.rows, d.temp_offset = i * per, w, h, 0, 1, y0, rows, i * rows * tstride
    tab = (_lib.ResizeTableC * 2)()
    for t, (o, n_in, n_out, ksize, _) in zip(tab, descr):
        t.offset, t.in_size, t.out_size, t.ksize = o, n_in, n_out, ksize
    geo = (out_w, out_h, ox, oy, cw, ch)
    need = L.dsim_resize_u8_workspace_bytes(imgs, n, tab, 2, ints, *geo, src.numel())
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, ch, cw, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.dsim_resize_u8(src.data_ptr(), src.numel(), imgs, n, tables.data_ptr(), ints, tab, 2, *geo, out.data_ptr(),
                                    ws.data_ptr(), need, stream), "dsim_resize_u8")
    call()
    torch.cuda.synchronize()
    want = Image.fromarray(one[:3 * w * h].cpu().numpy().reshape(h, w, 3)).resize(
        (out_w, out_h), Image.Resampling.LANCZOS if filt == "lanczos" else Image.Resampling.BICUBIC).crop((ox, oy, ox + cw, oy + ch))
    assert np.array_equal(out[n - 1].cpu().numpy(), np.asarray(want))          # the thing timed is PIL's bytes
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    t = statistics.median(times)
    moved = n * (3 * w * rows + 2 * rows * tstride + 3 * cw * ch)
    return {"source": f"{w}x{h}", "output": f"{out_w}x{out_h} {filt}" + (f", window {cw}x{ch}" if crop else ""), "batch": n,
            "us_per_image": round(t / n * 1e6, 2), "call_ms_median": round(t * 1e3, 3), "call_ms_min_max": [round(min(times) * 1e3, 3),
                                                                                                         round(max(times) * 1e3, 3)],
            "MB_moved_per_image": round(moved / n / 1e6, 2), "GB_per_s": round(moved / t / 1e9, 1),
            "share_of_hbm_peak": round(moved / t / HBM_PEAK, 4)}


def files_in(args):
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder, image_preprocess
    from diffsim_amd.image import DecodePool
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.vit import DINOV2_PREPROCESS, Dinov2Score
    os.environ["DSIM_DECODE_PROCS"] = str(args.procs)                       # the ViT scorers' shared pool
    vae = VAEEncoder(C.VAE_SD15, S.make_state_dict(C.VAE_SD15, seed=1), torch.bfloat16, "cuda")
    ds = DiffSim(torch.bfloat16, "cuda", state_dict=S.make_state_dict(C.SD15, seed=0), vae=vae, encode_prompt=lambda p: None,
                 decode_procs=args.procs)
    dino = Dinov2Score(C.DINOV2_S14, S.make_state_dict(C.DINOV2_S14, 3), "cuda", torch.bfloat16, DINOV2_PREPROCESS)
    # from tensors: what the engines take when the host is out of the way
    px = torch.randint(0, 256, (32, 512, 512, 3), dtype=torch.uint8, device="cuda")
    vae.moments(image_preprocess(px, True))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(3):
        vae.moments(image_preprocess(px, True))
    torch.cuda.synchronize(); vae_rate = 96 / (time.perf_counter() - t0)
    pa, pb = torch.randn(256, 3, 224, 224), torch.randn(256, 3, 224, 224)
    dino.score_pixel_pairs(pa, pb, 6)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    dino.score_pixel_pairs(pa, pb, 6)
    torch.cuda.synchronize(); dino_rate = 512 / (time.perf_counter() - t0)
    out = {"decode_procs": args.procs, "host_cpus_usable": len(os.sched_getaffinity(0)), "images_per_set": args.images,
           "from_tensors_images_per_s": {"sd15_vae_encode_512": round(vae_rate, 1), "dinov2_s14_pairs_whole_call": round(dino_rate, 1)},
           "sets": []}
    with tempfile.TemporaryDirectory() as d:
        for w, h in ((768, 768), (2048, 1536)):
            paths = []
            for i in range(args.images):
                p = os.path.join(d, f"{w}x{h}_{i}.jpg")
                Image.fromarray(photo(w, h, 100 + i)).save(p, quality=92)
                paths.append(p)
            half = len(paths) // 2
            rows = list(zip(paths[:half], paths[half:]))
            res = {"source": f"{w}x{h} JPEG q92", "sd15_path_latents_images_per_s": {"off": [], "on": []},
                   "dinov2_dino_cross_images_per_s": {"off": [], "on": []}}
            for sc in (ds, dino):                                             # warm-up: workers started, tables built, engines sized
                for on in (False, True):
                    sc.gpu_resize = on
                    (path_latents(ds, rows[:4], (0, 1), 512, 2333, 16) if sc is ds else dino.dino_cross_score(paths[:4], paths[4:8], [6]))
            for _ in range(args.rounds):
                for on in (False, True):                                      # alternated: drift hits both alike
                    ds.gpu_resize = dino.gpu_resize = on
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    path_latents(ds, rows, (0, 1), 512, 2333, 16)
                    torch.cuda.synchronize()
                    res["sd15_path_latents_images_per_s"]["on" if on else "off"].append(round(len(paths) / (time.perf_counter() - t0), 1))
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    dino.dino_cross_score(paths[:half], paths[half:], [6])
                    torch.cuda.synchronize()
                    res["dinov2_dino_cross_images_per_s"]["on" if on else "off"].append(round(len(paths) / (time.perf_counter() - t0), 1))
            out["sets"].append(res)
    ds._decode.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_resize_bench.json"))
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_files", action="store_true")
    args = ap.parse_args()
    kernels = []
    for w, h in ((768, 768), (2048, 1536), (4032, 3024)):
        kernels.append(kernel_case(w, h, 512, 512, "lanczos", None))
        ow, oh = rz.shortest_edge(w, h, 256)
        kernels.append(kernel_case(w, h, ow, oh, "bicubic", ((ow - 224) // 2, (oh - 224) // 2, 224, 224)))
    result = {"probe": "device resize (dsim_resize_u8), MI355X", "hbm_peak_bytes_per_s": HBM_PEAK, "kernels": kernels}
    if not args.skip_files:
        result["files_in"] = files_in(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
