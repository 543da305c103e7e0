"""Image files -> latents and draws for every batched path (pairs, triplets, score matrices, similarity maps) and all three
scorer kinds.

The draw order is the one rule here that changes scores.  Every reference call (DiffSim.diffsim, diffsim/diffsim.py:98-197;
diffsim_xl.diffsim_score, diffsim_xl.py:65-155; diffsim_DiT.diffsim_score, diffsim_dit.py:74-142) reseeds one CPU generator
and draws, in this order, the VAE sample of image A, the VAE sample of image B, the noise of A, the noise of B.  A draw's
size depends only on the latent shape, so the four draws are the same tensors for every call of one image size: an image in
slot A always gets draw A, one in slot B draw B, whatever its partner.  ``path_latents`` states this once.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .engine import image_preprocess, latent_sample, resize_u8
from .image import DecodePool, load_image, process_image
from .scorer import get_generator, stack_rows       # noqa: F401  (stack_rows: latent rows -> engine batches, the other half)


_POOL = None
INPUT_CHUNK = 64                # images per decode request and device resize of a kind without draws (the ViT metrics)


def _shared_pool():
    """Decode pool for scorers that own none (diffsim_xl, diffsim_DiT): the host's cores divided among the node's ranks."""
    global _POOL
    if _POOL is None:
        _POOL = DecodePool()
    return _POOL


def raw_chunks(pool, rows, chunk: int):
    """The decoded images of `rows` (tuples of paths or PIL images), `chunk` rows at a time in row-major order, as lists of uint8
    (h, w, 3) arrays at the files' own sizes: decode-only requests to `pool`, two chunks ahead of the consumer."""
    starts = list(range(0, len(rows), chunk))

    def submit(i0):
        return pool.submit_raw([p for row in rows[i0:i0 + chunk] for p in row])
    pending = [submit(i0) for i0 in starts[:2]]
    for ci in range(len(starts)):
        arrays = [f.result() for f in pending.pop(0)]
        if ci + 2 < len(starts):
            pending.append(submit(starts[ci + 2]))
        yield arrays


def path_latents(scorer, rows: Sequence[Tuple[str, ...]], slots: Sequence[int], img_size, seed, chunk: int,
                 hip_vae: bool = True) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Latents of equal-length rows of image paths as one reference call per (slot-A image, slot-B image) would make them.
    slots[c] (0 = A, 1 = B) is the draw column c takes: pairs (0, 1), triplets (0, 1, 1) (the (A, C) call's C takes B's
    draw), a score matrix's sides (0,) and (1,).  Returns ([one (n, C, s, s) f32 tensor per column], noiseA, noiseB), the
    noises (1, C, s, s) f32 on the host.

    With the scorer's HIP VAE encoder (unless hip_vae=False): decode + resize run two chunks ahead on the host, and each
    chunk of `chunk` rows is one ``vae.moments`` with the columns interleaved; the four draws come from one reseeded
    generator and ``latent_sample`` applies them on the device.  With ``scorer.gpu_resize`` the host only decodes: the Lanczos
    resize is engine.resize_u8's, PIL's bytes, so the latents are the same bits (a kind without draws: its ``load_inputs``, whose f32 inputs are then returned
    on the device -- n x 3 x S x S x 4 bytes of device memory per column set, where the host path returns host tensors).  Otherwise the scorer's prepare_image_latents per image: slot
    A from a freshly reseeded generator, slot B from its state after slot A's draw, the noises after slot B's draw.  A call
    whose columns all sit in one slot spends one extra prepare on its first image to reach the other slot's state."""
    vae = getattr(scorer, "vae", None)
    k = len(slots)
    cols = [[] for _ in slots]
    gpu_resize = bool(getattr(scorer, "gpu_resize", False))
    if not scorer.draws:            # a kind without VAE and noise: its own input tensors, and placeholders where the noises go
        if gpu_resize and hasattr(scorer, "load_inputs"):
            pool = getattr(scorer, "_decode", None) or _shared_pool()
            x = torch.cat([scorer.load_inputs(arrays) for arrays in raw_chunks(pool, rows, max(1, INPUT_CHUNK // k))])
            cols = [x[c::k] for c in range(k)]
            none = torch.zeros((1,) + tuple(cols[0].shape[1:]))
            return cols, none, none
        cols = [torch.cat([scorer.load_input(row[c], img_size) for row in rows]) for c in range(k)]
        none = torch.zeros((1,) + tuple(cols[0].shape[1:]))
        return cols, none, none
    if vae is not None and hasattr(vae, "moments") and hip_vae:    # the HIP VAE encoder: chunked, look-ahead decode
        sf = vae.config.scaling_factor
        pool = getattr(scorer, "_decode", None) or _shared_pool()
        starts = list(range(0, len(rows), chunk))

        def submit(i0):
            return pool.submit([p for row in rows[i0:i0 + chunk] for p in row], img_size)
        raw = raw_chunks(pool, rows, chunk) if gpu_resize else None
        pending = [] if gpu_resize else [submit(i0) for i0 in starts[:2]]      # decode + resize run two chunks ahead of the GPU
        draws = None
        for ci, i0 in enumerate(starts):
            if gpu_resize:          # the host decoded only: process_image's Lanczos resize on the device too (dsim_resize_u8)
                px = resize_u8(next(raw), img_size, img_size, "lanczos", device=vae.device)
            else:
                px = DecodePool.gather(pending.pop(0)).to(vae.device, non_blocking=True)
                if ci + 2 < len(starts):
                    pending.append(submit(starts[ci + 2]))
            # process_image's arithmetic and the fp16 image cast on the device (bit-identical, dsim_image_preprocess)
            x = image_preprocess(px, scorer.image_half)
            mom = vae.moments(x)
            if draws is None:
                g = get_generator(seed, "cpu")
                shp = (1, mom.shape[1] // 2) + tuple(mom.shape[2:])
                eA = torch.randn(shp, generator=g, dtype=scorer.eps_dtype).float().to(vae.device)
                eB = torch.randn(shp, generator=g, dtype=scorer.eps_dtype).float().to(vae.device)
                nA = torch.randn(shp, generator=g, dtype=scorer.noise_draw).float()
                nB = torch.randn(shp, generator=g, dtype=scorer.noise_draw).float()
                draws = (eA, eB, nA, nB)
            for c, slot in enumerate(slots):
                cols[c].append(latent_sample(mom, draws[slot], sf, c, k, scorer.round16))
        return [torch.cat(col) for col in cols], draws[2], draws[3]
    state = {}              # generator state in front of slot B's draw (1) and of the noises (2)

    def prep(path, slot):
        if slot == 0:
            g = get_generator(seed, "cpu")
        else:
            g = torch.Generator("cpu")
            g.set_state(state[1])
        lat = scorer.prepare(scorer.load_input(path, img_size), g)
        state.setdefault(slot + 1, g.get_state())
        return lat
    for row in rows:
        for c, slot in enumerate(slots):
            if slot == 1 and 1 not in state:
                prep(row[c], 0)             # no slot-A column: slot A's draw, spent on this image
            cols[c].append(prep(row[c], slot))
    if 2 not in state:
        prep(rows[0][0], 1)                 # no slot-B column: slot B's draw, spent on the first image
    g = torch.Generator("cpu")
    g.set_state(state[2])
    shp = cols[0][0].shape
    nA = torch.randn(shp, generator=g, dtype=scorer.noise_draw).float()
    nB = torch.randn(shp, generator=g, dtype=scorer.noise_draw).float()
    return [torch.cat(col) for col in cols], nA, nB
