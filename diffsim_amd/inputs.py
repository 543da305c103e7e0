"""Image files -> latents and draws, and latent rows -> engine batches, for every batched path (pairs, triplets, score
matrices, similarity maps) and all three scorer kinds.

The draw order is the one rule here that changes scores.  Every reference call (DiffSim.diffsim, diffsim/diffsim.py:98-197;
diffsim_xl.diffsim_score, diffsim_xl.py:65-155; diffsim_DiT.diffsim_score, diffsim_dit.py:74-142) reseeds one CPU generator
and draws, in this order, the VAE sample of image A, the VAE sample of image B, the noise of A, the noise of B.  A draw's
size depends only on the latent shape, so the four draws are the same tensors for every call of one image size: an image in
slot A always gets draw A, one in slot B draw B, whatever its partner.  ``path_latents`` states this once.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .diffsim import DiffSim, _norm_layer, check_row_prompts, distinct_prompts, get_generator, row_prompts, single_prompt
from .image import DecodePool, load_image, process_image


class _Adapter:
    """What the batched paths need to know about a scorer kind -- the per-call arithmetic of its reference entry point,
    stated once: DiffSim.diffsim, diffsim_xl.diffsim_score, diffsim_DiT.diffsim_score."""

    def __init__(self, scorer):
        from .diffsim_dit import diffsim_DiT
        from .diffsim_xl import diffsim_xl
        self.s = scorer
        self.kind = "sd15" if isinstance(scorer, DiffSim) else ("xl" if isinstance(scorer, diffsim_xl) else
                                                                ("dit" if isinstance(scorer, diffsim_DiT) else None))
        if self.kind is None:
            raise TypeError(f"no triplet adapter for {type(scorer).__name__}")
        nd = getattr(scorer, "noise_dtype", torch.float32)
        vae = getattr(scorer, "vae", None)
        self.vae = vae
        self.fast = vae is not None and hasattr(vae, "moments")      # the HIP VAE encoder: chunked, look-ahead decode
        if self.kind == "sd15":
            self.image_half = scorer.vae_dtype == torch.float16      # image.to(dtype=float16), diffsim.py:93
            self.eps_dtype = nd                                      # latent_dist.sample draws in the pipeline dtype
            self.noise_draw = nd
            self.round16 = nd == torch.float16
        else:
            self.image_half = False                                  # the SDXL / DiT VAE runs in fp32 (diffsim_xl.py:61)
            self.eps_dtype = getattr(vae, "sample_dtype", torch.float32)
            self.noise_draw = nd if self.kind == "xl" else torch.float16      # DiT: randn_tensor(dtype=latents.dtype) = fp16
            self.round16 = True                                      # latents.to(dtype=float16), diffsim_xl.py:63 / diffsim_dit.py:59
        self._ctx = {}

    @property
    def mixes_prompts(self) -> bool:
        """Whether one engine batch may carry several prompts.  SD1.5-family: yes, a context table (nothing before the first
        cross-attention depends on the prompt).  DiT ignores the prompt (labels [1, 1000]).  SDXL: no -- its pooled prompt
        embedding enters the time embedding of every resnet, one per CFG half."""
        return self.kind != "xl"

    def group_key(self, prompt):
        """Rows of a path run with equal keys share engine batches: one group for the kinds that mix prompts, one per prompt
        for SDXL."""
        return prompt if not self.mixes_prompts else None

    def group_prompt(self, prompts: Sequence):
        """The prompt argument of one group's rows (group_key): SD1.5 the per-row list, or its one prompt when all rows share it;
        the others the group's one prompt."""
        if self.kind == "sd15" and len(distinct_prompts(prompts)[0]) > 1:
            return list(prompts)
        return prompts[0]

    def rows(self, prompt, n_rows: int, what: str = "triplets"):
        """A call's prompt argument checked against its rows: SD1.5 takes one prompt or one per row; SDXL one prompt per call (a
        string or its (context, pooled) tuple, or a list that repeats one); DiT ignores it."""
        if self.kind == "dit":
            return prompt
        if self.kind == "xl":
            if isinstance(prompt, list):
                prompt = check_row_prompts(prompt, n_rows, what)
                if len(distinct_prompts(prompt)[0]) > 1:
                    raise ValueError("SDXL takes one prompt per call: its pooled prompt embedding enters every resnet")
                return prompt[0]
            return prompt
        return check_row_prompts(prompt, n_rows, what)

    def chunk_prompt(self, prompt, i0: int, i1: int, per_row: int):
        """The prompt argument of the engine batch of rows [i0, i1) (each row's per_row images consecutive)."""
        return row_prompts(prompt, i0, i1, per_row) if self.kind == "sd15" else prompt

    def heads(self, block, layer):
        if self.kind == "dit":
            return self.s.engine(int(layer[0])).heads
        return self.s.engine(block, layer if self.kind == "xl" else _norm_layer(layer)).heads

    def engine(self, block, layer):
        if self.kind == "dit":
            return self.s.engine(int(layer[0]))
        return self.s.engine(block, layer if self.kind == "xl" else _norm_layer(layer))

    def auto_triplets(self, block, layer, n: int, n_ctx: int = 1) -> int:
        """Triplets per engine batch when the caller names none: the image count of the batch sweeps' optimum (SD1.5 and
        DiT: 128 images = 64 pairs, profiles/r04h_batch_sweep.txt; SDXL at 1024 px: 16), inside the 2 GiB activation bound
        and half of the free HBM."""
        eng = self.engine(block, layer)
        t = max(1, min((16 if self.kind == "xl" else 128) // 3, max(1, int(n))))
        mixed = {"n_ctx": 2} if n_ctx > 1 else {}                   # (a context table: its per-image buffers count too)
        if hasattr(eng, "max_images"):
            t = max(1, min(t, eng.max_images(**mixed) // 3))
        try:
            free, _total = torch.cuda.mem_get_info(self.s.device)
            while t > 1 and hasattr(eng, "workspace_bytes") and eng.workspace_bytes(3 * t, **mixed) > 0.5 * free:
                t = (t + 1) // 2
        except Exception:
            pass
        return t

    def features(self, lat, nz, prompt, block, layer, step):
        if self.kind == "sd15":
            return self.s.features(lat, nz, prompt, block, _norm_layer(layer), step)
        if self.kind == "xl":
            if prompt not in self._ctx:
                if self.s._encode_prompt is None:
                    raise RuntimeError("no text encoder plugged in: pass encode_prompt=...")
                self._ctx[prompt] = self.s._encode_prompt(prompt)    # (context, pooled): once per prompt, not once per pair
            ctx, pooled = self._ctx[prompt]
            return self.s.features(lat, nz, ctx, pooled, block, layer, step)
        return self.s.features(lat, nz, int(layer[0]), step)


def _prepare(scorer, ad: _Adapter, tensor, generator):
    """prepare_image_latents of the scorer kind, returned as the f32 values its pipeline carries on."""
    if ad.kind == "sd15":
        return scorer.prepare_image_latents(tensor, None, None, generator).to(ad.noise_draw).float()
    return scorer.prepare_image_latents(tensor, generator).float()


_POOL = None


def _shared_pool():
    """Decode pool for scorers that own none (diffsim_xl, diffsim_DiT): the host's cores divided among the node's ranks."""
    global _POOL
    if _POOL is None:
        _POOL = DecodePool()
    return _POOL


def path_latents(scorer, rows: Sequence[Tuple[str, ...]], slots: Sequence[int], img_size, seed, chunk: int,
                 hip_vae: bool = True) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Latents of equal-length rows of image paths as one reference call per (slot-A image, slot-B image) would make them.
    slots[c] (0 = A, 1 = B) is the draw column c takes: pairs (0, 1), triplets (0, 1, 1) (the (A, C) call's C takes B's
    draw), a score matrix's sides (0,) and (1,).  Returns ([one (n, C, s, s) f32 tensor per column], noiseA, noiseB), the
    noises (1, C, s, s) f32 on the host.

    With the scorer's HIP VAE encoder (unless hip_vae=False): decode + resize run two chunks ahead on the host, and each
    chunk of `chunk` rows is one ``vae.moments`` with the columns interleaved; the four draws come from one reseeded
    generator and ``latent_sample`` applies them on the device.  Otherwise the scorer's prepare_image_latents per image: slot
    A from a freshly reseeded generator, slot B from its state after slot A's draw, the noises after slot B's draw.  A call
    whose columns all sit in one slot spends one extra prepare on its first image to reach the other slot's state."""
    from .engine import image_preprocess, latent_sample
    ad = _Adapter(scorer)
    k = len(slots)
    cols = [[] for _ in slots]
    if ad.fast and hip_vae:
        vae = ad.vae
        sf = vae.config.scaling_factor
        pool = getattr(scorer, "_decode", None) or _shared_pool()
        starts = list(range(0, len(rows), chunk))

        def submit(i0):
            return pool.submit([p for row in rows[i0:i0 + chunk] for p in row], img_size)
        pending = [submit(i0) for i0 in starts[:2]]              # decode + resize run two chunks ahead of the GPU
        draws = None
        for ci, i0 in enumerate(starts):
            px = DecodePool.gather(pending.pop(0))
            if ci + 2 < len(starts):
                pending.append(submit(starts[ci + 2]))
            # process_image's arithmetic and the fp16 image cast on the device (bit-identical, dsim_image_preprocess)
            x = image_preprocess(px.to(vae.device, non_blocking=True), ad.image_half)
            mom = vae.moments(x)
            if draws is None:
                g = get_generator(seed, "cpu")
                shp = (1, mom.shape[1] // 2) + tuple(mom.shape[2:])
                eA = torch.randn(shp, generator=g, dtype=ad.eps_dtype).float().to(vae.device)
                eB = torch.randn(shp, generator=g, dtype=ad.eps_dtype).float().to(vae.device)
                nA = torch.randn(shp, generator=g, dtype=ad.noise_draw).float()
                nB = torch.randn(shp, generator=g, dtype=ad.noise_draw).float()
                draws = (eA, eB, nA, nB)
            for c, slot in enumerate(slots):
                cols[c].append(latent_sample(mom, draws[slot], sf, c, k, ad.round16))
        return [torch.cat(col) for col in cols], draws[2], draws[3]
    state = {}              # generator state in front of slot B's draw (1) and of the noises (2)

    def prep(path, slot):
        if slot == 0:
            g = get_generator(seed, "cpu")
        else:
            g = torch.Generator("cpu")
            g.set_state(state[1])
        lat = _prepare(scorer, ad, process_image(load_image(path), img_size), g)
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
    nA = torch.randn(shp, generator=g, dtype=ad.noise_draw).float()
    nB = torch.randn(shp, generator=g, dtype=ad.noise_draw).float()
    return [torch.cat(col) for col in cols], nA, nB


def stack_rows(cols: Sequence[torch.Tensor], noises: Sequence[torch.Tensor], i0: int, i1: int):
    """Engine batch of rows [i0, i1) of k latent columns (n, C, s, s): lat (k m, C, s, s) f32, each row's k images
    consecutive, and nz in the same layout from the columns' noises, each (1, C, s, s) shared by every row or (n, C, s, s)
    one per row."""
    n, shp, m = cols[0].shape[0], cols[0].shape[1:], i1 - i0
    lat = torch.stack([c[i0:i1] for c in cols], dim=1).reshape(len(cols) * m, *shp).float()
    nz = torch.stack([z[i0:i1] if z.shape[0] == n else z.expand(m, *shp) for z in noises], dim=1).reshape(len(cols) * m, *shp)
    return lat, nz
