"""Similarity maps: where on each image's grid two images match.

The DiffSim score breaks down exactly into per-token terms.  For direction a->b, cos(O_ab, O_aa) over the flattened
(B, H, N, D) tensors (diffsim.py:177-190) is sum_i dot_i / (|O_ab| |O_aa|), where dot_i sums over the CFG halves, the heads
and d at query token i; mse splits the same way, sum_i sqd_i / (B H N D).  Token i of direction a->b sits on image a's grid at
row i // w, column i % w (the U-Net's NCHW -> tokens flatten and DiT's patchify order).  So a pair has two maps, one on each
image, and their terms sum to the score.  ``engine.pair_score_maps`` computes them in the fused tail.

``local``: the token's own cosine of its O_ab and O_aa vectors (or their mean squared difference) -- how well that region matches.
``contrib``: the token's term of the score -- 0.5 * (contrib[:, 0].sum() + contrib[:, 1].sum()) is the pair's score.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .diffsim import get_generator
from .engine import image_preprocess, latent_sample, pair_score_maps
from .harness import _Adapter, _prepare, _shared_pool
from .image import DecodePool, load_image, process_image


def grid_shape(n_tokens: int) -> Tuple[int, int]:
    """(h, w) of a square token grid; a non-square token count is refused."""
    s = math.isqrt(int(n_tokens))
    if n_tokens < 1 or s * s != n_tokens:
        raise ValueError(f"{n_tokens} tokens do not form a square grid: maps need an h x w = s x s token grid")
    return s, s


class SimilarityMaps:
    """score (n,), local and contrib (n, 2, h, w) f32 tensors: pair p's direction 0 lies on image A's token grid, direction 1 on
    image B's; grid = (h, w), token i at (i // w, i % w).  Built from the flat (n, 2, N) maps of ``engine.pair_score_maps``."""

    def __init__(self, score: torch.Tensor, local: torch.Tensor, contrib: torch.Tensor):
        if local.shape != contrib.shape or local.ndim != 3 or local.shape[1] != 2 or local.shape[0] != score.shape[0]:
            raise ValueError(f"maps must be (n, 2, N) with n = len(score): {tuple(local.shape)}, {tuple(contrib.shape)}, "
                             f"{tuple(score.shape)}")
        n, _, N = local.shape
        self.grid = grid_shape(N)
        self.score = score
        self.local = local.reshape(n, 2, *self.grid)
        self.contrib = contrib.reshape(n, 2, *self.grid)

    def __len__(self) -> int:
        return self.score.shape[0]

    def __getitem__(self, i) -> "SimilarityMaps":
        """The pairs i (an index or a slice) as maps of their own."""
        sl = slice(i, i + 1) if isinstance(i, int) else i
        return SimilarityMaps(self.score[sl], self.local[sl].flatten(2), self.contrib[sl].flatten(2))

    def upsample(self, size: int, which: str = "local") -> torch.Tensor:
        """Bilinear (n, 2, size, size) maps for overlay on the size x size image (``img_size``); which: local or contrib."""
        m = {"local": self.local, "contrib": self.contrib}[which]
        return F.interpolate(m.float(), size=(int(size), int(size)), mode="bilinear", align_corners=False)


def _features_fn(ad: _Adapter, prompt, block, layer, step):
    """lat, nz -> (q, k, v) at the tap.  diffsim_xl also takes a (context, pooled) tuple as prompt (its score_latent_pairs
    signature); the other kinds go through the adapter."""
    if ad.kind == "xl" and isinstance(prompt, tuple):
        ctx, pooled = prompt
        return lambda lat, nz: ad.s.features(lat, nz, ctx, pooled, block, layer, step)
    return lambda lat, nz: ad.features(lat, nz, prompt, block, layer, step)


@torch.no_grad()
def score_latent_pair_maps(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                           similarity="cosine", batch_pairs: Optional[int] = None) -> SimilarityMaps:
    """Maps of pair i = (latA[i] in slot A, latB[i] in slot B), any scorer kind (DiffSim, diffsim_xl, diffsim_DiT): the pairs of
    ``score_latent_pairs``, in chunks of batch_pairs (None: 64 where it fits for DiffSim, the engine batch of
    ``auto_triplets`` otherwise) -- one feature batch and one maps launch per chunk.  noiseA / noiseB: (1, C, s, s) or (n, C, s, s).
    DiT takes target_layer as a list ([layer]), as the adapter does."""
    ad = _Adapter(scorer)
    dev = scorer.device
    n = latA.shape[0]
    shp = latA.shape[1:]
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    eng = ad.engine(target_block, target_layer)
    heads = eng.heads
    if batch_pairs is None:
        batch_pairs = scorer.auto_batch_pairs(eng, n, 1) if ad.kind == "sd15" else max(1, 3 * ad.auto_triplets(target_block, target_layer, n) // 2)
    if hasattr(eng, "max_images"):
        batch_pairs = min(batch_pairs, eng.max_images() // 2)          # every activation must stay < 2 GiB
    batch_pairs = max(1, int(batch_pairs))
    feats = _features_fn(ad, prompt, target_block, target_layer, target_step)
    score = local = contrib = None
    for i0 in range(0, n, batch_pairs):
        i1 = min(n, i0 + batch_pairs)
        m = i1 - i0
        lat = torch.stack([latA[i0:i1], latB[i0:i1]], dim=1).reshape(2 * m, *shp)
        nA = noiseA[i0:i1] if (noiseA.shape[0] == n and n > 1) else noiseA.expand(m, *shp)
        nB = noiseB[i0:i1] if (noiseB.shape[0] == n and n > 1) else noiseB.expand(m, *shp)
        nz = torch.stack([nA, nB], dim=1).reshape(2 * m, *shp)
        q, k, v = feats(lat, nz)
        ia = torch.arange(0, 2 * m, 2, dtype=torch.int32, device=dev)
        s, lo, co = pair_score_maps(q, k, v, ia, ia + 1, heads, similarity)
        if score is None:
            N = lo.shape[2]
            score = torch.empty(n, dtype=torch.float32, device=dev)
            local = torch.empty((n, 2, N), dtype=torch.float32, device=dev)
            contrib = torch.empty((n, 2, N), dtype=torch.float32, device=dev)
        score[i0:i1], local[i0:i1], contrib[i0:i1] = s, lo, co
    if score is None:
        raise ValueError("no pairs to map")
    return SimilarityMaps(score, local, contrib)


def path_pair_latents(scorer, pairs: Sequence[Tuple[str, str]], img_size, seed=2333):
    """(latA, latB, noiseA, noiseB) of (A, B) path pairs as one reference call per pair would make them (each reseeds: the four
    draws -- VAE sample A, VAE sample B, noise A, noise B -- are the same tensors for every pair).  The HIP VAE fast path where
    the scorer has one (images decoded ahead on the host, one encode per chunk), else the scorer's prepare_image_latents."""
    ad = _Adapter(scorer)
    if ad.fast:
        vae = ad.vae
        sf = vae.config.scaling_factor
        pool = getattr(scorer, "_decode", None) or _shared_pool()
        chunk = 16                      # pairs per VAE encode (32 images at 512 px keep its widest activation < 2 GiB)
        starts = list(range(0, len(pairs), chunk))

        def submit(i0):
            return pool.submit([p for ab in pairs[i0:i0 + chunk] for p in ab], img_size)
        pending = [submit(i0) for i0 in starts[:2]]              # decode + resize run two chunks ahead of the GPU
        draws = None
        lA, lB = [], []
        for ci, i0 in enumerate(starts):
            px = DecodePool.gather(pending.pop(0))
            if ci + 2 < len(starts):
                pending.append(submit(starts[ci + 2]))
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
            lA.append(latent_sample(mom, draws[0], sf, 0, 2, ad.round16))
            lB.append(latent_sample(mom, draws[1], sf, 1, 2, ad.round16))
        return torch.cat(lA), torch.cat(lB), draws[2], draws[3]
    lA, lB = [], []
    nA = nB = None
    for pa, pb in pairs:
        g = get_generator(seed, "cpu")
        lA.append(_prepare(scorer, ad, process_image(load_image(pa), img_size), g))
        lB.append(_prepare(scorer, ad, process_image(load_image(pb), img_size), g))
        if nA is None:
            nA = torch.randn(lA[-1].shape, generator=g, dtype=ad.noise_draw).float()
            nB = torch.randn(lB[-1].shape, generator=g, dtype=ad.noise_draw).float()
    return torch.cat(lA), torch.cat(lB), nA, nB


@torch.no_grad()
def score_path_pair_maps(scorer, pairs: Sequence[Tuple[str, str]], img_size, prompt, target_block="up_blocks", target_layer=0,
                         target_step=600, seed=2333, similarity="cosine", batch_pairs: Optional[int] = None) -> SimilarityMaps:
    """Maps of (A, B) path pairs: what one ``diffsim(A, B, ...)`` call per pair would score (``score_pairs``' draw order), with
    each pair's per-token terms on both images' grids."""
    if not pairs:
        raise ValueError("no pairs to map")
    latA, latB, nA, nB = path_pair_latents(scorer, list(pairs), img_size, seed)
    return score_latent_pair_maps(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity,
                                  batch_pairs)


def map_names(paths_a: Sequence[str], root: Optional[str] = None):
    """Map file name per query: its ranking file's name (``retrieval.ranking_names``) with .npz for .txt."""
    from .retrieval import ranking_names
    return [n[:-len(".txt")] + ".npz" for n in ranking_names(paths_a, root)]


def write_map_files(out_dir: str, paths_a: Sequence[str], paths_b: Sequence[str], idx: torch.Tensor, maps: SimilarityMaps,
                    query_root: Optional[str] = None):
    """One .npz per query beside its ranking file: gallery (the k ranked paths), score (k,), local and contrib (k, 2, h, w) --
    direction 0 on the query's grid, 1 on the gallery image's.  maps holds the n_a * k pairs query-major (idx: (n_a, k))."""
    import numpy as np
    names = map_names(paths_a, query_root)
    k = idx.shape[1]
    score, local, contrib = (t.detach().float().cpu().numpy() for t in (maps.score, maps.local, maps.contrib))
    files = []
    for i, name in enumerate(names):
        fn = os.path.join(out_dir, name)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        sl = slice(i * k, (i + 1) * k)
        np.savez(fn, gallery=np.array([paths_b[j] for j in idx[i].tolist()], dtype=str), score=score[sl], local=local[sl],
                 contrib=contrib[sl])
        files.append(fn)
    return files
