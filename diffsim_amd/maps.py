"""Similarity maps: where on each image's grid two images match.

The DiffSim score breaks down exactly into per-token terms.  For direction a->b, cos(O_ab, O_aa) over the flattened
(B, H, N, D) tensors (diffsim.py:177-190) is sum_i dot_i / (|O_ab| |O_aa|), where dot_i sums over the CFG halves, the heads
and d at query token i; mse splits the same way, sum_i sqd_i / (B H N D).  Token i of direction a->b sits on image a's grid at
row i // w, column i % w (the U-Net's NCHW -> tokens flatten and DiT's patchify order).  So a pair has two maps, one on each
image, and their terms sum to the score.  ``engine.pair_score_maps`` computes them in the fused tail.

``local``: the token's own cosine of its O_ab and O_aa vectors (or their mean squared difference) -- how well that region matches.
``contrib``: the token's term of the score -- 0.5 * (contrib[:, 0].sum() + contrib[:, 1].sum()) is the pair's score.

Region maps.  With token masks (regions.py) the functions below explain a REGION score instead: the attentions run over the on
tokens alone (``engine.pair_score_maps_regions``), the terms are the region score's own, and the off tokens hold exact zeros; the
maps then carry the masks.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .engine import pair_score_maps, pair_score_maps_regions, pair_score_maps_weights      # noqa: F401  (RegionKind.tail)
from .inputs import path_latents
from .regions import chunk_tails, grid_shape, kind_of, path_rows, tap_grid        # noqa: F401  (grid_shape: imported from here too)
from .retrieval import ranking_names


class SimilarityMaps:
    """score (n,), local and contrib (n, 2, h, w) f32 tensors: pair p's direction 0 lies on image A's token grid, direction 1 on
    image B's; grid = (h, w), token i at (i // w, i % w).  Built from the flat (n, 2, N) maps of ``engine.pair_score_maps``.
    mask: None, or for region maps the (n, 2, h, w) bool token masks the maps were computed over (off tokens hold zeros).
    weights: None, or for soft region maps the (n, 2, h, w) uint8 token weights; mask is then ``weights != 0``."""

    def __init__(self, score: torch.Tensor, local: torch.Tensor, contrib: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 weights: Optional[torch.Tensor] = None):
        if local.shape != contrib.shape or local.ndim != 3 or local.shape[1] != 2 or local.shape[0] != score.shape[0]:
            raise ValueError(f"maps must be (n, 2, N) with n = len(score): {tuple(local.shape)}, {tuple(contrib.shape)}, "
                             f"{tuple(score.shape)}")
        n, _, N = local.shape
        if weights is not None:
            if weights.dtype != torch.uint8 or weights.numel() != local.numel() or weights.shape[:2] != local.shape[:2]:
                raise ValueError(f"weights must be uint8 (n, 2, N) or (n, 2, h, w) like the maps: {weights.dtype}, {tuple(weights.shape)}")
            mask = weights != 0
        self.grid = grid_shape(N)
        self.score = score
        self.local = local.reshape(n, 2, *self.grid)
        self.contrib = contrib.reshape(n, 2, *self.grid)
        if mask is not None and (mask.dtype != torch.bool or mask.numel() != local.numel() or mask.shape[:2] != local.shape[:2]):
            raise ValueError(f"mask must be bool (n, 2, N) or (n, 2, h, w) like the maps: {mask.dtype}, {tuple(mask.shape)}")
        self.mask = None if mask is None else mask.reshape(n, 2, *self.grid)
        self.weights = None if weights is None else weights.reshape(n, 2, *self.grid)

    def __len__(self) -> int:
        return self.score.shape[0]

    def __getitem__(self, i) -> "SimilarityMaps":
        """The pairs i (an index or a slice) as maps of their own."""
        sl = slice(i, i + 1) if isinstance(i, int) else i
        return SimilarityMaps(self.score[sl], self.local[sl].flatten(2), self.contrib[sl].flatten(2),
                              None if self.mask is None else self.mask[sl], None if self.weights is None else self.weights[sl])

    def upsample(self, size: int, which: str = "local") -> torch.Tensor:
        """Bilinear (n, 2, size, size) maps for overlay on the size x size image (``img_size``); which: local or contrib."""
        m = {"local": self.local, "contrib": self.contrib}[which]
        return F.interpolate(m.float(), size=(int(size), int(size)), mode="bilinear", align_corners=False)


@torch.no_grad()
def score_latent_pair_maps(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                           similarity="cosine", batch_pairs: Optional[int] = None, *, maskA=None, maskB=None,
                           soft: bool = False) -> SimilarityMaps:
    """Maps of pair i = (latA[i] in slot A, latB[i] in slot B), any scorer kind (DiffSim, diffsim_xl, diffsim_DiT): the pairs of
    ``score_latent_pairs``, in chunks of batch_pairs (None: ``Scorer.auto_map_pairs``) -- one feature batch and one maps launch
    per chunk.  noiseA / noiseB: (1, C, s, s) or (n, C, s, s).  target_block / target_layer: the reference's flag pair
    (``Scorer.tap_of``; DiT: [layer]).
    maskA / maskB: region maps -- the masks of ``regions.score_latent_pair_regions`` ((n, h, w) or (n, N) on the tap's grid, no row
    empty; one of them None: whole images on that side); the score is then the region score and the maps carry the masks.
    soft: maskA / maskB are token weights, uint8 (n, h, w) or (n, N) as ``regions.score_latent_pair_weights`` takes them: the soft
    region maps (``engine.pair_score_maps_weights``); the score is the soft region score and the maps carry the weights."""
    dev = scorer.device
    n = latA.shape[0]
    tail, tail_of, carried = pair_score_maps, None, {}
    if soft and maskA is None and maskB is None:
        raise ValueError("soft=True weighs masks: give maskA and / or maskB")
    if maskA is not None or maskB is not None:
        kind = kind_of(soft)
        _grid, rows = kind.pair_rows(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1], n, maskA, maskB)
        maps_tail = kind.tail("maps", globals())
        tail, tail_of = None, chunk_tails(rows, lambda chunk, q, k, v, ia, ib, heads, sim: maps_tail(q, k, v, chunk, ia, ib, heads, sim))
        carried = {kind.carried: rows}
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    tap = scorer.tap_of(target_block, target_layer)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)
    score = local = contrib = None
    for i0, i1, (s, lo, co) in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, similarity, batch_pairs,
                                                  tail, tail_of=tail_of):
        if score is None:
            N = lo.shape[2]
            score = torch.empty(n, dtype=torch.float32, device=dev)
            local = torch.empty((n, 2, N), dtype=torch.float32, device=dev)
            contrib = torch.empty((n, 2, N), dtype=torch.float32, device=dev)
        score[i0:i1], local[i0:i1], contrib[i0:i1] = s, lo, co
    if score is None:
        raise ValueError("no pairs to map")
    return SimilarityMaps(score, local, contrib, **carried)


@torch.no_grad()
def score_path_pair_maps(scorer, pairs: Sequence[Tuple[str, str]], img_size, prompt, target_block="up_blocks", target_layer=0,
                         target_step=600, seed=2333, similarity="cosine", batch_pairs: Optional[int] = None, *, masks=None,
                         hip_vae: bool = True, soft: bool = False) -> SimilarityMaps:
    """Maps of (A, B) path pairs: what one ``diffsim(A, B, ...)`` call per pair would score (``score_pairs``' draw order), with
    each pair's per-token terms on both images' grids.
    masks: region maps -- one (mask_A, mask_B) per pair as ``regions.score_path_pair_regions`` takes them (each a path, a PIL
    image, a bool array on the token grid or None).  soft: the masks are soft masks (``regions.as_token_weights``)."""
    if not pairs:
        raise ValueError("no pairs to map")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    mA = mB = None
    if masks is not None:
        if len(masks) != len(pairs):
            raise ValueError(f"{len(masks)} mask pairs for {len(pairs)} pairs")
        mA, mB = path_rows(kind_of(soft), masks, tap_grid(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1]))
    return score_latent_pair_maps(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity,
                                  batch_pairs, maskA=mA, maskB=mB, soft=soft)


def map_names(paths_a: Sequence[str], root: Optional[str] = None):
    """Map file name per query: its ranking file's name (``retrieval.ranking_names``) with .npz for .txt."""
    return [n[:-len(".txt")] + ".npz" for n in ranking_names(paths_a, root)]


def write_map_files(out_dir: str, paths_a: Sequence[str], paths_b: Sequence[str], idx: torch.Tensor, maps: SimilarityMaps,
                    query_root: Optional[str] = None):
    """One .npz per query beside its ranking file: gallery (the k ranked paths), score (k,), local and contrib (k, 2, h, w) --
    direction 0 on the query's grid, 1 on the gallery image's.  maps holds the n_a * k pairs query-major (idx: (n_a, k)).  Region
    maps (maps.mask set) also write mask (k, 2, h, w) bool, soft region maps (maps.weights set) also weights (k, 2, h, w) uint8."""
    import numpy as np
    names = map_names(paths_a, query_root)
    k = idx.shape[1]
    score, local, contrib = (t.detach().float().cpu().numpy() for t in (maps.score, maps.local, maps.contrib))
    mask = None if maps.mask is None else maps.mask.detach().cpu().numpy()
    wts = None if maps.weights is None else maps.weights.detach().cpu().numpy()
    files = []
    for i, name in enumerate(names):
        fn = os.path.join(out_dir, name)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        sl = slice(i * k, (i + 1) * k)
        np.savez(fn, gallery=np.array([paths_b[j] for j in idx[i].tolist()], dtype=str), score=score[sl], local=local[sl],
                 contrib=contrib[sl], **({} if mask is None else {"mask": mask[sl]}), **({} if wts is None else {"weights": wts[sl]}))
        files.append(fn)
    return files
