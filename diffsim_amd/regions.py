"""Region scores: DiffSim of the part of each image the caller names.

Every image of a pair carries a token mask on the tap's grid; the region score is the reference's tail (diffsim.py:177-197) on
the masked tokens alone: the off tokens are neither queries nor keys, so the background takes part in no softmax -- which
multiplying a similarity map by a mask afterwards cannot undo.  ``engine.pair_score_regions`` computes it in the fused tail; with
full masks it is the DiffSim score.  Soft regions (``token_weights``, ``score_latent_pair_weights``) keep the coverage the
binarisation rounds away: a byte weight per token, which enters both attentions as a logit bias and the sums as a factor
(``engine.pair_score_weights``).  The reference declares the idea (``--use_mask``, argprocess.py:16) and its strongest
competitor on CUTE is built on it (metrics/foreground_feature_averaging.py); the masks here come from files or from the caller.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch

from .engine import pair_score_regions, pair_score_weights
from .inputs import path_latents
from .maps import grid_shape


def token_mask(mask_image, grid: Tuple[int, int]) -> torch.Tensor:
    """A mask image (PIL, any mode and size) on the (h, w) token grid: converted to "L", area-averaged onto the grid
    (``Image.BOX``), a token on where the average is >= 128.  A mask with no token on becomes all ones -- the whole image, the
    reference's own fallback (foreground_feature_averaging.py:70-71).  Returns a bool (h, w) tensor."""
    import numpy as np
    from PIL import Image
    h, w = int(grid[0]), int(grid[1])
    small = mask_image.convert("L").resize((w, h), Image.BOX)
    on = torch.from_numpy(np.asarray(small, dtype=np.uint8) >= 128)
    return on if bool(on.any()) else torch.ones(h, w, dtype=torch.bool)


def as_token_mask(mask, grid: Tuple[int, int]) -> torch.Tensor:
    """One image's mask -- a path, a PIL image, a bool array / tensor (h, w) or (N,) already on the grid, or None (the whole
    image) -- as a bool (h, w) tensor."""
    h, w = int(grid[0]), int(grid[1])
    if mask is None:
        return torch.ones(h, w, dtype=torch.bool)
    if isinstance(mask, (str, os.PathLike)):
        from PIL import Image
        with Image.open(mask) as im:
            return token_mask(im, grid)
    if hasattr(mask, "convert") and hasattr(mask, "resize"):
        return token_mask(mask, grid)
    t = torch.as_tensor(mask).detach().cpu()
    if t.numel() != h * w or t.ndim not in (1, 2):
        raise ValueError(f"a token mask of shape {tuple(t.shape)} does not lie on the {h} x {w} token grid")
    return (t != 0).reshape(h, w)


def token_weights(mask_image, grid: Tuple[int, int]) -> torch.Tensor:
    """A mask image on the (h, w) token grid as soft weights: converted to "L" and area-averaged onto the grid (``Image.BOX``) as
    ``token_mask`` does, the averaged byte kept -- a token's coverage, weight byte / 255 -- instead of thresholded.  A mask whose
    bytes are all 0 becomes all 255, the whole image (``token_mask``'s fallback).  Returns a uint8 (h, w) tensor;
    ``token_weights(m, g) >= 128`` is ``token_mask(m, g)`` wherever some token reaches 128."""
    import numpy as np
    from PIL import Image
    h, w = int(grid[0]), int(grid[1])
    small = mask_image.convert("L").resize((w, h), Image.BOX)
    b = torch.from_numpy(np.array(small, dtype=np.uint8))
    return b if bool(b.any()) else torch.full((h, w), 255, dtype=torch.uint8)


def as_token_weights(mask, grid: Tuple[int, int]) -> torch.Tensor:
    """One image's soft mask -- a path, a PIL image, a uint8 array / tensor (h, w) or (N,) already on the grid (the bytes), a bool
    one (255 where on), a float one with values in [0, 1] (rounded to round(255 w)), or None (the whole image) -- as a uint8 (h, w)
    tensor."""
    h, w = int(grid[0]), int(grid[1])
    if mask is None:
        return torch.full((h, w), 255, dtype=torch.uint8)
    if isinstance(mask, (str, os.PathLike)):
        from PIL import Image
        with Image.open(mask) as im:
            return token_weights(im, grid)
    if hasattr(mask, "convert") and hasattr(mask, "resize"):
        return token_weights(mask, grid)
    t = torch.as_tensor(mask).detach().cpu()
    if t.numel() != h * w or t.ndim not in (1, 2):
        raise ValueError(f"token weights of shape {tuple(t.shape)} do not lie on the {h} x {w} token grid")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8) * 255
    elif t.dtype.is_floating_point:
        if not bool(((t >= 0) & (t <= 1)).all()):
            raise ValueError("float token weights must lie in [0, 1]")
        t = torch.floor(255.0 * t.double() + 0.5).to(torch.uint8)
    elif t.dtype != torch.uint8:
        raise ValueError(f"token weights must be uint8 bytes, bool or floats in [0, 1]: {t.dtype}")
    return t.reshape(h, w)


def load_token_masks(paths: Sequence[Optional[str]], grid: Tuple[int, int]) -> torch.Tensor:
    """(n, h, w) bool: the mask files on the token grid (``token_mask``); a None entry is the whole image."""
    return torch.stack([as_token_mask(p, grid) for p in paths]) if len(paths) else torch.zeros((0, *grid), dtype=torch.bool)


def mask_path_for(image: str, image_root: str, mask_root: str) -> Optional[str]:
    """The mask file of <image_root>/rel/name.ext: <mask_root>/rel/name.png, else <mask_root>/rel/name.ext; None when neither
    exists."""
    rel = os.path.relpath(image, image_root)
    for cand in (os.path.splitext(rel)[0] + ".png", rel):
        p = os.path.join(mask_root, cand)
        if os.path.isfile(p):
            return p
    return None


def triplet_mask_paths(triplets, image_root: str, mask_root: str):
    """([(ref, left, right) mask paths or None per (A, B, C, prompt) triplet], the number of distinct images without a mask)"""
    found = {}
    for t in triplets:
        for p in t[:3]:
            if p not in found:
                found[p] = mask_path_for(p, image_root, mask_root)
    return [tuple(found[p] for p in t[:3]) for t in triplets], sum(1 for m in found.values() if m is None)


def tap_grid(scorer, tap, latent_side: int) -> Tuple[int, int]:
    """(h, w) of the token grid of a tap for latents of the given side."""
    _eng, shapes = scorer.sweep_engine([tap], int(latent_side))
    return grid_shape(shapes[0][0])


def _grid_rows(m, n: int, grid: Tuple[int, int], name: str, what: str) -> torch.Tensor:
    """(n, h, w) or (n, N) values per token checked against the tap's grid: (n, N) on the CPU"""
    N = grid[0] * grid[1]
    t = torch.as_tensor(m).detach().cpu()
    if t.ndim not in (2, 3) or t.shape[0] != n or (t.ndim == 3 and tuple(t.shape[1:]) != tuple(grid)) or (t.ndim == 2 and t.shape[1] != N):
        raise ValueError(f"{name}: {what} of shape {tuple(t.shape)} for {n} images on a {grid[0]} x {grid[1]} token grid: "
                         f"({n}, {grid[0]}, {grid[1]}) or ({n}, {N})")
    return t.reshape(n, N)


def _flat_masks(m, n: int, grid: Tuple[int, int], name: str) -> torch.Tensor:
    """(n, h, w) or (n, N) masks checked on the host against the tap's grid: (n, N) bool on the CPU, no row empty"""
    t = (_grid_rows(m, n, grid, name, "masks") != 0)
    empty = (~t.any(1)).nonzero().flatten().tolist()
    if empty:
        raise ValueError(f"{name}: the mask of image {empty[0]} has no token on (an empty region has no score)")
    return t


def _flat_weights(m, n: int, grid: Tuple[int, int], name: str) -> torch.Tensor:
    """_flat_masks for soft weights: (n, h, w) or (n, N) uint8 bytes checked against the tap's grid, (n, N) on the CPU, no row all 0"""
    t = _grid_rows(m, n, grid, name, "weights")
    if t.dtype != torch.uint8:
        raise ValueError(f"{name}: token weights are uint8 bytes (as_token_weights makes them): {t.dtype}")
    empty = (~(t != 0).any(1)).nonzero().flatten().tolist()
    if empty:
        raise ValueError(f"{name}: the weights of image {empty[0]} are all 0 (an image without weight has no score)")
    return t


def pair_token_masks(scorer, tap, latent_side: int, n: int, maskA, maskB):
    """((h, w), (n, 2, N) bool on the scorer's device) for n pairs at a tap: maskA / maskB as ``score_latent_pair_regions`` takes
    them, either may be None (whole images).  Row [i, 0] is image A_i's mask and [i, 1] image B_i's: a chunk's rows interleave as
    its images do (``Scorer.pair_chunks``)."""
    grid = tap_grid(scorer, tap, latent_side)
    whole = torch.ones((n, grid[0] * grid[1]), dtype=torch.bool)
    mA = whole if maskA is None else _flat_masks(maskA, n, grid, "maskA")
    mB = whole if maskB is None else _flat_masks(maskB, n, grid, "maskB")
    return grid, torch.stack([mA, mB], dim=1).to(scorer.device)


def pair_token_weights(scorer, tap, latent_side: int, n: int, weightA, weightB):
    """``pair_token_masks`` for soft masks: ((h, w), (n, 2, N) uint8 on the scorer's device); weightA / weightB as
    ``score_latent_pair_weights`` takes them, either may be None (whole images, byte 255)."""
    grid = tap_grid(scorer, tap, latent_side)
    whole = torch.full((n, grid[0] * grid[1]), 255, dtype=torch.uint8)
    wA = whole if weightA is None else _flat_weights(weightA, n, grid, "weightA")
    wB = whole if weightB is None else _flat_weights(weightB, n, grid, "weightB")
    return grid, torch.stack([wA, wB], dim=1).to(scorer.device)


@torch.no_grad()
def score_latent_pair_regions(scorer, latA, latB, noiseA, noiseB, maskA, maskB, prompt, target_block="up_blocks", target_layer=0,
                              target_step=600, similarity="cosine", batch_pairs: Optional[int] = None) -> torch.Tensor:
    """Region scores of pair i = (latA[i] over maskA[i] in slot A, latB[i] over maskB[i] in slot B), any scorer kind: the pairs of
    ``score_latent_pairs``, in chunks of batch_pairs (None: ``Scorer.auto_map_pairs``) -- one feature batch and one region tail
    per chunk.  maskA / maskB: (n, h, w) or (n, N) bool on any device, on the tap's token grid (``tap_grid``), no row empty.
    Returns the (n,) f32 scores on the device."""
    dev = scorer.device
    n = latA.shape[0]
    tap = scorer.tap_of(target_block, target_layer)
    grid = tap_grid(scorer, tap, latA.shape[-1])
    mA, mB = _flat_masks(maskA, n, grid, "maskA"), _flat_masks(maskB, n, grid, "maskB")
    both = torch.stack([mA, mB], dim=1).to(dev)               # (n, 2, N): a chunk's rows interleave as its images do
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)

    def tail_of(i0, i1):
        chunk = both[i0:i1].reshape(2 * (i1 - i0), -1).contiguous()
        return lambda q, k, v, ia, ib, heads, sim: pair_score_regions(q, k, v, chunk, ia, ib, heads, sim)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    for i0, i1, s in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, similarity, batch_pairs, None,
                                        tail_of=tail_of):
        score[i0:i1] = s
    if n == 0:
        raise ValueError("no pairs to score")
    return score


@torch.no_grad()
def score_path_pair_regions(scorer, pairs: Sequence[Tuple[str, str]], masks: Sequence[Tuple[object, object]], img_size, prompt,
                            target_block="up_blocks", target_layer=0, target_step=600, seed=2333, similarity="cosine",
                            batch_pairs: Optional[int] = None, hip_vae: bool = True) -> torch.Tensor:
    """Region scores of (A, B) path pairs with ``score_pairs``' draw order; masks: one (mask_A, mask_B) per pair, each a path, a
    PIL image, a bool array on the token grid or None (``as_token_mask``)."""
    if not pairs:
        raise ValueError("no pairs to score")
    if len(masks) != len(pairs):
        raise ValueError(f"{len(masks)} mask pairs for {len(pairs)} pairs")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    grid = tap_grid(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1])
    mA = torch.stack([as_token_mask(m[0], grid) for m in masks])
    mB = torch.stack([as_token_mask(m[1], grid) for m in masks])
    return score_latent_pair_regions(scorer, latA, latB, nA, nB, mA, mB, prompt, target_block, target_layer, target_step,
                                     similarity, batch_pairs)


@torch.no_grad()
def score_latent_pair_weights(scorer, latA, latB, noiseA, noiseB, weightA, weightB, prompt, target_block="up_blocks", target_layer=0,
                              target_step=600, similarity="cosine", batch_pairs: Optional[int] = None) -> torch.Tensor:
    """Soft region scores of pair i = (latA[i] weighted by weightA[i] in slot A, latB[i] by weightB[i] in slot B):
    ``score_latent_pair_regions`` with a byte weight per token (``engine.pair_score_weights``) instead of a bit.  weightA / weightB:
    (n, h, w) or (n, N) uint8 on any device, on the tap's token grid (``tap_grid``), no row all 0.  Returns the (n,) f32 scores on
    the device."""
    dev = scorer.device
    n = latA.shape[0]
    tap = scorer.tap_of(target_block, target_layer)
    grid = tap_grid(scorer, tap, latA.shape[-1])
    wA, wB = _flat_weights(weightA, n, grid, "weightA"), _flat_weights(weightB, n, grid, "weightB")
    both = torch.stack([wA, wB], dim=1).to(dev)               # (n, 2, N): a chunk's rows interleave as its images do
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)

    def tail_of(i0, i1):
        chunk = both[i0:i1].reshape(2 * (i1 - i0), -1).contiguous()
        return lambda q, k, v, ia, ib, heads, sim: pair_score_weights(q, k, v, chunk, ia, ib, heads, sim)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    for i0, i1, s in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, similarity, batch_pairs, None,
                                        tail_of=tail_of):
        score[i0:i1] = s
    if n == 0:
        raise ValueError("no pairs to score")
    return score


@torch.no_grad()
def score_path_pair_weights(scorer, pairs: Sequence[Tuple[str, str]], masks: Sequence[Tuple[object, object]], img_size, prompt,
                            target_block="up_blocks", target_layer=0, target_step=600, seed=2333, similarity="cosine",
                            batch_pairs: Optional[int] = None, hip_vae: bool = True) -> torch.Tensor:
    """Soft region scores of (A, B) path pairs with ``score_pairs``' draw order; masks: one (mask_A, mask_B) per pair, each a path,
    a PIL image, an array on the token grid or None (``as_token_weights``)."""
    if not pairs:
        raise ValueError("no pairs to score")
    if len(masks) != len(pairs):
        raise ValueError(f"{len(masks)} mask pairs for {len(pairs)} pairs")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    grid = tap_grid(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1])
    wA = torch.stack([as_token_weights(m[0], grid) for m in masks])
    wB = torch.stack([as_token_weights(m[1], grid) for m in masks])
    return score_latent_pair_weights(scorer, latA, latB, nA, nB, wA, wB, prompt, target_block, target_layer, target_step,
                                     similarity, batch_pairs)
