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

import math
import os
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch

from .engine import pair_score_regions, pair_score_weights       # noqa: F401  (RegionKind.tail finds them by name)
from .inputs import path_latents


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


def grid_shape(n_tokens: int) -> Tuple[int, int]:
    """(h, w) of a square token grid; a non-square token count is refused."""
    s = math.isqrt(int(n_tokens))
    if n_tokens < 1 or s * s != n_tokens:
        raise ValueError(f"{n_tokens} tokens do not form a square grid: maps need an h x w = s x s token grid")
    return s, s


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


class RegionKind(NamedTuple):
    """How a region is stated: a row of token bytes per image, bound to a chunk and handed to a tail.  HARD: bool masks, a token
    in or out; SOFT: uint8 weights, byte / 255.  Everything that differs between the two is a field here."""
    soft: bool
    on_grid: Callable               # one image's mask (a path, a PIL image, an array, None) -> its (h, w) row
    dtype: torch.dtype              # of the rows
    whole: object                   # a token's value in a whole image
    arg: str                        # the rows' argument names, <arg>A and <arg>B, and their noun in the messages
    empty: str                      # the refusal of image {}'s row when it has nothing on
    carried: str                    # the argument that carries the rows in SimilarityMaps and Alignment
    score: str                      # the names of the four engine tails, each with the rows behind the features,
    maps: str                       #   and of the matrix workspace query (``tail``)
    align: str
    matrix: str
    matrix_workspace_bytes: str
    cell_matrix: str                #   the matrix whose set-B rows belong to the cell (exemplar-guided retrieval), and its query
    cell_matrix_workspace_bytes: str

    def tail(self, form: str, bindings) -> Callable:
        """The kind's engine tail of a form (score, maps, align, matrix, cell_matrix and the two workspace queries) out of `bindings`, the calling
        module's globals(): every module calls its own binding of an engine tail, as it does engine.pair_score's
        (``Scorer.pair_tail``), so a stand-in bound there serves that module alone."""
        return bindings[getattr(self, form)]

    def whole_rows(self, n: int, N: int, device=None) -> torch.Tensor:
        """(n, N) rows of whole images"""
        return torch.full((n, N), self.whole, dtype=self.dtype, device=device)

    def flat_rows(self, m, n: int, grid: Tuple[int, int], name: str) -> torch.Tensor:
        """(n, h, w) or (n, N) rows checked on the host against the tap's grid: (n, N) on the CPU, no row empty.  Masks become bool
        whatever their dtype; weights are uint8 bytes already."""
        t = _grid_rows(m, n, grid, name, self.arg + "s")
        if not self.soft:
            t = t != 0
        elif t.dtype != torch.uint8:
            raise ValueError(f"{name}: token weights are uint8 bytes (as_token_weights makes them): {t.dtype}")
        empty = (~(t != 0).any(1)).nonzero().flatten().tolist()
        if empty:
            raise ValueError(f"{name}: " + self.empty.format(empty[0]))
        return t

    def set_rows(self, masks, n: int, grid, dev, name: str) -> torch.Tensor:
        """(n, N) rows on dev, one per image of a set (``on_grid``: paths, PIL images, arrays on the grid, None entries); masks
        None: whole images.  A row with nothing on is the whole image, as a mask file's is."""
        N = grid[0] * grid[1]
        if masks is None:
            return self.whole_rows(n, N, dev)
        if len(masks) != n:
            raise ValueError(f"{name}: {len(masks)} masks for {n} images")
        rows = torch.stack([self.on_grid(m, grid) for m in masks]).reshape(n, -1) if n else torch.zeros((0, N), dtype=self.dtype)
        rows = torch.where((rows != 0).any(1, keepdim=True), rows, torch.full_like(rows, self.whole))
        return rows.to(dev).contiguous()

    def pair_rows(self, scorer, tap, latent_side: int, n: int, rowsA, rowsB):
        """((h, w), (n, 2, N) rows on the scorer's device) for n pairs at a tap; rowsA / rowsB: (n, h, w) or (n, N) on the tap's grid,
        no row empty, either may be None (whole images).  Row [i, 0] is image A_i's and [i, 1] image B_i's."""
        grid = tap_grid(scorer, tap, latent_side)
        whole = self.whole_rows(n, grid[0] * grid[1])
        rA = whole if rowsA is None else self.flat_rows(rowsA, n, grid, self.arg + "A")
        rB = whole if rowsB is None else self.flat_rows(rowsB, n, grid, self.arg + "B")
        return grid, torch.stack([rA, rB], dim=1).to(scorer.device)


HARD = RegionKind(False, as_token_mask, torch.bool, True, "mask", "the mask of image {} has no token on (an empty region has no score)",
                  "mask", "pair_score_regions", "pair_score_maps_regions", "pair_align_regions", "score_matrix_regions",
                  "score_matrix_regions_workspace_bytes", "score_matrix_cell_regions", "score_matrix_cell_regions_workspace_bytes")
SOFT = RegionKind(True, as_token_weights, torch.uint8, 255, "weight",
                  "the weights of image {} are all 0 (an image without weight has no score)", "weights",
                  "pair_score_weights", "pair_score_maps_weights", "pair_align_weights", "score_matrix_weights",
                  "score_matrix_weights_workspace_bytes", "score_matrix_cell_weights", "score_matrix_cell_weights_workspace_bytes")


def kind_of(soft: bool) -> RegionKind:
    return SOFT if soft else HARD


def chunk_tails(rows: torch.Tensor, tail: Callable):
    """The ``tail_of`` of ``Scorer.pair_chunks`` for n pairs with the token rows `rows`, (n, 2, N) on the device: tail_of(i0, i1) is
    `tail` with the chunk's rows -- (2 (i1 - i0), N), interleaved as its images are: A0, B0, A1, B1, ... -- bound in front of
    pair_chunks' own arguments (q, k, v, idx_a, idx_b, heads, similarity)."""
    def tail_of(i0, i1):
        chunk = rows[i0:i1].reshape(2 * (i1 - i0), -1).contiguous()
        return lambda *args: tail(chunk, *args)
    return tail_of


def path_rows(kind: RegionKind, masks: Sequence[Tuple[object, object]], grid: Tuple[int, int]):
    """One (mask_A, mask_B) per pair, each a path, a PIL image, an array on the grid or None, as the two (n, h, w) row stacks"""
    return tuple(torch.stack([kind.on_grid(m[c], grid) for m in masks]) for c in (0, 1))


def pair_token_masks(scorer, tap, latent_side: int, n: int, maskA, maskB):
    """((h, w), (n, 2, N) bool on the scorer's device) for n pairs at a tap: maskA / maskB as ``score_latent_pair_regions`` takes
    them, either may be None (whole images).  Row [i, 0] is image A_i's mask and [i, 1] image B_i's: a chunk's rows interleave as
    its images do (``Scorer.pair_chunks``)."""
    return kind_of(False).pair_rows(scorer, tap, latent_side, n, maskA, maskB)


def pair_token_weights(scorer, tap, latent_side: int, n: int, weightA, weightB):
    """``pair_token_masks`` for soft masks: ((h, w), (n, 2, N) uint8 on the scorer's device); weightA / weightB as
    ``score_latent_pair_weights`` takes them, either may be None (whole images, byte 255)."""
    return kind_of(True).pair_rows(scorer, tap, latent_side, n, weightA, weightB)


def _latent_pair_scores(kind: RegionKind, scorer, latA, latB, noiseA, noiseB, rowsA, rowsB, prompt, target_block, target_layer,
                        target_step, similarity, batch_pairs) -> torch.Tensor:
    dev = scorer.device
    n = latA.shape[0]
    tap = scorer.tap_of(target_block, target_layer)
    grid = tap_grid(scorer, tap, latA.shape[-1])
    rA, rB = kind.flat_rows(rowsA, n, grid, kind.arg + "A"), kind.flat_rows(rowsB, n, grid, kind.arg + "B")
    both = torch.stack([rA, rB], dim=1).to(dev)               # (n, 2, N): a chunk's rows interleave as its images do
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)
    score_tail = kind.tail("score", globals())
    tail_of = chunk_tails(both, lambda rows, q, k, v, ia, ib, heads, sim: score_tail(q, k, v, rows, ia, ib, heads, sim))
    score = torch.empty(n, dtype=torch.float32, device=dev)
    for i0, i1, s in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, similarity, batch_pairs, None,
                                        tail_of=tail_of):
        score[i0:i1] = s
    if n == 0:
        raise ValueError("no pairs to score")
    return score


def _path_pair_scores(kind: RegionKind, scorer, pairs, masks, img_size, prompt, target_block, target_layer, target_step, seed, similarity,
                      batch_pairs, hip_vae) -> torch.Tensor:
    if not pairs:
        raise ValueError("no pairs to score")
    if len(masks) != len(pairs):
        raise ValueError(f"{len(masks)} mask pairs for {len(pairs)} pairs")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    grid = tap_grid(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1])
    rA, rB = path_rows(kind, masks, grid)
    return _latent_pair_scores(kind, scorer, latA, latB, nA, nB, rA, rB, prompt, target_block, target_layer, target_step, similarity,
                               batch_pairs)


@torch.no_grad()
def score_latent_pair_regions(scorer, latA, latB, noiseA, noiseB, maskA, maskB, prompt, target_block="up_blocks", target_layer=0,
                              target_step=600, similarity="cosine", batch_pairs: Optional[int] = None) -> torch.Tensor:
    """Region scores of pair i = (latA[i] over maskA[i] in slot A, latB[i] over maskB[i] in slot B), any scorer kind: the pairs of
    ``score_latent_pairs``, in chunks of batch_pairs (None: ``Scorer.auto_map_pairs``) -- one feature batch and one region tail
    per chunk.  maskA / maskB: (n, h, w) or (n, N) bool on any device, on the tap's token grid (``tap_grid``), no row empty.
    Returns the (n,) f32 scores on the device."""
    return _latent_pair_scores(kind_of(False), scorer, latA, latB, noiseA, noiseB, maskA, maskB, prompt, target_block, target_layer,
                               target_step, similarity, batch_pairs)


@torch.no_grad()
def score_path_pair_regions(scorer, pairs: Sequence[Tuple[str, str]], masks: Sequence[Tuple[object, object]], img_size, prompt,
                            target_block="up_blocks", target_layer=0, target_step=600, seed=2333, similarity="cosine",
                            batch_pairs: Optional[int] = None, hip_vae: bool = True) -> torch.Tensor:
    """Region scores of (A, B) path pairs with ``score_pairs``' draw order; masks: one (mask_A, mask_B) per pair, each a path, a
    PIL image, a bool array on the token grid or None (``as_token_mask``)."""
    return _path_pair_scores(kind_of(False), scorer, pairs, masks, img_size, prompt, target_block, target_layer, target_step, seed,
                             similarity, batch_pairs, hip_vae)


@torch.no_grad()
def score_latent_pair_weights(scorer, latA, latB, noiseA, noiseB, weightA, weightB, prompt, target_block="up_blocks", target_layer=0,
                              target_step=600, similarity="cosine", batch_pairs: Optional[int] = None) -> torch.Tensor:
    """Soft region scores of pair i = (latA[i] weighted by weightA[i] in slot A, latB[i] by weightB[i] in slot B):
    ``score_latent_pair_regions`` with a byte weight per token (``engine.pair_score_weights``) instead of a bit.  weightA / weightB:
    (n, h, w) or (n, N) uint8 on any device, on the tap's token grid (``tap_grid``), no row all 0.  Returns the (n,) f32 scores on
    the device."""
    return _latent_pair_scores(kind_of(True), scorer, latA, latB, noiseA, noiseB, weightA, weightB, prompt, target_block, target_layer,
                               target_step, similarity, batch_pairs)


@torch.no_grad()
def score_path_pair_weights(scorer, pairs: Sequence[Tuple[str, str]], masks: Sequence[Tuple[object, object]], img_size, prompt,
                            target_block="up_blocks", target_layer=0, target_step=600, seed=2333, similarity="cosine",
                            batch_pairs: Optional[int] = None, hip_vae: bool = True) -> torch.Tensor:
    """Soft region scores of (A, B) path pairs with ``score_pairs``' draw order; masks: one (mask_A, mask_B) per pair, each a path,
    a PIL image, an array on the token grid or None (``as_token_weights``)."""
    return _path_pair_scores(kind_of(True), scorer, pairs, masks, img_size, prompt, target_block, target_layer, target_step, seed,
                             similarity, batch_pairs, hip_vae)
