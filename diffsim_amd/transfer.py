"""Exemplar-guided regions: a mask on one image picks the other's region.

The common evaluation setup has a reference image with a known object mask (a subject photo with its segmentation) and generated
images without masks.  The score is built on the cross-attention of one image's queries over the other's keys, and the share of a
token's attention that lands inside the other image's masked tokens says whether the token belongs to the same object:
``engine.pair_region_transfer`` returns that attention mass, sum_j Pm[u][j] w[j] with the token alignments' Pm (``engine.pair_align``)
and w the exemplar's token weights, without forming Pm.  The region of the unmasked image is ``textattn``'s rule applied to the mass
-- a token is on iff its mass is at least ``rel_threshold`` x the image's mean mass, float64 torch ops on the device; no token
passing, or a non-finite mass, is the whole image; a soft guide keeps the mass below the threshold as a token weight
(``textattn.soft_token_bytes``) -- and the pair is scored by the region tail (``engine.pair_score_regions``) or the soft region tail
(``engine.pair_score_weights``) over (the exemplar's mask, the transferred region).

Two cases never reach the kernel, because rounding would otherwise decide them: an exemplar whose bytes are all 255 (no mask, a
full mask) has mass 1 +- rounding everywhere, and the other image is the whole image; an exemplar whose bytes are all 0 is the whole
image, as an empty mask is everywhere in regions.py, and the first case applies.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .engine import pair_region_transfer, pair_score_regions, pair_score_weights, region_transfer_matrix      # noqa: F401  (RegionKind.tail)
from .inputs import path_latents
from .regions import chunk_tails, kind_of, tap_grid
from .textattn import soft_token_bytes


def region_of_mass(mass: torch.Tensor, full: torch.Tensor, rel_threshold: float, soft: bool = False) -> torch.Tensor:
    """The region rule on masses: mass (n, N) f32 and full (n,) bool (the row's exemplar is fully on: the row is the whole image
    whatever its mass), on one device.  Hard: (n, N) bool, token u on iff (double)mass[u] >= rel_threshold * mean(mass) in float64;
    a row where no token passes or a value is non-finite is all on.  soft: (n, N) uint8, ``soft_token_bytes`` of the mass and that
    mask (255 wherever the hard rule says on)."""
    s = mass.double()
    hard = s >= float(rel_threshold) * s.mean(1, keepdim=True)
    whole = full | ~torch.isfinite(s).all(1) | ~hard.any(1)
    hard = hard | whole[:, None]
    return soft_token_bytes(mass, hard, rel_threshold) if soft else hard


class ExemplarGuide:
    """What an exemplar-guided run carries: the threshold, whether the regions are soft, and the running size of the regions it has
    made (``on_fraction``: the mean share of tokens on, or the mean weight when soft)."""

    def __init__(self, rel_threshold: float = 1.0, soft: bool = False):
        self.soft = bool(soft)
        self.rel_threshold = float(rel_threshold)
        if not (self.rel_threshold >= 0.0) or self.rel_threshold == float("inf"):
            raise ValueError(f"rel_threshold must be finite and >= 0: {rel_threshold}")
        self._on = None             # device scalars: tokens on, tokens seen
        self._seen = 0

    def regions(self, q, k, heads: int, rows: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor, return_mass: bool = False):
        """The mask rows (bool, hard guide) or weight rows (uint8, soft guide) of a chunk's images, (images, N) on the device, with
        the row of every image idx_b[p] replaced by the region image idx_a[p]'s row transfers to it: one transfer launch, directions=2,
        over the pairs whose exemplar is neither fully on nor empty (those two make the other image whole without a launch; an empty
        exemplar row is returned all on).  An image that is idx_b of several pairs keeps the last pair's region.  q, k: the chunk's
        features; ia, ib: int32 (pairs,).  return_mass: also the (pairs, N) f32 mass on the idx_b images' grids (1 where no launch was
        needed)."""
        want = kind_of(self.soft).dtype
        if rows.dtype != want or rows.ndim != 2:
            raise ValueError(f"a {'soft' if self.soft else 'hard'} guide takes (images, N) {want} rows: {rows.dtype} {tuple(rows.shape)}")
        la, lb = ia.long(), ib.long()
        bytes_ = rows if self.soft else rows.to(torch.uint8) * 255
        bytes_ = torch.where((bytes_ != 0).any(1, keepdim=True), bytes_, torch.full_like(bytes_, 255))      # an empty row: the whole image
        full = (bytes_[la] == 255).all(1)                        # (pairs,)
        mass = torch.ones((ia.numel(), rows.shape[1]), dtype=torch.float32, device=rows.device)
        live = (~full).nonzero().flatten()                       # (one device read per chunk: which pairs need the kernel)
        if live.numel():
            sub = pair_region_transfer(q, k, bytes_.contiguous(), ia[live].contiguous(), ib[live].contiguous(), heads, directions=2)
            mass[live] = sub[:, 1]
        region = region_of_mass(mass, full, self.rel_threshold, self.soft)
        out = bytes_ if self.soft else bytes_ != 0
        out[lb] = region
        self.account(region)
        return (out, mass) if return_mass else out

    def account(self, region: torch.Tensor):
        """Adds transferred regions (bool masks or uint8 weights, any shape with the tokens last) to ``on_fraction``'s running sums:
        what ``regions`` and ``cell_regions`` both do with the regions they make.  No device read."""
        on = region.sum(dtype=torch.float64) / (255.0 if self.soft else 1.0)
        self._on = on if self._on is None else self._on + on
        self._seen += region.numel()

    def cell_regions(self, fa, fb, heads: int, rows_a: torch.Tensor):
        """The regions of a score matrix's cells: (regions (n_a, n_b, N) bool or uint8, mass (n_a, n_b, N) f32) on the device, row
        [i][j] what exemplar fa[i]'s row rows_a[i] transfers to gallery image fb[j] -- ``regions``' values for the pair (fa[i], fb[j]),
        bit for bit, from one transfer-matrix launch (``engine.region_transfer_matrix``) and one pass of the region rule over the
        (n_a n_b, N) masses with an exemplar's ``full`` repeated along its row.  fa, fb: the sets' (q, k, v); rows_a: (n_a, N) rows of
        the guide's kind, no row empty (``RegionKind.set_rows`` makes them).  An exemplar that is fully on makes every gallery image
        of its row whole, with mass 1, as ``regions`` does without a launch; with every exemplar fully on nothing is launched."""
        want = kind_of(self.soft).dtype
        if rows_a.dtype != want or rows_a.ndim != 2:
            raise ValueError(f"a {'soft' if self.soft else 'hard'} guide takes (n_a, N) {want} rows: {rows_a.dtype} {tuple(rows_a.shape)}")
        n_a, n_b, N = rows_a.shape[0], fb[0].shape[0], rows_a.shape[1]
        bytes_ = rows_a if self.soft else rows_a.to(torch.uint8) * 255
        bytes_ = torch.where((bytes_ != 0).any(1, keepdim=True), bytes_, torch.full_like(bytes_, 255))      # an empty row: the whole image
        full = (bytes_ == 255).all(1)                            # (n_a,)
        mass = torch.ones((n_a, n_b, N), dtype=torch.float32, device=rows_a.device)
        if not bool(full.all()):                                 # (one device read per chunk: whether the kernel is needed)
            mass = torch.where(full[:, None, None], mass, region_transfer_matrix(fa, fb, bytes_.contiguous(), heads))
        region = region_of_mass(mass.reshape(n_a * n_b, N), full.repeat_interleave(n_b), self.rel_threshold, self.soft)
        self.account(region)
        return region.reshape(n_a, n_b, N), mass

    @property
    def on_fraction(self) -> float:
        """Mean share of tokens on (soft: mean weight) over every transferred region made so far (one device read)."""
        return float(self._on) / self._seen if self._seen else float("nan")


def require_exemplar_regions(scorer):
    """NotImplementedError unless the scorer kind has exemplar-guided regions (DiffSim, diffsim_xl, diffsim_DiT)."""
    if not getattr(scorer, "exemplar_regions", False):
        raise NotImplementedError(f"{type(scorer).__name__} has no exemplar-guided regions: they need --metric diffsim, diffsim_xl or dit")


def exemplar_rows(maskA, n: int, grid: Tuple[int, int], soft: bool) -> torch.Tensor:
    """The exemplars' masks on the token grid: maskA None (every exemplar whole), or n entries, each a path, a PIL image, an array on
    the grid or None (``regions.as_token_mask``; soft: ``regions.as_token_weights``).  (n, N) bool or uint8 on the CPU."""
    entries = [None] * n if maskA is None else list(maskA)
    if len(entries) != n:
        raise ValueError(f"{len(entries)} exemplar masks for {n} pairs")
    return torch.stack([kind_of(soft).on_grid(m, grid) for m in entries]).flatten(1)


@torch.no_grad()
def score_latent_pairs_exemplar(scorer, latA, latB, noiseA, noiseB, maskA, prompt, target_block="up_blocks", target_layer=0,
                                target_step=600, similarity="cosine", batch_pairs: Optional[int] = None, rel_threshold: float = 1.0,
                                soft: bool = False, return_regions: bool = False):
    """Exemplar-guided scores of pair i = (latA[i] over maskA[i] in slot A, latB[i] over the region maskA[i] transfers to it in slot B):
    the pairs of ``score_latent_pairs`` in chunks of batch_pairs -- one feature batch, one transfer launch and one region tail per
    chunk.  maskA: None, or one entry per pair (``exemplar_rows``).  soft: the exemplar's masks are token weights, the transferred
    regions ``soft_token_bytes`` of the mass, and the tail the soft region tail.  Returns the (n,) f32 scores on the device;
    return_regions: also the (n, 2, h, w) masks (soft: uint8 weights) the tail was given and the (n, h, w) f32 mass on B's grid."""
    require_exemplar_regions(scorer)
    dev = scorer.device
    n = latA.shape[0]
    if n == 0:
        raise ValueError("no pairs to score")
    guide = ExemplarGuide(rel_threshold, soft)
    tap = scorer.tap_of(target_block, target_layer)
    grid = tap_grid(scorer, tap, latA.shape[-1])
    kind = kind_of(soft)
    region_tail = kind.tail("score", globals())
    mA = exemplar_rows(maskA, n, grid, soft)
    both = torch.stack([mA, kind.whole_rows(*mA.shape)], dim=1).to(dev)     # (n, 2, N): a chunk's rows interleave as its images do
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)
    made, masses = [], []

    def tail(chunk, q, k, v, ia, ib, heads, sim):
        rows, mass = guide.regions(q, k, heads, chunk, ia, ib, return_mass=True)
        made.append(rows), masses.append(mass)
        return region_tail(q, k, v, rows.contiguous(), ia, ib, heads, sim)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    for i0, i1, s in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, similarity, batch_pairs, None,
                                        tail_of=chunk_tails(both, tail)):
        score[i0:i1] = s
    if not return_regions:
        return score
    return score, torch.cat(made).reshape(n, 2, *grid), torch.cat(masses).reshape(n, *grid)


@torch.no_grad()
def score_path_pairs_exemplar(scorer, pairs: Sequence[Tuple[str, str]], masks_a: Optional[Sequence], img_size, prompt,
                              target_block="up_blocks", target_layer=0, target_step=600, seed=2333, similarity="cosine",
                              batch_pairs: Optional[int] = None, rel_threshold: float = 1.0, soft: bool = False,
                              return_regions: bool = False, hip_vae: bool = True):
    """Exemplar-guided scores of (A, B) path pairs with ``score_pairs``' draw order (inputs.path_latents); masks_a: None, or one mask
    per pair for image A alone."""
    if not pairs:
        raise ValueError("no pairs to score")
    require_exemplar_regions(scorer)
    if masks_a is not None and len(masks_a) != len(pairs):
        raise ValueError(f"{len(masks_a)} exemplar masks for {len(pairs)} pairs")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    return score_latent_pairs_exemplar(scorer, latA, latB, nA, nB, masks_a, prompt, target_block, target_layer, target_step, similarity,
                                       batch_pairs, rel_threshold, soft, return_regions)


@torch.no_grad()
def path_transferred_region(scorer, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed,
                            rel_threshold: float = 1.0, soft: bool = False, batch_pairs: Optional[int] = None, hip_vae: bool = True):
    """(mass (h, w) f32, region (h, w) bool or uint8) on image_B's token grid: what mask_A on image_A transfers to image_B in one
    exemplar-guided call of the pair."""
    _s, regions, mass = score_path_pairs_exemplar(scorer, [(image_A, image_B)], [mask_A], img_size, prompt, target_block, target_layer,
                                                  target_step, seed, "cosine", batch_pairs, rel_threshold, soft, True, hip_vae)
    return mass[0], regions[0, 1]
