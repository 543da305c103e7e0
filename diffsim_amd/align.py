"""Token alignments: which token of the other image each token attends to.

The score tail is cross-attention of image A's queries over image B's keys (diffsim.py:177-180).  For direction a->b,
P_bh[i][j] = softmax_j(Q_a[b,h,i,:] . K_b[b,h,j,:] / sqrt(D)) and Pm is its mean over the CFG halves and the heads.  Direction 0
puts A's queries over B's keys and lies on A's token grid; direction 1 is the mirror and lies on B's.  Token j sits at row
j // w, column j % w (the U-Net's NCHW -> tokens flatten and DiT's patchify order).  ``engine.pair_align`` computes, per query
token, ``match`` = argmax_j Pm[i][j] (ties: the lowest j), ``weight`` = Pm[i][match] and ``expect`` = sum_j Pm[i][j] (row_j,
col_j), the soft-argmax position on the other image's grid.

Region alignments.  With token masks (regions.py) the softmax of a query token of R_a runs over the keys of R_b alone
(``engine.pair_align_regions``): match and expect still index the other image's full grid; the off query tokens carry match -1,
weight 0 and expect (-1, -1), and the alignment carries the masks.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch

from .engine import pair_align, pair_align_regions, pair_align_weights      # noqa: F401  (RegionKind.tail)
from .inputs import path_latents
from .regions import chunk_tails, grid_shape, kind_of, path_rows, tap_grid
from .retrieval import ranking_names


class Alignment:
    """match (int32) and weight (f32) (n, 2, h, w), expect (f32) (n, 2, h, w, 2): pair p's direction 0 lies on image A's token
    grid and points into image B's, direction 1 the other way round; grid = (h, w), token i at (i // w, i % w), and match holds
    flat token indices of the other grid.  Built from the flat (n, 2, N) / (n, 2, N, 2) tensors of ``engine.pair_align``.
    mask: None, or for region alignments the (n, 2, h, w) bool token masks (off tokens: match -1, weight 0, expect (-1, -1)).
    weights: None, or for soft region alignments the (n, 2, h, w) uint8 token weights; mask is then ``weights != 0``."""

    def __init__(self, match: torch.Tensor, weight: torch.Tensor, expect: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 weights: Optional[torch.Tensor] = None):
        if (match.ndim != 3 or match.shape[1] != 2 or weight.shape != match.shape or expect.shape != tuple(match.shape) + (2,)):
            raise ValueError(f"alignments must be (n, 2, N), (n, 2, N) and (n, 2, N, 2): {tuple(match.shape)}, "
                             f"{tuple(weight.shape)}, {tuple(expect.shape)}")
        n, _, N = match.shape
        if weights is not None:
            if weights.dtype != torch.uint8 or weights.numel() != match.numel() or weights.shape[:2] != match.shape[:2]:
                raise ValueError(f"weights must be uint8 (n, 2, N) or (n, 2, h, w) like match: {weights.dtype}, {tuple(weights.shape)}")
            mask = weights != 0
        self.grid = grid_shape(N)
        self.match = match.reshape(n, 2, *self.grid)
        self.weight = weight.reshape(n, 2, *self.grid)
        self.expect = expect.reshape(n, 2, *self.grid, 2)
        if mask is not None and (mask.dtype != torch.bool or mask.numel() != match.numel() or mask.shape[:2] != match.shape[:2]):
            raise ValueError(f"mask must be bool (n, 2, N) or (n, 2, h, w) like match: {mask.dtype}, {tuple(mask.shape)}")
        self.mask = None if mask is None else mask.reshape(n, 2, *self.grid)
        self.weights = None if weights is None else weights.reshape(n, 2, *self.grid)

    def __len__(self) -> int:
        return self.match.shape[0]

    def __getitem__(self, i) -> "Alignment":
        """The pairs i (an index or a slice) as an alignment of their own."""
        sl = slice(i, i + 1) if isinstance(i, int) else i
        return Alignment(self.match[sl].flatten(2), self.weight[sl].flatten(2), self.expect[sl].flatten(2, 3),
                         None if self.mask is None else self.mask[sl], None if self.weights is None else self.weights[sl])

    def points(self, size: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(src, dst), each f32 (n, 2, h, w, 2): the pixel centres (x, y) of every token and of its match on size x size images
        (``img_size``), for drawing the correspondences; token (r, c) is centred at ((c + 0.5) size / w, (r + 0.5) size / h)."""
        h, w = self.grid
        dev = self.match.device
        r = torch.arange(h, device=dev, dtype=torch.float32).view(h, 1).expand(h, w)
        c = torch.arange(w, device=dev, dtype=torch.float32).view(1, w).expand(h, w)
        src = torch.stack(((c + 0.5) * (size / w), (r + 0.5) * (size / h)), -1).expand(len(self), 2, h, w, 2)
        m = self.match.long()
        dst = torch.stack((((m % w).float() + 0.5) * (size / w), (torch.div(m, w, rounding_mode="floor").float() + 0.5) * (size / h)), -1)
        return src.contiguous(), dst


@torch.no_grad()
def score_latent_pair_alignment(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                                target_step=600, batch_pairs: Optional[int] = None, *, maskA=None, maskB=None,
                                soft: bool = False) -> Alignment:
    """Alignments of pair i = (latA[i] in slot A, latB[i] in slot B), any scorer kind: the pairs and the features of
    ``maps.score_latent_pair_maps``, in chunks of batch_pairs (None: ``Scorer.auto_map_pairs``) -- one feature batch and one
    ``engine.pair_align`` per chunk.
    maskA / maskB: region alignments -- the masks of ``regions.score_latent_pair_regions`` (one of them None: whole images on that
    side); the alignment then carries the masks.
    soft: maskA / maskB are uint8 token weights as ``regions.score_latent_pair_weights`` takes them: the soft region alignments
    (``engine.pair_align_weights``); the alignment then carries the weights."""
    dev = scorer.device
    n = latA.shape[0]
    tail_of, carried = None, {}
    if soft and maskA is None and maskB is None:
        raise ValueError("soft=True weighs masks: give maskA and / or maskB")
    if maskA is not None or maskB is not None:
        kind = kind_of(soft)
        grid, rows = kind.pair_rows(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1], n, maskA, maskB)
        align_tail = kind.tail("align", globals())
        tail_of = chunk_tails(rows, lambda chunk, q, k, v, ia, ib, heads, similarity: align_tail(q, k, chunk, ia, ib, heads, grid[1]))
        carried = {kind.carried: rows}
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    tap = scorer.tap_of(target_block, target_layer)
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)
    tail = lambda q, k, v, ia, ib, heads, similarity: pair_align(q, k, ia, ib, heads)       # noqa: E731  (no v, no similarity)
    match = weight = expect = None
    for i0, i1, (m, w, e) in scorer.pair_chunks(latA, latB, noiseA, noiseB, prompt, tap, target_step, None, batch_pairs, tail,
                                                tail_of=tail_of):
        if match is None:
            N = m.shape[2]
            match = torch.empty((n, 2, N), dtype=torch.int32, device=dev)
            weight = torch.empty((n, 2, N), dtype=torch.float32, device=dev)
            expect = torch.empty((n, 2, N, 2), dtype=torch.float32, device=dev)
        match[i0:i1], weight[i0:i1], expect[i0:i1] = m, w, e
    if match is None:
        raise ValueError("no pairs to align")
    return Alignment(match, weight, expect, **carried)


@torch.no_grad()
def score_path_pair_alignment(scorer, pairs: Sequence[Tuple[str, str]], img_size, prompt, target_block="up_blocks", target_layer=0,
                              target_step=600, seed=2333, batch_pairs: Optional[int] = None, *, masks=None,
                              hip_vae: bool = True, soft: bool = False) -> Alignment:
    """Alignments of (A, B) path pairs, on the latents and draws one ``diffsim(A, B, ...)`` call per pair would use
    (``inputs.path_latents``, as ``maps.score_path_pair_maps``).  masks: region alignments -- one (mask_A, mask_B) per pair as
    ``regions.score_path_pair_regions`` takes them.  soft: the masks are soft masks (``regions.as_token_weights``)."""
    if not pairs:
        raise ValueError("no pairs to align")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    mA = mB = None
    if masks is not None:
        if len(masks) != len(pairs):
            raise ValueError(f"{len(masks)} mask pairs for {len(pairs)} pairs")
        mA, mB = path_rows(kind_of(soft), masks, tap_grid(scorer, scorer.tap_of(target_block, target_layer), latA.shape[-1]))
    return score_latent_pair_alignment(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, batch_pairs,
                                       maskA=mA, maskB=mB, soft=soft)


def match_names(paths_a: Sequence[str], root: Optional[str] = None):
    """Match file name per query: its ranking file's name (``retrieval.ranking_names``) with .match.npz for .txt."""
    return [n[:-len(".txt")] + ".match.npz" for n in ranking_names(paths_a, root)]


def write_match_files(out_dir: str, paths_a: Sequence[str], paths_b: Sequence[str], idx: torch.Tensor, al: Alignment,
                      query_root: Optional[str] = None):
    """One .match.npz per query beside its ranking file: gallery (the k ranked paths), match (int32) and weight (k, 2, h, w),
    expect (k, 2, h, w, 2) -- direction 0 on the query's grid, 1 on the gallery image's.  al holds the n_a * k pairs query-major
    (idx: (n_a, k)).  Region alignments (al.mask set) also write mask (k, 2, h, w) bool, soft ones (al.weights set) also
    weights (k, 2, h, w) uint8."""
    import numpy as np
    names = match_names(paths_a, query_root)
    k = idx.shape[1]
    match, weight, expect = (t.detach().cpu().numpy() for t in (al.match, al.weight, al.expect))
    mask = None if al.mask is None else al.mask.detach().cpu().numpy()
    wts = None if al.weights is None else al.weights.detach().cpu().numpy()
    files = []
    for i, name in enumerate(names):
        fn = os.path.join(out_dir, name)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        sl = slice(i * k, (i + 1) * k)
        np.savez(fn, gallery=np.array([paths_b[j] for j in idx[i].tolist()], dtype=str), match=match[sl], weight=weight[sl],
                 expect=expect[sl], **({} if mask is None else {"mask": mask[sl]}), **({} if wts is None else {"weights": wts[sl]}))
        files.append(fn)
    return files
