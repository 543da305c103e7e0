"""Score matrices for retrieval: every query image against every gallery image.

The paper ranks a whole gallery against each query (the reference's ``retrieval_vis.py`` plots such lists).  A reference call
reseeds its generator, so the score of (query a, gallery b) depends on a only through its slot-A features (VAE draw A, noise A)
and on b only through its slot-B features (VAE draw B, noise B).  Here every image is pushed through the U-Net once -- n_a + n_b
forwards instead of 2 n_a n_b -- and ``engine.score_matrix`` computes each image's self-attention once and two cross attentions
per cell.  Cell (i, j) equals what ``diffsim(paths_a[i], paths_b[j], ...)`` / ``diffsim_latents`` return for that pair.

Query features are computed once and kept; the gallery runs in chunks of the scorer's engine batch (one feature batch and one
``score_matrix`` call per chunk), and the chunk is halved until the call's workspace fits a fixed share of the free HBM.

With ``masks_a`` / ``masks_b`` every image carries a token mask on the tap's grid and the matrix is the region score matrix
(``engine.score_matrix_regions``): cell (i, j) is ``regions.score_latent_pair_regions`` of that pair -- the masked object is
retrieved, the background takes part in no softmax -- at the same n_a + n_b forwards.  With ``soft=True`` the masks are token
weights (``regions.as_token_weights``) and the matrix is the soft score matrix (``engine.score_matrix_weights``): cell (i, j) is
``regions.score_latent_pair_weights`` of that pair.

In ``score_latent_matrix_exemplar`` (``score_path_matrix(exemplar=)``) only the queries carry masks, and every gallery image's region is the one the
query's mask transfers to it -- a region per CELL: per gallery chunk one ``engine.region_transfer_matrix`` launch, the region rule
(``transfer.region_of_mass``) on all its masses, and one cell-region matrix (``engine.score_matrix_cell_regions`` / ``_weights``).
Cell (i, j) is ``transfer.score_latent_pairs_exemplar`` of that pair: score, region and mass.

A scorer with a matrix tail of its own (``Scorer.matrix_tail``: the feature-cosine metrics of ``feats.py``) ranks through it: what the
query set contributes is computed once per call, each gallery chunk's once, and one ``engine.feature_matrix`` per chunk.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

from ._lib import DsimError
from .engine import (region_transfer_matrix_workspace_bytes, score_matrix, score_matrix_cell_regions,  # noqa: F401
                     score_matrix_cell_regions_workspace_bytes, score_matrix_cell_weights, score_matrix_cell_weights_workspace_bytes,
                     score_matrix_regions, score_matrix_regions_workspace_bytes, score_matrix_weights,
                     score_matrix_weights_workspace_bytes, score_matrix_workspace_bytes)          # (RegionKind.tail finds them)
from .inputs import path_latents
from .regions import kind_of, tap_grid
from .scorer import stack_rows
from .transfer import ExemplarGuide, require_exemplar_regions

IMAGE_EXTS = (".png", ".jpg", ".jpeg")
ENCODE_CHUNK = 16               # images per VAE encode, per side (32 at 512 px keep its widest activation < 2 GiB)
WORKSPACE_SHARE = 0.25          # of the free HBM, for one score_matrix call's workspace (self outputs + partial sums)


def list_images(root: str) -> List[str]:
    """Every .png / .jpg / .jpeg file (either case) under root, recursively, in sorted path order."""
    out = []
    for d, dirs, files in os.walk(root):
        dirs.sort()
        out += [os.path.join(d, f) for f in sorted(files) if f.lower().endswith(IMAGE_EXTS)]
    return sorted(out)


def _features(scorer, lat, noise, prompt, tap, step, batch: int):
    """(q, k, v) of n latents that all sit in one slot (one noise tensor), in engine batches of `batch` images."""
    n = lat.shape[0]
    parts = [scorer.tap_features(*stack_rows([lat], [noise], i0, min(n, i0 + batch)), prompt, tap, step)
             for i0 in range(0, n, batch)]
    if len(parts) == 1:
        return tuple(t.contiguous() for t in parts[0])
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def set_weights(masks, n: int, grid, dev, name: str) -> torch.Tensor:
    """(n, N) uint8 on dev, one row of token weights per image of a set (``regions.as_token_weights``: paths, PIL images, arrays on
    the grid, None entries); masks None: whole images (255).  An image whose weights are all 0 is the whole image, as an empty mask
    is (``RegionKind.set_rows`` on the soft kind)."""
    return kind_of(True).set_rows(masks, n, grid, dev, name)


@torch.no_grad()
def score_latent_matrix(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                        similarity="cosine", batch: Optional[int] = None, return_status: bool = False, *, masks_a=None, masks_b=None,
                        soft: bool = False):
    """(n_a, n_b) f32 device tensor: query latents latA in slot A (noiseA), gallery latents latB in slot B (noiseB), any
    scorer kind (DiffSim, diffsim_xl, diffsim_DiT).  noiseA / noiseB: (1, C, s, s), shared by every pair as in the reference.
    batch: gallery images per chunk (None: the images of the triplet engine batch, ``Scorer.auto_rows``).
    return_status: also the number of NaN / infinite cells.
    masks_a / masks_b: one token mask per query / gallery image on the tap's grid (``regions.tap_grid``; each a path, a PIL image,
    a bool array (h, w) or (N,), or None) -- the region score matrix; given only one, the other side is whole images; both None: the
    score matrix.
    soft: the masks are token weights (``regions.as_token_weights``: a mask file's area average per token, uint8 bytes, floats in
    [0, 1]) and the matrix is the soft score matrix; an image whose weights are all 0 is the whole image."""
    return _latent_matrix(scorer, latA, latB, noiseA, noiseB, prompt, target_block, target_layer, target_step, similarity, batch,
                          return_status, masks_a, masks_b, soft, None, False)


@torch.no_grad()
def score_latent_matrix_exemplar(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                                 similarity="cosine", batch: Optional[int] = None, return_status: bool = False, *, masks_a=None,
                                 exemplar: Optional[ExemplarGuide] = None, return_regions: bool = False):
    """``score_latent_matrix`` with exemplar-guided regions (the matrix form of ``transfer.score_latent_pairs_exemplar``; a function
    beside ``score_latent_matrix`` as that one is beside ``score_latent_pairs``): masks_a are the exemplars' masks (None: every
    exemplar whole), the gallery has none, and gallery image j's region against query i is what masks_a[i] transfers to it.
    exemplar: the ``transfer.ExemplarGuide`` with the threshold and the kind (soft: the masks are token weights and the transferred
    regions too); None: ``ExemplarGuide()``.  Its ``on_fraction`` accumulates over the cells.  Cell (i, j) is
    ``transfer.score_latent_pairs_exemplar`` of the pair (latA[i], latB[j]): score, region and mass, bit for bit.
    return_regions: the result is followed by the transferred regions (n_a, n_b, h, w), bool or uint8, and the masses
    (n_a, n_b, h, w) f32 on the gallery images' grids.  The other arguments: as ``score_latent_matrix``."""
    require_exemplar_regions(scorer)
    exemplar = ExemplarGuide() if exemplar is None else exemplar
    return _latent_matrix(scorer, latA, latB, noiseA, noiseB, prompt, target_block, target_layer, target_step, similarity, batch,
                          return_status, masks_a, None, exemplar.soft, exemplar, return_regions)


def _latent_matrix(scorer, latA, latB, noiseA, noiseB, prompt, target_block, target_layer, target_step, similarity, batch,
                   return_status, masks_a, masks_b, soft, exemplar, return_regions):
    """score_latent_matrix and score_latent_matrix_exemplar: one chunked gallery loop"""
    dev = scorer.device
    latA = latA.to(dev, torch.float32)
    latB = latB.to(dev, torch.float32)
    nA = noiseA.to(dev, torch.float32)
    nB = noiseB.to(dev, torch.float32)
    n_a, n_b = latA.shape[0], latB.shape[0]
    tap = scorer.tap_of(target_block, target_layer)
    mtail = getattr(scorer, "matrix_tail", lambda tap: None)(tap)
    if mtail is not None and (masks_a is not None or masks_b is not None):
        raise DsimError(f"{type(scorer).__name__} ranks with a matrix tail of its own (Scorer.matrix_tail): it has no region matrix")
    if mtail is None and getattr(scorer, "pair_tail", lambda tap: None)(tap) is not None:
        raise DsimError(f"{type(scorer).__name__} scores pairs with a tail of its own (Scorer.pair_tail): there is no score matrix "
                        "for it yet (clip_cross needs a projected matrix); score pairs or triplets instead")
    prompt = scorer.bind_prompt(prompt, n_a, "queries")             # (one prompt of the call)
    eng = scorer.engine_at(tap)
    heads = eng.heads
    if batch is None:
        batch = 3 * scorer.auto_rows(eng, max(n_a, n_b), 3)
    batch = max(1, int(batch))
    fa = _features(scorer, latA, nA, prompt, tap, target_step, batch)
    out = torch.empty((n_a, n_b), dtype=torch.float32, device=dev)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    _, B, N, HD = fa[0].shape
    chunk = min(batch, n_b) if n_b else 1
    masked = masks_a is not None or masks_b is not None or exemplar is not None
    workspace_bytes = score_matrix_workspace_bytes
    if mtail is not None and exemplar is not None:
        raise DsimError(f"{type(scorer).__name__} ranks with a matrix tail of its own (Scorer.matrix_tail): it has no region matrix")
    if masked:
        kind = kind_of(soft)
        grid = tap_grid(scorer, tap, latA.shape[-1])
        masks_a, masks_b = kind.set_rows(masks_a, n_a, grid, dev, "masks_a"), kind.set_rows(masks_b, n_b, grid, dev, "masks_b")
        workspace_bytes = kind.tail("matrix_workspace_bytes", globals())
        if exemplar is not None:            # the transfer's workspace is freed before the cell matrix asks for its own: the larger of the two
            cells_bytes = kind.tail("cell_matrix_workspace_bytes", globals())

            def workspace_bytes(*shape):
                return max(cells_bytes(*shape), region_transfer_matrix_workspace_bytes(*shape))
            made, masses = [], []
    elif soft:
        raise DsimError("soft=True weighs masks: give masks_a and / or masks_b")
    if mtail is not None:
        workspace_bytes = mtail.workspace_bytes
        ga = mtail.features(fa, heads)          # the query set's share of every chunk's matrix, once per call
    try:
        free, _total = torch.cuda.mem_get_info(dev)
        while chunk > 1 and workspace_bytes(n_a, chunk, B, heads, N, HD // heads, fa[0].dtype) > WORKSPACE_SHARE * free:
            chunk = (chunk + 1) // 2
    except RuntimeError:
        pass
    for j0 in range(0, n_b, chunk):
        j1 = min(n_b, j0 + chunk)
        fb = _features(scorer, latB[j0:j1], nB, prompt, tap, target_step, batch)
        if mtail is not None:
            s, st = mtail.matrix(ga, mtail.features(fb, heads))
        elif exemplar is not None:
            region, mass = exemplar.cell_regions(fa, fb, heads, masks_a)
            s, st = kind.tail("cell_matrix", globals())(fa, fb, masks_a, region.contiguous(), heads, similarity, return_status=True)
            st = st != 0
            if return_regions:
                made.append(region), masses.append(mass)
        elif masked:
            s, st = kind.tail("matrix", globals())(fa, fb, masks_a, masks_b[j0:j1], heads, similarity, return_status=True)      # (a row slice: contiguous)
            st = st != 0
        else:
            s, st = score_matrix(fa, fb, heads, similarity, return_status=True)
        out[:, j0:j1] = s
        bad += st.sum()
    res = (out, int(bad)) if return_status else (out,)
    if return_regions:
        res = (*res, torch.cat(made, dim=1).reshape(n_a, n_b, *grid), torch.cat(masses, dim=1).reshape(n_a, n_b, *grid))
    return res if len(res) > 1 else res[0]


@torch.no_grad()
def score_path_matrix(scorer, paths_a: Sequence[str], paths_b: Sequence[str], img_size, prompt, target_block="up_blocks",
                      target_layer=0, target_step=600, seed=2333, similarity="cosine", batch: Optional[int] = None,
                      return_status: bool = False, *, masks_a=None, masks_b=None, soft: bool = False,
                      exemplar: Optional[ExemplarGuide] = None, return_regions: bool = False):
    """The (len(paths_a), len(paths_b)) matrix of ``diffsim(paths_a[i], paths_b[j], ...)`` scores: the query images are
    encoded with the reseeded generator's slot-A VAE draw and noise, the gallery images with the slot-B ones
    (``inputs.path_latents``).  Through the scorer's HIP VAE fast path where it has one.  masks_a / masks_b: as
    ``score_latent_matrix`` takes them, one per path; soft: as there.  exemplar: a ``transfer.ExemplarGuide`` -- the
    exemplar-guided matrix (``score_latent_matrix_exemplar``): masks_a are the exemplars' masks and masks_b must be None;
    return_regions (with exemplar): as there."""
    if exemplar is not None:
        if masks_b is not None:
            raise DsimError("exemplar-guided matrix: the gallery's regions are the transferred ones, masks_b must be None")
        require_exemplar_regions(scorer)
    elif return_regions:
        raise DsimError("return_regions returns the transferred regions: it needs exemplar=")
    if not paths_a or not paths_b:
        if return_regions:
            raise ValueError("no cells to return regions of")
        empty = torch.empty((len(paths_a), len(paths_b)), dtype=torch.float32, device=scorer.device)
        return (empty, 0) if return_status else empty
    (latA,), nA, _ = path_latents(scorer, [(p,) for p in paths_a], (0,), img_size, seed, ENCODE_CHUNK)
    (latB,), _, nB = path_latents(scorer, [(p,) for p in paths_b], (1,), img_size, seed, ENCODE_CHUNK)
    if exemplar is not None:
        return score_latent_matrix_exemplar(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity,
                                            batch, return_status, masks_a=masks_a, exemplar=exemplar, return_regions=return_regions)
    return score_latent_matrix(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity, batch,
                               return_status, masks_a=masks_a, masks_b=masks_b, soft=soft)


def topk(matrix: torch.Tensor, k: int, similarity: str = "cosine"):
    """(values, indices) of the k best gallery entries per query row: descending for cosine, ascending for mse (the
    reference drivers' ordering rule, night_main.py:157-163).  Ties go to the lower gallery index."""
    m = matrix.detach().float().cpu()
    k = max(0, min(int(k), m.shape[1]))
    # a stable sort keeps equal scores in gallery order; NaN scores rank last either way
    key = torch.nan_to_num(-m if similarity == "cosine" else m, nan=float("inf"))
    idx = torch.sort(key, dim=1, stable=True).indices[:, :k]
    return torch.gather(m, 1, idx), idx


def ranking_names(paths_a: Sequence[str], root: Optional[str] = None) -> List[str]:
    """Ranking file name per query: ``<query path relative to root, extension dropped>.txt`` (root: the queries' common
    folder), so that a/cat.png and b/cat.png get a/cat.txt and b/cat.txt.  Two queries that would share a file (cat.png and
    cat.jpg in one folder) are refused rather than overwriting each other."""
    if not paths_a:
        return []
    root = root if root is not None else os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in paths_a])
    names = [os.path.splitext(os.path.relpath(os.path.abspath(p), root))[0] + ".txt" for p in paths_a]
    seen = {}
    for p, n in zip(paths_a, names):
        if n in seen:
            raise ValueError(f"queries {seen[n]} and {p} would both be ranked into {n}")
        seen[n] = p
    return names


def write_rankings(out_dir: str, paths_a: Sequence[str], paths_b: Sequence[str], matrix: torch.Tensor, k: int,
                   similarity: str = "cosine", query_root: Optional[str] = None) -> List[str]:
    """One ranking file per query under out_dir (``ranking_names``: the query's path relative to query_root with .txt): k lines
    ``<gallery path> <score>`` in rank order.  Returns the files."""
    names = ranking_names(paths_a, query_root)
    vals, idx = topk(matrix, k, similarity)
    files = []
    for i, name in enumerate(names):
        fn = os.path.join(out_dir, name)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        with open(fn, "w") as f:
            for v, j in zip(vals[i].tolist(), idx[i].tolist()):
                f.write(f"{paths_b[j]} {v:.8g}\n")
        files.append(fn)
    return files
