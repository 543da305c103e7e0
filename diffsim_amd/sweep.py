"""Tap sweeps: the score at several taps from one forward.

Choosing the tap (--target_block / --target_layer: which block's self-attention q/k/v the score is built on) is the tuning that
costs DiffSim users GPU time: the paper's ablations sweep blocks and layers, and every benchmark driver picks its own setting.
One tap per forward recomputes, for every deeper tap, the whole prefix the shallower taps already walked through -- and on the
files-in path it decodes and VAE-encodes every image again.  The executors walk the graph in order, so one walk to the deepest
requested tap hands out the q/k/v of every tap it passes (``engine.UNetEngine.qkv_taps`` / ``engine.DiTEngine.qkv_taps``):
each tap's features are bit for bit those of a one-tap forward, and so is every score row here.

Tap names (the reference's addressing, as ``engine.resolve_tap``; layers are explicit -- the reference quirk that turns a
single-valued --target_layer into 0 belongs to the reference-compatible entry points):
  SD1.5: (block, layer), block in down_blocks / mid_blocks / up_blocks (down_blocks[:-1], up_blocks[1:])
  SDXL:  (block, [b, a, t]) into down_blocks[1:] / up_blocks[:-1]; mid: ("mid_blocks", [a, t])
  DiT:   the block index
``"all"`` names every tap the model's addressing can name (``all_taps``).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .engine import pair_score
from .harness import path_triplet_scores, triplet_chunks
from .inputs import path_latents
from .scorer import all_taps, stack_rows

UNET_BLOCKS = ("down_blocks", "mid_blocks", "up_blocks")


def _key(tap):
    return tap if isinstance(tap, int) else (tap[0], tuple(tap[1]) if isinstance(tap[1], (list, tuple)) else tap[1])


def parse_tap_specs(specs: Sequence[str], metric: str, cfg=None):
    """--taps SPEC [SPEC ...] -> taps in the scorer's form, in the given order.  metric: diffsim (SD1.5, ``up_blocks:0``),
    diffsim_xl (``up_blocks:0,1,9``, ``mid_blocks:0,5``) or dit (``blocks:13``).  ``all`` alone: every tap of `cfg`
    (``all_taps``), or the string "all" when no cfg is given.  ValueError for an unknown block, the wrong number of indices
    for the model, a repeated tap, or (with cfg) a tap the model does not have."""
    specs = list(specs)
    if specs == ["all"]:
        return all_taps(cfg) if cfg is not None else "all"
    if not specs or "all" in specs:
        raise ValueError("--taps takes SPEC [SPEC ...] or `all` alone")
    out = []
    for s in specs:
        block, sep, idx = s.partition(":")
        try:
            vals = [int(v) for v in idx.split(",")] if sep and idx else None
        except ValueError:
            vals = None
        if vals is None:
            raise ValueError(f"tap {s!r}: expected BLOCK:INDEX[,INDEX...]")
        if metric == "dit":
            if block != "blocks" or len(vals) != 1:
                raise ValueError(f"tap {s!r}: DiT taps are blocks:LAYER")
            tap = vals[0]
        elif metric in ("clip_cross", "dino_cross", "dinofeats"):
            if block != "layers" or len(vals) != 1:
                raise ValueError(f"tap {s!r}: ViT taps are layers:LAYER")
            tap = vals[0]
        elif block not in UNET_BLOCKS:
            raise ValueError(f"tap {s!r}: unknown block {block!r} (one of {', '.join(UNET_BLOCKS)})")
        elif metric == "diffsim_xl":
            want = 2 if block == "mid_blocks" else 3
            if len(vals) != want:
                raise ValueError(f"tap {s!r}: SDXL {block} taps take {want} indices "
                                 f"({'attention,transformer_block' if want == 2 else 'block,attention,transformer_block'})")
            tap = (block, vals)
        else:
            if len(vals) != 1:
                raise ValueError(f"tap {s!r}: SD1.5 taps take one layer index")
            tap = (block, vals[0])
        if any(_key(tap) == _key(t) for t in out):
            raise ValueError(f"tap {s!r} is given twice")
        out.append(tap)
    if cfg is not None:
        known = {_key(t) for t in all_taps(cfg)}
        for s, t in zip(specs, out):
            if _key(t) not in known:
                raise ValueError(f"tap {s!r}: this model has no such tap")
    return out


def tap_label(tap) -> Tuple[str, list]:
    """(target_block, target_layer) that a one-tap run of the same tap prints in its `Experiment on ...` line (DiT: the layer)."""
    if isinstance(tap, int):
        return "blocks", [tap]
    block, layer = tap
    return block, list(layer) if isinstance(layer, (list, tuple)) else [layer]


@torch.no_grad()
def score_latent_pairs_taps(scorer, latA, latB, noiseA, noiseB, prompt, taps, target_step=600, similarity="cosine",
                            batch_pairs: Optional[int] = None) -> torch.Tensor:
    """(n_taps, n) f32 device tensor: row t is bit for bit what ``score_latent_pairs`` returns at taps[t] for the pairs
    (latA[i] in slot A, latB[i] in slot B), any scorer kind (DiffSim, diffsim_xl, diffsim_DiT).  One forward per chunk of
    batch_pairs pairs serves every tap (None: ``Scorer.auto_rows``); results do not depend on the chunk.  noiseA / noiseB: (1, C, s, s)
    or (n, C, s, s).  prompt: as the scorer's score_latent_pairs takes it (DiffSim: one or one per pair; diffsim_xl: (context,
    pooled) or a prompt string; DiT: ignored).  taps: a list in the scorer's tap form, or "all"."""
    taps = scorer.canonical_taps(taps)
    dev = scorer.device
    n = latA.shape[0]
    prompt = scorer.bind_prompt(prompt, n, "pairs")
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    eng, shapes = scorer.sweep_engine(taps, latA.shape[2])
    batch_pairs = _sweep_rows(scorer, eng, taps, shapes, n, 2, prompt, batch_pairs)
    out = torch.empty((len(taps), n), dtype=torch.float32, device=dev)
    tails = [scorer.pair_tail(t) for t in taps]
    for i0 in range(0, n, batch_pairs):
        i1 = min(n, i0 + batch_pairs)
        fs = scorer.taps_features(*stack_rows([latA, latB], [noiseA, noiseB], i0, i1), scorer.chunk_prompt(prompt, i0, i1, 2), taps,
                                  target_step)
        ia = torch.arange(0, 2 * (i1 - i0), 2, dtype=torch.int32, device=dev)
        for t, (q, k, v) in enumerate(fs):
            out[t, i0:i1] = (tails[t] or pair_score)(q, k, v, ia, ia + 1, shapes[t][1], similarity)
    return out


@torch.no_grad()
def score_path_pairs_taps(scorer, pairs: Sequence[Tuple[str, str]], img_size, prompt, taps, target_step=600, similarity="cosine",
                          seed=2333, batch_pairs: Optional[int] = None) -> torch.Tensor:
    """(n_taps, len(pairs)): row t is what one reference call per (A, B) path pair scores at taps[t] (``DiffSim.score_pairs``'
    latents and draw order, ``inputs.path_latents``); the images are decoded and VAE-encoded once for all taps."""
    if not pairs:
        raise ValueError("no pairs to score")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16)
    return score_latent_pairs_taps(scorer, latA, latB, nA, nB, prompt, taps, target_step, similarity, batch_pairs)


def _sweep_rows(scorer, eng, taps, shapes, n: int, per_row: int, prompt, rows: Optional[int]) -> int:
    """Rows per engine batch of a sweep: the caller's, or ``Scorer.auto_rows``; within the 2 GiB bound of every tap output."""
    mixed = {"n_ctx": 2} if scorer.n_ctx(prompt) > 1 else {}
    if rows is None:
        rows = scorer.auto_rows(eng, n, per_row, taps, shapes, **mixed)
    return max(1, min(int(rows), eng.max_images_taps(taps, **mixed) // per_row))


def _score_chunks_taps(scorer, ref, left, right, nA, nB, prompt, taps, step, similarity, batch_triplets):
    """harness._score_chunks at every tap (``harness.triplet_chunks``): each engine batch is one ``taps_features`` call."""
    n = ref.shape[0]
    prompt = scorer.bind_prompt(prompt, n)
    eng, shapes = scorer.sweep_engine(taps, ref.shape[2])
    batch_triplets = _sweep_rows(scorer, eng, taps, shapes, n, 3, prompt, batch_triplets)
    return triplet_chunks(scorer, ref, left, right, nA, nB, prompt, [h for _t, h, _d in shapes], similarity, batch_triplets,
                          lambda lat, nz, p: scorer.taps_features(lat, nz, p, taps, step), tails=[scorer.pair_tail(t) for t in taps])


def score_path_triplets_taps(scorer, triplets: Sequence[Tuple[str, str, str, str]], img_size: int, taps, target_step,
                             seed=2333, similarity="cosine", rank: int = 0, world: int = 1, batch_triplets: int = 10,
                             unet_triplets: Optional[int] = None, return_status: bool = False):
    """``harness.score_path_triplets`` at every tap: (s_ab, s_ac), each (n_taps, len(triplets)) f32 on every rank, row t bit for
    bit the one-tap scores at taps[t].  The same rank shard and score gathers (one per tap), prompts encoded once each, the
    reference image's features shared by its two pairs, the images decoded and encoded once for all taps.  return_status: also
    the per-tap list of NaN / inf pair score counts."""
    taps = scorer.canonical_taps(taps)
    all_l, all_r, nbad = path_triplet_scores(
        scorer, triplets, img_size, seed, rank, world, batch_triplets, len(taps),
        lambda *lat_prompt: _score_chunks_taps(scorer, *lat_prompt, taps, target_step, similarity, unet_triplets))
    return (all_l, all_r, [int(b) for b in nbad.tolist()]) if return_status else (all_l, all_r)
