"""Triplet / 2AFC benchmark harness with a per-(image, slot) feature cache.

The reference's drivers score every triplet with two full scorer calls, (A,B) and (A,C)
(``cute_main.py:111-132``, ``night_main.py:69-163``): image A is encoded, noised and pushed through
the U-Net twice with identical seed and slot, i.e. to bit-identical features.  Here the reference
image's features are computed once and shared by both pairs (3 U-Net forwards per triplet instead
of 4), every triplet of a chunk runs in one engine batch, and both scores of every triplet come
out of one fused tail launch (``dsim_pair_score`` takes index pairs into the feature tensor).

Decision rules mirror the reference:
  NIGHTS 2AFC  ``night_main.py:156-163``  cosine: predicted = 1 if s(ref,left) > s(ref,right) else 0;
                                          mse:    predicted = 1 if s(ref,left) < s(ref,right) else 0;
                                          correct when predicted == int(row['left_vote'])
  CUTE         ``cute_main.py:201-205``   correct when s(A,B) > s(A,C)  (B same instance, C other)
"""
from __future__ import annotations

import csv
import os
from typing import List, Optional, Sequence, Tuple

import torch

from .engine import pair_score, pair_score_regions, pair_score_weights      # noqa: F401  (RegionKind.tail)
from .inputs import path_latents
from .parallel import gather_scores, shard_triplets
from .regions import kind_of, tap_grid
from .scorer import stack_rows


@torch.no_grad()
def score_latent_triplets(scorer, lat_ref: torch.Tensor, lat_left: torch.Tensor, lat_right: torch.Tensor,
                          noiseA: torch.Tensor, noiseB: torch.Tensor, prompt, target_block="up_blocks", target_layer=0,
                          target_step=600, similarity="cosine", batch_triplets: Optional[int] = None, return_status: bool = False):
    """Scores (ref,left) and (ref,right) for every triplet; ref sits in slot A (noiseA), left and
    right in slot B (noiseB) exactly as two reference calls would place them.  Returns two (n,) f32
    device tensors that are bit-identical to 2n separate ``diffsim_latents`` calls (any scorer kind).
    batch_triplets=None: the engine batch of the measured optimum (``Scorer.auto_rows``).
    prompt: one for every triplet, or (DiffSim) a sequence of n, triplet i's: each engine batch then carries its triplets'
    prompts in one forward."""
    s_l, s_r, bad = _score_chunks(scorer, lat_ref, lat_left, lat_right, noiseA, noiseB, prompt, target_block, target_layer,
                                  target_step, similarity, batch_triplets)
    return (s_l[0], s_r[0], bad[0]) if return_status else (s_l[0], s_r[0])


def read_nights_csv(image_path: str, split: str = "val") -> List[dict]:
    """``data.csv`` of NIGHTS: split, ref_path, left_path, right_path, left_vote, prompt
    (night_main.py:53-67)."""
    rows = []
    with open(os.path.join(image_path, "data.csv"), mode="r") as f:
        for row in csv.DictReader(f):
            if row["split"] != split:
                continue
            rows.append({"ref": os.path.join(image_path, row["ref_path"]), "left": os.path.join(image_path, row["left_path"]),
                         "right": os.path.join(image_path, row["right_path"]), "vote": int(row["left_vote"]),
                         "prompt": f"An image of a {row['prompt'].lower()}"})
    return rows


def nights_decisions(s_left: torch.Tensor, s_right: torch.Tensor, similarity: str) -> torch.Tensor:
    if similarity == "mse":
        return (s_left < s_right).to(torch.int64)
    return (s_left > s_right).to(torch.int64)


def nights_accuracy(s_left, s_right, votes: Sequence[int], similarity: str = "cosine") -> float:
    pred = nights_decisions(s_left.cpu(), s_right.cpu(), similarity)
    v = torch.tensor(list(votes), dtype=torch.int64)
    return float((pred == v).float().mean() * 100.0) if len(v) else 0.0


def cute_accuracy(s_ab: torch.Tensor, s_ac: torch.Tensor) -> float:
    return float((s_ab.cpu() > s_ac.cpu()).float().mean() * 100.0) if s_ab.numel() else 0.0


@torch.no_grad()
def triplet_chunks(scorer, ref, left, right, nA, nB, prompt, heads, similarity, batch_triplets: int, feats, masks=None, text=None,
                   tails=None, soft: bool = False, exemplar=None):
    """(ref,left) and (ref,right) scores of latent triplets at every tap of a forward: 3 forwards per triplet (the reference
    image's features are shared), chunked engine batches, one fused tail launch per chunk and tap.  feats(lat, nz, prompt) ->
    [(q, k, v) per tap] is the forward of one engine batch, heads[t] tap t's head count.  masks: None, or the (ref, left, right)
    token masks, each (n, N) bool on the device: the region tail (regions.py) over each chunk's rows instead of the pair tail.
    text: None, or (guide, w): a textattn.TextGuide and its bound per-triplet weights; feats then returns (q, k, v, xq, xkv) per
    tap and the masks of the region tail are the text-guided regions of the chunk's images -- ref, left and right each their own,
    the ref's made once per triplet.  soft: the masks are (n, N) uint8 token weights (or the guide makes weights: TextGuide(soft=True))
    and the tail is the soft region tail, engine.pair_score_weights.  exemplar: None, or a transfer.ExemplarGuide (with masks): only the
    ref's masks count, and left and right each get the region the ref's mask transfers to them -- one transfer launch per chunk and tap,
    directions=2 over the chunk's (ia, ib), covers both; the guide's soft decides the tail.  tails: None, or each tap's ``Scorer.pair_tail`` (a None entry: engine.pair_score).  Returns
    the (nt, n) scores of both sides and the (nt,) NaN / inf counts."""
    n, nt, dev = ref.shape[0], len(heads), scorer.device
    s_l = torch.empty((nt, n), dtype=torch.float32, device=dev)
    s_r = torch.empty((nt, n), dtype=torch.float32, device=dev)
    bad = torch.zeros(nt, dtype=torch.int32, device=dev)
    for i0 in range(0, n, batch_triplets):
        i1 = min(n, i0 + batch_triplets)
        m = i1 - i0
        fs = feats(*stack_rows([ref, left, right], [nA, nB, nB], i0, i1), scorer.chunk_prompt(prompt, i0, i1, 3))
        base = torch.arange(0, 3 * m, 3, dtype=torch.int32, device=dev)
        ia, ib = torch.cat([base, base]), torch.cat([base + 1, base + 2])
        for t, (q, k, v, *xs) in enumerate(fs):
            if masks is None and text is None:
                s, st = ((tails[t] if tails else None) or pair_score)(q, k, v, ia, ib, heads[t], similarity, return_status=True)
            else:                                           # (the chunk's mask rows lie as its images do: ref, left, right)
                if text is not None:
                    rows, _counts = text[0].regions(*xs, heads[t], text[1], i0, i1, 3)
                else:
                    rows = torch.stack([mk[i0:i1] for mk in masks], dim=1).reshape(3 * m, -1).contiguous()
                    if exemplar is not None:
                        rows = exemplar.regions(q, k, heads[t], rows, ia, ib).contiguous()
                kind = kind_of(soft or (text is not None and getattr(text[0], "soft", False)))
                s, st = kind.tail("score", globals())(q, k, v, rows, ia, ib, heads[t], similarity, return_status=True)
                st = (st != 0).to(torch.int32)
            bad[t] += st.sum()
            s_l[t, i0:i1], s_r[t, i0:i1] = s[:m], s[m:]
    return s_l, s_r, bad


def _score_chunks(scorer, ref, left, right, nA, nB, prompt, block, layer, step, similarity, batch_triplets, masks=None, text=None,
                  soft: bool = False, exemplar=None):
    """triplet_chunks at the one tap (block, layer): each engine batch is one ``tap_features`` call.  masks: None, or one
    (ref, left, right) triple of masks per triplet (``regions.as_token_mask``), put on the tap's token grid here.  text: None, or
    a textattn.TextGuide: each engine batch is one ``tap_features_text`` call and the regions come from the text attention maps
    (per-row prompts give per-triplet weights).  soft (with masks): the masks become token weights (``regions.as_token_weights``) and
    the tail the soft region tail.  exemplar: None, or a transfer.ExemplarGuide: masks then holds ONE entry per triplet, the ref's mask
    (None: the whole image), and left and right get the regions it transfers to them (soft as the guide says)."""
    n = ref.shape[0]
    if exemplar is not None:
        masks, soft = _exemplar_masks(scorer, exemplar, masks, text, soft)
    if soft and masks is None:
        raise ValueError("soft=True weighs the tokens of masks=: it needs them (a text guide is soft by TextGuide(soft=True))")
    tap = scorer.tap_of(block, layer)
    if text is not None:
        if masks is not None:
            raise ValueError("a text-guided region and a mask file per image: one or the other")
        text = (text, text.bind(scorer, prompt, n))
    if masks is not None:
        grid = tap_grid(scorer, tap, ref.shape[-1])
        masks = [torch.stack([kind_of(soft).on_grid(mk[c], grid) for mk in masks]).flatten(1).to(scorer.device) for c in range(3)]
    ex = {} if exemplar is None else {"exemplar": exemplar}
    prompt = scorer.bind_prompt(prompt, n)
    eng = scorer.engine_at(tap)
    heads = eng.heads
    if batch_triplets is None:
        batch_triplets = scorer.auto_rows(eng, n, 3, n_ctx=scorer.n_ctx(prompt))
    if text is not None:
        return triplet_chunks(scorer, ref, left, right, nA, nB, prompt, [heads], similarity, batch_triplets,
                              lambda lat, nz, p: [scorer.tap_features_text(lat, nz, p, tap, step)], text=text)
    return triplet_chunks(scorer, ref, left, right, nA, nB, prompt, [heads], similarity, batch_triplets,
                          lambda lat, nz, p: [scorer.tap_features(lat, nz, p, tap, step)], *(() if masks is None else (masks,)),
                          tails=[scorer.pair_tail(tap)], **({"soft": True} if soft else {}), **ex)


def _exemplar_masks(scorer, exemplar, masks, text, soft: bool):
    """The checks of an exemplar-guided triplet run, and its masks as (ref, None, None) triples: (masks, the guide's soft)."""
    from .transfer import require_exemplar_regions
    require_exemplar_regions(scorer)
    if text is not None:
        raise ValueError("exemplar= and text=: an exemplar-guided region and a text-guided region, one or the other")
    if masks is None:
        raise ValueError("exemplar= transfers the ref's masks: it needs masks= (one entry per triplet, the ref's; None allowed)")
    if any(isinstance(mk, (tuple, list)) and len(mk) == 3 for mk in masks):
        raise ValueError("exemplar= takes one mask per triplet, the ref's: (ref, left, right) triples belong to a run without it")
    if soft and not exemplar.soft:
        raise ValueError("soft=True with a hard guide: a soft exemplar run is ExemplarGuide(soft=True)")
    return [(mk, None, None) for mk in masks], exemplar.soft


@torch.no_grad()
def path_triplet_scores(scorer, triplets: Sequence[Tuple[str, str, str, str]], img_size: int, seed, rank: int, world: int,
                        batch_triplets: int, nt: int, score, masks=None):
    """The skeleton of the path triplet runs: whole triplets sharded over ranks (the cached reference-image features stay
    local), grouped by ``Scorer.group_key``, each group's images through ``path_latents`` in chunks of batch_triplets and
    its latents through score(ref, left, right, nA, nB, prompt) -> (nt, n) scores of both sides and (nt,) NaN / inf counts.
    masks: None, or one entry per triplet; score then takes the group's entries as a seventh argument.
    Returns (s_ab, s_ac), each (nt, len(triplets)) on every rank, and the (nt,) counts summed over ranks."""
    n, dev = len(triplets), scorer.device
    sl, sr, order = [], [], []
    nbad = torch.zeros(nt, dtype=torch.int32, device=dev)
    # prompts differ per row.  SD1.5 and DiT: the whole shard is one group, its engine batches carry their rows' prompts (a
    # context table, each prompt encoded once); SDXL: one group per prompt (Scorer.group_key)
    groups = {}
    for j in shard_triplets(n, rank, world):
        groups.setdefault(scorer.group_key(triplets[j][3]), []).append(j)
    for idxs in groups.values():
        prompt = scorer.group_prompt([triplets[j][3] for j in idxs])
        (ref, left, right), nA, nB = path_latents(scorer, [triplets[j][:3] for j in idxs], (0, 1, 1), img_size, seed,
                                                  batch_triplets)
        a_, b_, bad = score(ref, left, right, nA, nB, prompt, *(() if masks is None else ([masks[j] for j in idxs],)))
        nbad += bad
        sl.append(a_); sr.append(b_); order += idxs
    if order:
        inv = torch.tensor(sorted(range(len(order)), key=lambda t: order[t]), dtype=torch.long, device=dev)
        loc_l, loc_r = torch.cat(sl, 1)[:, inv], torch.cat(sr, 1)[:, inv]
    else:
        loc_l = loc_r = torch.empty((nt, 0), dtype=torch.float32, device=dev)
    all_l = torch.stack([gather_scores(loc_l[t].contiguous(), n, rank, world) for t in range(nt)])
    all_r = torch.stack([gather_scores(loc_r[t].contiguous(), n, rank, world) for t in range(nt)])
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(nbad)
    return all_l, all_r, nbad


def score_path_triplets(scorer, triplets: Sequence[Tuple[str, str, str, str]], img_size: int, target_block, target_layer,
                        target_step, seed=2333, similarity="cosine", rank: int = 0, world: int = 1, batch_triplets: int = 10,
                        unet_triplets: Optional[int] = None, masks: Optional[Sequence] = None, text=None, soft: bool = False,
                        exemplar=None):
    """Scores s(A,B) and s(A,C) of every (A, B, C, prompt) path triplet -- the two scorer calls per triplet the
    reference's loops make (cute_main.py:111-132, night_main.py:69-90, style_main.py:150-175) -- for all three scorer
    kinds (DiffSim, diffsim_xl, diffsim_DiT): whole triplets sharded over ranks (the cached reference-image features stay
    local), prompts encoded once each, 3 forwards per triplet instead of 4, images of a chunk encoded together.

    Host work is only decode + Lanczos resize, on a thread pool that runs two chunks ahead of the GPU; the /255,
    (x-0.5)/0.5, NCHW and fp16-cast arithmetic of process_image and the posterior sampling run on the device
    (dsim_image_preprocess / dsim_latent_sample), bit-identically to the per-pair path.  masks: None, or one (ref, left, right)
    triple per triplet of mask paths, PIL images, bool arrays on the tap's token grid or None (the whole image): region scores
    (regions.py), what ``region_score(A, B, mask_A, mask_B, ...)`` and ``region_score(A, C, mask_A, mask_C, ...)`` return;
    with masks=None every call and launch is the unmasked run's.  soft=True (with masks): soft region scores -- each mask becomes
    byte weights on the token grid (``regions.as_token_weights``: the area average kept, not thresholded) and the tail is
    ``engine.pair_score_weights``; with soft=False every call and launch is the hard run's.  text: None, or a textattn.TextGuide (words, threshold):
    text-guided regions instead -- ref, left and right each get the region their own text attention map gives, the ref's once per
    triplet, a prompt per row giving weights per image; text.on_fraction is then the mean share of tokens on.  exemplar: None, or a
    transfer.ExemplarGuide (threshold, soft): exemplar-guided regions -- masks then holds one entry per triplet, the REF's mask alone
    (None allowed), and left and right each get the region that mask transfers to them (transfer.py); exemplar.on_fraction is then the
    mean share of tokens on; with text, or with (ref, left, right) triples, a ValueError; with exemplar=None every call and launch is
    the run's without it.  Returns
    (s_ab, s_ac, n_nonfinite):
    length-len(triplets) f32 tensors on every rank and the number of NaN/inf pair scores (NaN guard)."""
    # (batch_triplets sizes the decode / VAE-encode chunks; the U-Net batch is unet_triplets, or the scorer's auto_rows)
    if masks is not None and len(masks) != len(triplets):
        raise ValueError(f"{len(masks)} mask triples for {len(triplets)} triplets")
    if exemplar is not None:
        _exemplar_masks(scorer, exemplar, masks, text, soft)
    if masks is not None and text is not None:
        raise ValueError("a text-guided region and a mask file per image: one or the other")
    if soft and masks is None:
        raise ValueError("soft=True weighs the tokens of masks=: it needs them (a text guide is soft by TextGuide(soft=True))")
    all_l, all_r, nbad = path_triplet_scores(
        scorer, triplets, img_size, seed, rank, world, batch_triplets, 1,
        lambda *lat_prompt: _score_chunks(scorer, *lat_prompt[:6], target_block, target_layer, target_step, similarity, unet_triplets,
                                          *lat_prompt[6:], **({} if text is None else {"text": text}), **({"soft": True} if soft else {}),
                                          **({} if exemplar is None else {"exemplar": exemplar})),
        *(() if masks is None else (masks,)))
    return all_l[0], all_r[0], int(nbad)


@torch.no_grad()
def nights_eval(scorer, image_path: str, img_size: int, target_block, target_layer, target_step, seed=2333,
                similarity="cosine", rank: int = 0, world: int = 1, batch_triplets: int = 10) -> float:
    """The whole night_main.py loop (csv -> triplets -> 2AFC accuracy), triplets sharded over ranks."""
    rows = read_nights_csv(image_path)
    trip = [(r["ref"], r["left"], r["right"], r["prompt"]) for r in rows]
    all_l, all_r, _bad = score_path_triplets(scorer, trip, img_size, target_block, target_layer, target_step, seed, similarity,
                                             rank, world, batch_triplets)
    return nights_accuracy(all_l, all_r, [r["vote"] for r in rows], similarity)
