"""Text-guided regions: the prompt's cross-attention picks the tokens.

The reference declares ``--use_text_attn``, "use the cross-attention results of text to guide conditional similarity"
(argprocess.py:17), and builds nothing behind it.  Every run already carries what names the object: the prompt, and a U-Net whose
cross-attention says which image tokens listen to which prompt tokens.  ``UNetEngine.qkv_text`` runs the tapped block on to its own
cross-attention (two steps behind the tap, on the score's token grid), ``engine.text_attention`` turns its operands into the text
attention map T (n, N, L) of the conditional CFG half, the saliency T @ w of the prompt tokens that matter and the region of the
tokens at or above ``rel_threshold`` x the image's mean saliency; the text-guided score of a pair is the region score
(regions.py, ``engine.pair_score_regions``) over those regions.  A region with no token on is the whole image.  A soft guide
(``TextGuide(soft=True)``) keeps the saliency below the threshold as a token weight instead of cutting it (``soft_token_bytes``), and
the score is the soft region score (``engine.pair_score_weights``).
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

from .engine import pair_score_regions, pair_score_weights, text_attention      # noqa: F401  (RegionKind.tail)
from .inputs import path_latents
from .regions import grid_shape, kind_of
from .scorer import single_prompt, stack_rows


def _content_span(ids: Sequence[int], eos: int) -> Tuple[int, int]:
    """[first, end) of the content tokens: strictly between BOS (position 0) and the first EOS; a prompt truncated before its EOS
    runs to the end."""
    end = next((i for i in range(1, len(ids)) if ids[i] == eos), len(ids))
    return 1, end


def prompt_token_weights(tokenize: Callable[[str], torch.Tensor], prompt, words: Optional[Sequence[str]] = None) -> torch.Tensor:
    """The (L,) f32 weights of a prompt's tokens for the saliency.  tokenize(str) -> (1, L) token ids, BOS first and EOS behind the
    last content token (a scorer's ``tokenize``: the tokenizer its encode_prompt uses).  words None: every content token -- the
    positions strictly between BOS and the first EOS -- gets 1.  Otherwise each word's own token run (the content tokens of
    tokenize(word); a word may be several tokens, or several words) is located inside the prompt's content tokens and every
    occurrence gets 1; a word that does not occur raises ValueError.  A prompt that is a context tensor has no tokens to look at:
    pass an (L,) weight tensor to the callers instead."""
    if not isinstance(prompt, str):
        raise ValueError("a prompt given as a context tensor has no tokens: pass the (L,) token weights themselves")
    if tokenize is None:
        raise ValueError("no tokenizer on the scorer (scorer.tokenize): pass the (L,) token weights themselves")
    ids = [int(v) for v in tokenize(prompt).reshape(-1).tolist()]
    eos = int(tokenize("").reshape(-1)[1])
    first, end = _content_span(ids, eos)
    w = torch.zeros(len(ids), dtype=torch.float32)
    if words is None or len(words) == 0:
        w[first:end] = 1.0
        return w
    for word in words:
        wid = [int(v) for v in tokenize(word).reshape(-1).tolist()]
        a, b = _content_span(wid, eos)
        run = wid[a:b]
        hits = [i for i in range(first, end - len(run) + 1) if ids[i:i + len(run)] == run] if run else []
        if not hits:
            raise ValueError(f"the word {word!r} does not occur in the prompt {prompt!r}")
        for i in hits:
            w[i:i + len(run)] = 1.0
    return w


def soft_token_bytes(saliency: torch.Tensor, mask: torch.Tensor, rel_threshold: float) -> torch.Tensor:
    """The saliency (n, N) f32 as uint8 token weights, with torch ops on its device: per image
    b = clamp(floor(255 s / (rel_threshold mean(s)) + 0.5), 0, 255) in float64 -- a token at the threshold or above, which the hard
    rule switches on (mask, the kernel's own decision), carries 255, the others their share.  Threshold 0, or an image whose saliency
    is non-finite or all zero: all 255, the whole image."""
    s = saliency.double()
    den = float(rel_threshold) * s.mean(1, keepdim=True)
    ok = torch.isfinite(s).all(1, keepdim=True) & (den > 0)
    full = torch.full_like(s, 255.0)
    b = torch.where(ok, torch.floor(255.0 * s / den + 0.5).clamp(0.0, 255.0), full)
    return torch.where(mask != 0, full, b).to(torch.uint8)


class TextGuide:
    """What a text-guided run carries: the words (None: every content token), the threshold, or explicit token weights -- (L,) for
    every image, or one row per pair / triplet -- and the running size of the regions it has made (``on_fraction``).  soft: the
    regions are uint8 token weights (``soft_token_bytes``) for the soft region tail, and on_fraction is the mean weight."""

    def __init__(self, words: Optional[Sequence[str]] = None, rel_threshold: float = 1.0, weights: Optional[torch.Tensor] = None,
                 soft: bool = False):
        self.soft = bool(soft)
        self.words = list(words) if words else None
        self.rel_threshold = float(rel_threshold)
        if not (self.rel_threshold >= 0.0) or self.rel_threshold == float("inf"):
            raise ValueError(f"rel_threshold must be finite and >= 0: {rel_threshold}")
        self.weights = weights
        self._on = None             # device scalars: tokens on, tokens seen
        self._seen = 0

    def bind(self, scorer, prompt, n_rows: int) -> torch.Tensor:
        """The weights of a call's rows on the device: (L,) for one prompt, (n_rows, L) for a prompt per row (each distinct prompt
        tokenized once).  prompt: what the caller was given, before the scorer binds it."""
        dev = scorer.device
        if self.weights is not None:
            w = torch.as_tensor(self.weights, dtype=torch.float32)
            if w.ndim not in (1, 2) or (w.ndim == 2 and w.shape[0] != n_rows):
                raise ValueError(f"token weights of shape {tuple(w.shape)} for {n_rows} rows: (L,) or ({n_rows}, L)")
            return w.to(dev).contiguous()
        tok = getattr(scorer, "tokenize", None)
        if single_prompt(prompt) or isinstance(prompt, tuple):       # (a tuple: SDXL's (context, pooled), which has no tokens)
            return prompt_token_weights(tok, prompt, self.words).to(dev)
        prompt = list(prompt)
        if len(prompt) != n_rows:
            raise ValueError(f"{len(prompt)} prompts for {n_rows} rows: one prompt, or one per entry")
        seen = {}
        rows = []
        for p in prompt:
            key = p if isinstance(p, str) else id(p)
            if key not in seen:
                seen[key] = prompt_token_weights(tok, p, self.words)
            rows.append(seen[key])
        return torch.stack(rows).to(dev).contiguous()

    def regions(self, xq, xkv, heads: int, w: torch.Tensor, i0: int, i1: int, per_row: int):
        """(mask bool (images, N), counts int32 (images,)) of the engine batch of rows [i0, i1), each row's per_row images
        consecutive: a row's weights are its images' weights.  A soft guide returns the uint8 token weights in the mask's place
        (the counts stay the hard rule's)."""
        wc = w if w.ndim == 1 else w[i0:i1].repeat_interleave(per_row, 0).contiguous()
        if self.soft:
            out = text_attention(xq, xkv, heads, wc, self.rel_threshold, want=("saliency", "mask", "counts"))
            b = soft_token_bytes(out["saliency"], out["mask"], self.rel_threshold)
            on = b.sum(dtype=torch.float64) / 255.0
            self._on = on if self._on is None else self._on + on
            self._seen += b.numel()
            return b, out["counts"]
        out = text_attention(xq, xkv, heads, wc, self.rel_threshold, want=("mask", "counts"))
        on = out["counts"].sum()
        self._on = on if self._on is None else self._on + on
        self._seen += out["mask"].numel()
        return out["mask"], out["counts"]

    @property
    def on_fraction(self) -> float:
        """Mean share of tokens on over every region made so far (one device read)."""
        return float(self._on) / self._seen if self._seen else float("nan")


def _tap_and_guide(scorer, prompt, n, target_block, target_layer, words, rel_threshold, weights, soft=False):
    if not hasattr(scorer, "features_text"):
        raise NotImplementedError(f"{type(scorer).__name__} has no text conditioning: no text attention maps")
    guide = TextGuide(words, rel_threshold, weights, soft)
    return scorer.tap_of(target_block, target_layer), guide, guide.bind(scorer, prompt, n)


@torch.no_grad()
def text_attention_maps(scorer, lat, noise, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                        batch: Optional[int] = None) -> torch.Tensor:
    """The text attention map of every image: (n, h, w, L) f32 on the device, [i, y, x, l] the share of image i's token (y, x)
    that listens to prompt token l on the conditional CFG half (heads averaged; rows sum to 1).  lat (n, C, s, s); noise
    (1, C, s, s) or (n, C, s, s); prompt: one, or one per image."""
    if not hasattr(scorer, "features_text"):
        raise NotImplementedError(f"{type(scorer).__name__} has no text conditioning: no text attention maps")
    dev = scorer.device
    n = lat.shape[0]
    if n == 0:
        raise ValueError("no images")
    tap = scorer.tap_of(target_block, target_layer)
    eng = scorer.engine_at(tap)
    heads = eng.heads
    lat, noise = lat.to(dev, torch.float32), noise.to(dev, torch.float32)
    bound = scorer.bind_prompt(prompt, n, "images")
    if batch is None:
        batch = 2 * scorer.auto_map_pairs(eng, n)
    if scorer.one_tap_bound:
        batch = min(batch, eng.max_images())
    out = []
    for i0 in range(0, n, max(1, int(batch))):
        i1 = min(n, i0 + max(1, int(batch)))
        _q, _k, _v, xq, xkv = scorer.tap_features_text(*stack_rows([lat], [noise], i0, i1), scorer.chunk_prompt(bound, i0, i1, 1), tap,
                                                       target_step)
        out.append(text_attention(xq, xkv, heads, want=("attn",))["attn"])
    attn = torch.cat(out)
    return attn.reshape(n, *grid_shape(attn.shape[1]), attn.shape[2])


@torch.no_grad()
def score_latent_pairs_text(scorer, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0, target_step=600,
                            similarity="cosine", words: Optional[Sequence[str]] = None, rel_threshold: float = 1.0,
                            weights: Optional[torch.Tensor] = None, batch_pairs: Optional[int] = None, return_regions: bool = False,
                            soft: bool = False):
    """Text-guided scores of pair i = (latA[i], latB[i]): each image's region from its own text attention map, then the region
    score over the two regions -- one forward (to the tapped block's cross-attention), one text-attention call and one region tail
    per chunk of batch_pairs.  prompt: one, or one per pair (then the weights are per pair too); words: the prompt words whose
    tokens count (None: every content token); weights: the (L,) or (n, L) token weights themselves (required when the prompt is a
    context tensor).  soft: soft regions -- the saliency becomes token weights (``soft_token_bytes``) and the tail is the soft region
    tail.  Returns the (n,) f32 scores on the device; return_regions: also the masks (n, 2, N) bool (soft: the uint8 weights) and
    counts (n, 2)."""
    dev = scorer.device
    n = latA.shape[0]
    if n == 0:
        raise ValueError("no pairs to score")
    tap, guide, w = _tap_and_guide(scorer, prompt, n, target_block, target_layer, words, rel_threshold, weights, soft)
    region_tail = kind_of(soft).tail("score", globals())
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    bound = scorer.bind_prompt(prompt, n, "pairs")
    if batch_pairs is None:
        batch_pairs = scorer.auto_map_pairs(scorer.engine_at(tap), n)
    masks, counts = [], []

    def text_of(i0, i1, xq, xkv, heads):
        mask, cnt = guide.regions(xq, xkv, heads, w, i0, i1, 2)
        masks.append(mask), counts.append(cnt)
        return lambda q, k, v, ia, ib, heads_, sim: region_tail(q, k, v, mask, ia, ib, heads_, sim)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    for i0, i1, s in scorer.pair_chunks(latA, latB, noiseA, noiseB, bound, tap, target_step, similarity, batch_pairs, None,
                                        text_of=text_of):
        score[i0:i1] = s
    if not return_regions:
        return score
    return score, torch.cat(masks).reshape(n, 2, -1), torch.cat(counts).reshape(n, 2)


@torch.no_grad()
def score_path_pairs_text(scorer, pairs: Sequence[Tuple[str, str]], img_size, prompt, target_block="up_blocks", target_layer=0,
                          target_step=600, seed=2333, similarity="cosine", words: Optional[Sequence[str]] = None,
                          rel_threshold: float = 1.0, weights: Optional[torch.Tensor] = None, batch_pairs: Optional[int] = None,
                          return_regions: bool = False, hip_vae: bool = True, soft: bool = False):
    """Text-guided scores of (A, B) path pairs with ``score_pairs``' draw order (inputs.path_latents)."""
    if not pairs:
        raise ValueError("no pairs to score")
    (latA, latB), nA, nB = path_latents(scorer, list(pairs), (0, 1), img_size, seed, 16, hip_vae=hip_vae)
    return score_latent_pairs_text(scorer, latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity, words,
                                   rel_threshold, weights, batch_pairs, return_regions, **({"soft": True} if soft else {}))
