"""The reference's feature-cosine ablations on the HIP engine: ``diffeats`` and ``dinofeats``.

The paper sets its attention score (diffsim, dino_cross) against the plain cosine of the SAME layer's features; the reference ships
that baseline as ``--metric diffeats`` (``metrics/diffeats.py:136-205``, hook ``metrics/hooks.py:37-38``) and ``--metric dinofeats``
(``metrics/dino.py:163-183``, hook ``metrics/hooks.py:34-35``).  Both features are the tapped self-attention's own output, which the
engine builds from the q, k, v it already hands out (``engine.attn_features``); a pair is one dot product
(``engine.feature_pair_score``) and a retrieval matrix one Gram product (``engine.feature_matrix``).

Reference quirks, kept:
  * diffeats (SD1.5 only): the hook sits on the tapped ``attn1``, so F = to_out.0(merge_heads(SDPA(q, k, v))) + bias over both CFG
    halves -- no residual, no rescale, dropout the identity; each image's F is min-max normalised over ALL its B N C values, then the
    cosine (eps 1e-8).  The ``similarity`` argument is ignored: always a cosine.  A one-element ``target_layer`` list becomes its
    element -- it is NOT forced to 0 as ``DiffSim.diffsim`` forces it (diffeats.py:143-144).  Blocks and draw order are diffsim's.
  * dinofeats: the hook sits on Dinov2SelfAttention and stores ``output[0]``, the context layer: F = merge_heads(SDPA(q, k, v)) of
    norm1(h_L), class token included, no projection, no normalisation.  target_layer and preprocessing are dino_cross's.

``FeatureView(scorer)`` wraps a loaded DiffSim or Dinov2Score and speaks the Scorer protocol, so pairs, triplets, tap sweeps and
retrieval matrices run through the paths the attention scores use.
"""
from __future__ import annotations

from typing import Dict

import torch

from .engine import attn_features, feature_matrix, feature_matrix_workspace_bytes, feature_pair_score
from .inputs import path_latents

METRIC_OF = {"DiffSim": "diffeats", "Dinov2Score": "dinofeats"}


def unet_tap_attention(cfg, tap) -> str:
    """The state-dict prefix of the attn1 an SD1.5 tap (block, layer) hooks: down_blocks[:-1][l] / mid_block / up_blocks[1:][l],
    attentions[-1].transformer_blocks[-1] (diffeats.py:156-171)."""
    block, layer = tap[0], int(tap[1])
    n = len(cfg.block_out_channels)
    if block == "down_blocks":
        name, level, attn = f"down_blocks.{layer}", layer, cfg.layers_per_block - 1
    elif block == "mid_blocks":
        name, level, attn = "mid_block", n - 1, 0
    else:
        name, level, attn = f"up_blocks.{layer + 1}", n - 2 - layer, cfg.layers_per_block
    return f"{name}.attentions.{attn}.transformer_blocks.{cfg.depth(level) - 1}.attn1."


class FeatureView:
    """A loaded DiffSim (diffeats) or Dinov2Score (dinofeats) seen as the feature-cosine metric of the same model: everything is
    the wrapped scorer's -- engines, draws, prompts, batching -- except the tap rule, the pair tail and the matrix tail."""

    def __init__(self, scorer):
        kind = type(scorer).__name__
        if kind not in METRIC_OF:
            metric = {"CLIPScore": "clipfeats"}.get(kind, "diffeats")
            raise NotImplementedError(f"{metric}: no feature metric for {kind} (diffeats runs on SD1.5's DiffSim, dinofeats on "
                                      "Dinov2Score)")
        self.scorer = scorer
        self.metric = METRIC_OF[kind]
        self._spec: Dict[object, dict] = {}

    def __getattr__(self, name):
        if name == "scorer":                    # (not set yet: a view that failed to build, or one being copied)
            raise AttributeError(name)
        return getattr(self.scorer, name)

    exemplar_regions = False                # (stated here: __getattr__ would answer with the wrapped scorer's)

    def exemplar_region_score(self, *args, **kwargs):
        """A feature cosine has no region tail, so no exemplar-guided regions either."""
        raise NotImplementedError(f"{self.metric} has no exemplar-guided regions: they need --metric diffsim, diffsim_xl or dit")

    transferred_region = exemplar_region_score

    # ---- the Scorer protocol: what this view changes (scorer.py)
    def tap_of(self, target_block, target_layer):
        """diffeats: a one-element target_layer list is its element, taken literally (diffeats.py:143-144); dinofeats: dino_cross's
        rule."""
        if self.metric != "diffeats":
            return self.scorer.tap_of(target_block, target_layer)
        if isinstance(target_layer, (list, tuple)):
            if len(target_layer) != 1:
                raise ValueError(f"--target_layer {target_layer!r}: diffeats takes one layer index")
            target_layer = target_layer[0]
        return target_block, int(target_layer)

    def spec(self, tap) -> dict:
        """engine.attn_features' keyword arguments at `tap`: DiffSim the tapped attn1's to_out.0 (weight in the compute dtype, f32
        bias, cached per tap) and the min-max normalisation; Dinov2Score neither."""
        key = tuple(tap) if isinstance(tap, (list, tuple)) else tap
        if key not in self._spec:
            if self.metric == "diffeats":
                s, p = self.scorer, unet_tap_attention(self.scorer.cfg, tap)
                self._spec[key] = {"w_out": s.state_dict[p + "to_out.0.weight"].to(s.device, s.dtype).contiguous(),
                                   "bias": s.state_dict[p + "to_out.0.bias"].to(s.device, torch.float32).contiguous(), "minmax": True}
            else:
                self._spec[key] = {"minmax": False}
        return self._spec[key]

    def pair_tail(self, tap):
        """A callable with engine.pair_score's signature: the features of the call's images, each once, then their pairs' cosines.
        `similarity` is ignored, as in the reference."""
        spec = self.spec(tap)

        def tail(q, k, v, idx_a, idx_b, heads, similarity="cosine", return_status=False):
            return feature_pair_score(*attn_features(q, k, v, heads, **spec), idx_a, idx_b, return_status)
        return tail

    def matrix_tail(self, tap):
        """The matrix tail at `tap` (retrieval.score_latent_matrix): .features((q, k, v), heads) -> a set's (feats, stats), computed
        once per set; .matrix(fa, fb) -> engine.feature_matrix with return_status; .workspace_bytes(n_a, n_b, B, heads, N, D, dtype)."""
        return _MatrixTail(self.spec(tap))


class _MatrixTail:
    def __init__(self, spec):
        self.spec = spec

    def features(self, qkv, heads: int):
        return attn_features(*qkv, heads, **self.spec)

    def matrix(self, fa, fb):
        return feature_matrix(fa, fb, return_status=True)

    @staticmethod
    def workspace_bytes(n_a, n_b, B, heads, N, D, dtype) -> int:
        return feature_matrix_workspace_bytes(n_a, n_b, B * N * heads * D, dtype)


@torch.no_grad()
def diffeats(image_A, image_B, img_size, scorer, prompt, target_block, target_layer, target_step, seed=2333, device=None,
             similarity="cosine"):
    """Same contract as the reference's ``diffeats`` (metrics/diffeats.py:142-205) with a loaded DiffSim (or its FeatureView) where
    the reference takes the pipeline: image paths or PIL images in, a (1,) tensor out.  `device` and `similarity` are ignored."""
    view = scorer if isinstance(scorer, FeatureView) else FeatureView(scorer)
    if view.metric != "diffeats":
        raise NotImplementedError(f"diffeats runs on SD1.5's DiffSim, not on {type(view.scorer).__name__}")
    tap = view.tap_of(target_block, target_layer)
    (latA, latB), nA, nB = path_latents(view, [(image_A, image_B)], (0, 1), img_size, seed, 1)
    ds = view.scorer
    out = torch.empty(1, dtype=torch.float32, device=ds.device)
    for i0, i1, s in ds.pair_chunks(latA.to(ds.device), latB.to(ds.device), nA, nB, ds.bind_prompt(prompt, 1, "pairs"), tap, target_step,
                                    "cosine", 1, view.pair_tail(tap)):
        out[i0:i1] = s
    return out
