"""The reference's ViT metrics on the HIP engine: ``clip_cross`` and ``dino_cross``.

Mirrors ``metrics/clip_i.py:113-159`` (``CLIPScore.attention_calc`` / ``clip_cross_score``), ``metrics/dino.py:120-161``
(``Dinov2Score.attention_calc`` / ``dino_cross_score``) and the hooks of ``metrics/hooks.py:3-32``: DiffSim's method on a ViT -- tap
q / k / v of one self-attention layer, attend A -> B and A -> A, cosine of the two outputs, mean of both directions.  One image is one
batch element (the tails' B = 1); there is no VAE, no noise, no seed and no slot, so score(A, A) = 1.

Reference quirks, kept:
  * CLIP's hook sits on the encoder LAYER and projects the layer's input: q, k, v = q_proj / k_proj / v_proj of h_L, NOT layer-normed.
  * CLIP's tail applies the layer's out_proj (bias included) to every attention output before the cosine (engine.pair_score_proj).
  * DINOv2's hook sits on attention.attention: q, k, v of norm1(h_L); its tail is the plain pair tail.
  * --image_size is not consulted: the image processor's resize / crop decide the side.
"""
from __future__ import annotations

import functools
import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from PIL import Image

from . import sweep
from ._lib import DsimError
from .config import CLIP_B32, DINOV2_S14, ViTConfig
from .engine import ViTEngine, pair_score, pair_score_proj
from .image import load_image
from .inputs import path_latents
from .scorer import Scorer

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Preprocess:
    """What HF CLIPImageProcessor / BitImageProcessor do to one PIL image: RGB, shortest edge to `resize` (PIL bicubic, the long
    edge int(resize * long / short)), centre crop `crop`, / 255, (x - mean) / std -> (1, 3, crop, crop) f32."""

    def __init__(self, resize: int, crop: int, mean: Sequence[float], std: Sequence[float], resample: int = Image.Resampling.BICUBIC):
        self.resize, self.crop, self.resample = int(resize), int(crop), resample
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)

    @classmethod
    def from_dir(cls, model_path: str, default: "Preprocess") -> "Preprocess":
        """`default` overridden by <model_path>/preprocessor_config.json (size, crop_size, image_mean, image_std, resample)."""
        p = os.path.join(model_path, "preprocessor_config.json")
        if not os.path.exists(p):
            return default
        with open(p) as f:
            j = json.load(f)

        def side(v, keys, fallback):
            if v is None:
                return fallback
            if isinstance(v, dict):
                for k in keys:
                    if k in v:
                        return int(v[k])
                raise ValueError(f"{p}: cannot read a side from {v!r}")
            return int(v)
        return cls(side(j.get("size"), ("shortest_edge", "height"), default.resize),
                   side(j.get("crop_size"), ("height", "shortest_edge"), default.crop),
                   j.get("image_mean", default.mean), j.get("image_std", default.std), j.get("resample", default.resample))

    def __call__(self, image) -> torch.Tensor:
        im = image.convert("RGB")
        w, h = im.size
        short, long = (w, h) if w <= h else (h, w)
        ns, nl = self.resize, int(self.resize * long / short)
        im = im.resize((ns, nl) if w <= h else (nl, ns), resample=self.resample)
        w, h = im.size
        c = self.crop
        if w < c or h < c:
            raise ValueError(f"image {w}x{h} after the resize is smaller than the {c} px crop")
        left, top = (w - c) // 2, (h - c) // 2
        arr = np.asarray(im.crop((left, top, left + c, top + c)), dtype=np.float32) * np.float32(1.0 / 255.0)
        arr = (arr - self.mean) / self.std
        return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)[None]))

    def batch(self, arrays, device) -> torch.Tensor:
        """``torch.cat([self(Image.fromarray(a)) for a in arrays])`` for uint8 (h, w, 3) RGB arrays, bit for bit, on `device`: the
        shortest-edge rule per image, engine.resize_u8 with the centre crop as its window (images of one output size share a
        call; the cropped-away part is never computed), then the same f32 arithmetic and HWC -> CHW there.  A `resample` other
        than bicubic or Lanczos is resized on the host."""
        from . import resize as rz
        from .engine import resize_u8
        name = rz.filter_name(self.resample)
        if name is None:
            return torch.cat([self(Image.fromarray(a)) for a in arrays]).to(device)
        c, groups = self.crop, {}
        for i, a in enumerate(arrays):
            h, w = a.shape[:2]
            ow, oh = rz.shortest_edge(w, h, self.resize)
            if ow < c or oh < c:
                raise ValueError(f"image {ow}x{oh} after the resize is smaller than the {c} px crop")
            groups.setdefault((ow, oh), []).append(i)
        px = torch.empty((len(arrays), c, c, 3), dtype=torch.uint8, device=device)
        for (ow, oh), idx in groups.items():
            got = resize_u8([arrays[i] for i in idx], ow, oh, name, ((ow - c) // 2, (oh - c) // 2, c, c), device=device)
            if len(groups) == 1:
                px = got
            else:
                px[torch.tensor(idx, device=device)] = got
        x = px.to(torch.float32) * float(np.float32(1.0 / 255.0))
        x = (x - torch.from_numpy(self.mean).to(device)) / torch.from_numpy(self.std).to(device)
        return x.permute(0, 3, 1, 2).contiguous()


CLIP_PREPROCESS = Preprocess(224, 224, CLIP_MEAN, CLIP_STD)
DINOV2_PREPROCESS = Preprocess(256, 224, IMAGENET_MEAN, IMAGENET_STD)


# ---- HF state-dict keys -> the engine's neutral keys (config.vit_param_shapes) --------------------------------------------
def _prefix(sd, leaf: str) -> str:
    hits = [k for k in sd if k.endswith(leaf)]
    if len(hits) != 1:
        raise ValueError(f"expected one key ending in {leaf!r}, found {hits}")
    return hits[0][: -len(leaf)]


def neutral_state_dict(sd: Dict[str, torch.Tensor], cfg: ViTConfig) -> Dict[str, torch.Tensor]:
    """An HF CLIPVisionModel / CLIPModel (keys with or without the ``vision_model.`` prefix) or Dinov2Model state dict under the
    engine's neutral keys: q / k / v stacked into attn.qkv, tables flattened to (N, C) and (C,).  Keys the path never reads (the text
    tower, post_layernorm, the mask token, the final layernorm) are dropped."""
    out: Dict[str, torch.Tensor] = {}
    if cfg.kind == "clip":
        p = _prefix(sd, "embeddings.class_embedding")
        out["cls_token"] = sd[p + "embeddings.class_embedding"].reshape(-1)
        out["pos_embed"] = sd[p + "embeddings.position_embedding.weight"]
        out["x_embedder.proj.weight"] = sd[p + "embeddings.patch_embedding.weight"]
        out["pre_norm.weight"], out["pre_norm.bias"] = sd[p + "pre_layrnorm.weight"], sd[p + "pre_layrnorm.bias"]
        names = {"norm1": "layer_norm1", "norm2": "layer_norm2", "attn.proj": "self_attn.out_proj", "mlp.fc1": "mlp.fc1",
                 "mlp.fc2": "mlp.fc2"}
        layer, qkv = p + "encoder.layers.{}.", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")
    elif cfg.kind == "dinov2":
        p = _prefix(sd, "embeddings.cls_token")
        out["cls_token"] = sd[p + "embeddings.cls_token"].reshape(-1)
        pos = sd[p + "embeddings.position_embeddings"]
        out["pos_embed"] = pos.reshape(pos.shape[-2], pos.shape[-1])
        out["x_embedder.proj.weight"] = sd[p + "embeddings.patch_embeddings.projection.weight"]
        out["x_embedder.proj.bias"] = sd[p + "embeddings.patch_embeddings.projection.bias"]
        names = {"norm1": "norm1", "norm2": "norm2", "attn.proj": "attention.output.dense", "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
        layer, qkv = p + "encoder.layer.{}.", ("attention.attention.query", "attention.attention.key", "attention.attention.value")
    else:
        raise ValueError(f"unknown ViT kind {cfg.kind!r}")
    for i in range(cfg.depth):
        src, dst = layer.format(i), f"blocks.{i}."
        if src + "mlp.weights_in.weight" in sd:
            raise ValueError("SwiGLU DINOv2 checkpoints (use_swiglu_ffn) are not supported")
        for n, h in names.items():
            for leaf in ("weight", "bias"):
                out[f"{dst}{n}.{leaf}"] = sd[f"{src}{h}.{leaf}"]
        for leaf in ("weight", "bias"):
            out[f"{dst}attn.qkv.{leaf}"] = torch.cat([sd[f"{src}{n}.{leaf}"] for n in qkv])
        if cfg.layer_scale:
            out[dst + "ls1"], out[dst + "ls2"] = sd[src + "layer_scale1.lambda1"], sd[src + "layer_scale2.lambda1"]
    return out


def vit_config_from_json(j: dict, kind: str) -> ViTConfig:
    """HF config.json (CLIPVisionConfig, a CLIPConfig's vision_config, or Dinov2Config) -> ViTConfig; the crop side is set later from
    the preprocessor."""
    if kind == "clip":
        j = j.get("vision_config", j)
        d = CLIP_B32
        if j.get("hidden_act", "quick_gelu") != "quick_gelu":
            raise ValueError(f"CLIP hidden_act {j['hidden_act']!r}: only quick_gelu towers are supported")
        side, patch = int(j.get("image_size", d.image_size)), int(j.get("patch_size", d.patch_size))
        return ViTConfig("clip", side, patch, int(j.get("hidden_size", d.hidden_size)), int(j.get("num_hidden_layers", d.depth)),
                         int(j.get("num_attention_heads", d.num_heads)), int(j.get("intermediate_size", d.mlp_dim)), side // patch,
                         float(j.get("layer_norm_eps", d.ln_eps)))
    d = DINOV2_S14
    if j.get("use_swiglu_ffn", False):
        raise ValueError("SwiGLU DINOv2 checkpoints (use_swiglu_ffn) are not supported")
    if j.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"DINOv2 hidden_act {j['hidden_act']!r}: only gelu is supported")
    hidden, patch = int(j.get("hidden_size", d.hidden_size)), int(j.get("patch_size", d.patch_size))
    return ViTConfig("dinov2", d.image_size, patch, hidden, int(j.get("num_hidden_layers", d.depth)),
                     int(j.get("num_attention_heads", d.num_heads)), int(j.get("mlp_ratio", 4)) * hidden,
                     int(j.get("image_size", 518)) // patch, float(j.get("layer_norm_eps", d.ln_eps)))


class _ViTScore(Scorer):
    """What CLIPScore and Dinov2Score share.  The "latents" of the batched paths are the preprocessed pixels (n, 3, S, S); the
    noises are placeholders; a tap is the layer index.  One engine per image side (the position table is per side), the tap moved."""
    draws = False
    canonical_tap = staticmethod(int)
    vae = None

    def __init__(self, cfg: ViTConfig, state_dict: Dict[str, torch.Tensor], device="cuda", torch_dtype=torch.bfloat16,
                 preprocess: Optional[Preprocess] = None):
        self.cfg, self.state_dict, self.dtype = cfg, state_dict, torch_dtype
        self.device = torch.device("cuda:0" if device == "cuda" else device)
        self.preprocess = preprocess or self.default_preprocess
        self.side = self.preprocess.crop
        self._engines: Dict[int, ViTEngine] = {}

    def exemplar_region_score(self, *args, **kwargs):
        """The ViT metrics have no region tails, so no exemplar-guided regions either."""
        raise NotImplementedError(f"{type(self).__name__} has no exemplar-guided regions: they need --metric diffsim, diffsim_xl or dit")

    transferred_region = exemplar_region_score

    def engine(self, layer: int, side: Optional[int] = None) -> ViTEngine:
        side = self.side if side is None else int(side)
        eng = self._engines.get(side)
        if eng is None:
            eng = self._engines[side] = ViTEngine(self.cfg, self.state_dict, self.dtype, int(layer), str(self.device), side)
        eng.set_tap(int(layer))
        self.side = side
        return eng

    # ---- the Scorer protocol: this kind's facts (scorer.py)
    def tap_of(self, target_block, target_layer):
        """The reference's rule: a one-element list means that layer index (the block flag is ignored)."""
        if isinstance(target_layer, (list, tuple)):
            if len(target_layer) != 1:
                raise ValueError(f"--target_layer {target_layer!r}: the ViT metrics take one layer index")
            target_layer = target_layer[0]
        return int(target_layer)

    def engine_at(self, tap):
        return self.engine(tap)

    def sweep_engine(self, taps, side: int):
        if not taps:
            raise DsimError("no taps")
        have = self._engines.get(int(side))
        eng = have if have is not None else self.engine(taps[0], side)
        self.side = int(side)
        return eng, [(eng.tokens, eng.heads, eng.head_dim)] * len(taps)

    def load_input(self, path, img_size):
        """img_size is not consulted, as in the reference: the image processor's resize and crop decide the side."""
        return self.preprocess(load_image(path))

    def load_inputs(self, arrays):
        """load_input of many decoded images (uint8 (h, w, 3) arrays) at once, on the device: Preprocess.batch."""
        return self.preprocess.batch(arrays, self.device)

    def tap_features(self, lat, nz, prompt, tap, step):
        return self.features(lat, tap)

    def taps_features(self, lat, nz, prompt, taps, step):
        return self.features_taps(lat, taps)

    @torch.no_grad()
    def features(self, pixels, target_layer: int):
        """q, k, v (n, 1, N, C) of the hooked layer for normalised pixels (n, 3, S, S)."""
        return self.engine(int(target_layer), pixels.shape[-1]).qkv(pixels.to(self.device, torch.float32).contiguous())

    @torch.no_grad()
    def features_taps(self, pixels, layers):
        if not layers:
            raise ValueError("no taps")
        eng, _ = self.sweep_engine([int(l) for l in layers], pixels.shape[-1])
        return eng.qkv_taps(pixels.to(self.device, torch.float32).contiguous(), [int(l) for l in layers])

    @torch.no_grad()
    def score_pixel_pairs(self, pixA, pixB, target_layer: int, similarity="cosine", batch_pairs: Optional[int] = None,
                          tail=None) -> torch.Tensor:
        """(n,) scores of the pairs (pixA[i], pixB[i]) of preprocessed pixels, in engine batches of batch_pairs (None: auto_rows).
        tail: None (the kind's own pair tail), or a callable with engine.pair_score's signature."""
        tap, n = int(target_layer), pixA.shape[0]
        self.side = int(pixA.shape[-1])
        if batch_pairs is None:
            batch_pairs = self.auto_rows(self.engine_at(tap), n, 2)
        none = torch.zeros((1,) + tuple(pixA.shape[1:]))
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        for i0, i1, s in self.pair_chunks(pixA, pixB, none, none, None, tap, 0, similarity, batch_pairs,
                                            tail or self.pair_tail(tap) or pair_score):
            out[i0:i1] = s
        return out

    def _cross_score(self, images1, images2, target_layer, tail_of=None):
        images1 = images1 if isinstance(images1, list) else [images1]
        images2 = images2 if isinstance(images2, list) else [images2]
        if len(images1) != len(images2):
            raise ValueError(f"Number of images1 ({len(images1)}) and images2 ({len(images2)}) should be same.")
        (pa, pb), _, _ = path_latents(self, list(zip(images1, images2)), (0, 1), None, None, len(images1))
        tap = self.tap_of(None, target_layer)
        return self.score_pixel_pairs(pa, pb, tap, tail=None if tail_of is None else tail_of(tap))

    @torch.no_grad()
    def score_pairs_taps(self, pairs, layers, similarity="cosine") -> torch.Tensor:
        """(n_taps, len(pairs)) scores of (A, B) path pairs, the images preprocessed once and one forward per batch serving every
        layer (sweep.score_path_pairs_taps); row t is bit for bit the one-tap scores at layers[t]."""
        return sweep.score_path_pairs_taps(self, pairs, None, None, layers, 0, similarity, None)


class CLIPScore(_ViTScore):
    """``clip_cross`` (metrics/clip_i.py:129-159): HF CLIPVisionModel, the hook on encoder.layers[L], the projected tail."""
    default_preprocess = CLIP_PREPROCESS

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._proj: Dict[int, tuple] = {}

    def pair_tail(self, tap):
        """pair_score_proj bound to layer `tap`'s out_proj (weight in the compute dtype, f32 bias)."""
        if tap not in self._proj:
            w = self.state_dict[f"blocks.{tap}.attn.proj.weight"].to(self.device, self.dtype).contiguous()
            b = self.state_dict[f"blocks.{tap}.attn.proj.bias"].to(self.device, torch.float32).contiguous()
            self._proj[tap] = (w, b)
        w, b = self._proj[tap]
        return functools.partial(pair_score_proj, w_out=w, bias=b)

    @torch.no_grad()
    def clip_cross_score(self, images1, images2, target_layer):
        """Same contract as the reference's ``CLIPScore.clip_cross_score``: PIL images or paths (one or a list each), a (1,) tensor
        per pair."""
        return self._cross_score(images1, images2, target_layer)


class Dinov2Score(_ViTScore):
    """``dino_cross`` (metrics/dino.py:133-161): HF Dinov2Model, the hook on encoder.layer[L].attention.attention, the plain tail."""
    default_preprocess = DINOV2_PREPROCESS

    @torch.no_grad()
    def dino_cross_score(self, images1, images2, target_layer):
        """Same contract as the reference's ``Dinov2Score.dino_cross_score``."""
        return self._cross_score(images1, images2, target_layer)

    @torch.no_grad()
    def dino_feature_score(self, images1, images2, target_layer):
        """``dinofeats`` (metrics/dino.py:163-183): the cosine of the hooked attention's context layers, class token included
        (feats.py).  PIL images or paths, one or a list each, as dino_cross_score takes them; a score per pair (the reference
        flattens a whole list into ONE cosine: the same number for the single pair its drivers pass)."""
        from .feats import FeatureView
        return self._cross_score(images1, images2, target_layer, FeatureView(self).pair_tail)
