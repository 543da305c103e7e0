"""Float64 restatement of the ViT metrics (clip_cross, dino_cross) in plain torch: both forwards, both taps, both tails and the HF key
maps.  The reference for tests/test_vit_host.py (which pins it against transformers' CLIPVisionModel / Dinov2Model in double) and
tests/test_gpu_vit.py.  Written from the model definitions, not from diffsim_amd/vit.py or csrc/vit.hip.

State dicts here use the engine's neutral keys (include/diffsim_amd.h): cls_token, pos_embed (stored grid), x_embedder.proj.*,
pre_norm.*, blocks.N.{norm1, attn.qkv, attn.proj, ls1, norm2, mlp.fc1, mlp.fc2, ls2}.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


# ---- HF keys -> neutral keys ------------------------------------------------------------------------------------------------------
def clip_keys(depth: int, prefix: str = ""):
    """{neutral key: HF CLIPVisionModel key or the (q, k, v) triple stacked into it}; prefix "" or "vision_model."."""
    m = {"cls_token": "embeddings.class_embedding", "pos_embed": "embeddings.position_embedding.weight",
         "x_embedder.proj.weight": "embeddings.patch_embedding.weight", "pre_norm.weight": "pre_layrnorm.weight",
         "pre_norm.bias": "pre_layrnorm.bias"}
    for i in range(depth):
        b, h = f"blocks.{i}.", f"encoder.layers.{i}."
        for leaf in ("weight", "bias"):
            m[b + "norm1." + leaf] = h + "layer_norm1." + leaf
            m[b + "norm2." + leaf] = h + "layer_norm2." + leaf
            m[b + "attn.proj." + leaf] = h + "self_attn.out_proj." + leaf
            m[b + "mlp.fc1." + leaf] = h + "mlp.fc1." + leaf
            m[b + "mlp.fc2." + leaf] = h + "mlp.fc2." + leaf
            m[b + "attn.qkv." + leaf] = tuple(h + f"self_attn.{n}_proj." + leaf for n in "qkv")
    return {k: (prefix + v if isinstance(v, str) else tuple(prefix + x for x in v)) for k, v in m.items()}


def dinov2_keys(depth: int, prefix: str = ""):
    m = {"cls_token": "embeddings.cls_token", "pos_embed": "embeddings.position_embeddings",
         "x_embedder.proj.weight": "embeddings.patch_embeddings.projection.weight",
         "x_embedder.proj.bias": "embeddings.patch_embeddings.projection.bias"}
    for i in range(depth):
        b, h = f"blocks.{i}.", f"encoder.layer.{i}."
        m[b + "ls1"], m[b + "ls2"] = h + "layer_scale1.lambda1", h + "layer_scale2.lambda1"
        for leaf in ("weight", "bias"):
            m[b + "norm1." + leaf] = h + "norm1." + leaf
            m[b + "norm2." + leaf] = h + "norm2." + leaf
            m[b + "attn.proj." + leaf] = h + "attention.output.dense." + leaf
            m[b + "mlp.fc1." + leaf] = h + "mlp.fc1." + leaf
            m[b + "mlp.fc2." + leaf] = h + "mlp.fc2." + leaf
            m[b + "attn.qkv." + leaf] = tuple(h + f"attention.attention.{n}." + leaf for n in ("query", "key", "value"))
    return {k: (prefix + v if isinstance(v, str) else tuple(prefix + x for x in v)) for k, v in m.items()}


def to_neutral(hf_sd, kind: str, depth: int, prefix: str = ""):
    keys = clip_keys(depth, prefix) if kind == "clip" else dinov2_keys(depth, prefix)
    out = {}
    for k, h in keys.items():
        t = torch.cat([hf_sd[x] for x in h]) if isinstance(h, tuple) else hf_sd[h]
        if k == "cls_token":
            t = t.reshape(-1)
        if k == "pos_embed":
            t = t.reshape(t.shape[-2], t.shape[-1])
        out[k] = t
    return out


def to_hf(sd, kind: str, depth: int, prefix: str = ""):
    """The inverse: a neutral state dict under HF keys (HF shapes), for writing checkpoints and for loading HF modules."""
    keys = clip_keys(depth, prefix) if kind == "clip" else dinov2_keys(depth, prefix)
    out = {}
    for k, h in keys.items():
        t = sd[k]
        if isinstance(h, tuple):
            for x, part in zip(h, t.chunk(3)):
                out[x] = part.contiguous()
            continue
        if kind == "dinov2" and k == "cls_token":
            t = t.reshape(1, 1, -1)
        if kind == "dinov2" and k == "pos_embed":
            t = t.reshape(1, *t.shape)
        out[h] = t.contiguous()
    return out


# ---- the forward ------------------------------------------------------------------------------------------------------------------
def pos_at(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """The stored table (1 + g0^2, C) at a grid x grid patch grid, as HF interpolate_pos_encoding: untouched when the grids agree,
    else the patch rows bicubic (align_corners False) IN FLOAT32 (HF casts to f32 for the interpolation whatever the model dtype)."""
    g0 = int(round(math.sqrt(pos.shape[0] - 1)))
    if g0 == grid:
        return pos.double()
    patch = pos[1:].float().reshape(1, g0, g0, -1).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1].float(), patch.permute(0, 2, 3, 1).reshape(grid * grid, -1)]).double()


def _act(x, kind):
    return x * torch.sigmoid(1.702 * x) if kind == "clip" else 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _sdpa(q, k, v, heads):
    """softmax(q k^T / sqrt(D)) v per head; q (nq, N, C), k / v (nq, Nk, C) -> (nq, N, C)"""
    n, N, C = q.shape
    D = C // heads
    sp = lambda t: t.reshape(n, -1, heads, D).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(D), dim=-1)
    return (p @ sp(v)).transpose(1, 2).reshape(n, N, C)


def hidden_states(sd, cfg, pixels: torch.Tensor, upto: int):
    """[h_0 .. h_upto] (each (n, N, C) f64): the inputs of blocks 0 .. upto (HF's hidden_states[l])."""
    sd = {k: v.double() for k, v in sd.items() if k != "pos_embed"} | {"pos_embed": sd["pos_embed"]}
    x = pixels.double()
    n, p = x.shape[0], cfg.patch_size
    g = x.shape[-1] // p
    tok = F.conv2d(x, sd["x_embedder.proj.weight"], sd.get("x_embedder.proj.bias"), stride=p).flatten(2).transpose(1, 2)
    h = torch.cat([sd["cls_token"].expand(n, 1, -1), tok], 1) + pos_at(sd["pos_embed"], g)
    if cfg.kind == "clip":
        h = _ln(h, sd, "pre_norm", cfg.ln_eps)
    out = [h]
    for i in range(upto):
        b = f"blocks.{i}."
        y = _ln(h, sd, b + "norm1", cfg.ln_eps)
        q, k, v = F.linear(y, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).chunk(3, -1)
        a = F.linear(_sdpa(q, k, v, cfg.num_heads), sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        h = h + (a * sd[b + "ls1"] if cfg.kind == "dinov2" else a)
        y = _ln(h, sd, b + "norm2", cfg.ln_eps)
        m = F.linear(_act(F.linear(y, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]), cfg.kind), sd[b + "mlp.fc2.weight"],
                     sd[b + "mlp.fc2.bias"])
        h = h + (m * sd[b + "ls2"] if cfg.kind == "dinov2" else m)
        out.append(h)
    return out


def tap_qkv(sd, cfg, pixels: torch.Tensor, layer: int):
    """q, k, v (n, N, C) f64 as the reference's hooks store them at `layer`: CLIP projects the encoder layer's raw input (hooks.py:
    3-17), DINOv2 norm1's output (the input of attention.attention, hooks.py:19-32)."""
    h = hidden_states(sd, cfg, pixels, layer)[layer]
    b = f"blocks.{layer}."
    if cfg.kind == "dinov2":
        h = F.layer_norm(h, (h.shape[-1],), sd[b + "norm1.weight"].double(), sd[b + "norm1.bias"].double(), cfg.ln_eps)
    return F.linear(h, sd[b + "attn.qkv.weight"].double(), sd[b + "attn.qkv.bias"].double()).chunk(3, -1)


# ---- the tails --------------------------------------------------------------------------------------------------------------------
def _direction(x, y, similarity):
    x, y = x.reshape(-1), y.reshape(-1)
    if similarity == "mse":
        return ((x - y) ** 2).mean()
    return (x * y).sum() / (x.norm().clamp_min(1e-8) * y.norm().clamp_min(1e-8))


def pair_tail(qa, ka, va, qb, kb, vb, heads, similarity="cosine", w_out=None, bias=None):
    """One pair's score in f64; q, k, v (B, N, C).  w_out / bias: the projected tail (CLIP), P = SDPA(...) w_out^T + bias."""
    ts = [t.double() for t in (qa, ka, va, qb, kb, vb)]
    qa, ka, va, qb, kb, vb = ts
    o = lambda q, k, v: _sdpa(q, k, v, heads) if w_out is None else F.linear(_sdpa(q, k, v, heads), w_out.double(), bias.double())
    return 0.5 * (_direction(o(qa, kb, vb), o(qa, ka, va), similarity) + _direction(o(qb, ka, va), o(qb, kb, vb), similarity))


def pair_scores(q, k, v, ia, ib, heads, similarity="cosine", w_out=None, bias=None):
    """pair_tail over index pairs into features [n_feat][B][N][C] -> f64 (n_pairs,)"""
    return torch.stack([pair_tail(q[a], k[a], v[a], q[b], k[b], v[b], heads, similarity, w_out, bias) for a, b in zip(ia, ib)])


def score(sd, cfg, pix_a, pix_b, layer, similarity="cosine"):
    """clip_cross / dino_cross of preprocessed pixel pairs (n, 3, S, S) each -> f64 (n,)"""
    fa, fb = tap_qkv(sd, cfg, pix_a, layer), tap_qkv(sd, cfg, pix_b, layer)
    w = b = None
    if cfg.kind == "clip":
        w, b = sd[f"blocks.{layer}.attn.proj.weight"], sd[f"blocks.{layer}.attn.proj.bias"]
    return torch.stack([pair_tail(fa[0][i:i + 1], fa[1][i:i + 1], fa[2][i:i + 1], fb[0][i:i + 1], fb[1][i:i + 1], fb[2][i:i + 1],
                                  cfg.num_heads, similarity, w, b) for i in range(pix_a.shape[0])])
