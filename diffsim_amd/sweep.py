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

from .diffsim import single_prompt
from .engine import pair_score
from .inputs import _Adapter, path_latents, stack_rows
from .parallel import gather_scores, shard_triplets

UNET_BLOCKS = ("down_blocks", "mid_blocks", "up_blocks")


def all_taps(cfg) -> list:
    """Every tap the model's addressing names, in walk order: SD1.5 7, SDXL 70 (24 down, 10 mid, 36 up), DiT its depth."""
    from .config import DiTConfig
    if isinstance(cfg, DiTConfig):
        return list(range(cfg.depth))
    n, lpb = len(cfg.block_out_channels), cfg.layers_per_block
    down = [t == "CrossAttnDownBlock2D" for t in cfg.down_block_types]
    up = [t == "CrossAttnUpBlock2D" for t in cfg.up_block_types]
    if not cfg.sdxl_tap:        # down_blocks[:-1][l], mid, up_blocks[1:][l]; attentions[-1].transformer_blocks[-1]
        return ([("down_blocks", l) for l in range(n - 1) if down[l]] + [("mid_blocks", 0)] +
                [("up_blocks", l) for l in range(n - 1) if up[l + 1]])
    taps = []                   # down_blocks[1:][b], up_blocks[:-1][b]: every attention and transformer block
    for b in range(n - 1):
        if down[b + 1]:
            taps += [("down_blocks", [b, a, t]) for a in range(lpb) for t in range(cfg.depth(b + 1))]
    taps += [("mid_blocks", [0, t]) for t in range(cfg.depth(n - 1))]
    for b in range(n - 1):
        if up[b]:
            taps += [("up_blocks", [b, a, t]) for a in range(lpb + 1) for t in range(cfg.depth(n - 1 - b))]
    return taps


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


def _taps(ad: _Adapter, taps) -> list:
    if isinstance(taps, str):
        if taps != "all":
            raise ValueError(f"taps={taps!r}: a list of taps or 'all'")
        return all_taps(ad.s.cfg)
    if ad.kind == "dit":
        return [int(t) for t in taps]
    if ad.kind == "xl":
        return [(b, [int(v) for v in l]) for b, l in taps]
    return [(b, int(l)) for b, l in taps]


def _engine(ad: _Adapter, taps, side: int):
    """The scorer's engine (created at the first tap if the scorer has none yet; its own tap is not moved after that) and the
    (tokens, heads, head_dim) of every tap at latent side `side`."""
    if not taps:
        from . import _lib
        raise _lib.DsimError("no taps")
    if ad.kind == "dit":
        eng = ad.s._engine if ad.s._engine is not None else ad.s.engine(int(taps[0]))
        return eng, [(eng.tokens, eng.heads, eng.head_dim)] * len(taps)
    if ad.s._base is None:
        ad.s.engine(*taps[0])
    eng = ad.s._base
    eng.set_sample_size(int(side))
    return eng, [eng.tap_shape(b, l) for b, l in taps]


def _features_fn(ad: _Adapter, prompt, taps, step):
    """lat, nz, rows -> [(q, k, v) per tap] from one forward over the rows (i0, i1, images per row) of the call.  DiffSim takes
    one prompt or one per row, diffsim_xl a (context, pooled) tuple or a prompt string (encoded once), DiT ignores the prompt."""
    if ad.kind == "sd15":
        return lambda lat, nz, rows: ad.s.features_taps(lat, nz, ad.chunk_prompt(prompt, *rows), taps, step)
    if ad.kind == "xl":
        if isinstance(prompt, tuple):
            ctx, pooled = prompt
        else:
            if ad.s._encode_prompt is None:
                raise RuntimeError("no text encoder plugged in: pass encode_prompt=...")
            ctx, pooled = ad.s._encode_prompt(prompt)
        return lambda lat, nz, rows: ad.s.features_taps(lat, nz, ctx, pooled, taps, step)
    return lambda lat, nz, rows: ad.s.features_taps(lat, nz, taps, step)


def auto_rows(ad: _Adapter, eng, taps, shapes, n_rows: int, per_row: int, n_ctx: int = 1) -> int:
    """Rows (pairs: 2 images, triplets: 3) per engine batch of a sweep when the caller names none: the batch sweeps' optimum
    (SD1.5 and DiT 128 images, SDXL 16: _Adapter.auto_triplets), within the 2 GiB bound of every activation and tap output, and
    with the arena plus the q/k/v of EVERY tap inside half of the free HBM (all seven SD1.5 taps of 64 pairs hold ~7 GB)."""
    m = max(1, min((16 if ad.kind == "xl" else 128) // per_row, int(n_rows)))
    mixed = {"n_ctx": 2} if n_ctx > 1 else {}          # (a context table: its per-image buffers count too)
    m = max(1, min(m, eng.max_images_taps(taps, **mixed) // per_row))
    es = torch.empty((), dtype=ad.s.dtype).element_size()
    per_image = sum(3 * 2 * t * h * d * es for t, h, d in shapes)
    try:
        free, _total = torch.cuda.mem_get_info(ad.s.device)
    except Exception:
        return m
    while m > 1 and eng.taps_workspace_bytes(per_row * m, taps, **mixed) + per_row * m * per_image > 0.5 * free:
        m = (m + 1) // 2
    return m


@torch.no_grad()
def score_latent_pairs_taps(scorer, latA, latB, noiseA, noiseB, prompt, taps, target_step=600, similarity="cosine",
                            batch_pairs: Optional[int] = None) -> torch.Tensor:
    """(n_taps, n) f32 device tensor: row t is bit for bit what ``score_latent_pairs`` returns at taps[t] for the pairs
    (latA[i] in slot A, latB[i] in slot B), any scorer kind (DiffSim, diffsim_xl, diffsim_DiT).  One forward per chunk of
    batch_pairs pairs serves every tap (None: ``auto_rows``); results do not depend on the chunk.  noiseA / noiseB: (1, C, s, s)
    or (n, C, s, s).  prompt: as the scorer's score_latent_pairs takes it (DiffSim: one or one per pair; diffsim_xl: (context,
    pooled) or a prompt string; DiT: ignored).  taps: a list in the scorer's tap form, or "all"."""
    ad = _Adapter(scorer)
    taps = _taps(ad, taps)
    dev = scorer.device
    n = latA.shape[0]
    prompt = ad.rows(prompt, n, "pairs")
    latA, latB = latA.to(dev, torch.float32), latB.to(dev, torch.float32)
    noiseA, noiseB = noiseA.to(dev, torch.float32), noiseB.to(dev, torch.float32)
    eng, shapes = _engine(ad, taps, latA.shape[2])
    mixed = {"n_ctx": 2} if ad.kind == "sd15" and not single_prompt(prompt) else {}
    if batch_pairs is None:
        batch_pairs = auto_rows(ad, eng, taps, shapes, n, 2, **mixed)
    batch_pairs = max(1, min(int(batch_pairs), eng.max_images_taps(taps, **mixed) // 2))
    feats = _features_fn(ad, prompt, taps, target_step)
    out = torch.empty((len(taps), n), dtype=torch.float32, device=dev)
    for i0 in range(0, n, batch_pairs):
        i1 = min(n, i0 + batch_pairs)
        fs = feats(*stack_rows([latA, latB], [noiseA, noiseB], i0, i1), (i0, i1, 2))
        ia = torch.arange(0, 2 * (i1 - i0), 2, dtype=torch.int32, device=dev)
        for t, (q, k, v) in enumerate(fs):
            out[t, i0:i1] = pair_score(q, k, v, ia, ia + 1, shapes[t][1], similarity)
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


def _score_chunks_taps(ad: _Adapter, ref, left, right, nA, nB, prompt, taps, step, similarity, batch_triplets):
    """harness._score_chunks at every tap: (nt, n) (ref,left) and (ref,right) scores and the (nt,) NaN / inf counts."""
    n, nt, dev = ref.shape[0], len(taps), ad.s.device
    prompt = ad.rows(prompt, n)
    eng, shapes = _engine(ad, taps, ref.shape[2])
    s_l = torch.empty((nt, n), dtype=torch.float32, device=dev)
    s_r = torch.empty((nt, n), dtype=torch.float32, device=dev)
    bad = torch.zeros(nt, dtype=torch.int32, device=dev)
    mixed = {"n_ctx": 2} if ad.kind == "sd15" and not single_prompt(prompt) else {}
    if batch_triplets is None:
        batch_triplets = auto_rows(ad, eng, taps, shapes, n, 3, **mixed)
    batch_triplets = max(1, min(int(batch_triplets), eng.max_images_taps(taps, **mixed) // 3))
    feats = _features_fn(ad, prompt, taps, step)
    for i0 in range(0, n, batch_triplets):
        i1 = min(n, i0 + batch_triplets)
        m = i1 - i0
        fs = feats(*stack_rows([ref, left, right], [nA, nB, nB], i0, i1), (i0, i1, 3))
        base = torch.arange(0, 3 * m, 3, dtype=torch.int32, device=dev)
        ia, ib = torch.cat([base, base]), torch.cat([base + 1, base + 2])
        for t, (q, k, v) in enumerate(fs):
            s, st = pair_score(q, k, v, ia, ib, shapes[t][1], similarity, return_status=True)
            bad[t] += st.sum()
            s_l[t, i0:i1], s_r[t, i0:i1] = s[:m], s[m:]
    return s_l, s_r, bad


@torch.no_grad()
def score_path_triplets_taps(scorer, triplets: Sequence[Tuple[str, str, str, str]], img_size: int, taps, target_step,
                             seed=2333, similarity="cosine", rank: int = 0, world: int = 1, batch_triplets: int = 10,
                             unet_triplets: Optional[int] = None, return_status: bool = False):
    """``harness.score_path_triplets`` at every tap: (s_ab, s_ac), each (n_taps, len(triplets)) f32 on every rank, row t bit for
    bit the one-tap scores at taps[t].  The same rank shard and score gathers (one per tap), prompts encoded once each, the
    reference image's features shared by its two pairs, the images decoded and encoded once for all taps.  return_status: also
    the per-tap list of NaN / inf pair score counts."""
    n = len(triplets)
    ad = _Adapter(scorer)
    taps = _taps(ad, taps)
    nt, dev = len(taps), scorer.device
    mine = shard_triplets(n, rank, world)
    sl, sr, order = [], [], []
    nbad = torch.zeros(nt, dtype=torch.int32, device=dev)
    groups = {}
    for j in mine:
        groups.setdefault(ad.group_key(triplets[j][3]), []).append(j)
    for _key_, idxs in groups.items():
        prompt = ad.group_prompt([triplets[j][3] for j in idxs])
        (ref, left, right), nA, nB = path_latents(scorer, [triplets[j][:3] for j in idxs], (0, 1, 1), img_size, seed,
                                                  batch_triplets)
        a_, b_, bad = _score_chunks_taps(ad, ref, left, right, nA, nB, prompt, taps, target_step, similarity, unet_triplets)
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
    return (all_l, all_r, [int(b) for b in nbad.tolist()]) if return_status else (all_l, all_r)
