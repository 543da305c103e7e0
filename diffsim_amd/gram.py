"""The reference's classical style baseline on the HIP engine: ``gram`` (``metrics/vgg_gram.py``).

torchvision's ``vgg19().features`` run up to module '28' (conv5_1 BEFORE its ReLU), the Gram matrix G = X X^T over the spatial axis
(512 x 512, not normalised), and a cosine.  The VGG forward and the Gram rows run in ``csrc/vgg.hip`` (``engine.VGGEngine``,
``engine.gram_rows``); a pair is one dot product of two f32 descriptors (``engine.feature_pair_score``) and a retrieval matrix one
Gram product of them (``engine.feature_matrix``).  No VAE, no noise, no seed, no prompt.

Reference quirks, kept:
  * ``style_grams_A[-1]`` (vgg_gram.py:81) indexes a TENSOR, not a list of per-layer matrices: it is the LAST ROW of the Gram matrix,
    so the reference's score is the cosine of the two 512-vectors G[511, :].  That is the default here; ``full=True``
    (``--gram_full``) is the cosine of the whole matrices, evidently what was meant.
  * Preprocessing is torchvision's ``Resize(img_size)`` on the PIL image (short side to img_size, the long side
    ``int(img_size * long / short)``, PIL's reducing BILINEAR; an image whose short side already is img_size passes unchanged),
    ``ToTensor`` and the ImageNet ``Normalize``.  Nothing is cropped: every image keeps its own H x W, so a batch is grouped by
    (H, W) and each group is one executor call.
Images are decoded by the project's DecodePool (EXIF orientation applied, as every metric here reads files).  Bilinear is not one of
the device resize's filters: with ``gpu_resize`` the images are resized by PIL on the host and counted as fallbacks.
fp16 activations can overflow with real VGG-19 weights (the executor does not rescale): bf16 is this metric's default.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from ._lib import DsimError
from .engine import RESIZE_COUNTS, VGGEngine, feature_matrix, feature_pair_score, gram_rows

VGG19_PLAN = (64, 64, "P", 128, 128, "P", 256, 256, 256, 256, "P", 512, 512, 512, 512, "P", 512)      # ... to conv5_1 (module '28')
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DECODE_CHUNK = 64               # images per decode request
TRIPLET_CHUNK = 48              # triplets whose descriptors are held at once
MATRIX_KCHUNK = 1024            # elements per f32 partial sum of a retrieval matrix cell (engine.feature_matrix k_chunk): Gram entries are
                                # all of one sign, and the default 16384-term chains round a 65536-element cell to 2e-6, these to 2e-7
MATRIX_PART_BYTES = 1 << 28     # partial sums one feature_matrix call may hold; the gallery is cut to fit (a cell depends on its two images alone)
ACT_BYTES = 3 << 29             # activation bytes one executor call may hold (its two ping-pong buffers at the first level)


def parse_plan(plan) -> Tuple:
    """A plan from config.json or a caller: conv output channels (positive multiples of 8) and "P" / "M" / 0 for a 2x2 max-pool; a
    conv first and last, no two pools in a row."""
    out = []
    for e in plan:
        if e in ("P", "M", 0) and not isinstance(e, bool):
            out.append("P")
        elif isinstance(e, int) and not isinstance(e, bool) and e > 0 and e % 8 == 0:
            out.append(int(e))
        else:
            raise ValueError(f"VGG plan entry {e!r}: conv output channels (a positive multiple of 8) or 'P' for a 2x2 max-pool")
    if not out or out[0] == "P" or out[-1] == "P":
        raise ValueError(f"VGG plan {list(plan)!r}: the first and the last entry are convs (the tap is the last conv's output)")
    if any(a == "P" and b == "P" for a, b in zip(out, out[1:])):
        raise ValueError(f"VGG plan {list(plan)!r}: a pool follows a conv")
    return tuple(out)


def conv_indices(plan) -> List[int]:
    """torchvision's ``features`` index of every conv of the plan: a conv and its ReLU take two slots, a pool one (VGG-19: 0, 2, 5, 7,
    10, 12, 14, 16, 19, 21, 23, 25, 28)."""
    out, i = [], 0
    for e in plan:
        if e == "P":
            i += 1
        else:
            out.append(i)
            i += 2
    return out


def neutral_state_dict(sd: Dict[str, torch.Tensor], plan) -> Dict[str, torch.Tensor]:
    """torchvision's ``features.N.{weight,bias}`` (with or without a prefix such as ``vgg.``) -> the engine's ``convs.I.{weight,bias}``,
    shapes checked against the plan; the classifier and the layers behind the tap are dropped."""
    plan = parse_plan(plan)
    hits = [k for k in sd if k.endswith("features.0.weight")]
    if len(hits) != 1:
        raise ValueError(f"expected one key ending in 'features.0.weight', found {hits}")
    prefix = hits[0][: -len("0.weight")]
    out, cin = {}, None
    for i, (idx, cout) in enumerate(zip(conv_indices(plan), [e for e in plan if e != "P"])):
        for leaf in ("weight", "bias"):
            key = f"{prefix}{idx}.{leaf}"
            if key not in sd:
                raise ValueError(f"the checkpoint has no {key} (conv {i} of the plan)")
            out[f"convs.{i}.{leaf}"] = sd[key]
        w = out[f"convs.{i}.weight"]
        cin = w.shape[1] if cin is None else cin
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(out[f"convs.{i}.bias"].shape) != (cout,):
            raise ValueError(f"{prefix}{idx}.weight is {tuple(w.shape)}, the plan's conv {i} is ({cout}, {cin}, 3, 3)")
        cin = cout
    return out


def resized_size(w: int, h: int, size: int) -> Tuple[int, int]:
    """torchvision ``Resize(int)``'s output (w, h): the short side to `size`, the long side int(size * long / short), truncated."""
    return (int(size * w / h), size) if h <= w else (size, int(size * h / w))


def resize_image(im: Image.Image, size: int) -> Image.Image:
    """``Resize(size)`` on a PIL image: unchanged when its short side already is `size`, else PIL's reducing bilinear."""
    w, h = im.size
    if min(w, h) == size:
        return im
    return im.resize(resized_size(w, h, size), Image.BILINEAR)


class VGGGram:
    """``vgg_gram`` (metrics/vgg_gram.py) on the HIP engine.  cfg: the plan (VGG19_PLAN; a test may pass a small stack); state_dict:
    torchvision's keys."""
    draws = False
    vae = None
    gpu_resize = False

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device="cuda", dtype=torch.bfloat16):
        self.plan = parse_plan(VGG19_PLAN if cfg is None else cfg)
        self.dtype = dtype
        self.device = torch.device("cuda:0" if device == "cuda" else device)
        self.engine = VGGEngine(self.plan, neutral_state_dict(state_dict, self.plan), dtype, str(self.device))
        self.channels = self.engine.channels
        self._pool = None
        self._mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        self._std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)

    # ---- images -> normalised pixels ----------------------------------------------------------------------------------------------
    def _decoded(self, images: Sequence):
        """uint8 (h, w, 3) RGB arrays of paths or PIL images, DECODE_CHUNK at a time, two requests ahead"""
        from .image import DecodePool
        from .inputs import raw_chunks
        if self._pool is None:
            self._pool = DecodePool()
        for arrays in raw_chunks(self._pool, [(p,) for p in images], DECODE_CHUNK):
            yield from arrays

    def load_pixels(self, images: Sequence, img_size: int = 512) -> List[np.ndarray]:
        """The resized uint8 (H, W, 3) array of every image (vgg_gram.load_image up to ToTensor)."""
        out = []
        for a in self._decoded(images):
            im = resize_image(Image.fromarray(a), int(img_size))
            if self.gpu_resize and im.size != (a.shape[1], a.shape[0]):
                RESIZE_COUNTS["fallback"] += 1
            out.append(np.asarray(im))
        return out

    def normalise(self, arrays: Sequence[np.ndarray]) -> torch.Tensor:
        """ToTensor + Normalize of equally sized uint8 (H, W, 3) arrays, on the device: f32 (n, 3, H, W)"""
        px = torch.from_numpy(np.stack(arrays)).to(self.device)
        x = px.permute(0, 3, 1, 2).to(torch.float32).div(255)
        return ((x - self._mean) / self._std).contiguous()

    # ---- descriptors --------------------------------------------------------------------------------------------------------------
    def _rows(self, full: bool) -> Tuple[int, int]:
        return (0, self.channels) if full else (self.channels - 1, 1)

    @torch.no_grad()
    def descriptors_of_pixels(self, pixels: torch.Tensor, full: bool = False):
        """(descriptors f32 (n, L), stats f32 (n, 4)) of normalised pixels (n, 3, H, W) of one size: the Gram matrix's last row
        (L = C) or, full, all of it (L = C^2), in executor calls of as many images as fit."""
        n, _, H, W = pixels.shape
        first = next(e for e in self.plan if e != "P")
        cap = max(1, ACT_BYTES // (2 * H * W * first * (4 if self.dtype == torch.float32 else 2)))
        step = self.engine.max_images(H, W, min(cap, n))
        if step < 1:
            raise DsimError(f"an image of {H}x{W} does not fit the VGG executor (smaller than the pools allow, or an activation of 2 GiB)")
        row0, n_rows = self._rows(full)
        descs, stats = [], []
        for i0 in range(0, n, step):
            feat = self.engine.features(pixels[i0:i0 + step].to(self.device, torch.float32).contiguous())
            d, s = gram_rows(feat, row0, n_rows)
            descs.append(d.view(d.shape[0], -1))
            stats.append(s)
        return (descs[0], stats[0]) if len(descs) == 1 else (torch.cat(descs), torch.cat(stats))

    @torch.no_grad()
    def descriptors(self, images: Sequence, img_size: int = 512, full: bool = False, return_stats: bool = False):
        """f32 (n, L) descriptors of paths or PIL images, L = C or (full) C^2: decoded through the DecodePool, resized by PIL on the
        host, grouped by (H, W), each group encoded in one call (split only where it would not fit)."""
        images = list(images)
        L = self.channels ** 2 if full else self.channels
        desc = torch.empty((len(images), L), dtype=torch.float32, device=self.device)
        stats = torch.empty((len(images), 4), dtype=torch.float32, device=self.device)
        arrays = self.load_pixels(images, img_size)
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape[:2], []).append(i)
        for idx in groups.values():
            d, s = self.descriptors_of_pixels(self.normalise([arrays[i] for i in idx]), full)
            at = torch.tensor(idx, device=self.device)
            desc[at], stats[at] = d, s
        return (desc, stats) if return_stats else desc

    # ---- scores -------------------------------------------------------------------------------------------------------------------
    def _pairs(self, desc, stats, ia, ib, return_status):
        ia = torch.tensor(ia, dtype=torch.int32, device=self.device)
        ib = torch.tensor(ib, dtype=torch.int32, device=self.device)
        return feature_pair_score(desc, stats, ia, ib, return_status)

    @torch.no_grad()
    def gram_similarity(self, image_A, image_B, img_size: int = 512, full: bool = False) -> torch.Tensor:
        """Same contract as the reference's ``vgg_gram.gram_similarity``: two paths (or PIL images) in, a (1,) tensor out."""
        desc, stats = self.descriptors([image_A, image_B], img_size, full, return_stats=True)
        return self._pairs(desc, stats, [0], [1], False)

    @torch.no_grad()
    def score_path_pairs(self, pairs: Sequence[Tuple], img_size: int = 512, full: bool = False, return_status: bool = False):
        """(n,) scores of (A, B) pairs of paths or PIL images; return_status: also int32 (n,), 1 where a score is NaN / infinite."""
        pairs = list(pairs)
        if not pairs:
            out = torch.empty(0, dtype=torch.float32, device=self.device)
            return (out, torch.empty(0, dtype=torch.int32, device=self.device)) if return_status else out
        desc, stats = self.descriptors([p for pair in pairs for p in pair[:2]], img_size, full, return_stats=True)
        n = len(pairs)
        return self._pairs(desc, stats, list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), return_status)

    @torch.no_grad()
    def score_path_triplets(self, triplets: Sequence[Tuple], img_size: int = 512, full: bool = False):
        """(s_ab, s_ac, n_nonfinite) of (A, B, C, ...) triplets, as harness.score_path_triplets returns them: the reference image's
        descriptor is computed once per triplet and serves both of its pairs."""
        triplets = list(triplets)
        s_ab = torch.empty(len(triplets), dtype=torch.float32, device=self.device)
        s_ac = torch.empty_like(s_ab)
        bad = 0
        for i0 in range(0, len(triplets), TRIPLET_CHUNK):
            rows = triplets[i0:i0 + TRIPLET_CHUNK]
            m = len(rows)
            desc, stats = self.descriptors([p for row in rows for p in row[:3]], img_size, full, return_stats=True)
            ref = [3 * i for i in range(m)]
            s, st = self._pairs(desc, stats, ref + ref, [r + 1 for r in ref] + [r + 2 for r in ref], True)
            s_ab[i0:i0 + m], s_ac[i0:i0 + m] = s[:m], s[m:]
            bad += int(st.sum())
        return s_ab, s_ac, bad

    @torch.no_grad()
    def score_path_matrix(self, paths_a: Sequence, paths_b: Sequence, img_size: int = 512, full: bool = False,
                          return_status: bool = False):
        """(len(paths_a), len(paths_b)) f32 device tensor of every query against every gallery image: each image's descriptor once,
        then engine.feature_matrix with MATRIX_KCHUNK-element partial sums.  return_status: also the number of NaN / infinite cells."""
        if not paths_a or not paths_b:
            empty = torch.empty((len(paths_a), len(paths_b)), dtype=torch.float32, device=self.device)
            return (empty, 0) if return_status else empty
        fa = self.descriptors(paths_a, img_size, full, return_stats=True)
        fb = self.descriptors(paths_b, img_size, full, return_stats=True)
        splits = -(-fa[0].shape[1] // MATRIX_KCHUNK)
        step = max(1, MATRIX_PART_BYTES // (4 * splits * len(paths_a)))
        parts = [feature_matrix(fa, (fb[0][j:j + step].contiguous(), fb[1][j:j + step].contiguous()), return_status=True,
                                k_chunk=MATRIX_KCHUNK) for j in range(0, len(paths_b), step)]
        m = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts], 1)
        return (m, sum(int(p[1].sum()) for p in parts)) if return_status else m
