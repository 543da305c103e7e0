"""What the three scorer kinds share: the protocol the batched paths speak (pairs, triplets, score matrices, similarity maps, tap
sweeps) and the one-pair path calls over regions.  ``Scorer`` is the base of DiffSim, diffsim_xl and diffsim_DiT.  Each subclass states the per-call arithmetic of its
reference entry point (DiffSim.diffsim, diffsim_xl.diffsim_score, diffsim_DiT.diffsim_score) as attributes and a few one-line
methods; everything here is written against those, never against a class name.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import torch

from ._lib import DsimError
from .config import DiTConfig, ViTConfig


def get_generator(seed, device="cpu"):
    if seed is not None:
        if isinstance(seed, list):
            generator = [torch.Generator(device).manual_seed(int(s)) for s in seed]
        else:
            generator = torch.Generator(device).manual_seed(int(seed))
    else:
        generator = None
    return generator


class PromptTable(NamedTuple):
    """The prompt contexts of one engine batch that carries a prompt per image: the distinct contexts (n_ctx, 2, L, Dc) f32 on the
    device, in order of first appearance, and each image's row of that table."""
    table: torch.Tensor
    index: List[int]


def single_prompt(prompt) -> bool:
    """True for one prompt of the whole call (a string, a (2, L, Dc) context or a PromptTable already built), False for a sequence
    with one entry per pair / triplet / image."""
    return isinstance(prompt, (str, torch.Tensor, PromptTable))


def distinct_prompts(prompts) -> Tuple[list, List[int]]:
    """(the distinct entries of `prompts` in order of first appearance, each entry's position among them).  Strings are the same
    prompt when equal, tensors when they are the same object."""
    pos, firsts, index = {}, [], []
    for p in prompts:
        key = ("tensor", id(p)) if isinstance(p, torch.Tensor) else ("str", p)
        if key not in pos:
            pos[key] = len(firsts)
            firsts.append(p)
        index.append(pos[key])
    return firsts, index


def row_prompts(prompt, i0: int, i1: int, per_row: int):
    """The prompts of rows [i0, i1) of a batched call image by image, each row's `per_row` images consecutive as
    stack_rows lays them out; one prompt of the whole call stays as it is."""
    if single_prompt(prompt):
        return prompt
    return [p for p in prompt[i0:i1] for _ in range(per_row)]


def check_row_prompts(prompt, n_rows: int, what: str = "pairs"):
    """A per-row prompt sequence as a list (ValueError unless it has one entry per row); one prompt of the call unchanged."""
    if single_prompt(prompt):
        return prompt
    prompt = list(prompt)
    if len(prompt) != n_rows:
        raise ValueError(f"{len(prompt)} prompts for {n_rows} {what}: one prompt, or one per entry")
    return prompt


def stack_rows(cols: Sequence[torch.Tensor], noises: Sequence[torch.Tensor], i0: int, i1: int):
    """Engine batch of rows [i0, i1) of k latent columns (n, C, s, s): lat (k m, C, s, s) f32, each row's k images
    consecutive, and nz in the same layout from the columns' noises, each (1, C, s, s) shared by every row or (n, C, s, s)
    one per row."""
    n, shp, m = cols[0].shape[0], cols[0].shape[1:], i1 - i0
    lat = torch.stack([c[i0:i1] for c in cols], dim=1).reshape(len(cols) * m, *shp).float()
    nz = torch.stack([z[i0:i1] if z.shape[0] == n else z.expand(m, *shp) for z in noises], dim=1).reshape(len(cols) * m, *shp)
    return lat, nz


def all_taps(cfg) -> list:
    """Every tap the model's addressing names, in walk order: SD1.5 7, SDXL 70 (24 down, 10 mid, 36 up), DiT and ViT their depth."""
    if isinstance(cfg, (DiTConfig, ViTConfig)):
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


class Scorer:
    """A subclass provides ``engine(*tap address)``, ``features`` / ``features_taps`` / ``prepare_image_latents`` with its
    reference's signatures, and the facts and one-line methods below.  The defaults are those of the two kinds whose VAE runs in
    fp32 and hands fp16 latents on (diffsim_xl.py:61-63, diffsim_dit.py:54-59)."""

    # ---- the draw rule (inputs.path_latents): how one reference call draws and rounds an image's latents and noise
    image_half = False                      # whether the image is cast to fp16 in front of the VAE
    round16 = True                          # whether the sampled latents round through fp16
    noise_draw = torch.float16              # dtype the noise is drawn in

    @property
    def eps_dtype(self):
        """dtype the VAE sample is drawn in."""
        return getattr(self.vae, "sample_dtype", torch.float32)

    def prepare(self, tensor, generator):
        """prepare_image_latents of one image, returned as the f32 values the pipeline carries on."""
        return self.prepare_image_latents(tensor, generator).float()

    draws = True                            # whether a call draws at all (VAE sample, noise); False: the input tensors are the
                                            #   "latents", the noises are placeholders and tap_features ignores noise, prompt, step

    gpu_resize = False                      # files-in calls: decode on the host, PIL's resize on the device (engine.resize_u8,
                                            #   bit for bit); False: decode and resize on the host

    def load_input(self, path, img_size):
        """One image (a path or a PIL image) as the kind's (1, 3, S, S) f32 input tensor on the host: the reference's
        process_image (Lanczos resize to img_size, [-1, 1]) in front of the VAE."""
        from .image import load_image, process_image
        return process_image(load_image(path), img_size)

    def pair_tail(self, tap):
        """The pair tail of the kind at `tap`, a callable with engine.pair_score's signature; None: engine.pair_score itself, the
        plain DiffSim tail (the batched paths then call their own module's binding of it)."""
        return None

    def matrix_tail(self, tap):
        """The matrix tail of the kind at `tap` (retrieval.score_latent_matrix): an object with .features((q, k, v), heads) -> what
        a set of images contributes, computed once per set, .matrix(fa, fb) -> ((n_a, n_b) scores, int32 status) and
        .workspace_bytes(n_a, n_b, B, heads, N, D, dtype); None: engine.score_matrix on the sets' q, k, v (a kind with a pair tail
        of its own and no matrix tail has no score matrix)."""
        return None

    # ---- batching facts
    mixes_prompts = True                    # whether one engine batch may carry several prompts (group_key)
    per_row_prompts = False                 # whether a call takes a prompt per row (a context table in the engine)
    engine_images = 128                     # images per engine batch at the batch sweeps' optimum (profiles/r04h_batch_sweep.txt)
    one_tap_bound = True                    # whether the engine's max_images / workspace_bytes bound a one-tap batch (auto_rows)

    def group_key(self, prompt):
        """Rows of a path run with equal keys share engine batches: one group for the kinds that mix prompts, else one per
        prompt."""
        return prompt if not self.mixes_prompts else None

    def group_prompt(self, prompts: Sequence):
        """The prompt argument of one group's rows (group_key): the per-row list where the kind takes one and the rows differ,
        else the group's one prompt."""
        if self.per_row_prompts and len(distinct_prompts(prompts)[0]) > 1:
            return list(prompts)
        return prompts[0]

    def prompt_rows(self, prompt, n_rows: int, what: str = "triplets"):
        """A call's prompt argument checked against its rows: one prompt or one per row where the kind takes that; a kind that
        ignores the prompt returns it untouched."""
        return check_row_prompts(prompt, n_rows, what) if self.per_row_prompts else prompt

    def bind_prompt(self, prompt, n_rows: int, what: str = "triplets"):
        """prompt_rows, then whatever the kind encodes once per call: what tap_features / taps_features take as `prompt`."""
        return self.prompt_rows(prompt, n_rows, what)

    def chunk_prompt(self, prompt, i0: int, i1: int, per_row: int):
        """The prompt argument of the engine batch of rows [i0, i1) (each row's per_row images consecutive)."""
        return row_prompts(prompt, i0, i1, per_row) if self.per_row_prompts else prompt

    def n_ctx(self, prompt) -> int:
        """2 when the engine batches of a call with this (bound) prompt carry a context table, else 1."""
        return 2 if self.per_row_prompts and not single_prompt(prompt) else 1

    def auto_rows(self, eng, n_rows: int, per_row: int, taps=None, shapes=(), n_ctx: int = 1, streams: int = 1, images=None) -> int:
        """Rows (pairs: 2 images, triplets: 3) per engine batch when the caller names none: the batch sweeps' optimum
        (`engine_images`), within the job and the 2 GiB bound of every activation, halved until the arenas of the `streams` in use
        fit half of the free HBM.  taps / shapes (sweep_engine's): a sweep, whose bound covers every tap output and whose arena
        counts with the q/k/v of EVERY tap (all seven SD1.5 taps of 64 pairs hold ~7 GB).  n_ctx > 1: a context table, whose
        per-image buffers count too.  A kind without `one_tap_bound` gets the optimum within the job for its one-tap calls."""
        m = max(1, min((self.engine_images if images is None else images) // per_row, max(1, int(n_rows))))
        if not taps and not self.one_tap_bound:
            return m
        mixed = {"n_ctx": 2} if n_ctx > 1 else {}
        cap = eng.max_images_taps(taps, **mixed) if taps else eng.max_images(**mixed)
        m = max(1, min(m, cap // per_row))
        try:
            free, _total = torch.cuda.mem_get_info(self.device)
        except Exception:
            return m
        outs = sum(3 * 2 * t * h * d for t, h, d in shapes) * torch.empty((), dtype=self.dtype).element_size()
        while m > 1:
            k = per_row * m
            need = eng.taps_workspace_bytes(k, taps, **mixed) + k * outs if taps else eng.workspace_bytes(k, **mixed)
            if need * max(1, min(int(streams), -(-int(n_rows) // m))) <= 0.5 * free:
                break
            m = (m + 1) // 2
        return m

    def auto_map_pairs(self, eng, n: int) -> int:
        """Pairs per engine batch of the map paths when the caller names none: the images of the triplet batch."""
        return max(1, 3 * self.auto_rows(eng, n, 3) // 2)

    # ---- tap addressing: a tap is what engine(*tap) / features(..., *tap, step) take
    def tap_of(self, target_block, target_layer):
        """The reference's (--target_block, --target_layer) flag pair as the scorer's tap."""
        return target_block, target_layer

    def engine_at(self, tap):
        return self.engine(*tap)

    def canonical_taps(self, taps) -> list:
        """A sweep's taps in the scorer's form; "all": every tap the model's addressing names."""
        if isinstance(taps, str):
            if taps != "all":
                raise ValueError(f"taps={taps!r}: a list of taps or 'all'")
            return all_taps(self.cfg)
        return [self.canonical_tap(t) for t in taps]

    def sweep_engine(self, taps, side: int):
        """The scorer's engine (created at the first tap if the scorer has none yet; its own tap is not moved after that) and the
        (tokens, heads, head_dim) of every tap at latent side `side`."""
        if not taps:
            raise DsimError("no taps")
        if self._base is None:
            self.engine_at(taps[0])
        self._base.set_sample_size(int(side))
        return self._base, [self._base.tap_shape(b, l) for b, l in taps]

    # ---- one features signature; `prompt` is what bind_prompt (then chunk_prompt) returned
    def tap_features(self, lat, nz, prompt, tap, step):
        return self.features(lat, nz, prompt, *tap, step)

    def taps_features(self, lat, nz, prompt, taps, step):
        return self.features_taps(lat, nz, prompt, taps, step)

    def tap_features_text(self, lat, nz, prompt, tap, step):
        """tap_features plus the tapped block's cross-attention operands, (q, k, v, xq, xkv) (UNetEngine.qkv_text): the kinds with
        a text-conditioned U-Net provide ``features_text``."""
        if not hasattr(self, "features_text"):
            raise NotImplementedError(f"{type(self).__name__} has no text conditioning: no text attention maps")
        return self.features_text(lat, nz, prompt, *tap, step)

    def pair_chunks(self, latA, latB, noiseA, noiseB, prompt, tap, step, similarity, batch_pairs: int, tail, tail_of=None,
                    text_of=None):
        """Yields (i0, i1, tail(q, k, v, idx_a, idx_b, heads, similarity)) for the pairs (latA[i] in slot A, latB[i] in slot B) in
        engine batches of batch_pairs; tail: engine.pair_score or engine.pair_score_maps.  tail_of(i0, i1), when given, returns
        the tail of that chunk instead (regions.py binds each chunk's mask rows, which lie as its images do: A0, B0, A1, B1, ...).
        text_of(i0, i1, xq, xkv, heads), when given, does the same from the chunk's cross-attention operands (textattn.py: the
        regions come from the text attention maps), and the features come from tap_features_text."""
        n = latA.shape[0]
        eng = self.engine_at(tap)
        heads = eng.heads
        if self.one_tap_bound:
            batch_pairs = min(batch_pairs, eng.max_images() // 2)               # every activation must stay < 2 GiB
        batch_pairs = max(1, int(batch_pairs))
        for i0 in range(0, n, batch_pairs):
            i1 = min(n, i0 + batch_pairs)
            rows, chunk_prompt = stack_rows([latA, latB], [noiseA, noiseB], i0, i1), self.chunk_prompt(prompt, i0, i1, 2)
            if text_of is None:
                q, k, v = self.tap_features(*rows, chunk_prompt, tap, step)
                chunk_tail = tail if tail_of is None else tail_of(i0, i1)
            else:
                q, k, v, xq, xkv = self.tap_features_text(*rows, chunk_prompt, tap, step)
                chunk_tail = text_of(i0, i1, xq, xkv, heads)
            ia = torch.arange(0, 2 * (i1 - i0), 2, dtype=torch.int32, device=self.device)
            yield i0, i1, chunk_tail(q, k, v, ia, ia + 1, heads, similarity)

    # ---- the one-pair path calls: two image files in, the per-token and region forms of the kind's one-pair score (DiffSim.diffsim,
    #      diffsim_xl.diffsim_score, diffsim_DiT.diffsim_score) out.  Written against three facts of the kind.
    path_hip_vae = False                    # whether the files are encoded through the HIP VAE fast path (inputs.path_latents)
    path_batch_pairs = None                 # pairs per engine batch (None: Scorer.auto_map_pairs)

    def path_tap(self, prompt, target_block, target_layer):
        """(prompt, target_block, target_layer) as the batched module functions take the reference's flag pair from this kind"""
        return prompt, target_block, target_layer

    def _path_pair_latents(self, image_A, image_B, img_size, seed):
        """(latentsA, latentsB, noiseA, noiseB) as f32 tensors: what one reference call draws for the two image files."""
        from .inputs import path_latents
        (latA, latB), nA, nB = path_latents(self, [(image_A, image_B)], (0, 1), img_size, seed, 1, hip_vae=self.path_hip_vae)
        return latA, latB, nA, nB

    @torch.no_grad()
    def alignment(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed="2333"):
        """Which token of the other image each token of one pair attends to: an :class:`~diffsim_amd.align.Alignment` of one pair
        (direction 0 on image_A's grid, 1 on image_B's)."""
        from . import align
        return align.score_path_pair_alignment(self, [(image_A, image_B)], img_size, *self.path_tap(prompt, target_block, target_layer),
                                               target_step, seed, self.path_batch_pairs, hip_vae=self.path_hip_vae)

    @torch.no_grad()
    def region_score(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                     seed="2333", similarity="cosine"):
        """The one-pair score of the masked part of each image (regions.py): the score tail over the tokens of mask_A on image_A and
        of mask_B on image_B alone.  A mask is a path, a PIL image, a bool array on the tap's token grid, or None (the whole
        image); full masks give the unmasked score.  Returns a (1,) tensor."""
        from . import regions
        return regions.score_path_pair_regions(self, [(image_A, image_B)], [(mask_A, mask_B)], img_size,
                                               *self.path_tap(prompt, target_block, target_layer), target_step, seed, similarity,
                                               batch_pairs=self.path_batch_pairs, hip_vae=self.path_hip_vae)

    @torch.no_grad()
    def soft_region_score(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                          seed="2333", similarity="cosine"):
        """:meth:`region_score` with a weight per token instead of a bit (regions.py, ``engine.pair_score_weights``): a mask's area
        average on the token grid is the token's weight, so a partly covered token counts partly -- as a key through a logit bias in
        both attentions, as a query through a factor on its terms.  A mask is a path, a PIL image, a uint8 / bool / [0, 1] float
        array on the tap's token grid, or None (the whole image); masks of 0 and 255 alone give :meth:`region_score`'s score.
        Returns a (1,) tensor."""
        from . import regions
        return regions.score_path_pair_weights(self, [(image_A, image_B)], [(mask_A, mask_B)], img_size,
                                               *self.path_tap(prompt, target_block, target_layer), target_step, seed, similarity,
                                               batch_pairs=self.path_batch_pairs, hip_vae=self.path_hip_vae)

    def _path_region_maps(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed,
                          similarity, **soft):
        from . import maps
        return maps.score_path_pair_maps(self, [(image_A, image_B)], img_size, *self.path_tap(prompt, target_block, target_layer),
                                         target_step, seed, similarity, self.path_batch_pairs, masks=[(mask_A, mask_B)],
                                         hip_vae=self.path_hip_vae, **soft)

    def _path_region_alignment(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed,
                               **soft):
        from . import align
        return align.score_path_pair_alignment(self, [(image_A, image_B)], img_size, *self.path_tap(prompt, target_block, target_layer),
                                               target_step, seed, self.path_batch_pairs, masks=[(mask_A, mask_B)],
                                               hip_vae=self.path_hip_vae, **soft)

    @torch.no_grad()
    def region_similarity_maps(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                               seed="2333", similarity="cosine"):
        """:meth:`region_score` of one image pair with its per-token terms on both images' grids: a
        :class:`~diffsim_amd.maps.SimilarityMaps` of one pair whose attentions ran over the masked tokens alone (zeros at the off
        tokens; ``.mask`` holds the two token masks).  Masks as :meth:`region_score` takes them."""
        return self._path_region_maps(image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed,
                                      similarity)

    @torch.no_grad()
    def soft_region_similarity_maps(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                                    seed="2333", similarity="cosine"):
        """:meth:`soft_region_score` of one image pair with its per-token terms on both images' grids: a
        :class:`~diffsim_amd.maps.SimilarityMaps` of one pair (``.weights`` holds the two uint8 token weights, ``.mask`` is
        ``weights != 0``; zeros at the tokens of weight 0).  ``local`` is a token's own value, ``contrib`` carries its weight.
        Masks as :meth:`soft_region_score` takes them."""
        return self._path_region_maps(image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed,
                                      similarity, soft=True)

    @torch.no_grad()
    def region_alignment(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                         seed="2333"):
        """Which token of the other image's region each token of a region attends to: an :class:`~diffsim_amd.align.Alignment` of
        one pair whose softmaxes ran over the other image's masked tokens alone (off tokens: match -1; ``.mask`` holds the two
        token masks).  Masks as :meth:`region_score` takes them."""
        return self._path_region_alignment(image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                                           seed)

    @torch.no_grad()
    def soft_region_alignment(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                              seed="2333"):
        """:meth:`region_alignment` with soft masks: every softmax runs over the other image's tokens of weight > 0 with ln(weight)
        added to the logits (an :class:`~diffsim_amd.align.Alignment` of one pair; ``.weights`` holds the two uint8 token weights;
        tokens of weight 0: match -1).  Masks as :meth:`soft_region_score` takes them."""
        return self._path_region_alignment(image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step,
                                           seed, soft=True)

    @torch.no_grad()
    def text_region_score(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed="2333",
                          similarity="cosine", words=None, rel_threshold=1.0):
        """The one-pair score of the part of each image the prompt names (textattn.py; the reference's declared and unbuilt
        ``--use_text_attn``, argprocess.py:17): each image's region is the tokens whose text attention to `words` (None: every
        content token of the prompt) is at least rel_threshold x the image's mean.  Returns a (1,) tensor."""
        from . import textattn
        return textattn.score_path_pairs_text(self, [(image_A, image_B)], img_size, *self.path_tap(prompt, target_block, target_layer),
                                              target_step, seed, similarity, words, rel_threshold, hip_vae=self.path_hip_vae)

    @torch.no_grad()
    def text_attention_map(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed="2333"):
        """The text attention maps of the two images of one pair: (2, h, w, L) f32 on the tap's token grid."""
        from . import textattn
        latA, latB, nA, nB = self._path_pair_latents(image_A, image_B, img_size, seed)
        return textattn.text_attention_maps(self, torch.cat([latA, latB]), torch.cat([nA, nB]),
                                            *self.path_tap(prompt, target_block, target_layer), target_step)

    @torch.no_grad()
    def exemplar_region_score(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed="2333",
                              similarity="cosine", rel_threshold=1.0, soft=False):
        """:meth:`region_score` with a mask for image_A alone (transfer.py): image_B's region is the tokens whose attention mass into
        mask_A's tokens is at least rel_threshold x the image's mean; soft: token weights on both sides.  Returns a (1,) tensor."""
        from . import transfer
        return transfer.score_path_pairs_exemplar(self, [(image_A, image_B)], [mask_A], img_size,
                                                  *self.path_tap(prompt, target_block, target_layer), target_step, seed, similarity,
                                                  self.path_batch_pairs, rel_threshold, soft, hip_vae=self.path_hip_vae)

    @torch.no_grad()
    def transferred_region(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed="2333",
                           rel_threshold=1.0, soft=False):
        """(mass (h, w) f32, region (h, w) bool -- soft: uint8 weights) on image_B's token grid: what :meth:`exemplar_region_score`
        transfers from mask_A."""
        from . import transfer
        return transfer.path_transferred_region(self, image_A, image_B, mask_A, img_size,
                                                *self.path_tap(prompt, target_block, target_layer), target_step, seed, rel_threshold,
                                                soft, self.path_batch_pairs, hip_vae=self.path_hip_vae)
