"""DiffSim scorer with the reference's entry points, backed by the MI355X engine.

Mirrors ``/root/reference/diffsim/diffsim.py``:
  * ``get_generator``            :16-25
  * ``DiffSim.__init__``         :80-90   (pipeline load -> here: config + state dict + encoders)
  * ``prepare_image_latents``    :92-96
  * ``DiffSim.diffsim``          :98-197  same argument names, returns a (1,) tensor
and folds in what ``DiffSimPipeline.step`` does around the U-Net call
(``/root/reference/diffsim/diffsim_pipeline.py:125-221``): prompt context, index -> timestep,
noise draw, add_noise, CFG duplication.  Deliberate differences (SURVEY.md Appendix C "fix"
rows, none of which changes a score): the U-Net stops at the tap, no hook is leaked per call,
the prompt context and image-slot features are cached, both images run in one batch.

The VAE encoder and CLIP text encoder are "next" rows of the scope table: they are
pluggable (``vae`` with diffusers' ``encode(x).latent_dist.sample(generator)`` surface and an
``encode_prompt(prompt) -> (2, L, Dc)`` callable).  Without them only the latents-in entry
points work; the path-based ones raise.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

from concurrent.futures import ThreadPoolExecutor

import torch

from . import scheduler as sched
from . import align, maps, retrieval, sweep
from .config import SD15, UNetConfig
from .engine import UNetEngine, _LatentDist, image_preprocess, pair_score, resize_u8
from .image import DecodePool, host_threads, load_image, process_image
from .inputs import path_latents
from .scorer import (PromptTable, Scorer, check_row_prompts, distinct_prompts, get_generator, row_prompts,  # noqa: F401
                     single_prompt, stack_rows)


def _norm_layer(target_layer) -> int:
    # diffsim/diffsim.py:99-100: a single-valued --target_layer is coerced to 0
    if isinstance(target_layer, int):
        return target_layer
    if len(target_layer) == 1:
        return 0
    # the reference indexes a ModuleList with the list itself -> TypeError; keep the error
    raise TypeError("list indices must be integers or slices, not list")


class DiffSim(Scorer):
    per_row_prompts = True          # a context table: nothing before the first cross-attention depends on the prompt

    def __init__(self, torch_dtype=torch.bfloat16, device="cuda", ip_adapter=False, *,
                 unet_config: UNetConfig = SD15, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 vae=None, encode_prompt: Optional[Callable[[str], torch.Tensor]] = None,
                 vae_dtype=torch.float16, use_graphs: bool = False, noise_dtype=torch.float32, dedup_cfg: bool = True,
                 fusion: Optional[int] = None, decode_procs: Optional[int] = None):
        if ip_adapter:
            raise NotImplementedError("IP-Adapter mode is out of scope (SURVEY.md section 2 row 3)")
        if state_dict is None:
            raise ValueError("state_dict (diffusers-keyed U-Net weights) is required: no checkpoint is bundled")
        # torch.float16 is what every reference driver passes (cute_main.py:31): the kernels then compute in IEEE fp16
        # (v_mfma_f32_16x16x32_f16, same rate as bf16); torch.bfloat16 is the headline mode, torch.float32 the parity mode
        if torch_dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("torch_dtype must be torch.float32, torch.bfloat16 or torch.float16")
        self.dtype = torch_dtype
        self.device = torch.device("cuda:0" if device == "cuda" else device)
        self.ip_adapter = False
        self.cfg = unet_config
        self.state_dict = state_dict
        self.vae = vae
        self.vae_dtype = vae_dtype
        self._encode_prompt = encode_prompt
        self.use_graphs = use_graphs            # replay each U-Net forward as one hipGraph (small, launch-bound batches)
        # dtype of the generator draws and of the add_noise arithmetic.  float32 = the reference run as an fp32 CPU
        # pipeline (the north_star parity setting).  float16 = the reference as its drivers construct it
        # (DiffSim(torch.float16), diffsim.py:79-83): randn_tensor(dtype=latents.dtype) draws in fp16 -- a different
        # random stream from the fp32 draw of the same seed -- the VAE sample is drawn in fp16 too, and
        # scheduler.add_noise runs in fp16 (diffsim_pipeline.py:174-183)
        if noise_dtype not in (torch.float32, torch.float16):
            raise ValueError("noise_dtype must be torch.float32 or torch.float16")
        self.noise_dtype = noise_dtype
        if vae is not None and hasattr(vae, "sample_dtype"):
            vae.sample_dtype = noise_dtype
        # default (opt out with dedup_cfg=False): conv_in, the first resnet and the first transformer's self-attention are
        # identical in the two CFG halves (torch.cat([latents] * 2), diffsim_pipeline.py:208); compute them once per image.
        # Bit-identical scores (tests/test_gpu_round2.py::test_cfg_dedup_is_bit_identical), ~6 % faster.  bench.py's headline
        # line passes dedup_cfg=False: it executes every algorithmic FLOP of the reference's duplicated batch.
        self.dedup_cfg = bool(dedup_cfg)
        self.fusion = fusion                    # None = the library default (every fused kernel); 0 = one launch per layer
        self._base: Optional[UNetEngine] = None
        self._engines: Dict[Tuple[str, int], object] = {}
        self._ctx: Dict[str, torch.Tensor] = {}
        self._pool = ThreadPoolExecutor(max_workers=host_threads())     # host-side image decode / resize: cores / ranks of the node
        # files-in paths: decode + Lanczos resize run ahead of the GPU in worker processes (decode_procs > 0; None = the
        # DSIM_DECODE_PROCS environment default) or threads (0); started lazily, on the first path batch
        self._decode = DecodePool(decode_procs)
        self._streams: List[torch.cuda.Stream] = []          # side streams of score_latent_pairs
        # tokenize(str) -> (1, L) ids, the tokenizer behind encode_prompt (loader.py sets it): which prompt tokens a word is,
        # for the text-guided regions (textattn.py)
        self.tokenize: Optional[Callable[[str], torch.Tensor]] = None

    # ------------------------------------------------------------------------------------------
    def engine(self, target_block: str, target_layer: int) -> UNetEngine:
        """The engine positioned at a tap.  ONE packed weight copy (per scorer, i.e. per dtype) serves every tap:
        the handle's tap is moved, nothing is re-packed."""
        key = (target_block, int(target_layer))
        if key not in self._engines:
            if self._base is None:
                self._base = UNetEngine(self.cfg, self.state_dict, self.dtype, target_block, int(target_layer),
                                        str(self.device))
                self._base.use_graphs = self.use_graphs
                if self.dedup_cfg:
                    self._base.set_cfg_dedup(True)
                if self.fusion is not None:
                    self._base.set_fusion(self.fusion)
            self._engines[key] = self._base.view(target_block, int(target_layer))
            self._engines[key].tokens            # moves the tap once: a missing weight raises here, not mid-run
        return self._engines[key]

    # ---- the Scorer protocol: this kind's facts (scorer.py)
    image_half = property(lambda self: self.vae_dtype == torch.float16)     # image.to(dtype=float16), diffsim.py:93
    noise_draw = property(lambda self: self.noise_dtype)                    # randn_tensor(dtype=latents.dtype): the pipeline dtype
    eps_dtype = property(lambda self: self.noise_dtype)                     # latent_dist.sample draws in the pipeline dtype too
    round16 = property(lambda self: self.noise_dtype == torch.float16)      # the fp16 pipeline holds its latents in fp16

    def prepare(self, tensor, generator):
        return self.prepare_image_latents(tensor, None, None, generator).to(self.noise_draw).float()

    path_hip_vae = True                     # the one-pair path calls encode through the HIP VAE (scorer.py)
    exemplar_regions = True                 # the kind has exemplar-guided regions (transfer.py)

    def path_tap(self, prompt, target_block, target_layer):
        return prompt, target_block, _norm_layer(target_layer)

    def tap_of(self, target_block, target_layer):
        return target_block, _norm_layer(target_layer)

    @staticmethod
    def canonical_tap(tap):
        return tap[0], int(tap[1])

    def auto_map_pairs(self, eng, n: int) -> int:
        return self.auto_rows(eng, n, 2)                        # 64 where it fits, as score_latent_pairs on one stream

    def context(self, prompt: Union[str, torch.Tensor]) -> torch.Tensor:
        """[uncond, cond] prompt embeddings (2, L, Dc) f32 on the device; cached per prompt
        (the reference re-encodes the constant prompt on every call, diffsim_pipeline.py:125)."""
        if isinstance(prompt, torch.Tensor):
            return prompt.to(self.device, torch.float32).contiguous()
        if prompt not in self._ctx:
            if self._encode_prompt is None:
                raise RuntimeError("no text encoder plugged in: pass encode_prompt=... or a (2,L,Dc) tensor as prompt")
            self._ctx[prompt] = self._encode_prompt(prompt).to(self.device, torch.float32).contiguous()
        return self._ctx[prompt]

    def prompt_table(self, prompts: Sequence[Union[str, torch.Tensor]]):
        """The contexts of one engine batch from a prompt per image (strings or (2, L, Dc) tensors): the (2, L, Dc) context itself
        when they all name one prompt, else a PromptTable of the distinct ones in order of first appearance, each encoded once
        (through the context() cache)."""
        firsts, index = distinct_prompts(prompts)
        if not firsts:
            raise ValueError("no prompts")
        if len(firsts) == 1:
            return self.context(firsts[0])
        return PromptTable(torch.stack([self.context(p) for p in firsts]), index)

    def _contexts(self, prompt, n: int):
        """(ctx, ctx_index) of an engine call over n images: one prompt -> ((2, L, Dc), None); a prompt per image (n entries) or a
        PromptTable -> (table, index), or the one context they all name."""
        if not single_prompt(prompt):
            prompt = self.prompt_table(check_row_prompts(prompt, n, "images"))
        if isinstance(prompt, PromptTable):
            if len(prompt.index) != n:
                raise ValueError(f"a prompt table of {len(prompt.index)} images for {n} images")
            return prompt.table, prompt.index
        return self.context(prompt), None

    def prepare_image_latents(self, image, vae=None, device=None, generator=None):
        vae = vae or self.vae
        if vae is None:
            raise RuntimeError("no VAE plugged in: use the latents-in entry points (diffsim_latents / score_latent_pairs)")
        if isinstance(getattr(vae, "device", None), torch.device):
            image = image.to(vae.device)          # cast on the device: the same RNE rounding, without 4 ms of host time
        image = image.to(dtype=self.vae_dtype)
        lat = vae.encode(image).latent_dist.sample(generator=generator)
        return vae.config.scaling_factor * lat

    def _pair_latents(self, tensor_A, tensor_B, generator):
        """Latents of both images.  With the HIP VAE encoder the two images go through ONE encode (its kernels are
        batch-invariant bit for bit) and are then sampled in the reference's order -- A's draw, then B's."""
        vae = self.vae
        if vae is not None and hasattr(vae, "moments") and tensor_A.shape == tensor_B.shape:
            x = torch.cat([tensor_A, tensor_B]).to(vae.device).to(dtype=self.vae_dtype)
            mom = vae.moments(x)
            sf = vae.config.scaling_factor
            return (sf * _LatentDist(mom[0:1], self.noise_dtype).sample(generator=generator),
                    sf * _LatentDist(mom[1:2], self.noise_dtype).sample(generator=generator))
        return (self.prepare_image_latents(tensor_A, vae, None, generator),
                self.prepare_image_latents(tensor_B, vae, None, generator))

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features(self, latents: torch.Tensor, noise: torch.Tensor, prompt, target_block, target_layer, target_step):
        """latents/noise (n,4,s,s) -> q,k,v [n][2][N][H*D] (compute dtype, on device).  prompt: one for every image (a string or
        a (2, L, Dc) context), or a sequence of n, one per image: all prompts then run in ONE forward (a context table), each
        image's rows bit for bit those of a call with its own prompt alone."""
        eng = self.engine(target_block, target_layer)
        *args, idx = self._forward_inputs(eng, latents, noise, prompt, target_step)
        return eng.qkv(*args, ctx_index=idx)

    @torch.no_grad()
    def features_text(self, latents: torch.Tensor, noise: torch.Tensor, prompt, target_block, target_layer, target_step):
        """:meth:`features` and the tapped block's cross-attention operands, (q, k, v, xq, xkv): UNetEngine.qkv_text."""
        eng = self.engine(target_block, target_layer)
        *args, idx = self._forward_inputs(eng, latents, noise, prompt, target_step)
        return eng.qkv_text(*args, ctx_index=idx)

    @torch.no_grad()
    def features_taps(self, latents: torch.Tensor, noise: torch.Tensor, prompt, taps, target_step):
        """:meth:`features` at every tap of `taps` ([(target_block, layer)], layers explicit) from ONE U-Net forward: a list of
        (q, k, v), entry i bit for bit what features() gives at taps[i] (sweep.py)."""
        if not taps:
            raise ValueError("no taps")
        if self._base is None:
            self.engine(*taps[0])
        eng = self._base                # the sweep does not move the handle's tap
        *args, idx = self._forward_inputs(eng, latents, noise, prompt, target_step)
        return eng.qkv_taps(*args, [(b, int(l)) for b, l in taps], ctx_index=idx)

    def _forward_inputs(self, eng, latents, noise, prompt, target_step):
        """(latents, noise, sqrt_abar, sqrt_1m_abar, ctx, ctx_index) of the engine call at target_step; sets the engine's
        timestep.  ctx_index is None for one prompt, else each image's row of the context table ctx."""
        t = sched.timestep_from_index(int(target_step))
        eng.set_timestep(t)
        sa, sb = sched.noise_coefficients(t)
        if self.noise_dtype == torch.float16:
            # PNDMScheduler.add_noise on fp16 tensors: alphas_cumprod cast to fp16, sqrt and 1-x in fp16, the two
            # products and the sum each rounded to fp16 (elementwise, so the batch can be done on the device)
            dev = self.device
            ac = sched.alphas_cumprod()[t].to(torch.float16)
            a16, b16 = ac ** 0.5, (1 - ac) ** 0.5
            xt = a16.to(dev) * latents.to(dev, torch.float16) + b16.to(dev) * noise.to(dev, torch.float16)
            lat = xt.float().contiguous()
            ctx, idx = self._contexts(prompt, latents.shape[0])
            ctx16 = ctx.to(torch.float16).float()         # the fp16 text encoder's output (elementwise: each context of a table alike)
            return lat, torch.zeros_like(lat), 1.0, 0.0, ctx16, idx
        lat = latents.to(self.device, torch.float32).contiguous()
        nz = noise.to(self.device, torch.float32).contiguous()
        ctx, idx = self._contexts(prompt, latents.shape[0])
        return lat, nz, sa, sb, ctx, idx

    def auto_batch_pairs(self, eng, n_pairs: int, streams: int = 2, target: int = 64) -> int:
        """Pairs per chunk when the caller names none: `target` (the sweep's optimum on a 288 GB part) within what fits
        (Scorer.auto_rows)."""
        return self.auto_rows(eng, n_pairs, 2, streams=streams, images=2 * target)

    @torch.no_grad()
    def score_latent_pairs(self, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                           target_step=600, similarity="cosine", batch_pairs: Optional[int] = None, streams: int = 2) -> torch.Tensor:
        """Batched latents-in scoring: pair i = (latA[i], latB[i]) -> scores (n,) f32 on device.
        noiseA/noiseB are (1,4,s,s) (shared by every pair: each reference call reseeds) or (n,4,s,s).
        prompt: one for every pair, or a sequence of n (strings or (2, L, Dc) contexts), pair i's prompt: a chunk then runs its
        pairs' prompts in one forward (each distinct one encoded once), and each score is bit for bit the one-prompt call's.
        Consecutive chunks of `batch_pairs` pairs are enqueued on `streams` HIP streams in turn, so the HBM-bound kernels of
        one chunk overlap the MFMA-bound kernels of the next (same kernels, same scores).  Each stream in use owns one
        workspace arena of the engine (streams = 2 -> two arenas, ~0.75 GB per pair of the chunk size each).
        batch_pairs=None picks the measured optimum (profiles/r04h_batch_sweep.txt: 64 pairs per chunk, 662 pairs/s against
        603 at 16) within what fits: every activation < 2 GiB and the arenas of the streams in use inside the free HBM."""
        n = latA.shape[0]
        prompt = check_row_prompts(prompt, n)
        eng = self.engine(target_block, target_layer)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        if batch_pairs is None:
            batch_pairs = self.auto_batch_pairs(eng, n, streams)
        batch_pairs = max(1, min(batch_pairs, eng.max_images(n_ctx=1 if single_prompt(prompt) else 2) // 2))      # every activation must stay < 2 GiB
        starts = list(range(0, n, batch_pairs))
        ns = max(1, min(int(streams), len(starts)))
        if self.use_graphs or getattr(eng, "_profiling", False):
            ns = 1          # (per-launch profile brackets are only a kernel's own time when nothing overlaps it)
        main = torch.cuda.current_stream(self.device)
        chunk_prompts = [row_prompts(prompt, i0, min(n, i0 + batch_pairs), 2) for i0 in starts]
        if ns > 1:
            if len(self._streams) < ns:
                self._streams += [torch.cuda.Stream(device=self.device) for _ in range(ns - len(self._streams))]
            # everything the chunks share is produced on the main stream BEFORE the side streams fork from it: the prompt
            # contexts (every chunk's context table) and the timestep tables (set_timestep enqueues kernels; a later chunk on
            # another stream would see "already set" on the host while those kernels are still running)
            chunk_prompts = [self.context(p) if single_prompt(p) else self.prompt_table(p) for p in chunk_prompts]
            eng.set_timestep(sched.timestep_from_index(int(target_step)))
            for st in self._streams[:ns]:
                st.wait_stream(main)
        for ci, i0 in enumerate(starts):
            i1 = min(n, i0 + batch_pairs)
            m = i1 - i0
            with torch.cuda.stream(self._streams[ci % ns] if ns > 1 else main):
                lat, nz = stack_rows([latA, latB], [noiseA, noiseB], i0, i1)
                q, k, v = self.features(lat, nz, chunk_prompts[ci], target_block, target_layer, target_step)
                ia = torch.arange(0, 2 * m, 2, dtype=torch.int32, device=self.device)
                out[i0:i1] = pair_score(q, k, v, ia, ia + 1, eng.heads, similarity)
        if ns > 1:
            for st in self._streams[:ns]:
                main.wait_stream(st)
        return out

    @torch.no_grad()
    def diffsim_latents(self, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                        target_step=600, similarity="cosine") -> torch.Tensor:
        return self.score_latent_pairs(latA, latB, noiseA, noiseB, prompt, target_block, _norm_layer(target_layer),
                                       target_step, similarity)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def diffsim(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, ip_adapter=False,
                seed="2333", device="cuda", similarity="cosine"):
        """Same contract as the reference's ``DiffSim.diffsim`` (diffsim/diffsim.py:98-197)."""
        if ip_adapter:
            raise NotImplementedError("IP-Adapter mode is out of scope")
        target_layer = _norm_layer(target_layer)
        latentsA, latentsB, noiseA, noiseB = self._path_pair_latents(image_A, image_B, img_size, seed)
        return self.score_latent_pairs(latentsA, latentsB, noiseA, noiseB, prompt, target_block, target_layer, target_step,
                                       similarity)

    def _path_pair_latents(self, image_A, image_B, img_size, seed):
        """(latentsA, latentsB, noiseA, noiseB) as f32 tensors: what one reference call draws for the two image files."""
        if self.gpu_resize and hasattr(self.vae, "moments"):    # decode on the host, process_image on the device: the same bits
            px = resize_u8([f.result() for f in self._decode.submit_raw([image_A, image_B])], img_size, img_size, "lanczos",
                           device=self.vae.device)
            t = image_preprocess(px)
            return self._pair_draws(t[0:1], t[1:2], seed)
        # decode + Lanczos resize of the two images on two host threads (PIL releases the GIL); same tensors as serially
        fa = self._pool.submit(lambda: process_image(load_image(image_A), img_size))
        tensor_B = process_image(load_image(image_B), img_size)
        return self._pair_draws(fa.result(), tensor_B, seed)

    def _pair_draws(self, tensor_A, tensor_B, seed):
        generator = get_generator(seed, "cpu")                   # reference CPU path: CPU generator
        latentsA, latentsB = self._pair_latents(tensor_A, tensor_B, generator)
        # DiffSimPipeline.step draws the noise right after prepare_latents: A's step first, then B's
        noiseA = torch.randn(latentsA.shape, generator=generator, dtype=self.noise_dtype)
        noiseB = torch.randn(latentsB.shape, generator=generator, dtype=self.noise_dtype)
        if self.noise_dtype == torch.float16:      # the fp16 pipeline holds its latents in fp16
            latentsA, latentsB = latentsA.to(torch.float16), latentsB.to(torch.float16)
        return latentsA.float(), latentsB.float(), noiseA.float(), noiseB.float()

    @torch.no_grad()
    def score_pairs(self, pairs: Sequence[Tuple[str, str]], img_size, prompt, target_block, target_layer, target_step,
                    seed="2333", similarity="cosine", batch_pairs: Optional[int] = None) -> torch.Tensor:
        """Batched equivalent of calling :meth:`diffsim` once per (A, B) path pair."""
        target_layer = _norm_layer(target_layer)
        # batch_pairs=None: 16 pairs per VAE encode (32 images at 512 px keep its widest activation < 2 GiB), and
        # score_latent_pairs picks its own chunk (64 where it fits)
        (latA, latB), nA, nB = path_latents(self, list(pairs), (0, 1), img_size, seed, 16 if batch_pairs is None else batch_pairs)
        return self.score_latent_pairs(latA, latB, nA, nB, prompt, target_block, target_layer, target_step, similarity,
                                       batch_pairs)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def score_matrix(self, paths_a: Sequence[str], paths_b: Sequence[str], img_size, prompt, target_block, target_layer,
                     target_step, seed="2333", similarity="cosine", batch: Optional[int] = None) -> torch.Tensor:
        """(len(paths_a), len(paths_b)) matrix of :meth:`diffsim` scores, every image pushed through the U-Net once
        (retrieval.score_path_matrix)."""
        return retrieval.score_path_matrix(self, paths_a, paths_b, img_size, prompt, target_block, _norm_layer(target_layer), target_step,
                                           seed, similarity, batch)

    @torch.no_grad()
    def score_latent_matrix(self, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                            target_step=600, similarity="cosine", batch: Optional[int] = None) -> torch.Tensor:
        """(n_a, n_b) matrix of :meth:`diffsim_latents` scores of (latA[i], latB[j]) (retrieval.score_latent_matrix)."""
        return retrieval.score_latent_matrix(self, latA, latB, noiseA, noiseB, prompt, target_block, _norm_layer(target_layer),
                                             target_step, similarity, batch)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def similarity_maps(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed="2333",
                        similarity="cosine"):
        """:meth:`diffsim`'s score of one image pair with its per-token terms on both images' grids: a
        :class:`~diffsim_amd.maps.SimilarityMaps` of one pair (direction 0 on image_A's grid, 1 on image_B's)."""
        latentsA, latentsB, noiseA, noiseB = self._path_pair_latents(image_A, image_B, img_size, seed)
        return self.score_latent_pair_maps(latentsA, latentsB, noiseA, noiseB, prompt, target_block, target_layer, target_step,
                                           similarity)

    @torch.no_grad()
    def score_latent_pair_maps(self, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                               target_step=600, similarity="cosine", batch_pairs: Optional[int] = None):
        """Maps of the pairs of :meth:`score_latent_pairs` (maps.score_latent_pair_maps)."""
        return maps.score_latent_pair_maps(self, latA, latB, noiseA, noiseB, prompt, target_block, _norm_layer(target_layer),
                                           target_step, similarity, batch_pairs)

    @torch.no_grad()
    def score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, prompt, target_block="up_blocks", target_layer=0,
                                    target_step=600, batch_pairs: Optional[int] = None):
        """Alignments of the pairs of :meth:`score_latent_pairs` (align.score_latent_pair_alignment)."""
        return align.score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, prompt, target_block, _norm_layer(target_layer),
                                                 target_step, batch_pairs)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, prompt, taps, target_step=600, similarity="cosine",
                                batch_pairs: Optional[int] = None) -> torch.Tensor:
        """(n_taps, n) scores: row t is :meth:`score_latent_pairs` at taps[t], every tap from one forward per chunk
        (sweep.score_latent_pairs_taps).  taps: [(target_block, layer)] with explicit layers, or "all"."""
        return sweep.score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, prompt, taps, target_step, similarity, batch_pairs)

    @torch.no_grad()
    def score_pairs_taps(self, pairs: Sequence[Tuple[str, str]], img_size, prompt, taps, target_step, seed="2333",
                         similarity="cosine") -> torch.Tensor:
        """(n_taps, len(pairs)) scores: row t is :meth:`score_pairs` at taps[t]; the images are decoded and encoded once for all
        taps (sweep.score_path_pairs_taps)."""
        return sweep.score_path_pairs_taps(self, pairs, img_size, prompt, taps, target_step, similarity, seed)
