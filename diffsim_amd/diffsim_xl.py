"""DiffSim-XL scorer (SDXL U-Net) with the reference's entry points, backed by the MI355X engine.

Mirrors ``/root/reference/diffsim/diffsim_xl.py`` (``diffsim_xl.__init__`` :48-56, ``prepare_image_latents``
:58-63, ``diffsim_score`` :65-155) and what ``DiffSimXLPipeline.step`` does around the U-Net call
(``/root/reference/diffsim/diffsim_xl_pipeline.py:163-323``): prompt + pooled embeddings, Euler
index -> (t, sigma), latents * init_noise_sigma + sigma*noise, / sqrt(sigma^2+1), CFG duplication,
``added_cond_kwargs = {text_embeds, time_ids}``.  ``target_layer`` is the reference's 3-int address
``[block, attention, transformer_block]`` (2 ints for mid_blocks).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch

from . import align, maps, sweep
from . import scheduler as sched
from .config import SDXL, UNetConfig
from .engine import UNetEngine, pair_score
from .scorer import Scorer, check_row_prompts, distinct_prompts


class diffsim_xl(Scorer):
    mixes_prompts = False       # the pooled prompt embedding enters the time embedding of every resnet, one per CFG half
    engine_images = 16          # the batch sweeps' optimum at 1024 px

    def __init__(self, torch_dtype=torch.bfloat16, device="cuda", ip_adapter=False, *, unet_config: UNetConfig = SDXL,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, vae=None,
                 encode_prompt: Optional[Callable[[str], Tuple[torch.Tensor, torch.Tensor]]] = None,
                 noise_dtype=torch.float32):
        if ip_adapter:
            raise NotImplementedError("IP-Adapter mode is out of scope")
        if state_dict is None:
            raise ValueError("state_dict (diffusers-keyed SDXL U-Net weights) is required")
        self.dtype = torch_dtype
        self.device = torch.device("cuda:0" if device == "cuda" else device)
        self.ip_adapter = False
        self.cfg, self.state_dict, self.vae, self._encode_prompt = unet_config, state_dict, vae, encode_prompt
        # float32: the reference's arithmetic carried out in fp32 (draws included) -- the parity setting.
        # float16: the literal fp16 pipeline -- latents arrive fp16 (diffsim_xl.py:63), prepare_latents multiplies them
        # by init_noise_sigma in fp16, randn_tensor(dtype=latents.dtype) draws in fp16 (a different random stream),
        # add_noise and scale_model_input run in fp16 (diffsim_xl_pipeline.py:204-225, 309)
        if noise_dtype not in (torch.float32, torch.float16):
            raise ValueError("noise_dtype must be torch.float32 or torch.float16")
        self.noise_dtype = noise_dtype
        self._base: Optional[UNetEngine] = None
        self._engines: Dict[tuple, object] = {}
        self.tokenize = None        # tokenize(str) -> (1, L) ids of the first text encoder's tokenizer (loader.py sets it; textattn.py)

    def engine(self, target_block: str, target_layer):
        """The engine positioned at a tap; one packed weight copy serves every tap."""
        key = (target_block, tuple(int(v) for v in target_layer))
        if key not in self._engines:
            if self._base is None:
                self._base = UNetEngine(self.cfg, self.state_dict, self.dtype, target_block, list(key[1]), str(self.device))
            self._engines[key] = self._base.view(target_block, list(key[1]))
            self._engines[key].tokens
        return self._engines[key]

    # ---- the Scorer protocol: this kind's facts (scorer.py)
    noise_draw = property(lambda self: self.noise_dtype)        # randn_tensor(dtype=latents.dtype) of the pipeline run
    exemplar_regions = True     # the kind has exemplar-guided regions (transfer.py)

    @staticmethod
    def canonical_tap(tap):
        return tap[0], [int(v) for v in tap[1]]

    def prompt_rows(self, prompt, n_rows: int, what: str = "triplets"):
        """One prompt per call: a string, its (context, pooled) tuple, or a list that repeats one."""
        if isinstance(prompt, list):
            prompt = check_row_prompts(prompt, n_rows, what)
            if len(distinct_prompts(prompt)[0]) > 1:
                raise ValueError("SDXL takes one prompt per call: its pooled prompt embedding enters every resnet")
            return prompt[0]
        return prompt

    def bind_prompt(self, prompt, n_rows: int, what: str = "triplets"):
        """(context, pooled): a prompt string is encoded here, once per call and not once per engine batch."""
        prompt = self.prompt_rows(prompt, n_rows, what)
        if isinstance(prompt, tuple):
            return prompt
        if self._encode_prompt is None:
            raise RuntimeError("no text encoder plugged in: pass encode_prompt=...")
        return self._encode_prompt(prompt)

    def tap_features(self, lat, nz, prompt, tap, step):
        return self.features(lat, nz, *prompt, *tap, step)

    def taps_features(self, lat, nz, prompt, taps, step):
        return self.features_taps(lat, nz, *prompt, taps, step)

    def tap_features_text(self, lat, nz, prompt, tap, step):
        return self.features_text(lat, nz, *prompt, *tap, step)

    def prepare_image_latents(self, image, generator=None):
        if self.vae is None:
            raise RuntimeError("no VAE plugged in: use score_latent_pairs")
        lat = self.vae.encode(image.to(dtype=torch.float32)).latent_dist.sample(generator=generator)
        lat = self.vae.config.scaling_factor * lat
        return lat.to(dtype=torch.float16)                         # diffsim_xl.py:63

    def time_ids(self) -> torch.Tensor:
        # original_size = target_size = (height, width) = unet.config.sample_size * vae_scale_factor -- the model's
        # NATIVE size (1024 for SDXL), whatever --image_size the latents were encoded at: step() is called without
        # height/width (diffsim_xl.py:109-125 -> diffsim_xl_pipeline.py:127-131, 231-246)
        side = float(self.cfg.sample_size * 8)
        return torch.tensor([[side, side, 0.0, 0.0, side, side]] * 2, dtype=torch.float32)

    @torch.no_grad()
    def features(self, latents, noise, ctx, pooled, target_block, target_layer, target_step):
        """latents / noise (n,4,s,s): any latent side s (img_size // 8), not only cfg.sample_size."""
        eng = self.engine(target_block, target_layer)
        return eng.qkv(*self._forward_inputs(eng, latents, noise, ctx, pooled, target_step))

    @torch.no_grad()
    def features_text(self, latents, noise, ctx, pooled, target_block, target_layer, target_step):
        """:meth:`features` and the tapped block's cross-attention operands, (q, k, v, xq, xkv): UNetEngine.qkv_text."""
        eng = self.engine(target_block, target_layer)
        return eng.qkv_text(*self._forward_inputs(eng, latents, noise, ctx, pooled, target_step))

    @torch.no_grad()
    def features_taps(self, latents, noise, ctx, pooled, taps, target_step):
        """:meth:`features` at every tap of `taps` ([(target_block, [b, a, t])]; mid: [a, t]) from ONE U-Net forward: a list of
        (q, k, v), entry i bit for bit what features() gives at taps[i] (sweep.py)."""
        if not taps:
            raise ValueError("no taps")
        if self._base is None:
            self.engine(*taps[0])
        eng = self._base                # the sweep does not move the handle's tap
        return eng.qkv_taps(*self._forward_inputs(eng, latents, noise, ctx, pooled, target_step),
                            [(b, [int(v) for v in l]) for b, l in taps])

    def _forward_inputs(self, eng, latents, noise, ctx, pooled, target_step):
        """(x, noise, a, b, ctx) of the engine call at target_step; sets the engine's conditioning."""
        t, a, b = sched.sdxl_step_coefficients(int(target_step))
        if self.noise_dtype == torch.float16:       # the fp16 text encoders' outputs
            ctx, pooled = ctx.to(torch.float16).float(), pooled.to(torch.float16).float()
        eng.set_conditioning(t, pooled, self.time_ids())
        ctx = ctx.to(self.device, torch.float32).contiguous()
        if self.noise_dtype == torch.float16:
            ts, sig, init = sched.euler_tables()
            sg = torch.tensor(float(sig[int(target_step)]), dtype=torch.float32)
            dev = self.device
            x = latents.to(dev, torch.float16) * init                          # prepare_latents: fp16 * python float
            x = x + noise.to(dev, torch.float16) * sg.to(torch.float16).to(dev)  # add_noise: sigmas cast to the sample dtype
            x = x / ((sg ** 2 + 1) ** 0.5).to(dev)                              # scale_model_input: fp16 / 0-dim fp32 -> fp16
            x = x.float().contiguous()
            return x, torch.zeros_like(x), 1.0, 0.0, ctx
        return latents.to(self.device, torch.float32).contiguous(), noise.to(self.device, torch.float32).contiguous(), a, b, ctx

    @torch.no_grad()
    def score_latent_pairs(self, latA, latB, noiseA, noiseB, ctx, pooled, target_block, target_layer, target_step,
                           similarity="cosine", batch_pairs: int = 8) -> torch.Tensor:
        out = torch.empty(latA.shape[0], dtype=torch.float32, device=self.device)
        for i0, i1, s in self.pair_chunks(latA, latB, noiseA, noiseB, (ctx, pooled), (target_block, target_layer), target_step,
                                          similarity, batch_pairs, pair_score):
            out[i0:i1] = s
        return out

    @torch.no_grad()
    def diffsim_score(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, similarity, seed):
        """Same contract as the reference's ``diffsim_xl.diffsim_score`` (diffsim/diffsim_xl.py:65-155)."""
        latentsA, latentsB, noiseA, noiseB, ctx, pooled = self._path_pair_inputs(image_A, image_B, img_size, prompt, seed)
        return self.score_latent_pairs(latentsA, latentsB, noiseA, noiseB, ctx, pooled, target_block, target_layer, target_step,
                                       similarity)

    def _path_pair_inputs(self, image_A, image_B, img_size, prompt, seed):
        """(latentsA, latentsB, noiseA, noiseB, ctx, pooled): what one reference call draws and encodes."""
        ctx, pooled = self.bind_prompt(prompt, 1)
        return (*self._path_pair_latents(image_A, image_B, img_size, seed), ctx, pooled)

    @torch.no_grad()
    def similarity_maps(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, similarity, seed):
        """:meth:`diffsim_score` with the per-token terms on both images' grids (a maps.SimilarityMaps of one pair)."""
        latentsA, latentsB, noiseA, noiseB, ctx, pooled = self._path_pair_inputs(image_A, image_B, img_size, prompt, seed)
        return self.score_latent_pair_maps(latentsA, latentsB, noiseA, noiseB, ctx, pooled, target_block, target_layer,
                                           target_step, similarity)

    @torch.no_grad()
    def score_latent_pair_maps(self, latA, latB, noiseA, noiseB, ctx, pooled, target_block, target_layer, target_step,
                               similarity="cosine", batch_pairs: int = 8):
        """Maps of the pairs of :meth:`score_latent_pairs` (maps.score_latent_pair_maps)."""
        return maps.score_latent_pair_maps(self, latA, latB, noiseA, noiseB, (ctx, pooled), target_block, target_layer, target_step,
                                           similarity, batch_pairs)

    @torch.no_grad()
    def score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, ctx, pooled, target_block, target_layer, target_step,
                                    batch_pairs: int = 8):
        """Alignments of the pairs of :meth:`score_latent_pairs` (align.score_latent_pair_alignment)."""
        return align.score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, (ctx, pooled), target_block, target_layer,
                                                 target_step, batch_pairs)

    @torch.no_grad()
    def score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, ctx, pooled, taps, target_step, similarity="cosine",
                                batch_pairs: Optional[int] = None) -> torch.Tensor:
        """(n_taps, n) scores: row t is :meth:`score_latent_pairs` at taps[t] (sweep.score_latent_pairs_taps)."""
        return sweep.score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, (ctx, pooled), taps, target_step, similarity,
                                             batch_pairs)

    @torch.no_grad()
    def score_pairs_taps(self, pairs, img_size, prompt, taps, target_step, similarity="cosine", seed=2333) -> torch.Tensor:
        """(n_taps, len(pairs)) scores of (A, B) path pairs, the images encoded once for all taps (sweep.score_path_pairs_taps)."""
        return sweep.score_path_pairs_taps(self, pairs, img_size, prompt, taps, target_step, similarity, seed)
