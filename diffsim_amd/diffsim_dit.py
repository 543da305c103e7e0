"""DiffSim-DiT scorer with the reference's entry points, backed by the MI355X engine.

Mirrors ``/root/reference/diffsim/diffsim_dit.py``: ``diffsim_DiT.__init__`` :30-61 (model + VAE + DDIM scheduler),
``prepare_image_latents`` :54-59, ``add_noise`` :63-72, ``diffsim_score`` :74-142 (labels [1, 1000], hook on
``model.blocks[target_layer[0]].attn``, ``p_sample`` at t = 1000 - target_step, shared score tail).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import align, maps, sweep
from . import scheduler as sched
from ._lib import DsimError
from .config import DIT_XL2, DiTConfig
from .engine import DiTEngine, pair_score
from .inputs import path_latents
from .scorer import Scorer


class diffsim_DiT(Scorer):
    """The prompt is ignored (labels [1, 1000]); the noise is drawn in the fp16 of the latents (randn_tensor(dtype=latents.dtype)):
    the base's defaults.  A tap is the block index."""
    canonical_tap = staticmethod(int)
    one_tap_bound = False       # DiTEngine.qkv plans no image bound: a one-tap batch is neither capped nor halved for the free HBM

    def __init__(self, img_size=256, target_step=600, device="cuda", ckpt=None, *, dit_config: DiTConfig = DIT_XL2,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, vae=None, torch_dtype=torch.bfloat16,
                 fp8_attention: bool = False):
        if state_dict is None:
            raise ValueError("state_dict (DiT weights under DiT/modelsdit.py keys) is required; no checkpoint is bundled")
        if img_size // 8 != dit_config.input_size:
            raise ValueError("img_size must be 8 * dit_config.input_size")
        self.cfg, self.state_dict, self.vae = dit_config, state_dict, vae
        self.dtype = torch_dtype
        self.device = torch.device("cuda:0" if device == "cuda" else device)
        self.fp8_attention = fp8_attention      # e4m3 MFMAs for QK^T and PV inside the DiT blocks (opt-in)
        self._engine: Optional[DiTEngine] = None

    def engine(self, layer: int) -> DiTEngine:
        """The engine with its tap at blocks[layer]: ONE packed weight copy, the tap is moved (dsim_dit_set_tap)."""
        if self._engine is None:
            self._engine = DiTEngine(self.cfg, self.state_dict, self.dtype, int(layer), str(self.device))
            if self.fp8_attention:
                self._engine.set_attention(True)
        self._engine.set_tap(int(layer))
        return self._engine

    # ---- the Scorer protocol: this kind's facts (scorer.py)
    path_batch_pairs = 32       # the one-pair path calls' engine batch
    exemplar_regions = True     # the kind has exemplar-guided regions (transfer.py): no text is involved

    def path_tap(self, prompt, target_block, target_layer):
        return None, "none", [int(target_layer[0])]

    def tap_of(self, target_block, target_layer):
        return int(target_layer[0])                 # the hook on model.blocks[target_layer[0]].attn

    def engine_at(self, tap):
        return self.engine(tap)

    def sweep_engine(self, taps, side: int):
        if not taps:
            raise DsimError("no taps")
        eng = self._engine if self._engine is not None else self.engine(taps[0])
        return eng, [(eng.tokens, eng.heads, eng.head_dim)] * len(taps)

    def tap_features(self, lat, nz, prompt, tap, step):
        return self.features(lat, nz, tap, step)

    def taps_features(self, lat, nz, prompt, taps, step):
        return self.features_taps(lat, nz, taps, step)

    def prepare_image_latents(self, image, generator=None):
        if self.vae is None:
            raise RuntimeError("no VAE plugged in: use score_latent_pairs")
        lat = self.vae.encode(image.to(dtype=torch.float32)).latent_dist.sample(generator=generator)
        return (self.vae.config.scaling_factor * lat).to(dtype=torch.float16)      # diffsim_dit.py:59

    @torch.no_grad()
    def features(self, latents, noise, target_layer: int, target_step: int):
        eng = self.engine(int(target_layer))
        eng.set_conditioning(sched.dit_model_timestep(int(target_step)), 1, self.cfg.num_classes)   # y = [1, null]
        sa, sb = sched.noise_coefficients(int(target_step))         # DDIM add_noise at t = target_step (SD1.5 betas)
        return eng.qkv(latents.to(self.device, torch.float32).contiguous(), noise.to(self.device, torch.float32).contiguous(),
                       sa, sb)

    @torch.no_grad()
    def features_taps(self, latents, noise, layers, target_step: int):
        """:meth:`features` at every block of `layers` from ONE forward: a list of (q, k, v), entry i bit for bit what features()
        gives at layers[i] (sweep.py).  The engine's tap does not move."""
        if not layers:
            raise ValueError("no taps")
        eng = self._engine if self._engine is not None else self.engine(int(layers[0]))
        eng.set_conditioning(sched.dit_model_timestep(int(target_step)), 1, self.cfg.num_classes)
        sa, sb = sched.noise_coefficients(int(target_step))
        return eng.qkv_taps(latents.to(self.device, torch.float32).contiguous(), noise.to(self.device, torch.float32).contiguous(),
                            sa, sb, [int(l) for l in layers])

    @torch.no_grad()
    def score_latent_pairs(self, latA, latB, noiseA, noiseB, target_layer: int, target_step: int, similarity="cosine",
                           batch_pairs: int = 32) -> torch.Tensor:
        out = torch.empty(latA.shape[0], dtype=torch.float32, device=self.device)
        for i0, i1, s in self.pair_chunks(latA, latB, noiseA, noiseB, None, int(target_layer), target_step, similarity, batch_pairs,
                                          pair_score):
            out[i0:i1] = s
        return out

    @torch.no_grad()
    def diffsim_score(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, similarity, seed):
        """Same contract as the reference's ``diffsim_DiT.diffsim_score`` (diffsim/diffsim_dit.py:74-142)."""
        (latA, latB), nA, nB = path_latents(self, [(image_A, image_B)], (0, 1), img_size, seed, 1, hip_vae=False)
        return self.score_latent_pairs(latA, latB, nA, nB, target_layer[0], target_step, similarity)

    @torch.no_grad()
    def similarity_maps(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, similarity, seed):
        """:meth:`diffsim_score` with the per-token terms on both images' grids (a maps.SimilarityMaps of one pair)."""
        (latA, latB), nA, nB = path_latents(self, [(image_A, image_B)], (0, 1), img_size, seed, 1, hip_vae=False)
        return self.score_latent_pair_maps(latA, latB, nA, nB, target_layer[0], target_step, similarity)

    @torch.no_grad()
    def score_latent_pair_maps(self, latA, latB, noiseA, noiseB, target_layer: int, target_step: int, similarity="cosine",
                               batch_pairs: int = 32):
        """Maps of the pairs of :meth:`score_latent_pairs` (maps.score_latent_pair_maps)."""
        return maps.score_latent_pair_maps(self, latA, latB, noiseA, noiseB, None, "none", [int(target_layer)], target_step, similarity,
                                           batch_pairs)

    def text_region_score(self, *args, **kwargs):
        """DiT is class-conditional: it has no prompt and no cross-attention, so no text-guided regions."""
        raise NotImplementedError("diffsim_DiT has no text conditioning (a class-conditional model without cross-attention): "
                                  "text-guided regions need --metric diffsim or diffsim_xl")

    text_attention_map = text_region_score

    @torch.no_grad()
    def score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, target_layer: int, target_step: int, batch_pairs: int = 32):
        """Alignments of the pairs of :meth:`score_latent_pairs` (align.score_latent_pair_alignment)."""
        return align.score_latent_pair_alignment(self, latA, latB, noiseA, noiseB, None, "none", [int(target_layer)], target_step,
                                                 batch_pairs)

    @torch.no_grad()
    def score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, layers, target_step: int, similarity="cosine",
                                batch_pairs: Optional[int] = None) -> torch.Tensor:
        """(n_taps, n) scores: row t is :meth:`score_latent_pairs` at layers[t] (sweep.score_latent_pairs_taps)."""
        return sweep.score_latent_pairs_taps(self, latA, latB, noiseA, noiseB, None, layers, target_step, similarity, batch_pairs)

    @torch.no_grad()
    def score_pairs_taps(self, pairs, img_size, layers, target_step, similarity="cosine", seed=2333) -> torch.Tensor:
        """(n_taps, len(pairs)) scores of (A, B) path pairs, the images encoded once for all blocks (sweep.score_path_pairs_taps)."""
        return sweep.score_path_pairs_taps(self, pairs, img_size, None, layers, target_step, similarity, seed)
