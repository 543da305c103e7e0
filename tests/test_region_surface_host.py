"""The region surface is frozen: the signatures of the engine tails, of the module functions over them and of the one-pair path
methods of the three scorer kinds, as literals; and every kind resolves each path method to the one function on ``Scorer``.

The literals are ``str(inspect.signature(...))`` of the functions before the path methods moved to ``Scorer``.  diffsim_xl and
diffsim_DiT then spelled `seed` and `similarity` of eight of those methods without defaults, where DiffSim has ``seed="2333",
similarity="cosine"``.  One function cannot have both spellings, so these two kinds gained DiffSim's defaults: every call that
bound before binds the same way.  Their literals stay the old ones and are compared with those two defaults taken off
(``_sig(..., drop=...)``); positional order, names and every other default are compared exactly.
"""
import inspect

import pytest

from diffsim_amd import align, engine, maps, regions, retrieval
from diffsim_amd.diffsim import DiffSim
from diffsim_amd.diffsim_dit import diffsim_DiT
from diffsim_amd.diffsim_xl import diffsim_xl
from diffsim_amd.scorer import Scorer

ENGINE = {
    'pair_score_maps': "(q: 'torch.Tensor', k: 'torch.Tensor', v: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False)",
    'pair_score_regions': "(q: 'torch.Tensor', k: 'torch.Tensor', v: 'torch.Tensor', mask: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_counts: 'bool' = False)",
    'pair_score_weights': "(q: 'torch.Tensor', k: 'torch.Tensor', v: 'torch.Tensor', weights_u8: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_sums: 'bool' = False)",
    'pair_score_maps_regions': "(q: 'torch.Tensor', k: 'torch.Tensor', v: 'torch.Tensor', mask: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_counts: 'bool' = False)",
    'pair_score_maps_weights': "(q: 'torch.Tensor', k: 'torch.Tensor', v: 'torch.Tensor', weights_u8: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_sums: 'bool' = False)",
    'pair_align': "(q: 'torch.Tensor', k: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', grid_w: 'Optional[int]' = None, return_attention: 'bool' = False, return_status: 'bool' = False)",
    'pair_align_regions': "(q: 'torch.Tensor', k: 'torch.Tensor', mask: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', grid_w: 'Optional[int]' = None, return_attention: 'bool' = False, return_status: 'bool' = False, return_counts: 'bool' = False)",
    'pair_align_weights': "(q: 'torch.Tensor', k: 'torch.Tensor', weights_u8: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', grid_w: 'Optional[int]' = None, return_attention: 'bool' = False, return_status: 'bool' = False, return_sums: 'bool' = False)",
    'score_matrix': "(fa, fb, heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False)",
    'score_matrix_regions': "(fa, fb, mask_a: 'torch.Tensor', mask_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_counts: 'bool' = False)",
    'score_matrix_weights': "(fa, fb, weights_a: 'torch.Tensor', weights_b: 'torch.Tensor', heads: 'int', similarity: 'str' = 'cosine', return_status: 'bool' = False, return_sums: 'bool' = False)",
    'pair_region_transfer': "(q: 'torch.Tensor', k: 'torch.Tensor', weights_u8: 'torch.Tensor', idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', heads: 'int', directions: 'int' = 3, return_status: 'bool' = False)",
}
MODULES = {
    'regions.score_latent_pair_regions': "(scorer, latA, latB, noiseA, noiseB, maskA, maskB, prompt, target_block='up_blocks', target_layer=0, target_step=600, similarity='cosine', batch_pairs: 'Optional[int]' = None) -> 'torch.Tensor'",
    'regions.score_latent_pair_weights': "(scorer, latA, latB, noiseA, noiseB, weightA, weightB, prompt, target_block='up_blocks', target_layer=0, target_step=600, similarity='cosine', batch_pairs: 'Optional[int]' = None) -> 'torch.Tensor'",
    'regions.score_path_pair_regions': "(scorer, pairs: 'Sequence[Tuple[str, str]]', masks: 'Sequence[Tuple[object, object]]', img_size, prompt, target_block='up_blocks', target_layer=0, target_step=600, seed=2333, similarity='cosine', batch_pairs: 'Optional[int]' = None, hip_vae: 'bool' = True) -> 'torch.Tensor'",
    'regions.score_path_pair_weights': "(scorer, pairs: 'Sequence[Tuple[str, str]]', masks: 'Sequence[Tuple[object, object]]', img_size, prompt, target_block='up_blocks', target_layer=0, target_step=600, seed=2333, similarity='cosine', batch_pairs: 'Optional[int]' = None, hip_vae: 'bool' = True) -> 'torch.Tensor'",
    'regions.pair_token_masks': "(scorer, tap, latent_side: 'int', n: 'int', maskA, maskB)",
    'regions.pair_token_weights': "(scorer, tap, latent_side: 'int', n: 'int', weightA, weightB)",
    'maps.score_latent_pair_maps': "(scorer, latA, latB, noiseA, noiseB, prompt, target_block='up_blocks', target_layer=0, target_step=600, similarity='cosine', batch_pairs: 'Optional[int]' = None, *, maskA=None, maskB=None, soft: 'bool' = False) -> 'SimilarityMaps'",
    'maps.score_path_pair_maps': "(scorer, pairs: 'Sequence[Tuple[str, str]]', img_size, prompt, target_block='up_blocks', target_layer=0, target_step=600, seed=2333, similarity='cosine', batch_pairs: 'Optional[int]' = None, *, masks=None, hip_vae: 'bool' = True, soft: 'bool' = False) -> 'SimilarityMaps'",
    'align.score_latent_pair_alignment': "(scorer, latA, latB, noiseA, noiseB, prompt, target_block='up_blocks', target_layer=0, target_step=600, batch_pairs: 'Optional[int]' = None, *, maskA=None, maskB=None, soft: 'bool' = False) -> 'Alignment'",
    'align.score_path_pair_alignment': "(scorer, pairs: 'Sequence[Tuple[str, str]]', img_size, prompt, target_block='up_blocks', target_layer=0, target_step=600, seed=2333, batch_pairs: 'Optional[int]' = None, *, masks=None, hip_vae: 'bool' = True, soft: 'bool' = False) -> 'Alignment'",
    'retrieval.score_latent_matrix': "(scorer, latA, latB, noiseA, noiseB, prompt, target_block='up_blocks', target_layer=0, target_step=600, similarity='cosine', batch: 'Optional[int]' = None, return_status: 'bool' = False, *, masks_a=None, masks_b=None, soft: 'bool' = False)",
    'retrieval.set_weights': "(masks, n: 'int', grid, dev, name: 'str') -> 'torch.Tensor'",
}
DIFFSIM = {
    'region_score': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine')",
    'soft_region_score': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine')",
    'region_similarity_maps': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine')",
    'soft_region_similarity_maps': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine')",
    'region_alignment': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333')",
    'soft_region_alignment': "(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed='2333')",
    'exemplar_region_score': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine', rel_threshold=1.0, soft=False)",
    'transferred_region': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', rel_threshold=1.0, soft=False)",
    'text_region_score': "(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine', words=None, rel_threshold=1.0)",
    'text_attention_map': "(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed='2333')",
    'alignment': "(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed='2333')",
}
DIFFSIM_XL = {
    'region_score': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'soft_region_score': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'region_similarity_maps': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'soft_region_similarity_maps': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'region_alignment': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed)',
    'soft_region_alignment': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed)',
    'exemplar_region_score': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine', rel_threshold=1.0, soft=False)",
    'transferred_region': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', rel_threshold=1.0, soft=False)",
    'text_region_score': '(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity, words=None, rel_threshold=1.0)',
    'text_attention_map': '(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed)',
    'alignment': '(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed)',
}
DIFFSIM_DIT = {
    'region_score': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'soft_region_score': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'region_similarity_maps': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'soft_region_similarity_maps': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed, similarity)',
    'region_alignment': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed)',
    'soft_region_alignment': '(self, image_A, image_B, mask_A, mask_B, img_size, prompt, target_block, target_layer, target_step, seed)',
    'exemplar_region_score': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', similarity='cosine', rel_threshold=1.0, soft=False)",
    'transferred_region': "(self, image_A, image_B, mask_A, img_size, prompt, target_block, target_layer, target_step, seed='2333', rel_threshold=1.0, soft=False)",
    'text_region_score': '(self, *args, **kwargs)',
    'text_attention_map': '(self, *args, **kwargs)',
    'alignment': '(self, image_A, image_B, img_size, prompt, target_block, target_layer, target_step, seed)',
}

MODS = {"regions": regions, "maps": maps, "align": align, "retrieval": retrieval}
KINDS = [(DiffSim, DIFFSIM), (diffsim_xl, DIFFSIM_XL), (diffsim_DiT, DIFFSIM_DIT)]
REFUSED = {(diffsim_DiT, "text_region_score"), (diffsim_DiT, "text_attention_map")}      # DiT has no text: its own NotImplementedError


def _sig(fn, drop=()):
    """str(signature), with the defaults of the parameters in `drop` taken off"""
    s = inspect.signature(fn)
    return str(s.replace(parameters=[p.replace(default=p.empty) if p.name in drop else p for p in s.parameters.values()]))


@pytest.mark.parametrize("name", sorted(ENGINE))
def test_engine_tail_signatures(name):
    assert _sig(getattr(engine, name)) == ENGINE[name]


@pytest.mark.parametrize("name", sorted(MODULES))
def test_module_function_signatures(name):
    mod, fn = name.split(".")
    assert _sig(getattr(MODS[mod], fn)) == MODULES[name]


@pytest.mark.parametrize("cls,want", KINDS, ids=[c.__name__ for c, _ in KINDS])
def test_path_method_signatures(cls, want):
    assert sorted(want) == sorted(DIFFSIM)
    for name, literal in want.items():
        had_defaults = "seed='2333'" in literal or (cls, name) in REFUSED
        assert _sig(getattr(cls, name), () if had_defaults else ("seed", "similarity")) == literal, name
    assert want is not DIFFSIM or all("seed='2333'" in v for v in want.values())          # DiffSim's are compared exactly


@pytest.mark.parametrize("cls", [c for c, _ in KINDS], ids=[c.__name__ for c, _ in KINDS])
def test_path_methods_are_the_scorers(cls):
    for name in DIFFSIM:
        if (cls, name) in REFUSED:
            assert getattr(cls, name) is not getattr(Scorer, name)
            with pytest.raises(NotImplementedError, match="diffsim_DiT has no text conditioning"):
                getattr(cls, name)(object.__new__(cls))
        else:
            assert getattr(cls, name) is getattr(Scorer, name), name
