"""tests/_walk64.py's instrument on the CPU, no GPU: does the bound metric(walk) <= MARGIN x metric(ref16) pass an honest 16-bit walk
and fail a defective one?  ref16 -- the oracle run natively in bf16 / fp16 -- stands in for the engine, on the TINY U-Net at a
16 x 16 latent and DIT_TINY, 3 images, step 600; the defects are planted with forward hooks, each the image of a bug a walk can have
and no kernel test sees: a row block a launch never wrote, one row, the two CFG contexts swapped, a resnet that loses its time
embedding, two skip tensors popped in the wrong order, a DiT gate that is not applied.

Asserted: the clean walk passes against itself and a second honest realisation (float64 with every leaf output rounded) passes too; in
fp16 every defect fails the bound at EVERY tap behind it and passes at every tap in front of it; in bf16 the row block, the swapped
contexts, the lost time embedding, the swapped skips and the DiT gate do.  ONE zeroed token row is barely seen in bf16 in the middle
of the net (x 2.6 at the mid block against MARGIN = 2, x 25 at the first tap behind it): bf16's own rounding is as large as what one
row in 256 contributes a few blocks later, so it is asserted at the first tap behind the defect only and the factors are printed.
That is why tests/test_gpu_walk64.py runs fp16 beside bf16.  Run with -s for the measured factors (quoted in tests/_walk64.py)."""
import functools

import pytest
import torch

from diffsim_amd import config as C, synth as S
from tests import _walk64 as W

DTYPES = [torch.bfloat16, torch.float16]
N_IMG = 3
UNET_TAPS = {"d0": ("down_blocks", 0), "d1": ("down_blocks", 1), "d2": ("down_blocks", 2), "m": ("mid_blocks", 0),
             "u0": ("up_blocks", 0), "u1": ("up_blocks", 1), "u2": ("up_blocks", 2)}          # in execution order


def _images(cfg, n):
    lat = torch.cat([S.make_pair_latents(cfg, i)[0] for i in range(n)])
    nz = S.draw_pair_noise(2334, lat[:1].shape)
    return lat, nz[2].repeat(n, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def _unet(dtype):
    """(R, native 16-bit model, batch, ref64, clean ref16, leaf16) of the TINY U-Net"""
    from oracle import cpu_ref as R
    cfg = C.TINY
    sd = W.engine_weights(S.make_state_dict(cfg, seed=0), dtype)
    lat, nz = _images(cfg, N_IMG)
    batch = W.unet_batch(cfg, lat, nz, S.make_context(cfg))
    m64 = W.oracle_unet(R, R.TINY, sd, dtype=torch.float64)
    ref64 = W.unet_walk(R, m64, batch, UNET_TAPS, dtype)
    hooks = W.round_leaves(m64, dtype)
    leaf16 = W.unet_walk(R, m64, batch, UNET_TAPS, dtype)
    for h in hooks:
        h.remove()
    m16 = W.oracle_unet(R, R.TINY, sd, dtype=dtype)
    ref16 = W.unet_walk(R, m16, batch, UNET_TAPS, dtype)
    return R, m16, batch, ref64, ref16, leaf16


DIT_LAYERS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _dit(dtype):
    from oracle import cpu_ref as R
    from diffsim_amd import scheduler as sched
    cfg = C.DIT_TINY
    sd = W.engine_weights(S.make_state_dict(cfg, seed=0), dtype)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(N_IMG, 4, cfg.input_size, cfg.input_size, generator=g)
    nz = torch.randn(1, 4, cfg.input_size, cfg.input_size, generator=g)
    sa, sb = sched.noise_coefficients(W.STEP)
    xt = sa * lat.double() + sb * nz.double()
    tm = sched.dit_model_timestep(W.STEP)
    m64 = W.oracle_dit(R, R.DIT_TINY, sd, torch.float64)
    walk = lambda m: W.dit_qkv_all(m, xt, tm, cfg.num_classes, DIT_LAYERS)
    ref64 = walk(m64)
    hooks = W.round_leaves(m64, dtype)
    leaf16 = walk(m64)
    for h in hooks:
        h.remove()
    m16 = W.oracle_dit(R, R.DIT_TINY, sd, dtype)
    return m16, walk, ref64, walk(m16), leaf16


# ---- the defects: each returns the hook's handle --------------------------------------------------------------------------------
def _ff0(m):
    return m.down_blocks[0].attentions[0].transformer_blocks[0].ff


def _zero_row_block(m):
    def hook(mod, inp, out):
        out = out.clone()
        out[:, 16:32] = 0
        return out
    return _ff0(m).register_forward_hook(hook)


def _zero_one_row(m):
    def hook(mod, inp, out):
        out = out.clone()
        out[1, 5] = 0
        return out
    return _ff0(m).register_forward_hook(hook)


def _swap_contexts(m):
    attn2 = m.down_blocks[0].attentions[0].transformer_blocks[0].attn2
    return attn2.register_forward_hook(lambda mod, inp, out: out.reshape(-1, 2, *out.shape[1:]).flip(1).reshape(out.shape))


def _lose_time_embedding(m):
    return m.down_blocks[1].resnets[0].time_emb_proj.register_forward_hook(lambda mod, inp, out: out * 0)


def _swap_skips(m):
    def pre(mod, args):
        skips = list(args[1])
        assert skips[-1].shape == skips[-2].shape
        skips[-1], skips[-2] = skips[-2], skips[-1]
        return (args[0], tuple(skips)) + tuple(args[2:])
    return m.up_blocks[1].register_forward_pre_hook(pre)


def _gate_of_one(m):
    def hook(mod, inp, out):
        out = out.clone()
        d = out.shape[1] // 6
        out[:, 2 * d:3 * d] = 1
        return out
    return m.blocks[0].adaLN_modulation.register_forward_hook(hook)


# defect -> (plant, the taps in front of it -- untouched); bf16_every: seen at every tap behind it in bf16 too
UNET_DEFECTS = {
    "1 row block of 16 zeroed": (_zero_row_block, (), True),
    "2 one token row zeroed": (_zero_one_row, (), False),
    "3 cond / uncond swapped": (_swap_contexts, (), True),
    "4 time_emb_proj zeroed": (_lose_time_embedding, ("d0",), True),
    "5 two skips swapped": (_swap_skips, ("d0", "d1", "d2", "m"), True),
}


def _report(what, dtype, rs, taps):
    per_tap = {t: W.worst(rs, t) for t in taps}
    print(f"\n{what} [{str(dtype)[6:]}]: " + "  ".join(f"{t} x{f:.1f}" for t, f in per_tap.items()))
    return per_tap


@pytest.mark.parametrize("dtype", DTYPES)
def test_honest_walks_pass(dtype):
    """ref16 against itself is at 1; float64 with leaf outputs rounded -- another honest 16-bit realisation -- stays inside MARGIN."""
    R, m16, batch, ref64, ref16, leaf16 = _unet(dtype)
    assert not W.violations(W.ratios(ref16, ref16, ref64))
    rs = W.ratios(leaf16, ref16, ref64)
    _report("U-Net leaf16 / ref16", dtype, rs, UNET_TAPS)
    print("  ref16 rms per tap: " + "  ".join(f"{r.tap}.{r.tensor} {r.scale:.2e}" for r in rs if r.metric == "rms"))
    assert not W.violations(rs), [str(r) for r in W.violations(rs)]
    m16d, walk, dref64, dref16, dleaf16 = _dit(dtype)
    rs = W.ratios(dleaf16, dref16, dref64)
    _report("DiT leaf16 / ref16", dtype, rs, DIT_LAYERS)
    assert not W.violations(rs), [str(r) for r in W.violations(rs)]
    # The other way round, ref16 on leaf16's scale.  leaf16 rounds at fewer points (no rounding inside a leaf's caller: residual adds,
    # GEGLU products, SiLU, the softmax), so ref16 sits at a systematic 1.5-1.7 x of it in rms: inside MARGIN.  The row metric is the
    # maximum over ~1500 rows and scatters around that by +-25 % between realisations (1.77 with torch's own fp16 conv2d, 2.12 with
    # _walk64._conv_through_f32 at one of 42 entries): printed, and held to the ceiling MARGIN must stay below
    back = W.ratios(ref16, leaf16, ref64)
    print("  ref16 / leaf16: rms x%.2f  row x%.2f" % (max(r.ratio for r in back if r.metric == "rms"),
                                                     max(r.ratio for r in back if r.metric == "row")))
    assert not W.violations([r for r in back if r.metric == "rms"])
    assert not W.violations(back, 4.0)


@pytest.mark.parametrize("name", sorted(UNET_DEFECTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_defects_fail_the_bound(dtype, name):
    plant, in_front, bf16_every = UNET_DEFECTS[name]
    R, m16, batch, ref64, ref16, _ = _unet(dtype)
    h = plant(m16)
    try:
        got = W.unet_walk(R, m16, batch, UNET_TAPS, dtype)
    finally:
        h.remove()
    rs = W.ratios(got, ref16, ref64)
    per_tap = _report(name, dtype, rs, UNET_TAPS)
    bad = {r.tap for r in W.violations(rs)}
    behind = [t for t in UNET_TAPS if t not in in_front]
    assert not bad & set(in_front), (name, sorted(bad))                  # nothing in front of the defect moves
    for t in in_front:
        assert per_tap[t] == 1.0
    if dtype == torch.float16 or bf16_every:
        assert bad >= set(behind), (name, dtype, per_tap)
    else:
        assert behind[0] in bad, (name, dtype, per_tap)                  # one row in bf16: the first tap behind it, at least


@pytest.mark.parametrize("dtype", DTYPES)
def test_dit_gate_defect_fails_the_bound(dtype):
    m16, walk, ref64, ref16, _ = _dit(dtype)
    h = _gate_of_one(m16)
    try:
        got = walk(m16)
    finally:
        h.remove()
    rs = W.ratios(got, ref16, ref64)
    per_tap = _report("6 DiT gate_msa of block 0 set to 1", dtype, rs, DIT_LAYERS)
    bad = {r.tap for r in W.violations(rs)}
    assert per_tap[0] == 1.0 and 0 not in bad                            # block 0's tap reads the input of its attention: in front
    assert bad >= {1, 2}, per_tap


def test_the_split_follows_the_pack():
    """engine_weights(): f32-kept tensors untouched, packed ones on the dtype's grid; the VAE's fold is one network with the
    original (conv_out then quant_conv) up to the rounding of the folded weight."""
    from oracle import cpu_ref as R
    sd = S.make_state_dict(C.TINY, seed=0)
    ew = W.engine_weights(sd, torch.bfloat16)
    for k in ("conv_in.weight", "time_embedding.linear_1.weight", "down_blocks.0.resnets.0.time_emb_proj.weight",
              "down_blocks.0.resnets.0.norm1.weight", "down_blocks.0.resnets.0.conv1.bias"):
        assert torch.equal(ew[k], sd[k]), k
    for k in ("down_blocks.0.resnets.0.conv1.weight", "down_blocks.0.attentions.0.proj_in.weight",
              "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight", "down_blocks.1.resnets.0.conv_shortcut.weight"):
        assert torch.equal(ew[k], sd[k].bfloat16().float()) and not torch.equal(ew[k], sd[k]), k
    dsd = S.make_state_dict(C.DIT_TINY, seed=0)
    dw = W.engine_weights(dsd, torch.float16)
    for k in ("pos_embed", "x_embedder.proj.weight", "y_embedder.embedding_table.weight", "t_embedder.mlp.0.weight",
              "blocks.0.adaLN_modulation.1.weight", "blocks.0.attn.qkv.bias"):
        assert torch.equal(dw[k], dsd[k]), k
    assert torch.equal(dw["blocks.0.attn.qkv.weight"], dsd["blocks.0.attn.qkv.weight"].half().float())
    vsd = S.make_state_dict(C.VAE_TINY, seed=3)
    a, _ = S.make_image_pair(0, 32)
    plain = {k: (v.float() if W.engine_keeps_f32(k, v.ndim) or k == "quant_conv.weight" else v.to(torch.float16).float())
             for k, v in vsd.items()}
    m_plain = W.oracle_vae(R, R.VAE_TINY, plain, torch.float64)
    m_fold = W.oracle_vae(R, R.VAE_TINY, W.engine_weights(vsd, torch.float16), torch.float64)
    p, f = W.vae_moments(m_plain, a), W.vae_moments(m_fold, a)
    assert p.shape == (1, 16, 8)
    assert 0 < W.metrics(f, p)[0] < 2.0 ** -11                            # one fp16 rounding of the folded weight, averaged
