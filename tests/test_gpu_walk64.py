"""The 16-bit executor walks against float64 at every tap (tests/_walk64.py: ref64, ref16, the two metrics, the bound
metric(engine) <= MARGIN x metric(ref16) per tap, per q / k / v, per metric).  The kernel families each have their float64 test; this
file holds what exists only in the walks that string them together -- arena discipline, buffer aliasing, leading dimensions,
skip-concat order, which launch a tap's q / k / v come from, per-image context offsets -- in the production modes, bf16 and fp16,
where the fused launches run (ff_fused_*, ln_linear_*, gn_linear_*, the all-fused transformer without its LayerNorm buffer, the tapped
q | k | v launch).  tests/test_walk64_host.py shows on the CPU which defects the bound sees.

  * SD1.5's channel plan at 16 x 16 and 32 x 32 latents, the smallest at which Walk::rowres_level holds (HW = 256 at the 320-channel
    level; at 32 also at the 640-channel level, and HW = 1024 at 320 channels): all seven taps from one forward (features_taps) and
    one at a time (features: the walk that ends in the tapped block), 3 distinct images, fusion masks DSIM_FUSE_ALL and 0, one case
    with a prompt per image (a context table).  The profile records must show the fused families inside the fused walk, the
    640-channel row-resident projections at 32, and none of them under mask 0: a walk that fell back to the unfused chain fails.
  * SDXL's channel plan with depths (1, 2, 2) at a 32 x 32 latent: taps across transformer blocks, linear projections, the text_time
    embedding (one time embedding per CFG half).
  * DiT-XL/2's width and heads (1152, 16 x 72), depth 3, 16 x 16 latent, every block a tap; bf16 also with fp8 (e4m3) attention,
    which has its own margin over the same ref16 and must differ from the plain walk.
  * The SD1.5 VAE encoder at 64 and 128 px, two images: the moments under the same metrics.

MEASURED worst engine / ref16 ratio over taps, tensors and both metrics, per (model, dtype, fusion mask); one MI355X, 2026-10-21,
the sweep and the one-tap walks alike (they are bit-identical).  Every one is below MARGIN = 2, so MARGIN stays where it started; the
engine sits at or below the reference's own 16-bit walk, as a walk that rounds at fewer points should:
  SD1.5 plan, side 16     bf16: FUSE_ALL 0.88, mask 0 0.89, prompt per image 0.86     fp16: FUSE_ALL 0.90, mask 0 0.92, per image 0.90
  SD1.5 plan, side 32     bf16: FUSE_ALL 0.91, mask 0 0.89                            fp16: FUSE_ALL 0.91, mask 0 0.91
  SDXL plan, side 32      bf16: 1.00                                                  fp16: 0.94
  DiT 1152 x 3, side 16   bf16: 0.75; with fp8 attention 0.94 (MARGIN_FP8 = 2)        fp16: 0.73
  VAE SD1.5               bf16: 0.88 at 64 px, 0.78 at 128 px                         fp16: 1.04 at 64 px, 0.86 at 128 px
(ref16 itself: 0.9-1.6 % rms in bf16, 0.1-0.2 % in fp16 at the U-Net taps; 1.3-1.4 % / 0.17 % for the VAE moments.)
"""
import dataclasses
import functools

import pytest
import torch

from diffsim_amd import config as C, synth as S
from tests import _walk64 as W

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
MARGIN_FP8 = W.MARGIN       # the DiT's e4m3 attention over the same ref16: measured 0.94 (0.83 / 0.94 behind one / two fp8 attentions)
N_IMG = 3
FUSED = ("ff_fused_", "ln_linear_", "gn_linear_")


def _dn(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f16"


def _images(cfg, n):
    lat = torch.cat([S.make_pair_latents(cfg, i)[0] for i in range(n)])
    nz = S.draw_pair_noise(2334, lat[:1].shape)
    return lat, torch.cat([nz[2 + i % 2] for i in range(n)])


def _engine_rows(f):
    """the engine's (q, k, v) [n][2][N][C] -> [2n][N][C] float64 on the host"""
    return tuple(t.reshape(-1, t.shape[-2], t.shape[-1]).cpu().double() for t in f)


def _hold(what, got, ref16, ref64, margin=W.MARGIN):
    rs = W.ratios(got, ref16, ref64)
    print(f"\nWALK64 {what}: worst x{W.worst(rs):.2f}  " + "  ".join(f"{t} x{W.worst(rs, t):.2f}" for t in ref64))
    bad = W.violations(rs, margin)
    assert not bad, (what, [str(r) for r in bad])
    return W.worst(rs)


def _profiled(eng, fn):
    eng.profile(True)
    try:
        out = fn()
        recs = [(fam, shape) for fam, _fl, _by, _ms, shape in eng.profile_records(detail=True)]
    finally:
        eng.profile(False)
    return out, recs


# ---- SD1.5's channel plan ------------------------------------------------------------------------------------------------------
SD15_TAPS = {"d0": ("down_blocks", 0), "d1": ("down_blocks", 1), "d2": ("down_blocks", 2), "m": ("mid_blocks", 0),
             "u0": ("up_blocks", 0), "u1": ("up_blocks", 1), "u2": ("up_blocks", 2)}           # in execution order


@functools.lru_cache(maxsize=None)
def _sd15_state():
    cfg = C.UNetConfig(sample_size=16)
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("conv_norm_out", "conv_out"))]
    return S.make_state_dict(cfg, seed=0, keys=keys)


class _SD15:
    """One dtype's oracle pair (float64 and native 16-bit, one weight set for every latent side), its references per (side, prompts)
    and its scorers per fusion mask."""

    def __init__(self, dtype):
        from oracle import cpu_ref as R
        self.R, self.dtype, self.sd = R, dtype, _sd15_state()
        ew = W.engine_weights(self.sd, dtype)
        self.m64 = W.oracle_unet(R, R.UNetConfig(sample_size=16), ew, dtype=torch.float64)
        self.m16 = W.oracle_unet(R, R.UNetConfig(sample_size=16), ew, dtype=dtype)
        self._refs, self._ds = {}, {}

    def inputs(self, side, mixed):
        cfg = C.UNetConfig(sample_size=side)
        lat, nz = _images(cfg, N_IMG)
        ctxs = [S.make_context(cfg, seed=100 + i) for i in range(N_IMG)] if mixed else S.make_context(cfg)
        return cfg, lat, nz, ctxs

    def refs(self, side, mixed=False):
        if (side, mixed) not in self._refs:
            cfg, lat, nz, ctxs = self.inputs(side, mixed)
            batch = W.unet_batch(cfg, lat, nz, ctxs)
            self._refs[(side, mixed)] = (W.unet_walk(self.R, self.m64, batch, SD15_TAPS, self.dtype),
                                         W.unet_walk(self.R, self.m16, batch, SD15_TAPS, self.dtype))
        return self._refs[(side, mixed)]

    def scorer(self, mask):
        from diffsim_amd.diffsim import DiffSim
        if mask not in self._ds:
            self._ds[mask] = DiffSim(torch_dtype=self.dtype, device="cuda", unet_config=C.UNetConfig(sample_size=16),
                                     state_dict=self.sd, fusion=mask)
        return self._ds[mask]


@pytest.fixture(scope="module", params=DTYPES, ids=_dn)
def sd15(request):
    yield _SD15(request.param)
    torch.cuda.empty_cache()


def _sd15_walks(sd15, side, mask, mixed=False):
    """features_taps over all seven taps, profiled, and features at each tap alone, both held to the bound; returns the sweep's
    profile records"""
    ref64, ref16 = sd15.refs(side, mixed)
    _, lat, nz, ctxs = sd15.inputs(side, mixed)
    ds = sd15.scorer(mask)
    taps = list(SD15_TAPS.values())
    ds.features_taps(lat[:1], nz[:1], ctxs[0] if mixed else ctxs, taps[:1], W.STEP)          # (creates the engine)
    got, recs = _profiled(ds._base, lambda: ds.features_taps(lat, nz, ctxs, taps, W.STEP))
    what = f"sd15 side {side} {_dn(sd15.dtype)} mask {mask}" + (" prompt per image" if mixed else "")
    _hold(what + " sweep", {n: _engine_rows(f) for n, f in zip(SD15_TAPS, got)}, ref16, ref64)
    one = {n: _engine_rows(ds.features(lat, nz, ctxs, b, l, W.STEP)) for n, (b, l) in SD15_TAPS.items()}
    _hold(what + " one tap", one, ref16, ref64)
    return recs


@pytest.mark.parametrize("side", [16, 32])
def test_sd15_fused_walk(sd15, side):
    from diffsim_amd import _lib
    recs = _sd15_walks(sd15, side, _lib.FUSE_ALL)
    fams = [f for f, _ in recs]
    dn = _dn(sd15.dtype)
    for fam in FUSED:
        assert fam + dn in fams, (fam, sorted(set(fams)))
    # the 640-channel row-resident projections (LayerNorm- and GroupNorm-fronted): where the 640-channel level has HW % 128 == 0
    wide = [(f, s) for f, s in recs if f.startswith(("ln_linear_", "gn_linear_")) and s.endswith("K640")]
    assert bool(wide) == (side == 32), wide
    if side == 32:
        assert {f for f, _ in wide} == {"ln_linear_" + dn, "gn_linear_" + dn}
    # the tapped q | k | v projection as one launch: N = 3 C
    assert any(f.startswith("gemm_") and " N960 K320" in s for f, s in recs)


@pytest.mark.parametrize("side", [16, 32])
def test_sd15_unfused_walk(sd15, side):
    recs = _sd15_walks(sd15, side, 0)
    assert not [f for f, _ in recs if f.startswith(FUSED)]


def test_sd15_prompt_per_image(sd15):
    """three images, three prompts: a context table, each batch element's K | V rows at its own offset"""
    from diffsim_amd import _lib
    recs = _sd15_walks(sd15, 16, _lib.FUSE_ALL, mixed=True)
    assert any(f.startswith("ctx_gather_") for f, _ in recs)
    # and the bound does tell the prompts apart: the one-prompt walk of the same images lies far outside it
    ref64, ref16 = sd15.refs(16, True)
    same64, _ = sd15.refs(16, False)
    assert {r.tap for r in W.violations(W.ratios(same64, ref16, ref64))} == set(SD15_TAPS)


# ---- SDXL's channel plan -------------------------------------------------------------------------------------------------------
SDXL_TAPS = {"d010": ("down_blocks", [0, 1, 0]), "d101": ("down_blocks", [1, 0, 1]), "m01": ("mid_blocks", [0, 1]),
             "u010": ("up_blocks", [0, 1, 0]), "u021": ("up_blocks", [0, 2, 1]), "u100": ("up_blocks", [1, 0, 0]),
             "u121": ("up_blocks", [1, 2, 1])}                                                # in execution order


@functools.lru_cache(maxsize=None)
def _sdxl_state():
    cfg = dataclasses.replace(C.SDXL, depth_per_level=(1, 2, 2), sample_size=32)
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("up_blocks.2", "conv_norm_out", "conv_out"))]
    return cfg, S.make_state_dict(cfg, seed=0, keys=keys)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_sdxl_walk(dtype):
    from oracle import cpu_ref as R
    from diffsim_amd.diffsim_xl import diffsim_xl
    cfg, sd = _sdxl_state()
    rcfg = dataclasses.replace(R.SDXL, depth_per_level=(1, 2, 2), sample_size=32)
    ctx, pooled = S.make_context(cfg), S.make_pooled(cfg)
    g = torch.Generator("cpu").manual_seed(2802)
    lat = torch.randn((N_IMG, 4, 32, 32), generator=g)
    nz = torch.randn((N_IMG, 4, 32, 32), generator=g)
    ew = W.engine_weights(sd, dtype)
    batch = W.unet_batch(cfg, lat, nz, ctx, pooled=pooled)
    ref64 = W.unet_walk(R, W.oracle_unet(R, rcfg, ew, dtype=torch.float64), batch, SDXL_TAPS, dtype)
    ref16 = W.unet_walk(R, W.oracle_unet(R, rcfg, ew, dtype=dtype), batch, SDXL_TAPS, dtype)
    del ew
    xl = diffsim_xl(dtype, "cuda", unet_config=cfg, state_dict=sd)
    taps = list(SDXL_TAPS.values())
    xl.features_taps(lat[:1], nz[:1], ctx, pooled, taps[:1], W.STEP)
    got, recs = _profiled(xl._base, lambda: xl.features_taps(lat, nz, ctx, pooled, taps, W.STEP))
    _hold(f"sdxl side 32 {_dn(dtype)} sweep", {n: _engine_rows(f) for n, f in zip(SDXL_TAPS, got)}, ref16, ref64)
    one = {n: _engine_rows(xl.features(lat, nz, ctx, pooled, b, l, W.STEP)) for n, (b, l) in SDXL_TAPS.items()}
    _hold(f"sdxl side 32 {_dn(dtype)} one tap", one, ref16, ref64)
    # 640 channels at HW = 256: the row-resident projections run here too (SDXL has no 320-channel attention, so no ff_fused)
    assert {f for f, s in recs if s.endswith("K640")} >= {"ln_linear_" + _dn(dtype), "gn_linear_" + _dn(dtype)}


# ---- DiT -----------------------------------------------------------------------------------------------------------------------
DIT_LAYERS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _dit_state():
    cfg = C.DiTConfig(input_size=16, depth=3)                       # DiT-XL/2's width and heads: 1152, 16 x 72
    return cfg, S.make_state_dict(cfg, seed=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_dit_walk(dtype):
    from oracle import cpu_ref as R
    from diffsim_amd import scheduler as sched
    from diffsim_amd.diffsim_dit import diffsim_DiT
    cfg, sd = _dit_state()
    assert (cfg.hidden_size, cfg.num_heads) == (1152, 16)
    rcfg = R.DiTConfig(input_size=16, depth=3)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(N_IMG, 4, 16, 16, generator=g)
    nz = torch.randn(N_IMG, 4, 16, 16, generator=g)
    sa, sb = sched.noise_coefficients(W.STEP)
    xt = sa * lat.double() + sb * nz.double()
    ew = W.engine_weights(sd, dtype)
    walk = lambda m: W.dit_qkv_all(m, xt, sched.dit_model_timestep(W.STEP), cfg.num_classes, DIT_LAYERS)
    ref64, ref16 = walk(W.oracle_dit(R, rcfg, ew, torch.float64)), walk(W.oracle_dit(R, rcfg, ew, dtype))

    def engine_walks(fp8):
        dd = diffsim_DiT(128, W.STEP, "cuda", dit_config=cfg, state_dict=sd, torch_dtype=dtype, fp8_attention=fp8)
        sweep = dict(zip(DIT_LAYERS, (_engine_rows(f) for f in dd.features_taps(lat, nz, list(DIT_LAYERS), W.STEP))))
        one = {l: _engine_rows(dd.features(lat, nz, l, W.STEP)) for l in DIT_LAYERS}
        _, recs = _profiled(dd._engine, lambda: dd.features(lat, nz, DIT_LAYERS[-1], W.STEP))
        return sweep, one, [f for f, _ in recs]
    sweep, one, fams = engine_walks(False)
    _hold(f"dit {_dn(dtype)} sweep", sweep, ref16, ref64)
    _hold(f"dit {_dn(dtype)} one tap", one, ref16, ref64)
    assert not any(f.startswith("attention_fp8") for f in fams)
    if dtype == torch.bfloat16:                                     # (the e4m3 attention exists for bf16 handles only)
        sweep8, one8, fams8 = engine_walks(True)
        _hold("dit bf16 fp8 attention sweep", sweep8, ref16, ref64, MARGIN_FP8)
        _hold("dit bf16 fp8 attention one tap", one8, ref16, ref64, MARGIN_FP8)
        assert fams8.count("attention_fp8_d72") == 2
        assert all(torch.equal(a, b) for a, b in zip(sweep8[0], sweep[0]))          # block 0's tap lies in front of every attention
        for l in (1, 2):
            assert not any(torch.equal(a, b) for a, b in zip(sweep8[l], sweep[l])), l


# ---- VAE -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vae_state():
    return S.make_state_dict(C.VAE_SD15, seed=3)


@pytest.mark.parametrize("px", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_vae_moments(dtype, px):
    from oracle import cpu_ref as R
    from diffsim_amd.engine import VAEEncoder
    sd = _vae_state()
    images = torch.cat(S.make_image_pair(0, px))
    ew = W.engine_weights(sd, dtype)
    ref64 = {"moments": (W.vae_moments(W.oracle_vae(R, R.VAE_SD15, ew, torch.float64), images),)}
    ref16 = {"moments": (W.vae_moments(W.oracle_vae(R, R.VAE_SD15, ew, dtype), images),)}
    got = VAEEncoder(C.VAE_SD15, sd, dtype).moments(images)
    assert got.shape == (2, 8, px // 8, px // 8)
    _hold(f"vae {px} px {_dn(dtype)}", {"moments": (W.nchw_rows(got.cpu()),)}, ref16, ref64)
