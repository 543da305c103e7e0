"""The kernels that address their operands through 32-bit buffer offsets, launched at the top of the range their launchers admit
(tests/_extent.py: the method -- a periodic operand, the stored output periodic bit for bit over the whole 2 GiB, period 0 and the
rows around the byte offsets 2^30 and 2^31 held to tests/_gemm64.py's float64 bound or to tests/_rowres64.py's bits, sentinels
around the output).  tests/test_extent_host.py shows on the CPU which planted defects the checks see.

Every case takes M (or the image count) as the largest the entry point admits -- floor((0x7fffffff - 1) / row bytes), one row
less where that is a multiple of a tile height -- asserts that one row (image) more is refused with DSIM_ERR_INVALID before
anything is written, and runs bf16, fp16 and, where the family has it, f32.

  * engine.op_gemm, linear: 320 -> 320 plain, and with a residual and ldo = N + 8; the tapped q | k | v (N = 960, out_split = 320);
    GEGLU 320 -> 2560; the DiT's gated residual (1152 -> 1152, gate per 256 rows); wb_rows with w_bytes at the bound.
  * engine.op_gemm, 3x3 conv (period: 2 images): 320 -> 320 at 64 x 64, plain and residual; 640 -> 640 at 32 x 32 (force_big);
    stride 2 from 64 x 64; the upsample from 32 x 32 at 640 channels (the OUTPUT at the bound); bias2 at side 14 (196-row images,
    a ragged last tile); 128 -> 128 at 256 x 256 with gn_part (16-bit), the last image's partial sums against float64 sums of the
    stored output.
  * op_ff_fused (C = 320), op_ln_linear (C = 320 and 640, N = C with x at the bound, N = 3 C with the output at the bound, with and
    without the LayerNorm) on the lattice families of tests/_rowres64.py / tests/_rowlin_forms.py: period 0 equals the family's
    expected bits, every period equals period 0.  op_gn_linear (C = 320 and 640, HW = 1024, period 4 images): the first 4 images
    equal a 4-image launch bit for bit (the shape tests/test_gpu_rowlin_forms.py holds to float64), every period equals period 0.

WHAT THE PLANNERS ADMIT (read from csrc/gemm.hip, csrc/rowres.hip; asserted below through the launch records):
  * tiles.  The issue names the 128 x 80, 128 x 160 and 256 x 320 tiles at N = 320.  At M ~ 3.3 M rows the plan leaves no choice:
    tile_choice() takes 256-row tiles from 256 tiles on, and 128 x 80 exists only where 128 x 160 gives <= one tile per CU, so
    every 16-bit case here runs 256 x 320 (256 x 192 for the DiT width, 256 x 128 for the gn case) and every f32 case 128 x 160
    (128 x 128 for the gated epilogue); force_big changes nothing.  The 128-row 16-bit tiles cannot be reached within a factor
    of 50 of the bound through the product's arguments (g_force_bm is a development-build switch).
  * out_split.  check_args() refuses (N / out_split) * out_split_stride >= 0x7fffffff, so the three tapped tensors TOGETHER stay
    under 2 GiB: each holds at most ~0.67 GiB and out_split_stride cannot exceed 2^31.  The case runs at that limit (the stride
    counts the 512-element gap) and asserts the refusal one row above.
  * convs.  M = B x Hout x Wout: at power-of-two sides M is a multiple of every tile height, so only the side-14 case has a
    ragged last tile.
  * the small-batch kernel (gemm_skinny.hip) is skipped without a test: skinny_applies() takes at most max(CUs, 64 regular tiles)
    tiles of <= 128 x 128, plain / residual only (no GEGLU, no out_split), so the bound could only be reached through N x K x es.
    The largest production-shaped weight on kSkinnyTiles is SD1.5's 1280 x 23040 conv (59 MB in 16 bits): a factor 36 below the
    bound, beyond the issue's factor of 4.
  * the walks.  UNetEngine.max_images() is the bound of its planner (unet.hip workspace_bytes()); the DiT's and the VAE's planners
    are asked directly (dsim_dit_workspace_bytes, dsim_dit_taps_workspace_bytes, dsim_vae_workspace_bytes).  THE FIX OF THIS FILE'S
    FIRST RUN: the one-tap DiT planner and the VAE planner stated no image bound -- they admitted 32768 and 16384 images, whose
    activations are far beyond 2 GiB, and by the code (launch_gemm calls gemm_fill_extents) the walk would then have been refused
    by its first oversized GEMM, after earlier launches, not before.  dit_plan() and vae_plan() now refuse a dry walk whose largest
    activation reaches 0x7fffffff bytes, as unet.hip's planners do, so the planners return 0 and dsim_dit_qkv / dsim_vae_encode
    return DSIM_ERR_INVALID before anything is enqueued.  VAEEncoder.moments() cuts its batches at 1 GiB of first-level activation,
    half of what the planner admits; it runs at that size too.
  * the matrix tails carry n_a + n_b on a 65535-wide grid axis, and score_matrix_regions indexes listed rows in 32-bit ELEMENTS: a
    set of 2^31 elements (2^32 bytes in 16 bits) is refused, so the 16-bit region matrix runs one image under 4 GiB per tensor
    (past 2^31 bytes, not past 2^32; the f32 one runs past 2^32).

The walks and the score tails:
  * SD1.5's channel plan (synthetic weights, keys up to the tap), latent side 64, tap down_blocks 0, exactly max_images() images that
    repeat two distinct latents: out[i] equals out[i mod 2] and out[0:2] a two-image call, bit for bit, for q, k and v; fusion masks
    DSIM_FUSE_ALL and 0, a context table of two prompts at max_images(n_ctx=2), qkv_taps over down_blocks 0 and 1 at
    max_images_taps; one image more is refused.  The same for the DiT (1152 wide, depth 1: qkv() and qkv_taps([0]) at the bound of
    both planners) and the VAE encoder at 64 px (dsim_vae_encode at its planner's bound, moments() at its own cut).
  * q, k, v [n][2][N][H D] with image n - 1 beyond 2^32 bytes, three images filled (index 0, the one that straddles 2^31 bytes,
    n - 1), the rest left uninitialised: pair_score and pair_score_maps (cosine, mse), pair_score_regions, pair_score_weights,
    pair_align and its two region forms, pair_region_transfer, attn_features + feature_pair_score equal the same call on the
    3-image tensor bit for bit -- d = 40 at N = 1024 in all three dtypes, the persistent d = 160 core at N = 256 in 16 bits.
    (engine.attn_features cuts the images into calls, so its kernels see near offsets; feature_pair_score is the call with the far
    offset, held on attn_features' far output and once more on a far feats tensor that holds the three images' rows alone.)
    score_matrix and score_matrix_regions: one query against a gallery of period 2 whose LAST TWO images, past 2^32 bytes, are
    two further distinct images with mask rows of their own: the columns before them are periodic and equal to the 1 x 2 matrix,
    the last two equal a 1 x 2 call on those images.  (An image is a power of two bytes at this geometry, so an offset taken
    modulo 2^32 lands on an image of the same parity: the periodic part alone would not see it, the last two columns do.)

MEASURED, one MI355X, 2026-10-21, the first run of these sizes: 80 cases pass; no kernel needed a change, two planners did (above).  Per case: tile,
M or B, byte extents of A and of the output, the refusal observed one step above, the worst error / bound on the float64 rows.
  lin320  f32  128x160 M 1677721  A 2147482880 B  out 1 x 2147482880 B  refused at M 1677722  worst err/bound 0.032
  lin320  bf16 256x320 M 3355443  A 2147483520 B  out 1 x 2147483520 B  refused at M 3355444  worst err/bound 0.981
  lin320  f16  256x320 M 3355443  A 2147483520 B  out 1 x 2147483520 B  refused at M 3355444  worst err/bound 0.903
  lin320_res_ldo  f32  128x160 M 1636801  A 2095105280 B  out 1 x 2147482912 B  refused at M 1636802  worst err/bound 0.032
  lin320_res_ldo  bf16 256x320 M 3273603  A 2095105920 B  out 1 x 2147483568 B  refused at M 3273604  worst err/bound 0.968
  lin320_res_ldo  f16  256x320 M 3273603  A 2095105920 B  out 1 x 2147483568 B  refused at M 3273604  worst err/bound 0.918
  qkv320_split  f32  128x160 M 545598  A  698365440 B  out 3 x  715824576 B  refused at M 545599  worst err/bound 0.037
  qkv320_split  bf16 256x320 M 1091199  A  698367360 B  out 3 x  715826544 B  refused at M 1091200  worst err/bound 0.983
  qkv320_split  f16  256x320 M 1091199  A  698367360 B  out 3 x  715826544 B  refused at M 1091200  worst err/bound 0.904
  geglu320  f32  128x128 M 419430  A  536870400 B  out 1 x 2147481600 B  refused at M 419431  worst err/bound 0.019
  geglu320  bf16 256x256 M 838860  A  536870400 B  out 1 x 2147481600 B  refused at M 838861  worst err/bound 0.963
  geglu320  f16  256x256 M 838860  A  536870400 B  out 1 x 2147481600 B  refused at M 838861  worst err/bound 0.798
  dit_gate  f32  128x128 M 466033  A 2147480064 B  out 1 x 2147480064 B  refused at M 466034  worst err/bound 0.165
  dit_gate  bf16 256x192 M 932067  A 2147482368 B  out 1 x 2147482368 B  refused at M 932068  worst err/bound 0.980
  dit_gate  f16  256x192 M 932067  A 2147482368 B  out 1 x 2147482368 B  refused at M 932068  worst err/bound 0.969
  conv320_64  f32  128x160 B 409  A 2144337920 B  out 1 x 2144337920 B  refused at B 410  worst err/bound 0.011
  conv320_64  bf16 256x320 B 819  A 2146959360 B  out 1 x 2146959360 B  refused at B 820  worst err/bound 0.940
  conv320_64  f16  256x320 B 819  A 2146959360 B  out 1 x 2146959360 B  refused at B 820  worst err/bound 0.665
  conv320_64_res  f32  128x160 B 409  A 2144337920 B  out 1 x 2144337920 B  refused at B 410  worst err/bound 0.012
  conv320_64_res  bf16 256x320 B 819  A 2146959360 B  out 1 x 2146959360 B  refused at B 820  worst err/bound 0.926
  conv320_64_res  f16  256x320 B 819  A 2146959360 B  out 1 x 2146959360 B  refused at B 820  worst err/bound 0.756
  conv640_32_big  f32  128x160 B 819  A 2146959360 B  out 1 x 2146959360 B  refused at B 820  worst err/bound 0.007
  conv640_32_big  bf16 256x320 B 1638  A 2146959360 B  out 1 x 2146959360 B  refused at B 1639  worst err/bound 0.893
  conv640_32_big  f16  256x320 B 1638  A 2146959360 B  out 1 x 2146959360 B  refused at B 1639  worst err/bound 0.522
  conv320_64_s2  f32  128x160 B 409  A 2144337920 B  out 1 x  536084480 B  refused at B 410  worst err/bound 0.010
  conv320_64_s2  bf16 256x320 B 819  A 2146959360 B  out 1 x  536739840 B  refused at B 820  worst err/bound 0.911
  conv320_64_s2  f16  256x320 B 819  A 2146959360 B  out 1 x  536739840 B  refused at B 820  worst err/bound 0.661
  conv640_up32  f32  128x160 B 204  A  534773760 B  out 1 x 2139095040 B  refused at B 205  worst err/bound 0.009
  conv640_up32  bf16 256x320 B 409  A  536084480 B  out 1 x 2144337920 B  refused at B 410  worst err/bound 0.858
  conv640_up32  f16  256x320 B 409  A  536084480 B  out 1 x 2144337920 B  refused at B 410  worst err/bound 0.550
  conv320_14_bias2  f32  128x160 B 8559  A 2147281920 B  out 1 x 2147281920 B  refused at B 8560  worst err/bound 0.009
  conv320_14_bias2  bf16 256x320 B 17119  A 2147407360 B  out 1 x 2147407360 B  refused at B 17120  worst err/bound 0.918
  conv320_14_bias2  f16  256x320 B 17119  A 2147407360 B  out 1 x 2147407360 B  refused at B 17120  worst err/bound 0.657
  conv128_256_gn  bf16 256x128 B 127  A 2130706432 B  out 1 x 2130706432 B  refused at B 128  worst err/bound 0.959
  conv128_256_gn  f16  256x128 B 127  A 2130706432 B  out 1 x 2130706432 B  refused at B 128  worst err/bound 0.835
  wb_rows  f32  128x128 M 8192, wb_stride 306483776: w_bytes 2147483584  refused at wb_stride 306483792  worst err/bound 0.027
  wb_rows  bf16 128x128 M 8192, wb_stride 306633568: w_bytes 2147483552  refused at wb_stride 306633584  worst err/bound 0.965
  wb_rows  f16  128x128 M 8192, wb_stride 306633568: w_bytes 2147483552  refused at wb_stride 306633584  worst err/bound 0.865
  op_ff_fused  bf16, f16: M 3355443, x and out 2147483520 B, refused at M 3355444; bit for bit on the lattice family
  op_ln_linear bf16, f16, with and without LayerNorm, bit for bit:  C 320 N 320: M 3355443 (x, out 2147483520 B; refused at 3355444)
      C 320 N 960: M 1118481 (out 2147483520 B; 1118482)   C 640 N 640: M 1677721 (x, out 2147482880 B; 1677722)
      C 640 N 1920: M 559240 (out 2147481600 B; 559241)
  op_gn_linear bf16, f16, HW 1024, bit for bit:  C 320: B 3276 (2146959360 B; refused at 3277)   C 640: B 1638 (2146959360 B; 1639)
  unet, side 64, tap d0, bf16 and f16:  FUSE_ALL max_images 136 (q, k, v 713031680 B each; 137 refused)   mask 0: 102 (103 refused)
      two prompts: max_images(n_ctx=2) 136 (137 refused)   sweep d0 + d1: max_images_taps 136 (137 refused)
  dit 1152 x 1, 64 tokens: 1820 images through qkv() and qkv_taps([0]) (q, k, v 536739840 B each; 1821 refused by both planners;
      before the fix the one-tap planner admitted 32768)   vae 64 px: 2047 images (2048 refused; before the fix 16384 admitted),
      moments() at its cut of 1024 per call
  pair tails: 16-bit n 3278, images at 0 / 1638 / 3277, the last starts at byte 4295229440; f32 n 1640, images at 0 / 819 / 1639, the
      last starts at byte 4296540160: every entry point bit for bit
  matrix tails (N 256, 8 heads of 16): score_matrix over 32771 images (4295360512 B per tensor) in 16 bits, 16387 (4295753728 B) in
      f32; score_matrix_regions over 16387 in f32, in 16 bits refused at 32771 (2^31 elements) and run over 32767 (4294836224 B)
Families skipped: the small-batch GEMM kernel (above: a factor 36 from the bound); the 128-row 16-bit GEMM tiles (unreachable at
these M); f32 for the row-resident kernels and the gn_part epilogue, which are 16-bit only in the product.
"""
import math

import pytest
import torch

from tests import _extent as E
from tests import _gemm64 as G
from tests import _rowlin_forms as F
from tests import _rowres64 as R

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}
SENT = -12345.0
GAP = 512                    # elements between out_split tensors
P = E.PERIOD
REFUSED = r"status -1\b"     # DSIM_ERR_INVALID as _lib.check() words it


def _eng():
    from diffsim_amd import engine
    return engine


def _err():
    from diffsim_amd import _lib
    return _lib.DsimError


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _gen(shape, g, scale=1.0):
    return torch.randn(*shape, generator=g, device="cuda") * scale


def _lin(C0, N, **kw):
    return dict(C0=C0, N=N, **kw)


def _conv(H, W, C0, N, **kw):
    return dict(conv=dict(stride=kw.pop("stride", 1), ups=kw.pop("ups", 0), pad=1), H=H, W=W, C0=C0, N=N, **kw)


# name -> problem, in tests/test_gpu_gemm64.py's keys; tile: the (bm, bn) the plan must take in (16-bit, f32)
CASES = {
    "lin320": _lin(320, 320, tile=((256, 320), (128, 160))),
    "lin320_res_ldo": _lin(320, 320, res=1, ldo_pad=8, tile=((256, 320), (128, 160))),
    "qkv320_split": _lin(320, 960, split=320, ldo_pad=8, tile=((256, 320), (128, 160))),
    "geglu320": _lin(320, 2560, geglu=1, tile=((256, 256), (128, 128))),
    "dit_gate": _lin(1152, 1152, gate=256, res=1, tile=((256, 192), (128, 128))),
    "conv320_64": _conv(64, 64, 320, 320, tile=((256, 320), (128, 160))),
    "conv320_64_res": _conv(64, 64, 320, 320, res=1, tile=((256, 320), (128, 160))),
    "conv640_32_big": _conv(32, 32, 640, 640, big=1, tile=((256, 320), (128, 160))),
    "conv320_64_s2": _conv(64, 64, 320, 320, stride=2, tile=((256, 320), (128, 160))),
    "conv640_up32": _conv(32, 32, 640, 640, ups=1, tile=((256, 320), (128, 160))),
    "conv320_14_bias2": _conv(14, 14, 320, 320, bias2=196, tile=((256, 320), (128, 160))),
    "conv128_256_gn": _conv(256, 256, 128, 128, gn=1, tile=((256, 128), None)),
}
NOTES = {}                   # (case, dtype) -> the line of the MEASURED table


def _runs():
    return [(n, dt) for n, c in CASES.items() for dt in DT if not (c.get("gn") and dt == "f32")]


def _setup(name, dt):
    """the case's geometry at the bound and its operands, allocated for the refused size (one row / image more)"""
    c, dtype = CASES[name], DT[dt]
    es = dtype.itemsize
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    N, C0 = c["N"], c["C0"]
    geglu, split = c.get("geglu", 0), c.get("split", 0)
    ncol = N // 2 if geglu else N
    cols = split or ncol
    ldo = cols + c.get("ldo_pad", 0)
    nout = N // split if split else 1
    s = dict(c=c, dtype=dtype, es=es, N=N, C0=C0, ncol=ncol, cols=cols, ldo=ldo, nout=nout, conv=c.get("conv"))
    if s["conv"]:
        H, W = c["H"], c["W"]
        Ho, Wo = G.conv_out_hw(H, W, **s["conv"])
        hw = Ho * Wo
        img_in, img_out = H * W * C0 * es, hw * ldo * es
        B, Br = E.bound_images(max(img_in, img_out))
        s.update(B=B, Br=Br, hw=hw, M=B * hw, Mr=Br * hw, period=2 * hw, K=9 * C0, rb_in=img_in // hw, rb_out=ldo * es)
        assert img_in % hw == 0
        s["a_full"] = E.periodic_rows(_gen((2, H, W, C0), g).to(dtype), Br)
        s["w"] = _gen((N, C0, 3, 3), g, 1 / math.sqrt(s["K"]))
    else:
        rb = max(C0, ldo) * es
        M, Mr = E.bound_rows(rb, fixed_bytes=GAP * es if split else 0, copies=nout)
        s.update(M=M, Mr=Mr, period=P, K=C0, rb_in=C0 * es, rb_out=ldo * es)
        s["a_full"] = E.periodic_rows(_gen((P, C0), g).to(dtype), Mr)
        s["w"] = _gen((N, C0), g, 1 / math.sqrt(C0))
    kw = dict(conv=s["conv"], bias=_gen((N,), g, 0.5), epi="geglu" if geglu else ("residual" if c.get("res") else "none"), ldo=ldo,
              force_big=c.get("big", 0))
    if c.get("bias2"):
        kw.update(bias2=_gen((N,), g, 0.5), rows_per_batch=c["bias2"])
    if c.get("gate"):
        kw.update(gate=_gen((ncol,), g), gate2=_gen((ncol,), g), rows_per_batch=c["gate"])
        assert P % (2 * c["gate"]) == 0                                  # the row parity is periodic too
    if c.get("res"):
        kw["residual"] = E.periodic_rows(_gen((s["period"], ldo), g).to(dtype), s["Mr"])
    s["kw"] = kw
    n, _ = E.out_layout(s["Mr"], ldo, nout, GAP)
    s["out"] = torch.full((n,), SENT, dtype=dtype, device="cuda")
    return s


def _args(s, refused):
    """(a0, out, keyword arguments) at M rows, or at the refused size"""
    M = s["Mr"] if refused else s["M"]
    kw = dict(s["kw"])
    n, per = E.out_layout(M, s["ldo"], s["nout"], GAP)
    if s["c"].get("split"):
        kw.update(out_split=s["c"]["split"], out_split_stride=per * s["es"])
    if s["c"].get("gn"):
        kw.update(gn_part=torch.full((M // s["hw"], s["hw"] // 64, s["N"] // 4, 2), float("nan"), device="cuda"), gn_hw=s["hw"])
    a0 = s["a_full"][:(s["Br"] if refused else s["B"])] if s["conv"] else s["a_full"][:M]
    return a0, s["out"][:n], kw, per


def _check_gn_last_image(s, out, kw):
    """tests/test_gpu_gemm64.py's _check_gn, the partial sums of the LAST image (its rows end at the bound)"""
    B, hw, N = s["B"], s["hw"], s["N"]
    part = kw["gn_part"]
    assert torch.isfinite(part).all(), "gn_part slots left unwritten"
    x = out[(B - 1) * hw * s["ldo"]:B * hw * s["ldo"]].view(hw, s["ldo"])[:, :N].double().view(hw // 64, 64, N // 4, 4)
    s1, s2, a1 = x.sum((1, 3)), (x * x).sum((1, 3)), x.abs().sum((1, 3))
    assert ((part[B - 1, ..., 0].double() - s1).abs() <= 256 * G.U32 * a1 + 1e-30).all(), "gn_part sums of the last image"
    assert ((part[B - 1, ..., 1].double() - s2).abs() <= 256 * G.U32 * s2 + 1e-30).all(), "gn_part sums of squares of the last image"
    assert torch.equal(part[2:B - (B % 2)].view(-1, 2, *part.shape[1:]), part[:2].unsqueeze(0).expand(B // 2 - 1, *part[:2].shape)), \
        "gn_part is not periodic in the images"


@pytest.mark.parametrize("name,dt", _runs())
def test_gemm_at_the_bound(name, dt):
    eng = _eng()
    s = _setup(name, dt)
    c, M, ldo, cols, nout, period, es = s["c"], s["M"], s["ldo"], s["cols"], s["nout"], s["period"], s["es"]
    # one row (image) more: refused, nothing written
    a0r, outr, kwr, _ = _args(s, True)
    with pytest.raises(_err(), match=REFUSED):
        eng.op_gemm(a0r, s["w"], outr, **kwr)
    torch.cuda.synchronize()
    assert bool((s["out"] == torch.tensor(SENT, dtype=s["dtype"], device="cuda")).all()), "the refused launch wrote"
    del a0r, outr, kwr
    a0, out, kw, per = _args(s, False)
    rec = eng.op_gemm(a0, s["w"], out, **kw)
    torch.cuda.synchronize()
    wrote = E.sentinels_ok(out, M, ldo, cols, nout, per, SENT)
    assert wrote is None, f"written outside the output: {wrote}"
    # (the buffer was allocated for the refused size: what lies behind the guard rows must stand as well)
    assert bool((s["out"][out.numel():] == torch.tensor(SENT, dtype=s["dtype"], device="cuda")).all()), "written behind the guard rows"
    tens = [out[j * per:j * per + M * ldo] for j in range(nout)]
    for j, t in enumerate(tens):
        assert bool(torch.isfinite(t.view(M, ldo)[:, :cols]).all()), f"non-finite output in tensor {j}"
        assert E.periodic_ok(t, M, ldo, period), \
            f"tensor {j}: rows {E.periodic_bad_rows(t, M, ldo, period)} differ from their image in period 0 (M = {M}, period {period})"
    # float64: period 0 as tests/test_gpu_gemm64.py subsets it, and the rows of the whole range the method names
    bnd = list(range(kw["rows_per_batch"], period, kw["rows_per_batch"])) if kw.get("rows_per_batch") else []
    bnd += [s["hw"]] if s["conv"] else []
    rows = torch.unique(torch.cat([G.row_subset(min(period, M), rec["bm"], bnd, n_random=64),
                                   E.required_rows(M, rec["bm"], (s["rb_in"], s["rb_out"]), n_random=64, seed=1)]))
    got = torch.cat([t.view(M, ldo)[rows.cuda(), :cols] for t in tens], 1)
    common = dict(conv=s["conv"], bias=kw["bias"], bias2=kw.get("bias2"), rows_per_batch=kw.get("rows_per_batch", 0), gate=kw.get("gate"),
                  gate2=kw.get("gate2"), epi=kw["epi"])
    if s["conv"]:
        # image b is image b mod 2 (a conv does not cross images; the per-half bias follows the image's parity)
        res = kw["residual"][:period] if c.get("res") else None
        ref = G.Gemm64(a0[:2], s["w"], s["dtype"], residual=res, rows=rows % period, **common)
    else:
        ref = G.Gemm64(a0, s["w"], s["dtype"], residual=kw["residual"][:M] if c.get("res") else None, rows=rows, **common)
    worst = ref.check(got, f"{name} {dt} {rec['family']}")
    if c.get("gn"):
        _check_gn_last_image(s, out, kw)
    unit = f"B {s['B']}" if s["conv"] else f"M {M}"
    NOTES[(name, dt)] = (f"{name:18s} {dt:4s} {rec['bm']}x{rec['bn']:<3d} {unit:10s} rows {M:8d}  A {a0.numel() * es:10d} B  out {nout} x "
                         f"{M * ldo * es:10d} B  refused at {'B ' + str(s['Br']) if s['conv'] else 'M ' + str(s['Mr'])}  worst err/bound {worst:.3f}")
    print("\nEXTENT " + NOTES[(name, dt)])
    # the plan's tile at this size (the module docstring: what the planners admit), and a ragged last tile wherever M can be ragged
    assert (rec["bm"], rec["bn"]) == c["tile"][1 if dt == "f32" else 0] and not rec["small"], rec
    if not s["conv"] or c.get("bias2"):
        assert M % rec["bm"] != 0, "the last M tile must be ragged"


@pytest.mark.parametrize("dt", list(DT))
def test_gemm_wb_rows_weights_at_the_bound(dt):
    """per-image weights (the VAE's P v shape: 1024-row blocks, K = 1024, N = 512) spread so that w_bytes ends at the bound: 8 blocks,
    wb_stride ~ 292 MiB; the whole output against float64"""
    eng = _eng()
    dtype = DT[dt]
    es = dtype.itemsize
    nb, wb, K, N = 8, 1024, 1024, 512
    M = nb * wb
    wmat = N * K * es
    stride = ((E.LIMIT - 1 - wmat) // (nb - 1)) // 16 * 16
    assert (nb - 1) * stride + wmat < E.LIMIT <= (nb - 1) * (stride + 16) + wmat
    g = torch.Generator(device="cuda").manual_seed(11)
    a0 = _gen((M, K), g).to(dtype)
    w = _gen((nb, N, K), g, 1 / math.sqrt(K))
    bias = _gen((N,), g, 0.5)
    out = torch.full(((M + 4) * N,), SENT, dtype=dtype, device="cuda")
    with pytest.raises(_err(), match=REFUSED):
        eng.op_gemm(a0, w, out, bias=bias, wb_rows=wb, wb_stride=stride + 16)
    torch.cuda.synchronize()
    assert bool((out == torch.tensor(SENT, dtype=dtype, device="cuda")).all()), "the refused launch wrote"
    rec = eng.op_gemm(a0, w, out, bias=bias, wb_rows=wb, wb_stride=stride)
    torch.cuda.synchronize()
    assert E.sentinels_ok(out, M, N, N, 1, M * N, SENT) is None
    worst = G.Gemm64(a0, w, dtype, bias=bias, wb_rows=wb).check(out[:M * N].view(M, N), f"wb_rows {dt} {rec['family']}")
    NOTES[("wb_rows", dt)] = (f"{'wb_rows':18s} {dt:4s} {rec['bm']}x{rec['bn']:<3d} M {M}, wb_stride {stride}: w_bytes {(nb - 1) * stride + wmat}  "
                              f"refused at wb_stride {stride + 16}  worst err/bound {worst:.3f}")
    print("\nEXTENT " + NOTES[("wb_rows", dt)])


# ---- the row-resident kernels ------------------------------------------------------------------------------------------------------
_LAT = {}


def _lattice(Cc, dt):
    """the lattice family's first P rows on the device (tests/_rowres64.py at 320 channels, tests/_rowlin_forms.py at 640)"""
    if (Cc, dt) not in _LAT:
        _LAT.clear()
        _LAT[(Cc, dt)] = R.lattice(P, DT[dt], P, "cuda") if Cc == R.C else F.lattice(P, Cc, DT[dt], P, "cuda", 3 * Cc)
    return _LAT[(Cc, dt)]


def _hold_rows(got, want0, M, what, x_row_bytes):
    """got [M][n] against the family's expected period want0 [P][n]: period 0 to the bit, every period equal to period 0, and
    required_rows() (around the byte offsets in x and in the output) to the bit once more, by index"""
    n = got.shape[1]
    R.assert_bits(got[:P], want0, what + ", period 0")
    assert E.periodic_ok(got.view(-1), M, n, P), f"{what}: rows {E.periodic_bad_rows(got.view(-1), M, n, P)} differ from period 0"
    rows = E.required_rows(M, R.TILE, (x_row_bytes, n * 2), n_random=64, seed=2).cuda()
    R.assert_bits(got[rows], want0[rows % P], what + ", the rows around 2^30 and the bound")


@pytest.mark.parametrize("dt", list(DT16))
def test_ff_fused_at_the_bound(dt):
    eng = _eng()
    t = _lattice(R.C, dt)
    M, Mr = E.bound_rows(R.C * 2)
    x = E.periodic_rows(t["x"], Mr)
    with pytest.raises(_err(), match=REFUSED):
        eng.op_ff_fused(x, *R.ff_args(t), 1e-5)
    got = eng.op_ff_fused(x[:M], *R.ff_args(t), 1e-5)
    _hold_rows(got, t["ff"], M, f"op_ff_fused M={M} {dt}", R.C * 2)
    NOTES[("ff_fused", dt)] = f"{'op_ff_fused':18s} {dt:4s} M {M}  x, out {M * R.C * 2} B  refused at M {Mr}  bit for bit"
    print("\nEXTENT " + NOTES[("ff_fused", dt)])


@pytest.mark.parametrize("dt", list(DT16))
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("Cc,Nn", [(320, 320), (320, 960), (640, 640), (640, 1920)])
def test_ln_linear_at_the_bound(Cc, Nn, ln, dt):
    eng = _eng()
    t = _lattice(Cc, dt)
    M, Mr = E.bound_rows(max(Cc, Nn) * 2)
    x = E.periodic_rows(t["x"], Mr)
    gm, bt = (t["gamma"], t["beta"]) if ln else (None, None)
    w = t["wl"][:Nn].contiguous()
    with pytest.raises(_err(), match=REFUSED):
        eng.op_ln_linear(x, gm, bt, w, 1e-5)
    got = eng.op_ln_linear(x[:M], gm, bt, w, 1e-5)
    _hold_rows(got, (t["lin_ln"] if ln else t["lin"])[:, :Nn].contiguous(), M, f"op_ln_linear C={Cc} N={Nn} ln={ln} M={M} {dt}",
               Cc * 2)
    NOTES[("ln_linear", Cc, Nn, ln, dt)] = (f"{'op_ln_linear':18s} {dt:4s} C {Cc} N {Nn:4d} ln {int(ln)} M {M}  x {M * Cc * 2} B  out {M * Nn * 2} B  "
                                            f"refused at M {Mr}  bit for bit")
    print("\nEXTENT " + NOTES[("ln_linear", Cc, Nn, ln, dt)])


@pytest.mark.parametrize("dt", list(DT16))
@pytest.mark.parametrize("Cc", [320, 640])
def test_gn_linear_at_the_bound(Cc, dt):
    eng = _eng()
    HW, PB = 1024, 4
    t = {k: v.cuda() for k, v in F.random_gn_inputs(PB, HW, Cc, DT[dt], HW + Cc).items()}
    B, Br = E.bound_images(HW * Cc * 2)
    x = E.periodic_rows(t["x"], Br)
    args = (t["gamma"], t["beta"], 32, t["w"], t["bias"], 1e-6)
    with pytest.raises(_err(), match=REFUSED):
        eng.op_gn_linear(x, *args)
    want0 = eng.op_gn_linear(t["x"], *args)
    got = eng.op_gn_linear(x[:B], *args)
    M = B * HW
    R.assert_bits(got[:PB].reshape(-1, Cc), want0.reshape(-1, Cc), f"op_gn_linear C={Cc} B={B} {dt}: the first {PB} images against a {PB}-image launch")
    assert E.periodic_ok(got.view(-1), M, Cc, PB * HW), \
        f"op_gn_linear C={Cc} B={B} {dt}: rows {E.periodic_bad_rows(got.view(-1), M, Cc, PB * HW)} differ from period 0"
    NOTES[("gn_linear", Cc, dt)] = f"{'op_gn_linear':18s} {dt:4s} C {Cc} HW {HW} B {B}  x, out {M * Cc * 2} B  refused at B {Br}  bit for bit"
    print("\nEXTENT " + NOTES[("gn_linear", Cc, dt)])


# ---- the walks at max_images() -----------------------------------------------------------------------------------------------------
# SD1.5's channel plan as tests/test_gpu_walk64.py builds it (synthetic weights, keys up to the tap), latent side 64, the tap at
# down_blocks 0: exactly max_images() images that repeat two distinct latents.  out[i] must equal out[i mod 2] bit for bit and
# out[0:2] a two-image call; max_images() + 1 is refused.
SIDE = 64
STEP = 600


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _hold_images(outs, small, n, what):
    """every tensor [n][...] of outs: images 0, 1 equal the two-image call's, image i equals image i mod 2"""
    for name, t, s2 in zip("qkv", outs, small):
        assert t.shape[0] == n and t.is_contiguous()
        assert _bits_equal(t[:2], s2), f"{what}: {name}[0:2] differs from the two-image call"
        row = t[0].numel()
        assert E.periodic_ok(t.view(-1), n, row, 2), f"{what}: {name} images {E.periodic_bad_rows(t.view(-1), n, row, 2)} differ from image i mod 2"
        assert bool(torch.isfinite(t[n - 1]).all())


def _two_latents(ch, side, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, ch, side, side, generator=g).cuda(), torch.randn(2, ch, side, side, generator=g).cuda()


@pytest.fixture(scope="module", params=list(DT16))
def unet(request):
    from diffsim_amd import config as C, scheduler as sched, synth as S
    from diffsim_amd.engine import UNetEngine
    cfg = C.UNetConfig(sample_size=SIDE)
    keys = [k for k in C.unet_param_shapes(cfg) if k.startswith(("conv_in", "time_embedding", "down_blocks.0", "down_blocks.1"))]
    eng = UNetEngine(cfg, S.make_state_dict(cfg, seed=0, keys=keys), DT[request.param], "down_blocks", 0)
    t = sched.timestep_from_index(STEP)
    eng.set_timestep(t)
    ctxs = torch.stack([S.make_context(cfg, seed=100 + i) for i in range(2)]).cuda()
    yield dict(eng=eng, dt=request.param, coef=sched.noise_coefficients(t), ctxs=ctxs)
    eng.close()
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mask", ["all", 0])
def test_unet_walk_at_max_images(unet, mask):
    from diffsim_amd import _lib
    eng, (sa, sb), ctx = unet["eng"], unet["coef"], unet["ctxs"][0]
    eng.set_fusion(_lib.FUSE_ALL if mask == "all" else 0)
    mx = eng.max_images()
    assert 16 <= mx < 4096 and eng.workspace_bytes(mx) > 0 and eng.workspace_bytes(mx + 1) == 0
    lat2, nz2 = _two_latents(4, SIDE, 7)
    lat, nz = E.periodic_rows(lat2, mx + 1), E.periodic_rows(nz2, mx + 1)
    with pytest.raises(_err()):
        eng.qkv(lat, nz, sa, sb, ctx)
    small = eng.qkv(lat2, nz2, sa, sb, ctx)
    outs = eng.qkv(lat[:mx], nz[:mx], sa, sb, ctx)
    what = f"unet {unet['dt']} fusion {mask} n {mx}"
    _hold_images(outs, small, mx, what)
    NOTES[("unet", unet["dt"], mask)] = f"{'unet d0 side 64':18s} {unet['dt']:4s} fusion {mask!s:3s} max_images {mx}: q, k, v {outs[0].numel() * 2} B each  refused at {mx + 1}"
    print("\nEXTENT " + NOTES[("unet", unet["dt"], mask)])


def test_unet_walk_with_a_context_table_at_max_images(unet):
    """two prompts: image i takes latent i mod 2 AND prompt i mod 2; the table's own max_images"""
    from diffsim_amd import _lib
    eng, (sa, sb), ctxs = unet["eng"], unet["coef"], unet["ctxs"]
    eng.set_fusion(_lib.FUSE_ALL)
    mx = eng.max_images(n_ctx=2)
    assert 16 <= mx <= eng.max_images() and eng.workspace_bytes(mx, 2) > 0 and eng.workspace_bytes(mx + 1, 2) == 0
    lat2, nz2 = _two_latents(4, SIDE, 8)
    lat, nz = E.periodic_rows(lat2, mx + 1), E.periodic_rows(nz2, mx + 1)
    with pytest.raises(_err()):
        eng.qkv(lat, nz, sa, sb, ctxs, ctx_index=[i % 2 for i in range(mx + 1)])
    small = eng.qkv(lat2, nz2, sa, sb, ctxs, ctx_index=[0, 1])
    outs = eng.qkv(lat[:mx], nz[:mx], sa, sb, ctxs, ctx_index=[i % 2 for i in range(mx)])
    _hold_images(outs, small, mx, f"unet {unet['dt']} context table n {mx}")
    # and the prompts are told apart: image 1 under prompt 0 is another tensor
    other = eng.qkv(lat2, nz2, sa, sb, ctxs, ctx_index=[0, 0])
    assert not _bits_equal(other[0][1], small[0][1])
    NOTES[("unet_ctx", unet["dt"])] = f"{'unet d0, 2 prompts':18s} {unet['dt']:4s} max_images(n_ctx=2) {mx}  refused at {mx + 1}"
    print("\nEXTENT " + NOTES[("unet_ctx", unet["dt"])])


def test_unet_tap_sweep_at_max_images(unet):
    from diffsim_amd import _lib
    eng, (sa, sb), ctx = unet["eng"], unet["coef"], unet["ctxs"][0]
    eng.set_fusion(_lib.FUSE_ALL)
    taps = [("down_blocks", 0), ("down_blocks", 1)]
    eng.set_sample_size(SIDE)
    mx = eng.max_images_taps(taps)
    assert 16 <= mx < 4096 and eng.taps_workspace_bytes(mx, taps) > 0 and eng.taps_workspace_bytes(mx + 1, taps) == 0
    lat2, nz2 = _two_latents(4, SIDE, 9)
    lat, nz = E.periodic_rows(lat2, mx + 1), E.periodic_rows(nz2, mx + 1)
    with pytest.raises(_err()):
        eng.qkv_taps(lat, nz, sa, sb, ctx, taps)
    small = eng.qkv_taps(lat2, nz2, sa, sb, ctx, taps)
    outs = eng.qkv_taps(lat[:mx], nz[:mx], sa, sb, ctx, taps)
    for (b, l), o, s2 in zip(taps, outs, small):
        _hold_images(o, s2, mx, f"unet {unet['dt']} sweep tap {b} {l} n {mx}")
    NOTES[("unet_taps", unet["dt"])] = f"{'unet sweep d0, d1':18s} {unet['dt']:4s} max_images_taps {mx}  refused at {mx + 1}"
    print("\nEXTENT " + NOTES[("unet_taps", unet["dt"])])


@pytest.mark.parametrize("dt", list(DT16))
def test_dit_walk_at_max_images(dt):
    """DiT-XL/2's width (1152, 16 heads), depth 1, a 16 x 16 latent (64 tokens).  The walk allocates its widest buffer, [M][4608],
    whatever the tap: both planners -- dsim_dit_workspace_bytes behind qkv(), dsim_dit_taps_workspace_bytes behind qkv_taps() --
    must admit exactly the batches that keep it under 2 GiB, and both entries run at that size"""
    from diffsim_amd import config as C, scheduler as sched, synth as S
    from diffsim_amd.engine import DiTEngine, _Handle
    cfg = C.DiTConfig(input_size=16, depth=1)
    assert cfg.hidden_size == 1152
    eng = DiTEngine(cfg, S.make_state_dict(cfg, seed=0), DT[dt], 0)
    eng.set_conditioning(sched.dit_model_timestep(STEP), 1, cfg.num_classes)
    sa, sb = sched.noise_coefficients(STEP)
    mx = eng.max_images_taps([0], upper=1 << 15)
    T, F_ = eng.tokens, cfg.mlp_ratio * cfg.hidden_size
    assert mx == (E.LIMIT - 1) // (2 * T * F_ * 2), mx                       # the planner's own statement of the bound
    assert eng.taps_workspace_bytes(mx, [0]) > 0 and eng.taps_workspace_bytes(mx + 1, [0]) == 0
    one_tap = lambda m: int(eng.L.dsim_dit_workspace_bytes(eng._h, m)) > 0
    assert _Handle._largest(one_tap, 1 << 15) == mx and not one_tap(mx + 1), "the one-tap planner admits a >= 2 GiB activation"
    lat2, nz2 = _two_latents(cfg.in_channels, 16, 10)
    lat, nz = E.periodic_rows(lat2, mx + 1), E.periodic_rows(nz2, mx + 1)
    with pytest.raises(_err()):
        eng.qkv_taps(lat, nz, sa, sb, [0])
    with pytest.raises(_err(), match=REFUSED):
        eng.qkv(lat, nz, sa, sb)
    small = eng.qkv_taps(lat2, nz2, sa, sb, [0])[0]
    outs = eng.qkv_taps(lat[:mx], nz[:mx], sa, sb, [0])[0]
    _hold_images(outs, small, mx, f"dit {dt} n {mx}")
    one = eng.qkv(lat[:mx], nz[:mx], sa, sb)                                  # the one-tap call at the same size: the same bits
    assert all(_bits_equal(a, b) for a, b in zip(one, outs)), "the one-tap qkv() differs from the sweep at the bound"
    del one
    NOTES[("dit", dt)] = f"{'dit 1152 x 1':18s} {dt:4s} max images {mx}, qkv() and qkv_taps([0]): q, k, v {outs[0].numel() * 2} B each  refused at {mx + 1}"
    print("\nEXTENT " + NOTES[("dit", dt)])
    eng.close()


@pytest.mark.parametrize("dt", list(DT16))
def test_vae_encoder_at_max_images(dt):
    """the SD1.5 VAE encoder at 64 px at the largest batch dsim_vae_workspace_bytes admits (every activation under 2 GiB), through
    dsim_vae_encode as VAEEncoder.moments() calls it -- moments() itself cuts its batches at half that, 1 GiB of first-level
    activation, and is run at that size and two images more (a second call) as well.  One image above the planner's bound
    dsim_vae_encode refuses with DSIM_ERR_INVALID and writes nothing"""
    from diffsim_amd import config as C, synth as S, _lib
    from diffsim_amd.engine import VAEEncoder, _Handle, _stream_ptr
    S_PX = 64
    enc = VAEEncoder(C.VAE_SD15, S.make_state_dict(C.VAE_SD15, seed=3), DT[dt])
    need = lambda m: int(enc.L.dsim_vae_workspace_bytes(enc._h, m, S_PX))
    mx = _Handle._largest(lambda m: need(m) > 0, 1 << 14)
    cut = (1 << 30) // (S_PX * S_PX * C.VAE_SD15.block_out_channels[0] * 2)
    assert cut == 1024 and cut <= mx < (1 << 14) and need(mx + 1) == 0, mx
    img2 = torch.cat(S.make_image_pair(0, S_PX)).cuda().float().contiguous()
    imgs = E.periodic_rows(img2, mx + 1)
    small = enc.moments(img2)

    def hold(out, n, what):
        assert torch.equal(out[:2].view(torch.int32), small.view(torch.int32)), f"{what}: moments[0:2] differ from the two-image call"
        assert bool(torch.isfinite(out).all())
        row = out[0].numel()
        assert E.periodic_ok(out.view(-1), n, row, 2), f"{what}: images {E.periodic_bad_rows(out.view(-1), n, row, 2)} differ from image i mod 2"

    def encode(m):
        out = torch.full((m, 2 * C.VAE_SD15.latent_channels, S_PX // 8, S_PX // 8), float("nan"), device="cuda")
        ws = enc._arena(need(mx))
        st = enc.L.dsim_vae_encode(enc._h, imgs.data_ptr(), m, S_PX, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        torch.cuda.synchronize()
        return st, out
    st, out = encode(mx + 1)
    assert st == -1 and bool(torch.isnan(out).all()), f"one image more: status {st}, must be DSIM_ERR_INVALID with nothing written"
    st, out = encode(mx)
    _lib.check(st, "dsim_vae_encode")
    hold(out, mx, f"dsim_vae_encode n {mx}")
    for n in (cut, cut + 2):
        hold(enc.moments(imgs[:n]), n, f"moments n {n}")
    NOTES[("vae", dt)] = f"{'vae sd15 64 px':18s} {dt:4s} max images {mx}  refused at {mx + 1}; moments() at its own cut, {cut} images per call"
    print("\nEXTENT " + NOTES[("vae", dt)])
    enc.close()


# ---- the score tails past 2^31 and 2^32 bytes ----------------------------------------------------------------------------------------
# q, k, v [n][2][N][H D] with n chosen so that image n - 1 starts beyond 2^32 bytes; only three images are filled -- index 0, the
# image that straddles 2^31 bytes and n - 1 -- and every entry point must return, bit for bit, what it returns on the 3-image tensor
# that holds those images, with the indices mapped (tail_core.h, align_core.h, attn160.hip: 64-bit image offsets).
TAIL_SHAPES = [("bf16", 1024, 8, 40), ("f16", 1024, 8, 40), ("f32", 1024, 8, 40),      # the d = 40 tiled tails at N = 1024
               ("bf16", 256, 8, 160), ("f16", 256, 8, 160)]                           # the persistent d = 160 core at its own N


def _far_features(dt, N, H, D):
    from tests.test_gpu_tails import _feats
    dtype = DT[dt]
    img = 2 * N * H * D * dtype.itemsize
    n = (1 << 32) // img + 2                        # image n - 1 starts at (n - 1) img > 2^32
    mid = ((1 << 31) - 1) // img                    # ... and image `mid` holds byte 2^31 - 1
    assert (n - 1) * img > (1 << 32) and mid * img < (1 << 31) < (mid + 1) * img + 1 and 0 < mid < n - 1
    small = _feats(3, N + D, dtype, N, H, D)
    where = [0, mid, n - 1]
    big = []
    for t in small:
        b = torch.empty((n,) + tuple(t.shape[1:]), dtype=dtype, device="cuda")
        for j, i in enumerate(where):
            b[i].copy_(t[j])
        big.append(b)
    return small, tuple(big), where, n, img


def _same(a, b):
    """bit for bit, NaNs included, for a tensor or a tuple of tensors"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


@pytest.mark.parametrize("dt,N,H,D", TAIL_SHAPES)
def test_pair_tails_past_4gib(dt, N, H, D):
    from tests.test_gpu_tails import _idx
    eng = _eng()
    small, big, where, n, img = _far_features(dt, N, H, D)
    (q3, k3, v3), (q, k, v) = small, big
    pairs = [(0, 1), (1, 2), (2, 0), (2, 2)]
    ia3, ib3 = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    ia, ib = _idx(*(where[a] for a, _ in pairs)), _idx(*(where[b] for _, b in pairs))
    g = torch.Generator().manual_seed(N)
    m3 = (torch.rand(3, N, generator=g) < 0.6).to(torch.uint8).cuda()
    w3 = torch.randint(0, 256, (3, N), generator=g, dtype=torch.uint8).cuda()
    mask, wts = (torch.zeros(n, N, dtype=torch.uint8, device="cuda") for _ in range(2))
    for j, i in enumerate(where):
        mask[i], wts[i] = m3[j], w3[j]
    bad = []

    def hold(name, far, near):
        if not _same(far, near):
            bad.append(name)
    for sim in ("cosine", "mse"):
        hold(f"pair_score {sim}", eng.pair_score(q, k, v, ia, ib, H, sim), eng.pair_score(q3, k3, v3, ia3, ib3, H, sim))
        hold(f"pair_score_maps {sim}", eng.pair_score_maps(q, k, v, ia, ib, H, sim), eng.pair_score_maps(q3, k3, v3, ia3, ib3, H, sim))
        hold(f"pair_score_regions {sim}", eng.pair_score_regions(q, k, v, mask, ia, ib, H, sim),
             eng.pair_score_regions(q3, k3, v3, m3, ia3, ib3, H, sim))
        hold(f"pair_score_weights {sim}", eng.pair_score_weights(q, k, v, wts, ia, ib, H, sim),
             eng.pair_score_weights(q3, k3, v3, w3, ia3, ib3, H, sim))
    hold("pair_align", eng.pair_align(q, k, ia, ib, H), eng.pair_align(q3, k3, ia3, ib3, H))
    hold("pair_align_regions", eng.pair_align_regions(q, k, mask, ia, ib, H), eng.pair_align_regions(q3, k3, m3, ia3, ib3, H))
    hold("pair_align_weights", eng.pair_align_weights(q, k, wts, ia, ib, H), eng.pair_align_weights(q3, k3, w3, ia3, ib3, H))
    hold("pair_region_transfer", eng.pair_region_transfer(q, k, wts, ia, ib, H), eng.pair_region_transfer(q3, k3, w3, ia3, ib3, H))
    # attn_features runs every image of the tensor, the unfilled ones included (engine.attn_features cuts the images into calls, so
    # its kernels see near offsets); feature_pair_score is the call that reaches image idx[p] of feats through a 64-bit offset.  It
    # is held twice: on attn_features' own far output, and on a far feats tensor that holds only the three images' rows
    fe3, st3 = eng.attn_features(q3, k3, v3, H)
    near_fp = eng.feature_pair_score(fe3, st3, ia3, ib3)
    assert bool(torch.isfinite(near_fp).all())
    sel = torch.tensor(where, device="cuda")
    fe, st = eng.attn_features(q, k, v, H)
    hold("attn_features", (fe[sel], st[sel]), (fe3, st3))
    hold("feature_pair_score", eng.feature_pair_score(fe, st, ia, ib), near_fp)
    del fe, st
    fe_far = torch.empty((n,) + tuple(fe3.shape[1:]), dtype=fe3.dtype, device="cuda")
    st_far = torch.full((n, 4), float("nan"), device="cuda")
    fe_far[sel], st_far[sel] = fe3, st3
    hold("feature_pair_score, scattered feats", eng.feature_pair_score(fe_far, st_far, ia, ib), near_fp)
    del fe_far, st_far
    near = eng.pair_score(q3, k3, v3, ia3, ib3, H, "cosine")
    assert bool(torch.isfinite(near).all()) and float((near[:3] - 1).abs().min()) > 1e-3 and abs(float(near[3]) - 1) <= 1e-5, near
    assert not bad, f"{dt} N={N} H={H} D={D} n={n}: differ from the 3-image call: {bad}"
    NOTES[("tails", dt, N, D)] = (f"{'pair tails':18s} {dt:4s} N {N} H {H} D {D}: n {n}, images at {where} (image {img} B, the last starts at "
                                  f"{(n - 1) * img} B): 10 entry points bit for bit")
    print("\nEXTENT " + NOTES[("tails", dt, N, D)])


@pytest.mark.parametrize("dt", list(DT))
def test_matrix_tails_over_a_gallery_past_4gib(dt):
    """one query against a gallery of period 2 whose q / k / v each pass 2^32 bytes, at the smallest geometry that gets there: the
    launchers carry n_a + n_b on a 65535-wide grid axis (tails.hip matrix_shape_served, asserted below through the workspace
    query), so an image must exceed 2^32 / 65534 bytes -- N = 256, 8 heads of 16: 128 KiB in 16 bits.  The columns are periodic bit
    for bit and equal the 1 x 2 matrix.  score_matrix_regions reads listed rows through 32-bit ELEMENT indices and refuses a set of
    2^31 elements or more: in 16 bits that is 2^32 bytes exactly, so there the form must refuse the gallery (a DsimError before any
    launch) and runs at the largest gallery it accepts, 4 GiB less one image; in f32 it runs on the whole gallery"""
    from tests.test_gpu_tails import _feats
    from diffsim_amd.engine import _Handle
    eng = _eng()
    N, H, D = 256, 8, 16
    dtype = DT[dt]
    img = 2 * N * H * D * dtype.itemsize
    nb = (1 << 32) // img + 3
    assert (nb - 1) * img > (1 << 32) and nb + 1 <= 65535
    assert eng.score_matrix_workspace_bytes(1, 65534, 2, H, N, D, dtype) > 0 and eng.score_matrix_workspace_bytes(1, 65535, 2, H, N, D, dtype) == 0
    f5 = _feats(5, 5, dtype, N, H, D)
    fa = tuple(t[:1].contiguous() for t in f5)
    fb2 = tuple(t[1:3].contiguous() for t in f5)
    fl2 = tuple(t[3:].contiguous() for t in f5)                    # two further images: the gallery's LAST two
    fb = tuple(E.periodic_rows(t, nb) for t in fb2)
    g = torch.Generator().manual_seed(3)
    ma = (torch.rand(1, N, generator=g) < 0.6).to(torch.uint8).cuda()
    mb2 = (torch.rand(2, N, generator=g) < 0.6).to(torch.uint8).cuda()
    ml2 = (torch.rand(2, N, generator=g) < 0.6).to(torch.uint8).cuda()
    mb = E.periodic_rows(mb2, nb)
    served = lambda m: eng.score_matrix_regions_workspace_bytes(1, m, 2, H, N, D, dtype) > 0
    nr = nb
    if not served(nb):
        assert nb * 2 * N * H * D >= (1 << 31), "refused below the documented 2^31 elements"
        with pytest.raises(_err()):
            eng.score_matrix_regions(fa, fb, ma, mb, H, "cosine")
        nr = _Handle._largest(served, nb)
        assert nr == ((1 << 31) - 1) // (2 * N * H * D) and nr * img > (1 << 31)
    else:
        assert nb * 2 * N * H * D < (1 << 31)

    def plant(n_, distinct):
        """images n_ - 2, n_ - 1 of the gallery and their mask rows: the two distinct images, or back to the period.  An image is a
        power of two bytes here, so an offset taken modulo 2^32 would land on an image of the same parity: only images that differ
        from their parity's show such a wrap"""
        src, msk = (fl2, ml2) if distinct else (tuple(torch.roll(t, n_ % 2, 0) for t in fb2), torch.roll(mb2, n_ % 2, 0))
        for t, u in zip(fb, src):
            t[n_ - 2:n_].copy_(u)
        mb[n_ - 2:n_].copy_(msk)
    what = []
    runs = (("score_matrix_regions", nr, lambda f, m: eng.score_matrix_regions(fa, f, ma, m, H, sim)),
            ("score_matrix", nb, lambda f, m: eng.score_matrix(fa, f, H, sim)))
    for name, n_, call in runs:
        assert (n_ - 2) * img > ((1 << 32) if n_ == nb else (1 << 31))
        plant(n_, True)
        for sim in ("cosine", "mse"):
            m, m2, ml = call(tuple(t[:n_] for t in fb), mb[:n_]), call(fb2, mb2), call(fl2, ml2)
            assert m.shape == (1, n_) and bool(torch.isfinite(m2).all()) and bool(torch.isfinite(ml).all())
            assert not _same(ml, m2) and not _same(ml, m2.flip(1))
            if not _same(m[:, n_ - 2:], ml):
                what.append(f"{name} {sim}: the last two columns {m[:, n_ - 2:].tolist()} are not the distinct images' {ml.tolist()}")
            if not (_same(m[:, :2], m2) and E.periodic_ok(m.view(-1), n_ - 2, 1, 2)):
                what.append(f"{name} {sim}: columns {E.periodic_bad_rows(m.view(-1), n_ - 2, 1, 2)}")
        plant(n_, False)
    assert not what, what
    NOTES[("matrix", dt)] = (f"{'matrix tails':18s} {dt:4s} N {N} H {H} D {D}: score_matrix over {nb} images, {nb * img} B per tensor; "
                             f"score_matrix_regions over {nr} images, {nr * img} B" + ("" if nr == nb else f" (refused at {nb}: 2^31 elements)"))
    print("\nEXTENT " + NOTES[("matrix", dt)])
